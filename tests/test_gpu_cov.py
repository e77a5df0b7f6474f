"""-m gpu: the BISCUITqc coverage tables on the device.  (1) bsx_cov_batch / bsx_cov_set_mask / bsx_cov_tables (k_cov.hip) against numpy
(np.add.at, cumsum, bincount) on a genome of three tiles with bases planted at every spot the last pass treats specially, designed jobs and
designed masks; (2) the HIP command line with --qc PREFIX --qc-cov against tests/cov_model.py over the SAM it wrote and against the CPU
checker's files (whose depth state is the host's), SAM unchanged, also with a --bsconv filter and with --markdup; (3) the tables of a stream
against the model and against the process's.  Every comparison is exact."""
import ctypes as C
import os
import numpy as np
import pytest
import simdata
import e2e_cases as E
import bsconv_cases as B
import cov_cases as CV
import cov_model as V
import qc_cases as QC
import qc_model as Q

pytestmark = pytest.mark.gpu
HIP = os.path.join(E.ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(E.ROOT, "oracle", "oracle_align")


# ------------------------------------------------------------------ (1) the kernels against numpy
def _genome(T):
    """contigs of T + 1, 37 and 2 T - 5 bases: C at T - 1 and G at T (a CpG whose C is the last position of tile 0); contig 1 ends in C and
    contig 2 begins with G (no CpG); C before an N run and G after it, an N run across the tile boundary at 2 T, single N's between C and G
    (pac holds a random base under every N)"""
    r = np.random.default_rng(5)
    c0, c1, c2 = (r.integers(0, 4, n).astype(np.uint8) for n in (T + 1, 37, 2 * T - 5))
    c0[T - 1], c0[T] = 1, 2
    c0[0], c0[1] = 1, 2                      # a CpG at the genome's first base
    c1[-1], c2[0] = 1, 2
    c2[-2], c2[-1] = 1, 2                    # ... and at its last
    at = T - 38                              # contig 2 starts at T + 38: its local T - 38 is global 2 T
    c2[at - 10:at + 10] = 4
    c2[at - 11], c2[at + 10] = 1, 2
    for k in range(40):                      # C N G, C N and N G
        p = 100 + 37 * k
        c2[p:p + 3] = (1, 4, 2)
    return [("t0", c0), ("t1", c1), ("t2", c2)]


def _expect(contigs, jobs, top=None, bot=None):
    """the tables by numpy: jobs = [(fpos, [(len, op)], q40)], masks = [(beg, end)] or None"""
    g = np.concatenate([c for _, c in contigs])
    L = len(g)
    diff = np.zeros((L + 1, 2), np.int64)
    for fpos, ops, q40 in jobs:
        y = fpos
        for n, op in ops:
            if op == "M":
                np.add.at(diff, ([y, y + n], [0, 0]), [1, -1])
                if q40:
                    np.add.at(diff, ([y, y + n], [1, 1]), [1, -1])
            if op in "MD":
                y += n
    dep = np.cumsum(diff, axis=0)[:L]
    cpg = np.zeros(L, bool)
    cpg[:-1] = (g[:-1] == 1) & (g[1:] == 2)
    ends = np.cumsum([len(c) for _, c in contigs])[:-1]
    cpg[ends - 1] = False                    # the C is a contig's last base
    cdep = np.minimum(dep[:-1], dep[1:])
    nb = int(dep[:, 0].max()) + 1
    out = []
    regions = [np.ones(L, bool)]
    for iv in ([] if top is None else [top, bot]):
        m = np.zeros(L, bool)
        for b, e in iv:
            m[b:e] = True
        regions.append(m)
    for m in regions:
        m2 = m.copy()
        m2[:-1] |= m[1:]                     # a CpG lies in a mask when either base does
        for cls in range(2):
            out.append(np.bincount(dep[m, cls], minlength=nb))
            sel = (cpg & m2)[:-1]
            out.append(np.bincount(cdep[sel, cls], minlength=nb))
    return out


def _job_arrays(jobs):
    from biscuit_amd import _lib as L_
    arr, pool = [], []
    for fpos, ops, q40 in jobs:
        arr.append((fpos, 0, 0, 0, len(pool), len(ops), L_.QC_COV | (L_.QC_COV_Q40 if q40 else 0) | L_.QC_STRAND))
        pool += [n << 4 | "MIDSH".index(op) for n, op in ops]
    return np.array(arr, dtype=np.dtype(L_.QcJob)).reshape(-1), np.array(pool, dtype=np.uint32)


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and (a == b).all(), (what, V.NAMES[i], a[:8].tolist(), b[:8].tolist(), np.flatnonzero(a != b)[:8].tolist() if a.shape == b.shape else (a.shape, b.shape))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device
    d = str(tmp_path_factory.mktemp("cov_k"))
    T = L_.COV_TILE
    contigs = _genome(T)
    simdata.write_genome(d + "/k.fa", contigs)
    Index.build(d + "/k.fa", d + "/k").close()
    idx = Index(d + "/k")
    dev = Device(0)
    dev.upload_index(idx)
    yield dev, contigs, T, idx.l_pac
    for k in ("cov_lds_bins", "cov_flush_tiles"):
        L_.tune(k, None)
    dev.close()
    idx.close()


def _designed(T, L):
    return [(0, [(50, "M")], True),                                           # at column 0
            (L - 30, [(30, "M")], False),                                     # ends on the genome's last base
            (T - 10, [(11, "M")], True),                                      # across the tile boundary at T
            (T + 60, [(5, "S"), (10, "M"), (2, "I"), (3, "M"), (4, "D"), (6, "M"), (3, "H")], True),
            (T - 1, [(1, "M")], False), (T - 1, [(1, "M")], True),            # only the C of the CpG at T - 1, T
            (T, [(1, "M")], False),                                           # only its G
            (0, [(1, "M")], False), (L - 1, [(1, "M")], True),                # the C of the first CpG, the G of the last
            (2 * T - 40, [(90, "M")], True), (T + 38 + 90, [(130, "M"), (1, "D"), (7, "M")], False)]      # over the N runs
    # (the model's rule, not the aligner's habits: depth is counted under N runs and across contig ends as well)


def _masks(T, L):
    top = [(31, 40), (64, 96), (100, 128), (160, 161), (300, 300 + 1500), (T - 1, T), (2 * T - 100, 2 * T + 100), (T + 38 - 10, T + 38)]
    bot = [(20, 50), (32, 33), (T, T + 1), (T - 5, T + 7), (L - 3, L), (0, 1), (900, 900)]
    return top, bot


def test_no_jobs_designed_jobs_batches_reads_and_reset(small):
    dev, contigs, T, L = small
    assert L == 3 * T + 33
    jobs = _designed(T, L)
    long_run = [(5, [(2 * T + 3, "M")], True)]                                # tile 1: a carry-in and no event
    dev.cov_reset()
    _same(dev.cov_tables(), _expect(contigs, []), "no jobs")
    a, pool = _job_arrays(long_run)
    dev.cov_batch(a, pool)
    _same(dev.cov_tables(), _expect(contigs, long_run), "one long run")
    dev.cov_reset()
    _same(dev.cov_tables(), _expect(contigs, []), "after reset")
    a, pool = _job_arrays(jobs)
    dev.cov_batch(a, pool)
    one = dev.cov_tables()
    _same(one, _expect(contigs, jobs), "designed jobs")
    assert one[1][1:].sum() > 0 and one[3][1:].sum() > 0 and (one[0] != one[2]).any()
    _same(dev.cov_tables(), one, "read twice")
    dev.cov_reset()
    for lo, hi in ((0, 1), (1, 4), (4, 4), (4, len(a))):                      # (the pool is shared: cig_off stays valid)
        dev.cov_batch(a[lo:hi], pool)
    _same(dev.cov_tables(), one, "several batches")
    a2, pool2 = _job_arrays(long_run)
    dev.cov_batch(a2, pool2)
    _same(dev.cov_tables(), _expect(contigs, jobs + long_run), "more jobs after a read")


def test_masks(small):
    dev, contigs, T, L = small
    from biscuit_amd import _lib as L_
    jobs = _designed(T, L) + [(5, [(2 * T + 3, "M")], False)]
    top, bot = _masks(T, L)
    a, pool = _job_arrays(jobs)
    dev.cov_reset()
    dev.cov_batch(a, pool)
    dev.cov_set_mask(L_.COV_MASK_TOPGC, top)
    with pytest.raises(L_.BsxError):
        dev.cov_tables()                                                      # one mask without the other
    dev.cov_set_mask(L_.COV_MASK_BOTGC, bot)
    got = dev.cov_tables()
    _same(got, _expect(contigs, jobs, top, bot), "masks")
    assert len(got) == 12 and all(t.sum() > 0 for t in got[4:])
    dev.cov_set_mask(L_.COV_MASK_TOPGC, bot)                                  # a mask set again replaces the one there was
    dev.cov_set_mask(L_.COV_MASK_BOTGC, [])
    _same(dev.cov_tables(), _expect(contigs, jobs, bot, []), "replaced and empty")
    for bad in ([(-1, 5)], [(5, 4)], [(0, L + 1)]):
        with pytest.raises(L_.BsxError):
            dev.cov_set_mask(0, bad)
    _same(dev.cov_tables(), _expect(contigs, jobs, bot, []), "after refused masks")
    dev.cov_reset()
    _same(dev.cov_tables(), _expect(contigs, []), "reset drops the masks")


@pytest.mark.parametrize("bins,flush", [(4, None), (None, None), (64, 1)])
def test_deep_positions_with_small_and_default_lds_histograms(small, bins, flush):
    dev, contigs, T, L = small
    from biscuit_amd import _lib as L_
    jobs = [(T - 50, [(100, "M")], k < 1000) for k in range(3000)] + _designed(T, L)
    top, bot = _masks(T, L)
    a, pool = _job_arrays(jobs)
    L_.tune("cov_lds_bins", bins)
    L_.tune("cov_flush_tiles", flush)
    try:
        dev.cov_reset()
        dev.cov_batch(a, pool)
        dev.cov_set_mask(0, top)
        dev.cov_set_mask(1, bot)
        got = dev.cov_tables()
        assert len(got[0]) >= 3001
        _same(got, _expect(contigs, jobs, top, bot), (bins, flush))
        for bad in (3, 1024, 0):
            L_.tune("cov_lds_bins", bad)
            with pytest.raises(L_.BsxError):
                dev.cov_tables()
    finally:
        L_.tune("cov_lds_bins", None)
        L_.tune("cov_flush_tiles", None)
        dev.cov_reset()


def test_an_out_of_range_job_is_refused_and_changes_nothing(small):
    dev, contigs, T, L = small
    from biscuit_amd import _lib as L_
    jobs = _designed(T, L)
    a, pool = _job_arrays(jobs)
    dev.cov_reset()
    dev.cov_batch(a, pool)
    want = _expect(contigs, jobs)
    for bad in ((-1, [(5, "M")], True), (L - 4, [(5, "M")], True), (L - 4, [(2, "M"), (3, "D")], True), (L + 1, [(1, "S")], True)):
        b, bpool = _job_arrays(jobs[:3] + [bad])
        with pytest.raises(L_.BsxError) as e:
            dev.cov_batch(b, bpool)
        assert "(-2)" in str(e.value)                                         # BSX_E_ARG
    b, bpool = _job_arrays(jobs[:3])
    b[2]["cig_off"] = len(bpool)                                              # CIGAR words beyond the pool
    with pytest.raises(L_.BsxError):
        dev.cov_batch(b, bpool)
    _same(dev.cov_tables(), want, "after refused batches")
    dev.cov_reset()


# ------------------------------------------------------------------ (2) the command line
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cov_gpu"))
    contigs = B.make_data(d, genome_bp=300000, n_pairs=3000, n_long=150)
    top, bot = CV.write_beds(d, contigs)
    return d, Q.read_fasta(d + "/g.fa"), top, bot


def test_hip_command_line_files_equal_model_and_cpu_checker(data):
    d, refs, top, bot = data
    seen = []
    for case, gc in (("pe150_b0", True), ("se150", False), ("long_1kb", False)):
        args = dict(E.CASES_CORE)[case]
        opts = ["--qc-topgc", top, "--qc-botgc", bot] if gc else []
        plain, _ = B.run(HIP, args, d)
        qsam, qfiles = QC.run_qc(HIP, [], args, d, d + "/hq_" + case)
        sam, files7, cov = CV.run_cov(HIP, opts, args, d, d + "/hip_" + case)
        assert sam == plain and files7 == qfiles and len(qfiles) == (7 if "b2.fq" in args else 6), case
        seen.append(CV.check_files(cov, sam, refs, top if gc else None, bot if gc else None, case))
        csam, cfiles7, ccov = CV.run_cov(CPU, opts, args, d, d + "/cpu_" + case)
        E.assert_same_sam(sam.encode(), csam.encode(), case)
        assert cov == ccov and files7 == cfiles7, case
    CV.assert_not_vacuous(seen)


def test_with_a_bsconv_filter_and_with_markdup(data):
    d, refs, top, bot = data
    args = dict(E.CASES_CORE)["pe150_b0"]
    plain, _ = B.run(HIP, args, d)
    sam, _, cov = CV.run_cov(HIP, ["--bsconv-max-cph", "3"], args, d, d + "/hip_flt")
    only, _ = B.run(HIP, ["--bsconv-max-cph", "3"] + args, d)
    assert sam == only and 0 < sam.count("\n") < plain.count("\n")
    flt = CV.check_files(cov, sam, refs, None, None, "filtered")
    for k in (1, 2):                                                          # 400 pairs and the same pairs again under other names
        rec = open(d + "/b%d.fq" % k).read().split("\n")[:1600]
        with open(d + "/d%d.fq" % k, "w") as f:
            f.write("\n".join(rec) + "\n" + "\n".join("@again_" + l[1:] if i % 4 == 0 else l for i, l in enumerate(rec)) + "\n")
    args = ["-@", "4", "g", "d1.fq", "d2.fq"]
    sam, _, cov = CV.run_cov(HIP, ["--markdup"], args, d, d + "/hip_md")
    only, _ = B.run(HIP, ["--markdup"] + args, d)
    assert sam == only and sum(1 for l in sam.split("\n") if l and l[0] != "@" and int(l.split("\t")[1]) & 0x400) > 0
    md = CV.check_files(cov, sam, refs, None, None, "markdup")                # 0x400 records count like any other
    assert md[0] != flt[0]


# ------------------------------------------------------------------ (3) a stream
def test_stream_tables_equal_the_model_and_the_process_tables(data):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device, default_opt, cov_tables_arrays
    d, refs, top, bot = data
    L = L_.lib()
    idx = Index(d + "/g")
    dev = Device(0)
    dev.upload_index(idx)
    opt = default_opt()
    opt.n_threads = 4
    opt.flag |= 0x10 | 0x2
    L.bsx_sim_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]
    L.bsx_sim_free_reads.argtypes = [C.c_void_p, C.c_int64]
    L.bsx_stream_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.bsx_stream_push.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.bsx_stream_flush.argtypes = [C.c_void_p]
    L.bsx_stream_close.argtypes = [C.c_void_p]
    L.bsx_stream_close.restype = None
    L.bsx_stream_set_qc.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_set_qc_cov.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_set_qc_cov_mask.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    L.bsx_stream_qc_cov_tables.argtypes = [C.c_void_p, C.c_void_p]
    L.bsx_process_qc_cov_tables.argtypes = [C.c_void_p]
    L.bsx_cov_tables_free.argtypes = [C.c_void_p]
    L.bsx_cov_tables_free.restype = None
    n_pairs, chunks, got = 2000, [], []
    names = list(refs)
    offs = np.concatenate([[0], np.cumsum([len(refs[n]) for n in names])])
    beds = [V.read_bed(top), V.read_bed(bot)]
    try:
        for how in ("stream", "process"):
            ch = []
            for k in range(2):
                p = C.c_void_p()
                L_.check(L.bsx_sim_pairs(idx.h, n_pairs, 150, 700 + k, 200, 500, 0.01, 0.2, C.byref(p)), "sim_pairs")
                ch.append(p)
            chunks += ch
            s = C.c_void_p()
            L_.check(L.bsx_stream_open(dev.h, C.byref(opt), idx.h, None, C.byref(s)), "stream_open")
            if how == "stream":
                assert L.bsx_stream_set_qc_cov(s, 1) == -2                    # needs set_qc before it
                L_.check(L.bsx_stream_set_qc(s, 1), "set_qc")
                L_.check(L.bsx_stream_set_qc_cov(s, 1), "set_qc_cov")
                for w in range(2):
                    iv = np.array([(offs[names.index(c)] + b, offs[names.index(c)] + e) for c, b, e in beds[w]], np.int64)
                    L_.check(L.bsx_stream_set_qc_cov_mask(s, w, len(iv), iv.ctypes.data_as(C.c_void_p)), "mask")
            else:
                L_.check(L.bsx_process_set_qc(1), "process_set_qc")
                L_.check(L.bsx_process_set_qc_cov(1), "process_set_qc_cov")
            for k in range(2):
                L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, ch[k]), "push")
            L_.check(L.bsx_stream_flush(s), "flush")
            t = L_.CovTables()
            L_.check(L.bsx_stream_qc_cov_tables(s, C.byref(t)) if how == "stream" else L.bsx_process_qc_cov_tables(C.byref(t)), "tables")
            got.append(cov_tables_arrays(t))
            L.bsx_cov_tables_free(C.byref(t))
            L.bsx_stream_close(s)
            if how == "process":
                L.bsx_process_set_qc_cov(0)
                L.bsx_process_set_qc(0)
        text = ""
        for k in range(2):
            rd = C.cast(chunks[k], C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        want = V.tables(text, refs, beds[0], beds[1])
        nb = max(want[0]) + 1
        assert len(got[0]) == 12 and len(got[1]) == 4 and nb >= 3
        for i in range(12):
            w = np.array([want[i].get(dd, 0) for dd in range(nb)], np.int64)
            assert (got[0][i] == w).all(), V.NAMES[i]
            if i < 4:
                assert (got[1][i] == w).all(), V.NAMES[i]
    finally:
        L.bsx_process_set_qc_cov(0)
        L.bsx_process_set_qc(0)
        for ch in chunks:
            L.bsx_sim_free_reads(ch, 2 * n_pairs)
        dev.close()
        idx.close()
