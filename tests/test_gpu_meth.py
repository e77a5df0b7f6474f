"""-m gpu: BISCUITqc's base-averaged conversion table on the device.  (1) bsx_meth_batch / bsx_meth_read / bsx_meth_tables (k_meth.hip) on the
three-contig, three-tile genome of tests/test_gpu_cov.py (CpGs on tile and contig edges, an N run across a tile boundary): a few hundred designed
jobs, all four counters at every position against a plain walk of the rule, the sums of every context against tests/meth_model.py; then jobs
repeated at chosen cytosines to plant exact and inexact ties of the beta and an uncallable site; (2) the HIP command line with --qc PREFIX
--qc-meth against the model over the SAM it wrote and against the CPU checker's file (whose counters are the host's), SAM unchanged, also with
--markdup and with a --bsconv filter; (3) the sums of a stream against the process's and the model's.  Every comparison is exact."""
import ctypes as C
import os
import numpy as np
import pytest
import simdata
import e2e_cases as E
import bsconv_cases as B
import meth_cases as MC
import meth_model as M
import qc_cases as QC
import qc_model as Q

pytestmark = pytest.mark.gpu
HIP = os.path.join(E.ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(E.ROOT, "oracle", "oracle_align")


# ------------------------------------------------------------------ (1) the kernels against a plain walk of the rule
class Job:
    """a record in the record's own orientation: seq = the whole read (H bases included), lowq = positions of it below the quality floor"""

    def __init__(self, fpos, ops, seq, rev=False, read2=False, tag=0, lowq=(), ov=(0, 0)):
        self.fpos, self.ops, self.seq, self.rev, self.read2, self.tag, self.lowq, self.ov = fpos, ops, np.asarray(seq, np.uint8), rev, read2, tag, set(lowq), ov
        assert len(self.seq) == sum(n for n, op in ops if op in "MISH")


def _make(r, g, fpos, ops, p_other=0.03, **kw):
    """a job whose read follows the genome g over its M columns: C or T over a C, G or A over a G, now and then another base"""
    seq, y = [], fpos
    for n, op in ops:
        if op == "M":
            for j in range(n):
                b = int(g[y + j])
                b = int(r.integers(0, 4)) if b == 4 or r.random() < p_other else b
                if b == 1 and r.random() < 0.5:
                    b = 3
                elif b == 2 and r.random() < 0.5:
                    b = 0
                seq.append(b)
            y += n
        elif op == "D":
            y += n
        else:
            seq += [int(x) for x in r.integers(0, 4, n)]
    return Job(fpos, ops, seq, **kw)


def _walk(g, jobs):
    """the rule of include/bsx.h (bsx_meth_job_t), column by column -> int64[L, 4]"""
    cnt = np.zeros((len(g), 4), np.int64)
    for J in jobs:
        rlen = len(J.seq)
        cols, x, y = [], 0, J.fpos
        for n, op in J.ops:
            if op == "M":
                cols += [(x + j, y + j) for j in range(n)]
                x += n
                y += n
            elif op == "D":
                y += n
            else:
                x += n
        strand = J.tag
        if J.tag not in (0, 1):
            good = [(q, f) for q, f in cols if q not in J.lowq]
            strand = 0 if sum(g[f] == 1 and J.seq[q] == 3 for q, f in good) >= sum(g[f] == 2 and J.seq[q] == 0 for q, f in good) else 1
        for q, f in cols:
            if q in J.lowq or q + 1 <= 3 or rlen < q + 1 + 3 or g[f] not in (1, 2) or (J.read2 and J.ov[0] <= f < J.ov[1]):
                continue
            own = g[f] == (2 if strand else 1)
            if J.seq[q] == g[f]:
                cnt[f, 0 if own else 2] += 1
            elif J.seq[q] == (3 if g[f] == 1 else 0):
                cnt[f, 1 if own else 3] += 1
    return cnt


def _arrays(jobs):
    """-> (_lib.MethJob array, pool, read buffer): the reads as sequenced (a reverse record's read is the complement of its SEQ from the far end)"""
    from biscuit_amd import _lib as L_
    arr, pool = [], []
    buf, offs = simdata.read_buffer([simdata.revcomp(J.seq) if J.rev else J.seq for J in jobs])
    for i, J in enumerate(jobs):
        cig = len(pool)
        pool += [n << 4 | "MIDSH".index(op) for n, op in J.ops]
        qm = len(pool)
        bits = np.ones(len(J.seq), np.uint8)
        bits[np.array(sorted(J.lowq), dtype=np.int64)] = 0
        words = np.packbits(np.concatenate([bits, np.zeros(-len(bits) % 32, np.uint8)]), bitorder="little").view("<u4")
        pool += [int(w) for w in words]
        arr.append((J.fpos, int(offs[i]), 0, len(J.seq), cig, len(J.ops), (L_.QC_REVERSE if J.rev else 0) | (L_.QC_READ2 if J.read2 else 0) | J.tag << 2, qm, 0, J.ov[0], J.ov[1]))
    return np.array(arr, dtype=np.dtype(L_.MethJob)).reshape(-1), np.array(pool, dtype=np.uint32), buf


def _model_sums(contigs, cnt):
    refs = {name: "".join("ACGTN"[b] for b in c) for name, c in contigs}
    per, at = {}, 0
    for name, c in contigs:
        per[name] = cnt[at:at + len(c)].tolist()
        at += len(c)
    K, S, unc = M.tables(per, refs)
    return np.array(K, np.int64), np.array(S, np.int64), unc


def _run(dev, jobs, cuts=None):
    a, pool, buf = _arrays(jobs)
    dev.set_reads(buf)
    cuts = cuts or [0, len(a)]
    for lo, hi in zip(cuts, cuts[1:]):                                        # (the pool and the read buffer are shared: offsets stay valid)
        dev.meth_batch(a[lo:hi], pool)


def _same_counters(dev, want, what):
    got = dev.meth_read(0, len(want))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device
    import test_gpu_cov as TC
    d = str(tmp_path_factory.mktemp("meth_k"))
    T = L_.COV_TILE
    contigs = TC._genome(T)
    simdata.write_genome(d + "/k.fa", contigs)
    Index.build(d + "/k.fa", d + "/k").close()
    idx = Index(d + "/k")
    dev = Device(0)
    dev.upload_index(idx)
    yield dev, contigs, T, idx.l_pac
    L_.tune("meth_flush_tiles", None)
    dev.close()
    idx.close()


def _designed(g, T, L):
    r = np.random.default_rng(11)
    S3, H4 = (3, "S"), (4, "H")
    jobs = [_make(r, g, 0, [S3, (50, "M"), S3]),                              # column 0 counts: q1 = 4
            _make(r, g, L - 30, [H4, (30, "M"), S3], tag=1),                  # ... and the genome's last base
            _make(r, g, 0, [(50, "M")]), _make(r, g, L - 30, [(30, "M")], rev=True),      # the end rules drop three columns on either side
            _make(r, g, T - 10, [S3, (21, "M"), S3]), _make(r, g, T - 10, [S3, (21, "M"), S3], tag=1, rev=True),      # across the tile boundary at T
            _make(r, g, T - 4, [(3, "H"), (4, "M"), (1, "I"), (1, "M"), (3, "S")], tag=1),
            _make(r, g, T + 60, [(5, "S"), (10, "M"), (2, "I"), (3, "M"), (4, "D"), (6, "M"), (3, "H")]),
            _make(r, g, T + 60, [(5, "H"), (10, "M"), (2, "I"), (3, "M"), (4, "D"), (6, "M"), (3, "S")], rev=True, tag=1, lowq=[5, 6, 17, 20]),
            _make(r, g, 2 * T - 40, [S3, (90, "M"), S3]), _make(r, g, 2 * T - 40, [S3, (90, "M"), S3], tag=1),      # over the N run
            _make(r, g, T + 38 + 90, [H4, (130, "M"), (1, "D"), (7, "M"), H4], tag=3),      # over the C N G triplets, inferred
            _make(r, g, T + 1 + 30, [S3, (20, "M"), S3]),                     # from contig t1 into t2: depth is counted, the sites are CN
            _make(r, g, 100, [S3, (700, "M"), (5, "D"), (800, "M"), (7, "I"), (600, "M"), S3], tag=3, lowq=range(0, 2100, 7)),      # longer than two LDS tiles
            _make(r, g, 40, [(2000, "M")], rev=True, read2=True, ov=(900, 1100), tag=1)]
    for k in range(320):                                                      # ordinary records of every kind
        n1, n2, n3 = (int(x) for x in r.integers(1, 60, 3))
        ops = [(int(r.integers(0, 6)), "SH"[k & 1]), (n1, "M"), (int(r.integers(1, 4)), "ID"[k >> 1 & 1]), (n2, "M"), (int(r.integers(1, 3)), "DI"[k >> 1 & 1]), (n3, "M"),
               (int(r.integers(0, 6)), "HS"[k & 1])]
        ops = [(n, op) for n, op in ops if n]
        span = sum(n for n, op in ops if op in "MD")
        fpos = int(r.integers(0, L - span + 1))
        rlen = sum(n for n, op in ops if op in "MISH")
        ov = (fpos + int(r.integers(0, span)), fpos + int(r.integers(0, span + 40))) if k % 3 == 0 else (0, 0)
        jobs.append(_make(r, g, fpos, ops, rev=bool(k & 4), read2=k % 3 == 0, tag=(0, 1, 3, 2)[k % 4] if k % 5 else 3,
                          lowq=[int(x) for x in r.integers(0, rlen, int(r.integers(0, 12)))], ov=ov))
    return jobs


def test_designed_jobs_every_counter_and_the_sums(small):
    from biscuit_amd import _lib as L_
    dev, contigs, T, L = small
    g = np.concatenate([c for _, c in contigs])
    assert L == 3 * T + 33 == len(g)
    dev.meth_reset()
    assert (dev.meth_read(0, L) == 0).all() and (dev.meth_tables()[0] == 0).all()      # no state yet
    jobs = _designed(g, T, L)
    want = _walk(g, jobs)
    assert (want[0] > 0).any() and (want[L - 1] > 0).any() and (want[T - 1] > 0).any() and (want[T] > 0).any() and (want[:, 3] > 0).any()
    assert want[2 * T - 10:2 * T + 10].sum() == 0 and want[2 * T - 11].sum() > 0      # nothing inside the N run, something at the C before it
    _run(dev, jobs)
    _same_counters(dev, want, "designed jobs")
    assert (dev.meth_read(T - 3, 7) == want[T - 3:T + 4]).all() and (dev.meth_read(L - 1, 1) == want[L - 1:]).all()      # windows
    K, S, unc = _model_sums(contigs, want)
    assert K.min() > 0 and unc > 0, (K, unc)
    k1, s1 = dev.meth_tables()
    assert (k1 == K).all() and (s1 == S).all(), (k1, K, s1, S)
    L_.tune("meth_flush_tiles", 1)                                            # a wave adds its sums after every tile
    k2, s2 = dev.meth_tables()
    L_.tune("meth_flush_tiles", None)
    assert (k2 == K).all() and (s2 == S).all()
    for bad in (0, 1025):
        L_.tune("meth_flush_tiles", bad)
        with pytest.raises(L_.BsxError):
            dev.meth_tables()
    L_.tune("meth_flush_tiles", None)
    dev.meth_reset()
    assert (dev.meth_read(0, L) == 0).all()
    _run(dev, jobs, cuts=[0, 1, 14, 14, 100, len(jobs)])                      # several batches
    _same_counters(dev, want, "several batches")
    _run(dev, jobs[:15])                                                      # more jobs after a read
    _same_counters(dev, want + _walk(g, jobs[:15]), "more jobs")
    dev.meth_reset()


def test_planted_ties_and_an_uncallable_site(small):
    dev, contigs, T, L = small
    g = np.concatenate([c for _, c in contigs])
    free = [p for p in range(200, T - 200) if g[p] == 1 and g[p + 1] < 4]      # cytosines of contig t0 with a context
    by_ctx = {x: [p for p in free if g[p + 1] == x] for x in range(4)}
    plan = [(by_ctx[0][0], 1, 16), (by_ctx[1][0], 3, 16), (by_ctx[2][0], 1, 80), (by_ctx[3][0], 3, 80), (by_ctx[0][1], 7, 80), (by_ctx[1][1], 1, 3), (by_ctx[2][1], 2, 3)]
    unc = by_ctx[3][1]
    one = [(3, "S"), (1, "M"), (3, "S")]                                      # the only column has q1 = 4 of 7
    jobs = []
    for p, ret, n in plan:
        jobs += [Job(p, one, [0, 0, 0, 1 if k < ret else 3, 0, 0, 0]) for k in range(n)]
    jobs += [Job(unc, one, [0, 0, 0, 1, 0, 0, 0]) for _ in range(19)] + [Job(unc, one, [0, 0, 0, 3, 0, 0, 0], tag=1)]      # 20 * 1 < 19 + 0 fails
    jobs += [Job(T - 1, one, [0, 0, 0, 1, 0, 0, 0]), Job(T, one, [0, 0, 0, 0, 0, 0, 0], tag=1)]      # the CpG across the tile boundary: ret at C, conv at G
    dev.meth_reset()
    _run(dev, jobs)
    want = _walk(g, jobs)
    for p, ret, n in plan:
        assert want[p].tolist() == [ret, n - ret, 0, 0]
    assert want[unc].tolist() == [19, 0, 0, 1] and want[T - 1].tolist() == [1, 0, 0, 0] and want[T].tolist() == [0, 1, 0, 0]
    _same_counters(dev, want, "planted")
    K, S, n_unc = _model_sums(contigs, want)
    # 0.0625 -> 0.062 and 0.1875 -> 0.188 (exact ties, to even); 1 / 80, 3 / 80, 7 / 80 in double lie above, below, below their ties
    assert K.tolist() == [2, 2, 4, 1, 0] and S.tolist() == [62 + 87, 188 + 333, 13 + 667 + 1000 + 0, 37, 0] and n_unc == 1
    k, s = dev.meth_tables()
    assert (k == K).all() and (s == S).all(), (k, s)
    dev.meth_reset()


def test_an_out_of_range_job_is_refused_and_changes_nothing(small):
    from biscuit_amd import _lib as L_
    dev, contigs, T, L = small
    g = np.concatenate([c for _, c in contigs])
    r = np.random.default_rng(3)
    jobs = _designed(g, T, L)[:12]
    dev.meth_reset()
    _run(dev, jobs)
    want = _walk(g, jobs)
    a, pool, buf = _arrays(jobs[:3] + [_make(r, g, L - 40, [(30, "M")])])
    for field, value in (("fpos", -1), ("fpos", L - 29), ("fpos", L), ("cig_off", len(pool)), ("qm_off", len(pool)), ("rlen", 0), ("rlen", 64)):
        b = a.copy()
        b[field][3] = value                                                   # (rlen 64: a second mask word, beyond the pool)
        with pytest.raises(L_.BsxError) as e:
            dev.meth_batch(b, pool)
        assert "(-2)" in str(e.value), field                                  # BSX_E_ARG
    _same_counters(dev, want, "after refused batches")
    with pytest.raises(L_.BsxError):
        dev.meth_read(L - 3, 4)
    dev.meth_reset()


# ------------------------------------------------------------------ (2) the command line
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("meth_gpu"))
    MC.make_data(d, genome_bp=300000, n_pairs=3000, n_long=150)
    return d, Q.read_fasta(d + "/g.fa")


def test_hip_command_line_file_equals_model_and_cpu_checker(data):
    d, refs = data
    seen = []
    for case, opts, args in (("pe150_b0", [], dict(E.CASES_CORE)["pe150_b0"]), ("markdup", ["--markdup"], ["-@", "4", "g", "d1.fq", "d2.fq"]),
                             ("filtered", ["--bsconv-max-cph", "3"], dict(E.CASES_CORE)["pe150_b0"])):
        only, _ = B.run(HIP, opts + args, d)
        qsam, qfiles = QC.run_qc(HIP, opts, args, d, d + "/hq_" + case)
        sam, files7, got = MC.run_meth(HIP, opts, args, d, d + "/hip_" + case)
        assert sam == only == qsam and files7 == qfiles and len(qfiles) == 7, case
        seen.append(MC.check_file(got, sam, refs, case))
        csam, cfiles7, cgot = MC.run_meth(CPU, opts, args, d, d + "/cpu_" + case)
        E.assert_same_sam(sam.encode(), csam.encode(), case)
        assert got == cgot and files7 == cfiles7, case
    assert seen[1][3]["dup"] > 0 and seen[2][3]["counted"] < seen[0][3]["counted"]
    MC.assert_not_vacuous(seen, record_filters=("unmapped", "secondary", "dup", "mapq", "improper"), also=("counted", "reverse", "S", "I", "D"))      # (inferred strands: (1) and (3))


# ------------------------------------------------------------------ (3) a stream
def test_stream_sums_equal_the_model_and_the_process_sums(data):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device, default_opt
    d, refs = data
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
    L.bsx_stream_set_qc_meth.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_qc_meth_tables.argtypes = [C.c_void_p, C.c_void_p]
    L.bsx_process_qc_meth_tables.argtypes = [C.c_void_p]
    n_pairs, chunks, got = 2000, [], []
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
                assert L.bsx_stream_set_qc_meth(s, 1) == -2                   # needs set_qc before it
                L_.check(L.bsx_stream_set_qc(s, 1), "set_qc")
                L_.check(L.bsx_stream_set_qc_meth(s, 1), "set_qc_meth")
            else:
                L_.check(L.bsx_process_set_qc(1), "process_set_qc")
                L_.check(L.bsx_process_set_qc_meth(1), "process_set_qc_meth")
            for k in range(2):
                L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, ch[k]), "push")
            L_.check(L.bsx_stream_flush(s), "flush")
            t = L_.MethTables()
            L_.check(L.bsx_stream_qc_meth_tables(s, C.byref(t)) if how == "stream" else L.bsx_process_qc_meth_tables(C.byref(t)), "tables")
            got.append((list(t.k), list(t.s)))
            L.bsx_stream_close(s)
            if how == "process":
                L.bsx_process_set_qc_meth(0)
                L.bsx_process_set_qc(0)
        text = ""
        for k in range(2):
            rd = C.cast(chunks[k], C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        _, K, S, unc, seen = M.process(text, refs)
        assert seen["counted"] > 1000 and min(K[:4]) >= 20
        assert got[0] == (K, S) and got[1] == (K, S), (got, K, S)
    finally:
        L.bsx_process_set_qc_meth(0)
        L.bsx_process_set_qc(0)
        for ch in chunks:
            L.bsx_sim_free_reads(ch, 2 * n_pairs)
        dev.close()
        idx.close()
