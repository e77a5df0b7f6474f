"""-m gpu: conversion by context on the device.  (a) bsx_global_batch_tags_ctx job by job against tests/bsconv_model.py applied to the job's
forward view; (b) the HIP command line with --bsconv and with a filter set against the CPU checker's (whose counts come from the host walk)
and the model, and bsx_stream_bsconv_totals against the model's sums; (c) two product processes over sockets against one."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import simdata
import e2e_cases as E
import bsconv_cases as B
import bsconv_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(ROOT, "oracle", "oracle_align")
LET = "ACGTN"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bsconv_gpu"))
    contigs = B.make_data(d, genome_bp=300000, n_pairs=3000, n_long=150)
    return d, contigs, M.read_fasta(d + "/g.fa")


def _cigar_ops(pool, off, n):
    return [(int(pool[off + k]) >> 4, "MIDSH"[int(pool[off + k]) & 0xf]) for k in range(n)]


def test_kernel_counts_equal_the_model_job_by_job(data):
    from biscuit_amd.api import Index, Device, default_opt, GLB_DT
    d, contigs, refs = data
    idx = Index(d + "/g")
    dev = Device(0)
    dev.upload_index(idx)
    try:
        l_pac = idx.l_pac
        offs_c = np.concatenate([[0], np.cumsum([len(g) for _, g in contigs])])
        assert offs_c[-1] == l_pac
        r = np.random.default_rng(77)
        seqs, meta = [], []
        while len(seqs) < 2400:
            ci = int(r.integers(0, len(contigs)))
            g = contigs[ci][1]
            k = len(seqs)
            qlen = int(r.choice([30, 60, 100, 150, 150, 250, 400, 700, 1000]) if k % 40 else r.integers(1100, 1400))
            L = qlen + int(r.integers(-3, 4))
            isn = np.flatnonzero(g == 4)
            how = k % 8
            if how == 0:
                s = 0                                             # touches the first base of the contig
            elif how == 1:
                s = len(g) - L                                    # ... the last
            elif how in (2, 3) and len(isn):                      # next to, across or inside an N run
                s = int(isn[int(r.integers(0, len(isn)))]) + int(r.integers(-L, 3))
            else:
                s = int(r.integers(0, len(g) - L))
            s = max(0, min(s, len(g) - L))
            f = g[s:s + L].copy()
            back = bool(r.random() < 0.5)                         # the read comes from the reverse strand
            src = simdata.revcomp(f) if back else f
            read = simdata.mutate(simdata.bisulfite(src, r, cpg_ret=0.6, other_ret=0.05), r, 0.02, 0.01 if k % 3 else 0.0)
            if len(read) < 20:
                continue
            if r.random() < 0.3:                                  # G>A reads as well (the other bisulfite strand's signal)
                read = simdata.revcomp(simdata.mutate(simdata.bisulfite(simdata.revcomp(src), r, cpg_ret=0.6, other_ret=0.05), r, 0.02, 0.0))
            seqs.append(read.astype(np.uint8))
            meta.append((ci, s, L, back))
        # three reads of 16 400 - 17 000 bases behind them (a stream of their own, so that the jobs above stay what they were): the DP rows of
        # these live in HBM (launch_global_hbm, its ctx form).  Both strands, one of them walked against the forward direction
        LONG = [(False, False), (True, False), (False, True)]      # (from the reverse strand, reversed view)
        n_short = len(seqs)
        r2 = np.random.default_rng(7717)
        for back, _ in LONG:
            while True:
                ci = int(r2.integers(0, len(contigs)))
                g = contigs[ci][1]
                L = int(r2.integers(16400, 17001))
                s = int(r2.integers(0, len(g) - L))
                if (g[s:s + L] == 4).sum() < 30:                   # short N runs only
                    break
            f = g[s:s + L].copy()
            src = simdata.revcomp(f) if back else f
            read = simdata.mutate(simdata.bisulfite(src, r2, cpg_ret=0.6, other_ret=0.05), r2, 0.02, 0.002)
            seqs.append(read.astype(np.uint8))
            meta.append((ci, s, L, back))
        buf, offs = simdata.read_buffer(seqs)
        opt = default_opt()
        dev.set_opt(opt)
        dev.set_reads(buf)
        jobs = np.zeros(len(seqs), dtype=GLB_DT)
        at = 0
        for k, (ci, s, L, back) in enumerate(meta):
            q = len(seqs[k])
            fs = int(offs_c[ci]) + s                              # forward coordinate of the window's first base
            flip = bool(r.random() < 0.25)                        # the view walks the window against the forward direction
            if k >= n_short:
                flip = LONG[k - n_short][1]
            if not back:
                tpos, tdir, qoff, qdir = (fs, 1, offs[k], 1) if not flip else (fs + L - 1, -1, offs[k] + q - 1, -1)
            else:                                                 # the reverse strand's coordinates: [2 l_pac - (fs + L), 2 l_pac - fs)
                rb, re = 2 * l_pac - (fs + L), 2 * l_pac - fs
                tpos, tdir, qoff, qdir = (re - 1, -1, offs[k] + q - 1, -1) if not flip else (rb, 1, offs[k], 1)
            cap = 64 + q // 8
            jobs[k] = (tpos, qoff, q, L, 60 if k < n_short else max(100, abs(L - q) + 3), 400, 0, 1, at, cap, qdir, tdir, int(r.integers(0, 2)), 1)
            at += cap
        res, pool, tags, md, ctx = dev.global_tags_ctx(jobs, at)
        res2, pool2, tags2, md2 = dev.global_tags(jobs, at)
        assert (res == res2).all() and (pool == pool2).all() and md == md2
        for name in ("NM", "ZC", "ZR", "l_md", "bss_u"):
            assert (tags[name] == tags2[name]).all(), name
        n_checked = n_special = n_onelane = n_indel = n_hbm = 0
        seen = np.zeros((2, 5, 2), np.int64)
        for k, (ci, s, L, back) in enumerate(meta):
            n_c = int(res[k]["n_cigar"])
            assert n_c > 0, (k, n_c)
            ops = _cigar_ops(pool, int(jobs[k]["cigar_off"]), n_c)
            q = len(seqs[k])
            view = seqs[k] if jobs[k]["qdir"] > 0 else seqs[k][::-1]
            comp = int(jobs[k]["tpos"]) >= l_pac
            dirf = -int(jobs[k]["tdir"]) if comp else int(jobs[k]["tdir"])
            fwd = np.where(view < 4, 3 - view, 4) if comp else view
            if dirf < 0:
                ops, fwd = ops[::-1], fwd[::-1]
            cigar = "".join("%d%s" % o for o in ops)
            want = M.walk(refs[contigs[ci][0]], s + 1, cigar, "".join(LET[int(b)] for b in fwd))
            w = np.array([[want[st][c] for c in LET] for st in (0, 1)])
            assert (ctx[k].astype(np.int64) == w).all(), (k, meta[k], jobs[k], cigar, ctx[k].tolist(), w.tolist())
            n_checked += 1
            seen += w
            g = contigs[ci][1]
            n_special += int(s == 0 or s + L == len(g) or (g[max(0, s - 1):s + L + 1] == 4).any())
            n_onelane += int(q > 1024)
            n_hbm += int(q > 16384)
            n_indel += int(any(o[1] in "ID" for o in ops))
        assert n_checked >= 2000 and n_special > 300 and n_onelane >= 20
        assert n_hbm == 3 and n_checked == n_short + 3 and all(16400 <= len(x) <= 17000 for x in seqs[n_short:])
        long_jobs = jobs[n_short:]
        assert {int(j["tpos"]) >= l_pac for j in long_jobs} == {False, True} and (long_jobs["tdir"] < 0).any() and (long_jobs["tdir"] > 0).any()
        assert (seen[:, :4] > 50).all() and (seen[:, 4] > 0).all()      # every bucket of both strands is exercised, the N bucket too
        assert len({(int(j["qdir"]), int(j["tpos"]) >= l_pac) for j in jobs}) == 4      # both directions on both strands
        assert n_indel > 200
    finally:
        dev.close()
        idx.close()


@pytest.mark.parametrize("case", ["pe150_b0", "se150", "long_1kb"])
def test_hip_command_line_equals_cpu_checker_and_model(data, case):
    d, contigs, refs = data
    args = dict(E.CASES_CORE)[case]
    plain, _ = B.run(HIP, args, d)
    assert "ZN:Z" not in plain
    for opts, conf in ((["--bsconv"], M.Conf()), (B.FILTERS[1][0], M.Conf(**B.FILTERS[1][1])), (B.FILTERS[0][0] + ["--bsconv-show-filtered"], M.Conf(show_filtered=True, **B.FILTERS[0][1]))):
        got, err = B.run(HIP, opts + args, d)
        want, werr = B.run(CPU, opts + args, d)
        E.assert_same_sam(got.encode(), want.encode(), "%s %s: HIP against the CPU checker" % (case, " ".join(opts)))
        assert B.stderr_counts(err) == B.stderr_counts(werr)
        B.check_against_model(plain, got, err, refs, conf, "%s %s: HIP against the model" % (case, " ".join(opts)))


def test_stream_totals_equal_the_models_sums(data):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device, default_opt
    d, contigs, refs = data
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
    L.bsx_stream_set_bsconv.argtypes = [C.c_void_p, C.c_void_p]
    L.bsx_stream_bsconv_totals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bsx_bsconv_conf_init.argtypes = [C.c_void_p]
    n_pairs, chunks = 3000, []
    try:
        for k in range(3):
            p = C.c_void_p()
            L_.check(L.bsx_sim_pairs(idx.h, n_pairs, 150, 500 + k, 200, 500, 0.01, 0.2, C.byref(p)), "sim_pairs")
            chunks.append(p)
        conf = L_.BsconvConf()
        L.bsx_bsconv_conf_init(C.byref(conf))
        assert (conf.max_cph, conf.max_cpy, conf.max_cph_frac, conf.annotate) == (-1, -1, 1.0, 0)
        conf.max_cph = 2
        s = C.c_void_p()
        L_.check(L.bsx_stream_open(dev.h, C.byref(opt), idx.h, None, C.byref(s)), "stream_open")
        L_.check(L.bsx_stream_set_bsconv(s, C.byref(conf)), "set_bsconv")
        for k in range(3):
            L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, chunks[k]), "push")
        L_.check(L.bsx_stream_flush(s), "flush")
        tot, n, nf = (C.c_uint64 * 8)(), C.c_uint64(), C.c_uint64()
        L_.check(L.bsx_stream_bsconv_totals(s, tot, C.byref(n), C.byref(nf)), "totals")
        L.bsx_stream_close(s)
        text = ""
        for k in range(3):
            rd = C.cast(chunks[k], C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        # the model over what was written: every kept record carries ZN; its sums are the totals
        want = [0] * 8
        lines = [l for l in text.split("\n") if l]
        for l in lines:
            zn = l.split("\t")[-1]
            assert zn.startswith("ZN:Z:")
            f = l.split("\t")
            keep, mzn, retn, conv, filtered = M.record(f[:-1], refs, M.Conf(max_cph=2))
            assert keep and mzn == zn, l[:300]
            for i, c in enumerate("ACGT"):
                want[2 * i] += retn[c]
                want[2 * i + 1] += conv[c]
        assert list(tot) == want and n.value - nf.value == len(lines) and 0 < nf.value < n.value and n.value >= 6 * n_pairs
    finally:
        for c in chunks:
            L.bsx_sim_free_reads(c, 2 * n_pairs)
        dev.close()
        idx.close()


def test_two_product_processes_give_one_process_sam_and_totals(data):
    d, contigs, refs = data
    args = ["--bsconv-max-cph", "1", "-@", "2", "g", "b1.fq", "b2.fq"]
    env = {"BSX_CHUNK_SIZE": "60000", "BSX_DEVICE": "0"}
    one, err1 = B.run(HIP, args, d, env=env)
    base = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID", "BSX_TUNE"):
        base.pop(k, None)
    procs = []
    for r in range(2):
        e = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=d + "/rdv2", BSX_TUNE="gather_transport=socket", BSX_OUT=d + "/two.sam")
        procs.append(subprocess.Popen([HIP] + args, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = [p.communicate(timeout=1200) for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][1].decode()[-3000:])
    two = E.strip_pg(open(d + "/two.sam", "rb").read()).decode()
    assert two == one and one.count("ZN:Z:") > 1000
    assert B.stderr_counts(outs[0][1].decode()) == B.stderr_counts(err1) and b"[M::bsconv]" not in outs[1][1]
