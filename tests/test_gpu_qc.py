"""-m gpu: the BISCUITqc tables on the device.  (1) bsx_qc_batch on jobs built from the HIP command line's own alignments, every counter against
tests/qc_model.py over the same records, in one batch and in several; (2) the HIP command line with --qc against the model and the CPU checker
(whose columns are walked on the host), SAM unchanged; (3) with a bsconv filter; (4) two product processes over sockets; (5) stream totals."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import simdata
import e2e_cases as E
import bsconv_cases as B
import qc_cases as QC
import qc_model as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(ROOT, "oracle", "oracle_align")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("qc_gpu"))
    contigs = B.make_data(d, genome_bp=300000, n_pairs=3000, n_long=150)
    return d, contigs, Q.read_fasta(d + "/g.fa")


def _jobs_of(sam, reads, offs_of, contig_off):
    """the mapped records of a SAM as bsx_qc_job_t's, flags as sam.c sets them -> (jobs, pool)"""
    from biscuit_amd import _lib as L_
    jobs, pool = [], []
    for l in sam.split("\n"):
        if not l or l[0] == "@":
            continue
        f = l.split("\t")
        flag, mapq = int(f[1]), int(f[4])
        if flag & 4:
            continue
        key = (f[0], flag & 0xc0)
        yd = [x for x in f[11:] if x.startswith("YD:A:")][0][5:]
        fl = (L_.QC_REVERSE if flag & 0x10 else 0) | (L_.QC_READ2 if flag & 0x80 else 0) | Q.TAGS[yd] << 2 | L_.QC_STRAND
        if mapq >= 40 and not flag & 0x100:
            fl |= L_.QC_CINREAD
            if (flag & 0x3) == 0x3 and not flag & 0x600:
                fl |= L_.QC_BSCONV
        ops = Q.parse_cigar(f[5])
        jobs.append((contig_off[f[2]] + int(f[3]) - 1, offs_of[key], 0, len(reads[key]), len(pool), len(ops), fl))
        pool += [n << 4 | "MIDSH".index(op) for n, op in ops]
    return np.array(jobs, dtype=np.dtype(L_.QcJob)), np.array(pool, dtype=np.uint32)


def test_kernel_counters_equal_the_model_in_one_batch_and_in_several(data):
    from biscuit_amd.api import Index, Device
    d, contigs, refs = data
    contig_off, at = {}, 0
    for name, g in contigs:
        contig_off[name] = at
        at += len(g)
    idx = Index(d + "/g")
    dev = Device(0)
    dev.upload_index(idx)
    counters, n_jobs = [], 0
    try:
        assert at == idx.l_pac
        for case in QC.CASES:
            args = dict(E.CASES_CORE)[case]
            sam, _ = B.run(HIP, args, d)
            reads, paired = QC.reads_of(d, args)
            keys = sorted(reads)
            buf, offs = simdata.read_buffer([np.array([CODE.get(c, 4) for c in reads[k].upper()], np.uint8) for k in keys])
            dev.set_reads(buf)
            jobs, pool = _jobs_of(sam, reads, {k: int(offs[i]) for i, k in enumerate(keys)}, contig_off)
            c = Q.process(sam, refs, reads)
            want = np.array(c.flat(), np.int64)
            dev.qc_read(reset=True)
            dev.qc_batch(jobs, pool)
            one = np.concatenate([x.ravel() for x in dev.qc_read(reset=True)])
            bad = np.flatnonzero(one != want)
            assert bad.size == 0, (case, bad[:10].tolist(), one[bad[:10]].tolist(), want[bad[:10]].tolist())
            cuts = [0, 1, len(jobs) // 3, len(jobs) // 3 + 7, len(jobs)]
            for a, b in zip(cuts, cuts[1:]):                # (the pool is shared: cig_off stays valid)
                dev.qc_batch(jobs[a:b], pool)
            several = np.concatenate([x.ravel() for x in dev.qc_read(reset=True)])
            assert (several == one).all(), case
            assert (np.concatenate([x.ravel() for x in dev.qc_read()]) == 0).all()      # reset zeroed the table
            counters.append(c)
            n_jobs += len(jobs)
        assert n_jobs >= 2000
        QC.assert_not_vacuous(counters)
    finally:
        dev.close()
        idx.close()


def test_hip_command_line_files_equal_model_and_cpu_checker(data):
    d, contigs, refs = data
    counters = []
    for case in QC.CASES:
        args = dict(E.CASES_CORE)[case]
        plain, _ = B.run(HIP, args, d)
        sam, files = QC.run_qc(HIP, [], args, d, d + "/hip_" + case)
        assert sam == plain, case
        reads, paired = QC.reads_of(d, args)
        counters.append(QC.check_files(files, sam, refs, reads, paired, case))
        csam, cfiles = QC.run_qc(CPU, [], args, d, d + "/cpu_" + case)
        E.assert_same_sam(sam.encode(), csam.encode(), case)
        assert files == cfiles and len(files) == (7 if paired else 6), case
    QC.assert_not_vacuous(counters)


def test_with_a_bsconv_filter_the_tables_are_the_models_over_the_filtered_sam(data):
    d, contigs, refs = data
    args = dict(E.CASES_CORE)["pe150_b0"]
    sam, files = QC.run_qc(HIP, ["--bsconv-max-cph", "3"], args, d, d + "/hip_flt")
    only, _ = B.run(HIP, ["--bsconv-max-cph", "3"] + args, d)
    plain, _ = B.run(HIP, args, d)
    assert sam == only and 0 < sam.count("\n") < plain.count("\n")
    reads, paired = QC.reads_of(d, args)
    c = QC.check_files(files, sam, refs, reads, paired, "filtered")
    assert c.all_tot == sum(1 for l in sam.split("\n") if l and l[0] != "@") and sum(c.conv) > 1000


def test_two_product_processes_write_the_one_process_files(data):
    d, contigs, refs = data
    args = ["-@", "2", "g", "b1.fq", "b2.fq"]
    env = {"BSX_CHUNK_SIZE": "60000", "BSX_DEVICE": "0"}
    one, files1 = QC.run_qc(HIP, [], args, d, d + "/one", env=env)
    base = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID", "BSX_TUNE"):
        base.pop(k, None)
    procs = []
    for r in range(2):
        e = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=d + "/rdvq2", BSX_TUNE="gather_transport=socket", BSX_OUT=d + "/twoq.sam")
        procs.append(subprocess.Popen([HIP, "--qc", d + "/two"] + args, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = [p.communicate(timeout=1200) for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][1].decode()[-3000:])
    assert E.strip_pg(open(d + "/twoq.sam", "rb").read()).decode() == one
    assert QC.read_files(d + "/two") == files1 and len(files1) == 7


def test_stream_totals_equal_the_model(data):
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
    L.bsx_stream_set_qc.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_qc_totals.argtypes = [C.c_void_p, C.c_void_p]
    n_pairs, chunks = 3000, []
    try:
        for k in range(3):
            p = C.c_void_p()
            L_.check(L.bsx_sim_pairs(idx.h, n_pairs, 150, 700 + k, 200, 500, 0.01, 0.2, C.byref(p)), "sim_pairs")
            chunks.append(p)
        s = C.c_void_p()
        L_.check(L.bsx_stream_open(dev.h, C.byref(opt), idx.h, None, C.byref(s)), "stream_open")
        L_.check(L.bsx_stream_set_qc(s, 1), "set_qc")
        for k in range(3):
            L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, chunks[k]), "push")
        L_.check(L.bsx_stream_flush(s), "flush")
        t = L_.QcTotals()
        L_.check(L.bsx_stream_qc_totals(s, C.byref(t)), "totals")
        L.bsx_stream_close(s)
        text = ""
        for k in range(3):
            rd = C.cast(chunks[k], C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        c = Q.process(text, refs)
        assert list(t.dev.readpos) + list(t.dev.conv) + list(t.dev.confusion) == c.flat() and sum(c.conv) > 10000
        assert list(t.mapq) == c.mapq and list(t.isize) == c.isize and list(t.strandcnt) == c.strandcnt
        assert (t.n_isize, t.all_tot, t.all_dup, t.q40_tot, t.q40_dup) == (c.n_isize, c.all_tot, 0, c.q40_tot, 0) and c.all_tot >= 6 * n_pairs
    finally:
        for ch in chunks:
            L.bsx_sim_free_reads(ch, 2 * n_pairs)
        dev.close()
        idx.close()
