"""-m gpu: the HIP kernels against outputs recorded from the REAL reference functions
(tests/golden/ref_vectors.npz, made by tests/golden/make_vectors.py from /root/reference/lib/aln; ref_vectors_long.npz, made by
tests/golden/make_vectors_long.py: the same three DP functions at the shapes where the dispatch in shim.hip changes kernel).
The DP kernels read their target from the HBM-resident packed reference, so the recorded target
sequences are concatenated into a scratch genome and indexed with the repo's builder."""
import ctypes as C
import os
import numpy as np
import pytest
import simdata
from biscuit_amd.api import Index, Device, default_opt, EXT_DT, SW_DT, GLB_DT, SEED_DT, SA_DT
from biscuit_amd import _lib as B

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def V():
    return np.load(os.path.join(HERE, "golden", "ref_vectors.npz"))


# the two recorded files: name -> (file, key prefix of its DP families)
FILES = {"short": ("ref_vectors.npz", ""), "long": ("ref_vectors_long.npz", "l")}


@pytest.fixture(scope="module")
def VS():
    return {k: np.load(os.path.join(HERE, "golden", f)) for k, (f, _) in FILES.items()}


# What each test must have compared, as the generators print it (make_vectors_long.py prints the tables of both files).  Equalities: a vector
# that drops out of a comparison fails its test.
# Extension, by form.  wavefront_per_job declines nothing; window (ext_dp_win) only a band of more than 256 columns (2 w + 1 > 256); the two
# k_ext4 forms only queries of more than 255 bases.  (Of ref_vectors.npz, 40 vectors have an N in the target or no target and cannot be laid
# into the scratch genome.)
EXT_COMPARED = {("short", "wavefront_per_job"): 360, ("short", "window"): 280, ("short", "quarter_wave_per_job"): 321, ("short", "lane_per_job"): 321,
                ("long", "wavefront_per_job"): 403, ("long", "window"): 282, ("long", "quarter_wave_per_job"): 12, ("long", "lane_per_job"): 12}
# wavefront_per_job by (class of the query length, class of the band's columns) -- the table of lane_extend_batch (shim.hip:1470: QCAP = {256, 1024,
# 16384, any}, BAND = {256, 512, 2048}, band = min(qlen, 2 w + 1)); a job runs in the larger of its two classes: k_extend<4>, <8>, <32>, and <32> with
# its rows in HBM (launch_extend_hbm)
EXT_QCAP, EXT_BAND = (256, 1024, 16384), (256, 512)
EXT_CLASSES = {"short": {(0, 0): 321, (1, 0): 33, (1, 1): 6},
               "long": {(0, 0): 15, (1, 0): 241, (1, 1): 104, (1, 2): 2, (2, 0): 23, (2, 1): 11, (2, 2): 4, (3, 0): 3}}
# Local alignment, by kernel class of lane_sw_batch (shim.hip:1532-1536): byte mode with up to 256 padded columns -> k_swl; the others by the
# query padded to a multiple of 8: up to 256, 1024, 3072 columns (4, 16, 48 register slots per lane)
SW_CLASSES = {"short": {"swl": 216, 256: 128, 1024: 56}, "long": {"swl": 30, 256: 2, 1024: 43, 3072: 43}}
# Global alignment, by class of lane_global_batch (shim.hip:1716: QCAP = {256, 1024, 16384, any}, BAND = {256, 1024, 2048}; the last one is
# launch_global_hbm), and the CIGARs compared.  Every vector of the long file is used; of the short one, those whose recorded band
# bis_bwa_gen_cigar2 would not narrow
GL_QCAP, GL_BAND = (256, 1024, 16384), (256, 1024)
GL_CLASSES = {"short": {0: 142, 1: 21}, "long": {0: 2, 1: 65, 2: 45, 3: 2}}
GL_CIGARS = {"short": 127, "long": 100}


def _genome_of_targets(tmp, name, tgt, toff):
    """concatenate the N-free targets into one contig; returns (Index, start offset per case or -1)"""
    start = np.full(len(toff) - 1, -1, np.int64)
    parts, at = [], 0
    for i in range(len(toff) - 1):
        t = tgt[toff[i]:toff[i + 1]]
        if len(t) == 0 or (t > 3).any():
            continue
        start[i] = at
        parts.append(t)
        at += len(t)
    g = np.concatenate(parts)
    fa = os.path.join(tmp, name + ".fa")
    simdata.write_genome(fa, [("t", g)])
    return Index.build(fa, os.path.join(tmp, name)), start


def _opt(a, b, gp, zdrop=100):
    o = default_opt()
    o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins, o.zdrop = a, b, gp[0], gp[1], gp[2], gp[3], zdrop
    B.lib().bsx_opt_fill_matrices(C.byref(o))
    return o


FORMS = ["wavefront_per_job", "window", "quarter_wave_per_job", "lane_per_job"]


def _extend_vs_recorded(VS, tmp_path, which_file, form, tune):
    """ksw_extend2 vectors recorded from the reference against k_extend (a wavefront per job, rows in LDS or, beyond 16 384 bases, in HBM), against
    ext_dp_win (the register window that follows the band: what a kilobase read's extensions go through), and against k_ext4 / k_extl
    (k_ext4.hip: a row of 16 lanes per job, the form the regions path runs; it holds queries up to 255 bases)"""
    V, p = VS[which_file], FILES[which_file][1]
    quarter = form in ("quarter_wave_per_job", "lane_per_job")
    if form != "wavefront_per_job":      # "2": then k_extl (a lane per job) over the same jobs, its answers replacing k_ext4's
        tune("ext4", {"window": "3", "quarter_wave_per_job": "1", "lane_per_job": "2"}[form])
    idx, start = _genome_of_targets(str(tmp_path), "ext", V[p + "ext_t"], V[p + "ext_toff"])
    dev = Device(0); dev.upload_index(idx)
    qo, to = V[p + "ext_qoff"], V[p + "ext_toff"]
    dev.set_reads(V[p + "ext_q"])
    par = V[p + "ext_par"]
    groups, classes = {}, {}
    for i in range(len(par)):
        if start[i] < 0 or (V[p + "ext_q"][qo[i]:qo[i + 1]] > 4).any():
            continue
        a, b, which, od, ed, oi, ei, w, eb, zd, h0 = [int(x) for x in par[i]]
        qlen = int(qo[i + 1] - qo[i])
        if quarter and qlen > 255:
            continue
        if form == "window" and 2 * w + 1 > 256:
            continue
        groups.setdefault((a, b, od, ed, oi, ei, zd), []).append(i)
        band = min(qlen, 2 * w + 1)
        k = (sum(qlen > x for x in EXT_QCAP), sum(band > x for x in EXT_BAND))
        classes[k] = classes.get(k, 0) + 1
    n = 0
    for key, ids in groups.items():
        dev.set_opt(_opt(key[0], key[1], key[2:6], key[6]))
        jobs = np.zeros(len(ids), dtype=EXT_DT)
        for k, i in enumerate(ids):
            a, b, which, od, ed, oi, ei, w, eb, zd, h0 = [int(x) for x in par[i]]
            jobs[k] = (start[i], qo[i], qo[i + 1] - qo[i], to[i + 1] - to[i], h0, w, eb, 1, 1, 1 if which == 1 else 0, 0)
        res = dev.extend(jobs)
        got = np.stack([res[f] for f in ("score", "qle", "tle", "gtle", "gscore", "max_off")], 1)
        bad = np.nonzero((got != V[p + "ext_out"][ids]).any(1))[0]
        assert len(bad) == 0, (key, [ids[x] for x in bad[:3]], jobs[bad[:3]], got[bad[:3]], V[p + "ext_out"][ids][bad[:3]])
        n += len(ids)
    assert n == EXT_COMPARED[which_file, form], n
    if which_file == "short" and form != "window":      # the floors these forms had before the counts; only 280 vectors have a band the window takes
        assert n > (200 if quarter else 300)
    if form == "wavefront_per_job":
        assert classes == EXT_CLASSES[which_file], classes
        if which_file == "long":      # every kernel class, and each by either way into it
            assert all(any(max(q, b) == c for (q, b), m in classes.items() if m > 0) for c in range(4))
            assert {(1, 0), (1, 1), (1, 2), (2, 0), (2, 2), (3, 0)} <= set(classes)
    dev.close()


@pytest.mark.parametrize("form", FORMS)
def test_extend_kernel_vs_reference_vectors(VS, tmp_path, form, tune):
    _extend_vs_recorded(VS, tmp_path, "short", form, tune)


@pytest.mark.parametrize("form", FORMS)
def test_extend_kernel_vs_long_reference_vectors(VS, tmp_path, form, tune):
    """the same over ref_vectors_long.npz: queries of 159..17 500 bases across every class edge, bands of 11..1023 columns"""
    _extend_vs_recorded(VS, tmp_path, "long", form, tune)


def _sw_vs_recorded(VS, tmp_path, which_file):
    """ksw_align2 vectors against k_swl (byte mode, four jobs to a wavefront) and the three register-slot classes of k_sw; the long file holds
    byte-mode jobs in which the reference's byte kernel reaches 255 -- the kernel has to answer what the reference answers then"""
    V, p = VS[which_file], FILES[which_file][1]
    idx, start = _genome_of_targets(str(tmp_path), "sw", V[p + "sw_t"], V[p + "sw_toff"])
    dev = Device(0); dev.upload_index(idx)
    qo = V[p + "sw_qoff"]
    dev.set_reads(V[p + "sw_q"])
    par = V[p + "sw_par"]
    groups, classes = {}, {}
    for i in range(len(par)):
        if start[i] < 0:
            continue
        a, b, which, od, ed, oi, ei, xtra = [int(x) for x in par[i]]
        groups.setdefault((a, b, od, ed, oi, ei), []).append(i)
        pad = 16 if xtra & 0x10000 else 8
        Q = (int(qo[i + 1] - qo[i]) + pad - 1) // pad * pad
        c = "swl" if pad == 16 and Q <= 256 else 256 if Q <= 256 else 1024 if Q <= 1024 else 3072
        classes[c] = classes.get(c, 0) + 1
    n = n_sat = 0
    for key, ids in groups.items():
        dev.set_opt(_opt(key[0], key[1], key[2:6]))
        jobs = np.zeros(len(ids), dtype=SW_DT)
        for k, i in enumerate(ids):
            a, b, which, od, ed, oi, ei, xtra = [int(x) for x in par[i]]
            jobs[k] = (start[i], qo[i], qo[i + 1] - qo[i], V[p + "sw_toff"][i + 1] - V[p + "sw_toff"][i], xtra, 1, 1, 0, 1 if which == 1 else 0)
        res = dev.sw(jobs)
        got = np.stack([res[f] for f in ("score", "te", "qe", "score2", "te2", "tb", "qb")], 1)
        bad = np.nonzero((got != V[p + "sw_out"][ids]).any(1))[0]
        assert len(bad) == 0, (key, [ids[x] for x in bad[:3]], got[bad[:3]], V[p + "sw_out"][ids][bad[:3]])
        n += len(ids)
        n_sat += int(((V[p + "sw_out"][ids][:, 0] == 255) & ((par[ids][:, 7] & 0x10000) != 0)).sum())
    assert classes == SW_CLASSES[which_file] and n == sum(SW_CLASSES[which_file].values()), (n, classes)
    if which_file == "short":
        assert n > 300
    else:
        assert n_sat == 10, n_sat
    dev.close()


def test_sw_kernel_vs_reference_vectors(VS, tmp_path):
    _sw_vs_recorded(VS, tmp_path, "short")


def test_sw_kernel_vs_long_reference_vectors(VS, tmp_path):
    """the same over ref_vectors_long.npz: 257..3072 columns in 16-bit mode, the stripe-count edges of k_swl, byte mode that saturates"""
    _sw_vs_recorded(VS, tmp_path, "long")


def _global_vs_recorded(VS, tmp_path, which_file):
    """k_global (K6) against ksw_global2 outputs recorded from the reference (gl_score / gl_cigar): the kernel folds the band set-up of
    bis_bwa_gen_cigar2 in (bwa.c:325-333: w = max(min((max_gap + |d| + 1) >> 1, w_), |d| + 3)), so the vectors used are the ones whose
    recorded band is the band that rule gives when it is passed as w_ (the long file was recorded under that rule: all of its vectors)."""
    V, p = VS[which_file], FILES[which_file][1]
    idx, start = _genome_of_targets(str(tmp_path), "gl", V[p + "gl_t"], V[p + "gl_toff"])
    dev = Device(0); dev.upload_index(idx)
    qo, to, co = V[p + "gl_qoff"], V[p + "gl_toff"], V[p + "gl_coff"]
    dev.set_reads(V[p + "gl_q"])
    par = V[p + "gl_par"]
    groups, classes = {}, {}
    for i in range(len(par)):
        if start[i] < 0 or (V[p + "gl_q"][qo[i]:qo[i + 1]] > 3).any():
            continue
        a, b, which, od, ed, oi, ei, w, wc = [int(x) for x in par[i]]
        lq, lt = int(qo[i + 1] - qo[i]), int(to[i + 1] - to[i])
        max_ins = int(float(((lq + 1) >> 1) * a - oi) / ei + 1.)
        max_del = int(float(((lq + 1) >> 1) * a - od) / ed + 1.)
        max_gap = max(max_ins, max_del, 1)
        if w > (max_gap + abs(lt - lq) + 1) >> 1:
            continue    # bis_bwa_gen_cigar2 would narrow this band
        groups.setdefault((a, b, od, ed, oi, ei), []).append(i)
        band = min(lq, 2 * w + 1)
        c = max(sum(lq > x for x in GL_QCAP), sum(band > x for x in GL_BAND))
        classes[c] = classes.get(c, 0) + 1
    n = n_cig = 0
    for key, ids in groups.items():
        dev.set_opt(_opt(key[0], key[1], key[2:6]))
        jobs = np.zeros(len(ids), dtype=GLB_DT)
        cig_off = 0
        for k, i in enumerate(ids):
            a, b, which, od, ed, oi, ei, w, wc = [int(x) for x in par[i]]
            cap = int(co[i + 1] - co[i]) + 8
            jobs[k] = (start[i], qo[i], qo[i + 1] - qo[i], to[i + 1] - to[i], w, 1 << 20, 0, 1, cig_off, cap, 1, 1, 1 if which == 1 else 0, wc)
            cig_off += cap
        res, pool = dev.global_(jobs, cig_off)
        for k, i in enumerate(ids):
            assert int(res[k]["score"]) == int(V[p + "gl_score"][i]), (key, i, res[k], V[p + "gl_score"][i])
            if int(par[i][8]):
                nc = int(res[k]["n_cigar"])
                off = int(jobs[k]["cigar_off"])
                assert list(pool[off:off + nc]) == list(V[p + "gl_cigar"][co[i]:co[i + 1]]), (key, i)
                n_cig += 1
        n += len(ids)
    assert classes == GL_CLASSES[which_file] and n == sum(GL_CLASSES[which_file].values()) and n_cig == GL_CIGARS[which_file], (n, n_cig, classes)
    if which_file == "short":
        assert n > 120 and n_cig > 80, (n, n_cig)
    else:
        assert n == len(par)      # no vector of the long file is left out
    dev.close()


def test_global_kernel_vs_reference_vectors(VS, tmp_path):
    _global_vs_recorded(VS, tmp_path, "short")


def test_global_kernel_vs_long_reference_vectors(VS, tmp_path):
    """the same over ref_vectors_long.npz: targets of 255..17 500 bases, bands of up to 2001 columns, CIGARs of dozens of operations from HBM rows"""
    _global_vs_recorded(VS, tmp_path, "long")


def test_fm_kernels_vs_reference_vectors(V, tmp_path):
    """K1-K3 on the committed 24 kb genome against vectors recorded from the real reference: the seeding kernel's interval
    lists == the lists the reference's bwt_smem1a / bwt_seed_strategy1 give when driven as mem_collect_intv drives them
    (memchain.c:50-106; tests/golden/make_vectors.py), interval for interval; every SMEM recorded for a single bwt_smem1a
    call with min_intv 1 is among them; bwt_sa agrees."""
    idx = Index.build(os.path.join(HERE, "golden", "g24k.fa"), str(tmp_path / "g"))
    dev = Device(0); dev.upload_index(idx)
    ro = V["fm_roff"]
    reads = [V["fm_reads"][ro[i]:ro[i + 1]] for i in range(len(ro) - 1)]
    buf, offs = simdata.read_buffer(reads)
    tasks = np.zeros(len(reads), dtype=SEED_DT)
    for i, r in enumerate(reads):
        tasks[i] = (offs[i], len(r), int(V["fm_par"][i][0]))
    opt = default_opt()
    dev.set_opt(opt)
    dev.set_reads(buf)
    iv, off = dev.seed(opt, tasks)
    co = V["fm_coff"] // 4
    assert (np.asarray(off) == co).all()
    assert (iv.reshape(-1) == V["fm_collect"]).all()
    assert int(co[-1]) > 1000
    so, n_in = V["fm_soff"], 0
    for i, par in enumerate(V["fm_par"]):
        if int(par[2]) != 1:      # min_intv of the recorded call: pass 1 runs with 1
            continue
        mine = {tuple(int(v) for v in row) for row in iv[off[i]:off[i + 1]]}
        sm = V["fm_smem"][so[i]:so[i + 1]].reshape(-1, 4)
        for row in sm:
            if (int(row[3]) & 0xffffffff) - (int(row[3]) >> 32) >= 19:
                assert tuple(int(v) for v in row) in mine, (i, row)
                n_in += 1
    assert n_in > 100
    ks = V["fm_k"][V["fm_k"] >= 1]
    for p in (0, 1):
        jobs = np.zeros(len(ks), dtype=SA_DT)
        jobs["k"] = ks; jobs["parent"] = p
        assert (dev.sa(jobs) == V["fm_sa_%d" % p]).all()
    dev.close()
