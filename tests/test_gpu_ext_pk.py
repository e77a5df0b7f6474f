"""-m gpu: the packed 16-bit extension row (csrc/hip/ext_pk.hpp: two columns per lane) through its test seam -- bsx_extend_batch under the
setting ext4=4, a wavefront per job around ext_dp_pk, the form the region kernels' inline extensions take when the scoring options pass the
guard of ext_pk_bound.h -- against the recorded ksw_extend2 outputs, against the reference's own ksw_extend2 on jobs designed for the
layout's seams (tests/ext_pk_cases.py), and on either side of the guard.  (k_ext4 keeps its 32-bit rows -- k_ext4.hip says why -- so the
quarter-wave forms are what tests/test_gpu_golden.py already pins; there is no packed k_ext4 to run the vectors through.)"""
import ctypes as C
import os
import numpy as np
import pytest
import ext_pk_cases as X
import oracle_lib
import test_gpu_golden as G
from biscuit_amd.api import Device, EXT_DT
from biscuit_amd import _lib as B

pytestmark = pytest.mark.gpu
FIELDS = ("score", "qle", "tle", "gtle", "gscore", "max_off")


def _forms(reset=False):
    """[launches with packed rows, launches with 32-bit rows] since the last reset"""
    c = (C.c_uint64 * 2)()
    B.check(B.lib().bsx_ext_forms(c, int(reset)), "bsx_ext_forms")
    return list(c)


@pytest.mark.parametrize("which_file", ["short", "long"])
def test_packed_wave_form_vs_recorded_vectors(which_file, tmp_path, tune):
    """every ext_* vector with a query of at most 255 bases: all six result fields, and as many vectors as the quarter-wave forms compare under
    the same filter"""
    V, p = np.load(os.path.join(G.HERE, "golden", G.FILES[which_file][0])), G.FILES[which_file][1]
    tune("ext4", "4")
    idx, start = G._genome_of_targets(str(tmp_path), "ext", V[p + "ext_t"], V[p + "ext_toff"])
    dev = Device(0); dev.upload_index(idx)
    qo, to, par = V[p + "ext_qoff"], V[p + "ext_toff"], V[p + "ext_par"]
    dev.set_reads(V[p + "ext_q"])
    groups = {}
    for i in range(len(par)):
        if start[i] < 0 or (V[p + "ext_q"][qo[i]:qo[i + 1]] > 4).any() or qo[i + 1] - qo[i] > 255:
            continue
        a, b, which, od, ed, oi, ei, w, eb, zd, h0 = [int(x) for x in par[i]]
        groups.setdefault((a, b, od, ed, oi, ei, zd), []).append(i)
    n = 0
    _forms(reset=True)
    for key, ids in groups.items():
        dev.set_opt(G._opt(key[0], key[1], key[2:6], key[6]))
        jobs = np.zeros(len(ids), dtype=EXT_DT)
        for k, i in enumerate(ids):
            a, b, which, od, ed, oi, ei, w, eb, zd, h0 = [int(x) for x in par[i]]
            jobs[k] = (start[i], qo[i], qo[i + 1] - qo[i], to[i + 1] - to[i], h0, w, eb, 1, 1, 1 if which == 1 else 0, 0)
        res = dev.extend(jobs)
        got = np.stack([res[f] for f in FIELDS], 1)
        bad = np.nonzero((got != V[p + "ext_out"][ids]).any(1))[0]
        assert len(bad) == 0, (key, [ids[x] for x in bad[:3]], jobs[bad[:3]], got[bad[:3]], V[p + "ext_out"][ids][bad[:3]])
        n += len(ids)
    assert n == G.EXT_COMPARED[which_file, "quarter_wave_per_job"], n
    packed, plain = _forms()
    assert packed + plain == len(groups) and packed > 0, (packed, plain, len(groups))
    dev.close()


@pytest.fixture(scope="module")
def seam_jobs(tmp_path_factory):
    """the designed jobs laid into a scratch genome, and the reference's answers, computed once"""
    cases = X.jobs()
    tgt = np.concatenate([c[6] for c in cases]); toff = np.concatenate([[0], np.cumsum([len(c[6]) for c in cases])])
    qry = np.concatenate([c[5] for c in cases]); qoff = np.concatenate([[0], np.cumsum([len(c[5]) for c in cases])])
    idx, start = G._genome_of_targets(str(tmp_path_factory.mktemp("pk")), "pk", tgt, toff)
    assert (start >= 0).all()
    port = oracle_lib.Port(idx)
    have_ref = port.use_reference_kernels()
    port.set_reads(qry)
    by_scoring = {}
    for si in range(len(X.SCORINGS)):
        ids = [k for k, c in enumerate(cases) if c[0] == si]
        jobs = np.zeros(len(ids), dtype=EXT_DT)
        for j, k in enumerate(ids):
            _, parent, w, eb, h0, q, t = cases[k]
            jobs[j] = (start[k], qoff[k], len(q), len(t), h0, w, eb, 1, 1, parent, 0)
        a, b, gp, zd = X.SCORINGS[si]
        port.set_opt(X.opt_of(a, b, gp, zd))
        want = port.extend(jobs) if have_ref else None
        by_scoring[si] = (jobs, want)
    return idx, qry, by_scoring, have_ref


@pytest.mark.parametrize("si", range(len(X.SCORINGS)))
def test_packed_wave_form_at_the_seams_vs_reference(seam_jobs, si, tune):
    idx, qry, by_scoring, have_ref = seam_jobs
    if not have_ref:
        pytest.skip("oracle/_ref (the reference's own ksw_extend2) has not been built")
    jobs, want = by_scoring[si]
    a, b, gp, zd = X.SCORINGS[si]
    tune("ext4", "4")
    dev = Device(0); dev.upload_index(idx)
    dev.set_reads(qry); dev.set_opt(X.opt_of(a, b, gp, zd))
    _forms(reset=True)
    res = dev.extend(jobs)
    assert _forms() == [1, 0]      # the packed rows ran
    got = np.stack([res[f] for f in FIELDS], 1); ref = np.stack([want[f] for f in FIELDS], 1)
    bad = np.nonzero((got != ref).any(1))[0]
    assert len(bad) == 0, (len(bad), jobs[bad[:3]], got[bad[:3]], ref[bad[:3]])
    assert len(jobs) == len(X.QLENS) * 16
    tune("ext_pk", "0")            # the same jobs through the 32-bit rows of the same build
    res = dev.extend(jobs)
    assert _forms() == [1, 1]
    assert (np.stack([res[f] for f in FIELDS], 1) == ref).all()
    dev.close()


@pytest.mark.parametrize("e_ins,packed", [(28, True), (29, False)])
def test_guard_picks_the_form(seam_jobs, e_ins, packed, tune):
    """-A 100 and a job whose largest H can reach 25 500: with a gap extension of 28 the scan operand stays at 32 640, inside 16 bits, and the
    packed rows run; with 29 it could reach 32 895 and the 32-bit rows run.  Both equal the reference"""
    idx, qry, by_scoring, have_ref = seam_jobs
    if not have_ref:
        pytest.skip("oracle/_ref (the reference's own ksw_extend2) has not been built")
    jobs = by_scoring[0][0].copy()
    jobs = jobs[jobs["qlen"] <= 155]
    jobs["h0"] = np.minimum(jobs["h0"] * 100, 25500 - jobs["qlen"] * 100)
    k = int(np.nonzero(jobs["qlen"] == 129)[0][0])
    jobs["h0"][k] = 25500 - 129 * 100      # the job that sets the batch's bound: h0 + qlen * 100 = 25 500
    o = X.opt_of(100, 4, (6, 1, 6, e_ins), 100)
    port = oracle_lib.Port(idx); assert port.use_reference_kernels()
    port.set_reads(qry); port.set_opt(o)
    want = port.extend(jobs)
    tune("ext4", "4")
    dev = Device(0); dev.upload_index(idx)
    dev.set_reads(qry); dev.set_opt(o)
    _forms(reset=True)
    res = dev.extend(jobs)
    assert _forms() == ([1, 0] if packed else [0, 1])
    assert (np.stack([res[f] for f in FIELDS], 1) == np.stack([want[f] for f in FIELDS], 1)).all()
    dev.close()
