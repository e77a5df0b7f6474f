"""-m gpu: the seed filter's two alignments against scores recorded from the reference's own ksw_align2 (tests/golden/ref_vectors_ssw.npz), through
the test seam of bsx_sw_batch -- the setting sw_form.  ssw16: the very launch of k_swl16 (k_seedsw.hip: sixteen jobs to a wavefront in packed
16-bit) that launch_seedsw makes, over the jobs in the order given, so that tests/ssw_cases.py decides who shares a wavefront and a register;
ssw32: the 32-bit alignment k_seedsw_apply makes for a seed without room in the job list (sw_pass<2>, <3>, <4> by the padded query).  The e2e
tests see these scores only as `score >= threshold`; here every score is compared, and every family's count."""
import ctypes as C
import numpy as np
import pytest
import simdata
import ssw_cases as S
from biscuit_amd.api import Index, Device, SW_DT, SWRES_DT

pytestmark = pytest.mark.gpu
FORMS = ("ssw16", "ssw32")
BSX_E_ARG = -2


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    """the vectors, and their targets laid into a scratch genome twice (ssw_cases.layout): (V, [(Index, tpos)] * 2)"""
    V = S.Vectors()
    d = tmp_path_factory.mktemp("ssw")
    lay = []
    for which in (0, 1):
        g, tpos = S.layout(V, which)
        fa = str(d / ("l%d.fa" % which))
        simdata.write_genome(fa, [("t", g)])
        lay.append((Index.build(fa, str(d / ("l%d" % which))), tpos, len(g)))
    return V, lay


def _device(V, lay, which):
    dev = Device(0); dev.upload_index(lay[which][0])
    dev.set_reads(V.q)
    return dev


def _jobs(V, tpos, lst):
    jobs = np.zeros(len(lst), dtype=SW_DT)
    for k, i in enumerate(lst):
        jobs[k] = (0, 0, 0, 0, 0, 1, 1, 0, 0) if i == S.FILLER else (tpos[i], V.qoff[i], V.qlen[i], V.tlen[i], 0x80000, 1, 1, 0, V.use_ct[i])
    return jobs


def _sw(dev, jobs):
    """bsx_sw_batch with its return code: (rc, results)"""
    jobs = np.ascontiguousarray(jobs, dtype=SW_DT)
    res = np.zeros(len(jobs), dtype=SWRES_DT)
    rc = dev.f["sw_batch"](dev.ctx, C.c_int64(len(jobs)), jobs.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p))
    return rc, res


def _compare(V, dev, tpos, key, lst):
    rc, res = _sw(dev, _jobs(V, tpos, lst))
    assert rc == 0, (key, rc)
    want = np.array([V.score[i] if i != S.FILLER else 0 for i in lst])
    bad = np.nonzero(res["score"] != want)[0]
    assert len(bad) == 0, (key, len(bad), [(lst[k], V.fams[V.fam[lst[k]]] if lst[k] != S.FILLER else "filler", int(res["score"][k]), int(want[k])) for k in bad[:6]])
    for f in ("te", "qe", "score2", "te2", "tb", "qb"):
        assert (res[f] == -1).all()


@pytest.mark.parametrize("ordering", S.ORDERINGS)
@pytest.mark.parametrize("form", FORMS)
def test_scores_equal_recorded(ctx, tune, form, ordering):
    """every vector, one batch per option set, under both layouts; the nearest option sets beyond the guard are refused by ssw16 and answered
    by ssw32"""
    V, lay = ctx
    tune("sw_form", form)
    ends = set()      # the strand ends touched by windows that this form scored
    for which in (0, 1):
        dev = _device(V, lay, which)
        tpos, l_pac = lay[which][1], lay[which][2]
        seen, n_refused = [], 0
        for key, ids in V.groups().items():
            lst = S.orderings(V, ids)[ordering]
            dev.set_opt(S.opt_of(key))
            if form == "ssw16" and V.refused[ids[0]]:
                rc, _ = _sw(dev, _jobs(V, tpos, lst))
                assert rc == BSX_E_ARG, (key, rc)
                n_refused += 1
                continue
            _compare(V, dev, tpos, key, lst)
            seen += [i for i in lst if i != S.FILLER]
        dev.close()
        if form == "ssw16":
            assert n_refused == S.N_REFUSED_SETS and V.family_counts(seen) == S.FAMILY_COUNTS_ADMITTED, V.family_counts(seen)
        else:
            assert V.family_counts(seen) == S.FAMILY_COUNTS, V.family_counts(seen)
            assert {120, 128, 136, 184, 192, 200} <= S.padded_queries(V, seen)      # both sides of the sw_pass<2|3|4> edges
        assert S.score_classes(V.score[sorted(set(seen))]) == (S.SCORE_CLASSES if form == "ssw32" else S.SCORE_CLASSES_ADMITTED)
        here = S.strand_ends(V, tpos, l_pac, seen)
        assert here == ({("start", 0), ("end", 1)} if which == 0 else {("start", 1), ("end", 2)}), (which, here)
        ends |= here
    # between the layouts: a window at tpos = 0, one ending at l_pac, one starting at l_pac, one ending at 2 l_pac
    assert ends == {("start", 0), ("end", 1), ("start", 1), ("end", 2)}, ends


@pytest.mark.parametrize("n", S.LIST_LENGTHS)
@pytest.mark.parametrize("form", FORMS)
def test_short_lists(ctx, tune, form, n):
    """lists that end inside a wavefront of sixteen, at its end, and one job into the next"""
    V, lay = ctx
    tune("sw_form", form)
    dev = _device(V, lay, n & 1)
    m = 0
    for key, ids in V.groups().items():
        if len(ids) < n or (form == "ssw16" and V.refused[ids[0]]):
            continue
        dev.set_opt(S.opt_of(key))
        _compare(V, dev, lay[n & 1][1], key, S.orderings(V, ids)["shuffled"][:n])
        m += 1
    dev.close()
    assert m >= 8, m


def test_grid_stride_loop(ctx, tune):
    """more jobs than one trip of the launch's waves takes (16 jobs x 256 CUs x 32 waves, twice over, and no multiple of 16): every copy of a
    job scores what the first copy does, and that is the recorded score"""
    V, lay = ctx
    tune("sw_form", "ssw16")
    key, ids = max(((k, v) for k, v in V.groups().items() if not V.refused[v[0]]), key=lambda kv: len(kv[1]))
    base = S.orderings(V, ids)["shuffled"]
    assert S.TILED > 2 * 16 * 256 * 32 and S.TILED % 16 and len(base) % 16
    reps = -(-S.TILED // len(base))
    jobs = np.tile(_jobs(V, lay[0][1], base), reps)[:S.TILED]
    dev = _device(V, lay, 0)
    dev.set_opt(S.opt_of(key))
    rc, res = _sw(dev, jobs)
    dev.close()
    assert rc == 0
    first = res["score"][:len(base)]
    assert (first == V.score[base]).all()
    want = np.tile(first, reps)[:S.TILED]
    bad = np.nonzero(res["score"] != want)[0]
    assert len(bad) == 0, (len(bad), bad[:5], res["score"][bad[:5]], want[bad[:5]])


def test_refused_option_sets(ctx, tune):
    """one more on the term each guard set pushes: ssw16 launches nothing and returns BSX_E_ARG, ssw32 answers the recorded scores"""
    V, lay = ctx
    dev = _device(V, lay, 1)
    n = 0
    for key, ids in V.groups().items():
        if not V.refused[ids[0]]:
            continue
        dev.set_opt(S.opt_of(key))
        tune("sw_form", "ssw16")
        rc, res = _sw(dev, _jobs(V, lay[1][1], ids))
        assert rc == BSX_E_ARG and (res["score"] == 0).all(), (key, rc)
        tune("sw_form", "ssw32")
        _compare(V, dev, lay[1][1], key, ids)
        n += len(ids)
    dev.close()
    assert n == S.FAMILY_COUNTS["refused"] + S.FAMILY_COUNTS["refused_ins"]


@pytest.mark.parametrize("form", FORMS)
def test_empty_target(ctx, tune, form):
    """a query against a target of no bases (the seam's range allows it: no row is computed) scores 0, alone in its list and in a register
    beside a job that has rows; its neighbours score what they were recorded with"""
    V, lay = ctx
    tune("sw_form", form)
    dev = _device(V, lay, 0)
    key, ids = next((k, v) for k, v in V.groups().items() if not V.refused[v[0]])
    dev.set_opt(S.opt_of(key))
    lst = ids[:19]
    for empty in ([0], [0, 3, 18], list(range(19))):
        jobs = _jobs(V, lay[0][1], lst)[:1 if empty == [0] else 19]
        for k in empty:
            jobs["tlen"][k] = 0
        rc, res = _sw(dev, jobs)
        assert rc == 0
        want = [0 if k in empty else int(V.score[lst[k]]) for k in range(len(jobs))]
        assert [int(x) for x in res["score"]] == want, (form, empty)
    dev.close()


def test_seam_declines_what_it_does_not_hold(ctx, tune):
    V, lay = ctx
    dev = _device(V, lay, 0)
    key = next(k for k, v in V.groups().items() if not V.refused[v[0]])
    dev.set_opt(S.opt_of(key))
    ok = _jobs(V, lay[0][1], V.groups()[key][:3])
    for form in FORMS:
        tune("sw_form", form)
        assert _sw(dev, ok)[0] == 0
        for field, value in (("qdir", -1), ("tdir", -1), ("qcomp", 1), ("qlen", 200), ("tlen", 200), ("tlen", -1), ("tpos", -1), ("tpos", 2 * lay[0][2])):
            bad = ok.copy()
            bad[field][1] = value
            assert _sw(dev, bad)[0] == BSX_E_ARG, (form, field, value)
    tune("sw_form", "ssw64")
    assert _sw(dev, ok)[0] == BSX_E_ARG
    dev.close()
