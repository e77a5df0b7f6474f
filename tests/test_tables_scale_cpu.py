"""CPU: the cases of tests/tables_scale_cases.py, which take the table passes of k_cov.hip and k_meth.hip past one trip per workgroup on the
device (tests/test_gpu_tables_scale.py), checked here without one.  (1) At n_cu = 2 (21 tiles) the fast references equal the slow ones the
suite already trusts: tests/test_gpu_cov.py's _expect, tests/test_gpu_meth.py's _walk and tests/meth_model.py's tables over the full arrays.
(2) At n_cu = 2 and at n_cu = 256 (the references alone) the cases reach what DESIGN.md section 5 says they reach, and the expectation
depends on the later trips: recomputed as a pass would give it that (a) restarted the depth carry at tile 1024, (b) took only the tiles of
its first trip, (c) painted only the first 8 n_cu mask intervals, (d) applied only the first sweep of jobs, it differs -- under (a) and (b) in
a table of each of the three regions (whole genome, top GC, bottom GC), under (c) in both masked regions (the whole-genome tables have no
mask), under (d) in the coverage tables and in a conversion sum.  These are conditions on the inputs: a pass on the device cannot be vacuous."""
import numpy as np
import pytest
import tables_scale_cases as S

T = 4096


@pytest.fixture(scope="module", params=[2, 256])
def cases(request):
    from biscuit_amd import _lib as L_
    assert L_.COV_TILE == T
    c = S.build(request.param, T)
    c.dep = S.cov_depth(c)
    c.want = S.cov_tables(c, c.dep, c.top, c.bot)
    c.pos, c.val = S.meth_counters(c, c.meth_jobs)
    c.sites = S.meth_sites(c, c.pos, c.val)
    return c


def test_fast_references_equal_the_slow_ones_at_two_compute_units():
    import test_gpu_cov as TC
    import test_gpu_meth as TM
    c = S.build(2, T)
    dep = S.cov_depth(c)
    jobs = S.cov_job_list(c)
    a, pool = S.cov_arrays(c)
    a2, pool2 = TC._job_arrays(jobs)
    assert a.tobytes() == a2.tobytes() and (pool == pool2).all()
    for fast, slow in ((S.cov_tables(c, dep), TC._expect(c.contigs, jobs)), (S.cov_tables(c, dep, c.top, c.bot), TC._expect(c.contigs, jobs, c.top, c.bot))):
        assert len(fast) == len(slow) and not S.changed(fast, slow)
    k = S.cov_sweep(2)
    assert not S.changed(S.cov_tables(c, S.cov_depth(c, k)), TC._expect(c.contigs, jobs[:k]))
    assert not S.changed(S.cov_tables(c, S.cov_depth(c, again=c.cov_designed[:9])), TC._expect(c.contigs, jobs + c.cov_designed[:9]))
    g = np.concatenate([s for _, s in c.contigs])
    assert (g == c.g).all()
    pos, val = S.meth_counters(c, c.meth_jobs)
    cnt = TM._walk(g, c.meth_jobs)
    assert (S.dense(pos, val, 0, c.L) == cnt).all() and (val.sum(axis=1) > 0).all() and (np.diff(pos) > 0).all()
    assert (S.dense(pos, val, 5000, 9000) == cnt[5000:9000]).all()
    K, S_, unc = TM._model_sums(c.contigs, cnt)
    sites = S.meth_sites(c, pos, val)
    k2, s2 = S.meth_tables(sites)
    assert (k2 == K).all() and (s2 == S_).all() and sites[3] == unc and unc > 0 and K.min() > 0


def test_the_cases_reach_the_later_trips(cases):
    c = cases
    S.assert_reach(c, c.dep, c.sites)
    kinds = [(J.tag, J.rev, J.read2, bool(J.lowq)) for J in c.meth_jobs]
    assert {k[0] for k in kinds} == {0, 1, 2, 3} and {k[1] for k in kinds} == {False, True} == {k[2] for k in kinds} == {k[3] for k in kinds}
    cols = [sum(n for n, op in J.ops if op == "M") for J in c.meth_jobs]
    assert 40 <= min(cols) and max(cols) <= 60
    if c.n_cu == 256:
        assert c.L == 8405025 and len(c.bulk_fpos) >= 600000 and len(c.meth_jobs) >= 10000 and c.G == [1024, 2048]


def _regions(idx):
    return {i // 4 for i in idx}


def test_the_expectation_depends_on_the_later_trips(cases):
    c = cases
    n_cu, want = c.n_cu, c.want
    if c.n_tiles > S.SCAN_STEP:                                                 # (a): there is no second scan step below 1025 tiles
        assert _regions(S.changed(S.cov_tables(c, S.fault_scan_restart(c, c.dep), c.top, c.bot, nb=len(want[0])), want)) == {0, 1, 2}
    else:
        assert n_cu == 2
    # (b) the counting pass, the tile sums and the largest depth, each without its later trips
    assert _regions(S.changed(S.cov_tables(c, c.dep, c.top, c.bot, counted=S.first_trip(c, 4 * n_cu)), want)) == {0, 1, 2}
    assert _regions(S.changed(S.cov_tables(c, S.fault_sums_first_trip(c, c.dep), c.top, c.bot, nb=len(want[0])), want)) == {0, 1, 2}
    nb = S.fault_max_first_trip(c, c.dep)
    short = S.cov_tables(c, c.dep, c.top, c.bot, nb=nb)
    assert nb < len(want[0]) and all(short[4 * r].sum() < want[4 * r].sum() for r in range(3))      # positions of every region are too deep for it
    # (b) the conversion pass without its later trips
    K, S_ = S.meth_tables(c.sites)
    k1, s1 = S.meth_tables(c.sites, counted=c.sites[0] < 8 * n_cu * T)
    assert (k1 < K).all() and (s1 < S_).all()
    # (c) the first 8 n_cu intervals of either mask alone
    assert _regions(S.changed(S.cov_tables(c, c.dep, c.top[:8 * n_cu], c.bot[:8 * n_cu]), want)) == {1, 2}
    # (d) the first sweep of jobs alone
    assert _regions(S.changed(S.cov_tables(c, S.cov_depth(c, S.cov_sweep(n_cu)), c.top, c.bot), want)) == {0, 1, 2}
    pos, val = S.meth_counters(c, c.meth_jobs[:S.meth_sweep(n_cu)])
    k1, s1 = S.meth_tables(S.meth_sites(c, pos, val))
    assert (k1 != K).any() and (s1 != S_).any() and len(pos) < len(c.pos)
