"""-m gpu: the table passes of k_cov.hip and k_meth.hip past one trip per workgroup.  The cases of tests/tables_scale_cases.py for this device's
compute-unit count: a genome of 8 n_cu + 5 tiles (8.4 Mbp at 256 compute units) whose FM indices the device builds, more coverage jobs
and conversion records than one sweep of the adding kernels takes, more mask intervals than the painting grid has workgroups, and bases,
jobs and records planted where a workgroup's second and third trips and the scan's second and third steps begin.  Every table, and every
counter of the conversion state, against the numpy references of that module, exactly; tests/test_tables_scale_cpu.py has shown on the CPU
that those expectations change when a pass forgets a later trip."""
import numpy as np
import pytest
import simdata
import tables_scale_cases as S
import cov_model as V

pytestmark = pytest.mark.gpu
SETTINGS = ("cov_lds_bins", "cov_flush_tiles", "meth_flush_tiles")


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device
    import test_gpu_meth as TM
    d = str(tmp_path_factory.mktemp("tables_scale"))
    dev = Device(0)
    c = S.build(dev.n_cu, L_.COV_TILE)
    simdata.write_genome(d + "/g.fa", c.contigs)
    idx = Index.from_fasta(d + "/g.fa")
    assert idx.l_pac == c.L
    dev.build_index(idx)
    c.dep = S.cov_depth(c)
    c.want4, c.want12 = S.cov_tables(c, c.dep), S.cov_tables(c, c.dep, c.top, c.bot)
    c.cov_a, c.cov_pool = S.cov_arrays(c)
    c.pos, c.val = S.meth_counters(c, c.meth_jobs)
    c.sites = S.meth_sites(c, c.pos, c.val)
    c.K, c.S = S.meth_tables(c.sites)
    c.meth_a, c.meth_pool, c.meth_buf = TM._arrays(c.meth_jobs)
    yield dev, c
    for k in SETTINGS:
        L_.tune(k, None)
    dev.close()
    idx.close()


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and (a == b).all(), (what, V.NAMES[i], a.shape, b.shape, np.flatnonzero(a != b)[:8].tolist() if a.shape == b.shape else None)


def _load_cov(dev, c, cuts=None, masks=True):
    dev.cov_reset()
    cuts = cuts or [0, len(c.cov_a)]
    for lo, hi in zip(cuts, cuts[1:]):                                        # (the pool is shared: cig_off stays valid)
        dev.cov_batch(c.cov_a[lo:hi], c.cov_pool)
    if masks:
        dev.cov_set_mask(0, c.top)
        dev.cov_set_mask(1, c.bot)


def test_the_genome_passes_every_threshold_on_this_device(big):
    dev, c = big
    assert dev.n_cu > 0 and c.n_cu == dev.n_cu
    assert c.n_tiles > 8 * dev.n_cu and c.n_tiles > 2048                      # fewer than 256 compute units: the scan's third step is not reached
    S.assert_reach(c, c.dep, c.sites)


def test_coverage_tables_without_and_with_masks_read_twice_and_after_more_jobs(big):
    dev, c = big
    _load_cov(dev, c, masks=False)
    _same(dev.cov_tables(), c.want4, "no masks")
    dev.cov_set_mask(0, c.top)
    dev.cov_set_mask(1, c.bot)
    got = dev.cov_tables()
    _same(got, c.want12, "masks")
    assert len(got) == 12 and len(got[0]) > S.LDS_BINS_MAX and all(t.sum() > 0 for t in got)
    _same(dev.cov_tables(), c.want12, "read twice")
    more = c.cov_designed[:40]                                                # the long run and the jobs at the first boundaries, once more
    import test_gpu_cov as TC
    a, pool = TC._job_arrays(more)
    dev.cov_batch(a, pool)
    _same(dev.cov_tables(), S.cov_tables(c, S.cov_depth(c, again=more), c.top, c.bot), "more jobs after a read")
    dev.cov_reset()


def test_coverage_jobs_as_three_batches(big):
    dev, c = big
    n = len(c.cov_a)
    _load_cov(dev, c, cuts=[0, 5, S.cov_sweep(c.n_cu) + 12, n])                 # the second one is more than a sweep of k_cov_add
    _same(dev.cov_tables(), c.want12, "three batches")
    dev.cov_reset()


def test_coverage_tables_whenever_the_histograms_are_flushed(big):
    """a grid of 4 n_cu: every workgroup takes two tiles and five take three, so flushing every second tile leaves a trip to come for those
    five and flushing every third happens only on them; four LDS bins send nearly every position to the bins in HBM"""
    from biscuit_amd import _lib as L_
    dev, c = big
    _load_cov(dev, c)
    try:
        for flush in (None, 1, 2, 3):
            for bins in (None, 4):
                L_.tune("cov_flush_tiles", flush)
                L_.tune("cov_lds_bins", bins)
                _same(dev.cov_tables(), c.want12, (flush, bins))
    finally:
        L_.tune("cov_lds_bins", None)
        L_.tune("cov_flush_tiles", None)
        dev.cov_reset()


def _load_meth(dev, c, cuts=None):
    dev.meth_reset()
    dev.set_reads(c.meth_buf)
    cuts = cuts or [0, len(c.meth_a)]
    for lo, hi in zip(cuts, cuts[1:]):                                        # (the pool and the read buffer are shared: offsets stay valid)
        dev.meth_batch(c.meth_a[lo:hi], c.meth_pool)


def _same_state(dev, c, what):
    """every counter of every position, a slice at a time: an addition in the wrong place is seen wherever it went"""
    step, seen = 1 << 20, 0
    for lo in range(0, c.L, step):
        hi = min(lo + step, c.L)
        got, want = dev.meth_read(lo, hi - lo), S.dense(c.pos, c.val, lo, hi)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (what, (lo + bad[:8]).tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        seen += int((got.sum(axis=1) > 0).sum())
    assert seen == len(c.pos)


def test_conversion_counters_of_every_position_and_the_tables(big):
    from biscuit_amd import _lib as L_
    dev, c = big
    _load_meth(dev, c)
    _same_state(dev, c, "one batch")
    k, s = dev.meth_tables()
    assert (k == c.K).all() and (s == c.S).all() and c.K.min() > 0, (k, c.K, s, c.S)
    try:
        for flush in (1, 2, None):                                            # a wave adds its sums after every tile, after every second, on its last trip
            L_.tune("meth_flush_tiles", flush)
            k, s = dev.meth_tables()
            assert (k == c.K).all() and (s == c.S).all(), (flush, k, c.K, s, c.S)
    finally:
        L_.tune("meth_flush_tiles", None)
    _same_state(dev, c, "after the table passes")                             # which only read
    dev.meth_reset()


def test_conversion_records_as_several_batches(big):
    dev, c = big
    sweep, n = S.meth_sweep(c.n_cu), len(c.meth_a)
    _load_meth(dev, c, cuts=[0, 1, sweep + 2, sweep + 2, n])                    # the second one is more than a sweep of k_meth_add
    assert sweep + 2 < n
    _same_state(dev, c, "several batches")
    k, s = dev.meth_tables()
    assert (k == c.K).all() and (s == c.S).all(), (k, c.K, s, c.S)
    dev.meth_reset()
