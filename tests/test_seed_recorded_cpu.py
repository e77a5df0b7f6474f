"""CPU: the recording of the designed strand searches of tests/seed_cases.py (tests/golden/ref_seeds.npz: the reference's own bwt_smem1a and
bwt_seed_strategy1 under mem_collect_intv's three passes) occupies every edge it was designed for, and the oracle's restatement, the classic
seeding machine (seed_core.hpp) and the table machine (seed_tab.hpp) at four table depths all return it list for list; the strand searches
meant to cross the first seeding pass's budget do, and the ordinary ones do not.  tests/test_gpu_seed_recorded.py holds the kernels to the
same file."""
import ctypes as C
import numpy as np
import pytest

import seed_cases as SC
import oracle_lib
from biscuit_amd.api import Index, default_opt, SEED_DT
from test_kernel_logic_host import _harness

MEM_CAP = 1 << 14      # entries of a strand search's list in the host machines: more than any recorded list


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    rec = SC.load()
    assert int(rec.z["genome_crc"]) == SC.genome_crc() and int(rec.z["reads_crc"]) == SC.reads_crc()
    d = tmp_path_factory.mktemp("seed_idx")
    SC.write_fasta(str(d / "g.fa"))
    idx = Index.build(str(d / "g.fa"), str(d / "g"))
    assert idx.l_pac == SC.l_pac()
    yield {"rec": rec, "idx": idx, "port": oracle_lib.Port(idx, n_threads=4)}
    idx.close()


def opt_of(optset):
    opt = default_opt()
    for k, v in SC.options(optset).items():
        assert hasattr(opt, k)
        setattr(opt, k, v)
    return opt


def batch(cs):
    """the cases' strand searches, parent 1 then 0 of each read -> (read buffer, tasks)"""
    buf, off = SC.read_buffer(cs)
    tasks = np.zeros(2 * len(cs), SEED_DT)
    for i, c in enumerate(cs):
        for k, parent in enumerate((1, 0)):
            tasks[2 * i + k] = (off[i], len(c["seq"]), parent)
    return buf, tasks


def differences(rec, optset, cs, intv, off):
    bad = []
    for i, c in enumerate(cs):
        for k, parent in enumerate((1, 0)):
            t = 2 * i + k
            d = SC.same_intervals(intv[off[t]:off[t + 1]], rec.intervals(optset, c["name"], parent))
            if d:
                bad.append("[%s] %s parent %d: %s" % (optset, c["name"], parent, d))
    return bad


def test_every_edge_is_occupied(env):
    rows = SC.coverage(env["rec"])
    for edge, ok, what in rows:
        print("%-4s %-34s %s" % ("ok" if ok else "MISS", edge, what))
    missing = [r for r in rows if not r[1]]
    assert not missing, "\n".join("%s: %s" % (e, w) for e, _, w in missing)
    assert SC.K() >= 8 and len(rows) > 100
    assert len(env["rec"].key) == 2 * sum(len(SC.optset_cases(o)) for o, _, _ in SC.OPTSETS)


@pytest.mark.parametrize("optset", [o for o, _, _ in SC.OPTSETS])
def test_the_restatement_equals_the_recording(env, optset):
    cs = SC.optset_cases(optset)
    buf, tasks = batch(cs)
    opt = opt_of(optset)
    port = env["port"]
    port.set_opt(opt)
    port.set_reads(buf)
    intv, off = port.seed(opt, tasks)
    bad = differences(env["rec"], optset, cs, intv, off)
    assert not bad, "%d of %d strand searches differ:\n%s" % (len(bad), len(tasks), "\n".join(bad[:25]))


def host_machine(env, optset, cs, K=None, one=None):
    """hostlogic_seed (K None) or hostlogic_seed_tab over the cases (one: a single strand search) -> (intervals, offsets, counters)"""
    H = _harness()
    H.hostlogic_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    H.hostlogic_seed_tab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    buf, tasks = batch(cs)
    if one is not None:
        tasks = tasks[one:one + 1].copy()
    opt = opt_of(optset)
    total = sum(int(env["rec"].stats(optset, c["name"], p)["intervals"]) for c in cs for p in (1, 0))
    out = np.zeros((total + 16, 4), np.uint64)
    off = np.zeros(len(tasks) + 1, np.int64)
    ctr = (C.c_uint64 * 3)()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    if K is None:
        rc = H.hostlogic_seed(env["idx"].h, C.byref(opt), P(buf), len(tasks), P(tasks), MEM_CAP, P(out), len(out), P(off), ctr)
    else:
        rc = H.hostlogic_seed_tab(env["idx"].h, C.byref(opt), P(buf), len(tasks), P(tasks), K, MEM_CAP, P(out), len(out), P(off), ctr)
    assert rc == 0, (optset, K, rc)
    return out, off, list(ctr)


@pytest.mark.parametrize("optset", [o for o, _, _ in SC.OPTSETS])
def test_the_classic_machine_equals_the_recording(env, optset):
    cs = SC.optset_cases(optset)
    intv, off, _ = host_machine(env, optset, cs)
    bad = differences(env["rec"], optset, cs, intv, off)
    assert not bad, "%d of %d strand searches differ:\n%s" % (len(bad), 2 * len(cs), "\n".join(bad[:25]))


@pytest.mark.parametrize("optset", [o for o, _, _ in SC.OPTSETS])
@pytest.mark.parametrize("depth", ["0", "2", "K-1", "K"])
def test_the_table_machine_equals_the_recording(env, optset, depth):
    K = {"0": 0, "2": 2, "K-1": SC.K() - 1, "K": SC.K()}[depth]
    cs = SC.optset_cases(optset)
    intv, off, _ = host_machine(env, optset, cs, K=K)
    bad = differences(env["rec"], optset, cs, intv, off)
    assert not bad, "%d of %d strand searches differ at depth %d:\n%s" % (len(bad), 2 * len(cs), K, "\n".join(bad[:25]))


def test_the_budget_cases_cross_the_budget_and_the_ordinary_ones_do_not(env):
    """requests (FM extensions of either kind and table look-ups: what k_seedt counts a strand search's trips by) of the table machine at
    the device's depth, one strand search at a time, against the first pass's budget of TRIP_BUDGET per 256 bases of read"""
    cs = SC.cases()
    n_over = n_under = 0
    for i, c in enumerate(cs):
        if not c["budget"]:
            continue
        budget = SC.TRIP_BUDGET * ((len(c["seq"]) + 255) >> 8)
        for k, parent in enumerate((1, 0)):
            _, _, ctr = host_machine(env, "default", cs, K=SC.K(), one=2 * i + k)
            requests = ctr[0] // 2 + ctr[1] + ctr[2]
            print("%-12s parent %d: %6d requests, budget %6d (%s)" % (c["name"], parent, requests, budget, c["budget"]))
            if c["budget"] == "over":
                assert requests > budget, (c["name"], parent, requests, budget)
                n_over += 1
            else:
                assert requests < budget, (c["name"], parent, requests, budget)
                n_under += 1
    assert n_over >= 8 and n_under >= 50
