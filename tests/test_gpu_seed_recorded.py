"""The seeding kernels (csrc/hip/k_seedt.hip over seed_tab.hpp, k_seed.hip over seed_core.hpp) against the reference's own interval lists,
recorded: Device.seed over the designed strand searches of tests/seed_cases.py must equal tests/golden/ref_seeds.npz per strand search --
every interval, every field, in order, and the offsets that follow from the counts -- with the cases alone, under each option set,
scattered among two thousand ordinary strand searches, in reversed order, in batches of 1, 63, 64 and 65, at other table depths, without
the table, and in the form the chunk-wide launch of bsx_regions_batch has (seed_batch_form=chunk: lists written where they stay, the trip
budget, the second and third pass, the gather) under the settings that move its edges.  Device.sa is held to the recorded bwt_sa.

tests/test_seed_recorded_cpu.py checks the recording's coverage of the edges, and the host machines and the restatement against it."""
import re
import time
import numpy as np
import pytest

import seed_cases as SC
from biscuit_amd import _lib as B
from biscuit_amd.api import Index, Device, default_opt, SEED_DT, SA_DT

pytestmark = pytest.mark.gpu

T0 = time.time()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    rec = SC.load()
    assert int(rec.z["genome_crc"]) == SC.genome_crc() and int(rec.z["reads_crc"]) == SC.reads_crc()
    d = tmp_path_factory.mktemp("seed_idx")
    SC.write_fasta(str(d / "g.fa"))
    idx = Index.build(str(d / "g.fa"), str(d / "g"))
    dev = Device(0)
    dev.upload_index(idx)
    assert dev.seed_table()[1] == SC.K()
    yield {"rec": rec, "idx": idx, "dev": dev}
    dev.close()
    idx.close()
    print("tests/test_gpu_seed_recorded.py: %.1f s from import to teardown" % (time.time() - T0))


def opt_of(optset):
    opt = default_opt()
    for k, v in SC.options(optset).items():
        setattr(opt, k, v)
    return opt


def ordinary(n, seed):
    """n reads of 150 bases from the unique part of the genome, every third reverse-complemented, with up to two substitutions"""
    bg = SC.genome()[1]["bg1"]
    r = SC.Ints(seed)
    out = []
    for k in range(n):
        at = r.below(len(bg) - 200)
        s = bg[at:at + 150].copy()
        for _ in range(k % 3):
            s[r.below(150)] = r.below(4)
        out.append(SC.revcomp(s) if k % 3 == 0 else s)
    return out


def device_seed(env, opt, tasks):
    try:
        return env["dev"].seed(opt, tasks)
    except RuntimeError as e:      # an error of the device, not a difference: nothing more is started on it
        pytest.exit("tests/test_gpu_seed_recorded.py: %s" % e, returncode=3)


def run(env, optset="default", n_ordinary=0, reverse=False, batch=None):
    """the strand searches of the option set's cases (parent 1 then 0 of each read), among 2 * n_ordinary others when asked, as one
    Device.seed call or in calls of exactly `batch` strand searches -> asserts that every one of them equals the recording"""
    dev, rec = env["dev"], env["rec"]
    cs = SC.optset_cases(optset)
    opt = opt_of(optset)
    reads = [(c["name"], c["seq"]) for c in cs] + [(None, s) for s in ordinary(n_ordinary, 77)]
    if n_ordinary:      # the cases scattered: a fixed permutation
        keys = SC.Ints(5).words(len(reads))
        reads = [reads[i] for i in np.argsort(keys, kind="stable")]
    if reverse:
        reads = reads[::-1]
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
    buf = np.concatenate([s for _, s in reads])
    tasks = np.zeros(2 * len(reads), SEED_DT)
    for i, (_, s) in enumerate(reads):
        for k, parent in enumerate((1, 0)):
            tasks[2 * i + k] = (off[i], len(s), parent)
    try:
        dev.set_opt(opt)
        dev.set_reads(buf)
    except RuntimeError as e:
        pytest.exit("tests/test_gpu_seed_recorded.py: %s" % e, returncode=3)
    lists = [None] * len(tasks)
    if batch is None:
        intv, ioff = device_seed(env, opt, tasks)
        assert ioff[0] == 0 and len(intv) == ioff[-1]
        for t in range(len(tasks)):
            lists[t] = intv[ioff[t]:ioff[t + 1]]
    else:      # exactly `batch` strand searches a call: the last call is filled up from the start of the list
        for a in range(0, len(tasks), batch):
            which = [(a + j) % len(tasks) for j in range(batch)]
            intv, ioff = device_seed(env, opt, tasks[which])
            assert ioff[0] == 0 and len(intv) == ioff[-1]
            for j, t in enumerate(which):
                lists[t] = intv[ioff[j]:ioff[j + 1]]
    bad, n = [], 0
    for i, (name, s) in enumerate(reads):
        if name is None:
            continue
        for k, parent in enumerate((1, 0)):
            n += 1
            d = SC.same_intervals(lists[2 * i + k], rec.intervals(optset, name, parent))
            if d:
                bad.append("[%s] %s parent %d (%d bases): %s" % (optset, name, parent, len(s), d))
    assert n == 2 * len(cs) and (optset != "default" or n == 2 * len(SC.cases()))
    assert not bad, "%d of %d strand searches differ from the reference's lists:\n%s" % (len(bad), n, "\n".join(bad[:25]))


# ------------------------------------------------------------------------------------------ the table form
def test_the_cases_alone(env):
    run(env)


@pytest.mark.parametrize("optset", [o for o, _, _ in SC.OPTSETS if o != "default"])
def test_under_each_option_set(env, optset):
    run(env, optset)


def test_the_cases_among_two_thousand_ordinary_strand_searches(env):
    run(env, n_ordinary=1000)


def test_the_cases_in_reversed_order(env):
    run(env, reverse=True)


@pytest.mark.parametrize("size", [1, 63, 64, 65])
def test_in_batches_of_exactly(env, size):
    run(env, batch=size)


# ------------------------------------------------------------------------------------------ table depth and the classic form
@pytest.mark.parametrize("depth", ["0", "2", "K-1"])
def test_at_other_table_depths(env, depth):
    k = {"0": 0, "2": 2, "K-1": SC.K() - 1}[depth]
    dev = env["dev"]
    try:
        B.tune("seed_tab_k", k)
        dev.upload_index(env["idx"])
        assert dev.seed_table()[1] == k
        run(env)
        run(env, "strict")
    finally:
        B.tune("seed_tab_k", None)
        dev.upload_index(env["idx"])
    assert dev.seed_table()[1] == SC.K()


def test_the_classic_form(env, tune):
    tune("seed_form", "classic")
    run(env)
    run(env, "strict")


# ------------------------------------------------------------------------------------------ the chunk's form
PASS_LINE = re.compile(r"\[M::seed_batch\] chunk form, pass (\d+): (\d+) strand searches, lists of (\d+) entries( written where they stay)?, budget (\d+), quota (\d+), "
                       r"(\d+) workgroups, (\d+) slabs: (\d+) left to be seeded again")


def passes(err):
    return [dict(zip(("pass", "n", "cap", "direct", "budget", "quota", "grid", "slabs", "left"), [int(v) if v and v.isdigit() else bool(v) for v in m.groups()]))
            for m in PASS_LINE.finditer(err)]


def test_the_chunk_form_under_the_default_settings(env, tune, capfd):
    """the launch bsx_regions_batch makes: lists written where they stay, a budget of TRIP_BUDGET requests per 256 bases.  The strand
    searches built to cross it (tests/test_seed_recorded_cpu.py counts their requests) are what the first pass leaves, the second pass has
    eight budgets, and those past that as well take the third"""
    tune("seed_batch_form", "chunk")
    tune("phases", 1)
    capfd.readouterr()
    run(env)
    ps = passes(capfd.readouterr().err)
    print(ps)
    n_over = 2 * sum(1 for c in SC.cases() if c["budget"] == "over")
    longest = max(len(c["seq"]) for c in SC.cases())
    assert len(ps) == 3 and [p["pass"] for p in ps] == [1, 2, 3], ps
    assert ps[0]["n"] == 2 * len(SC.cases()) and ps[0]["direct"] and ps[0]["cap"] == longest and ps[0]["budget"] == SC.TRIP_BUDGET and ps[0]["quota"] == 0
    assert ps[0]["left"] == n_over == ps[1]["n"], (ps, n_over)
    assert ps[1]["cap"] == 8 * longest and ps[1]["budget"] == 8 * SC.TRIP_BUDGET and not ps[1]["direct"]
    assert 0 < ps[1]["left"] < n_over and ps[2]["n"] == ps[1]["left"] and ps[2]["budget"] == 0 and ps[2]["left"] == 0


@pytest.mark.parametrize("knob,value", [("seed_mem_cap", 4), ("seed_mem_cap", 28), ("seed_trip_budget", 64), ("seed_trip_budget", 0), ("seed_direct", 0),
                                        ("seed_quota", 1), ("seed_budget2", 1)])
def test_the_chunk_form_under_each_setting(env, tune, capfd, knob, value):
    tune("seed_batch_form", "chunk")
    tune("phases", 1)
    tune(knob, value)
    capfd.readouterr()
    run(env)
    ps = passes(capfd.readouterr().err)
    print(ps)
    n, first = 2 * len(SC.cases()), ps[0]
    n_over = 2 * sum(1 for c in SC.cases() if c["budget"] == "over")
    assert first["pass"] == 1 and first["n"] == n and ps[-1]["left"] == 0
    if knob == "seed_mem_cap":      # lists of 4 / 28 entries: what has more intervals, or crosses the budget, is seeded again
        rec = env["rec"]
        more = sum(1 for c in SC.cases() for p in (1, 0) if rec.stats("default", c["name"], p)["intervals"] > value or c["budget"] == "over")
        assert first["cap"] == value and first["left"] == more and ps[1]["cap"] == max(8 * value, 1024), (ps, more)
    elif knob == "seed_trip_budget":
        assert first["budget"] == value and (first["left"] > n // 2 if value else len(ps) == 1 and first["left"] == 0), ps
    elif knob == "seed_direct":
        assert not first["direct"] and first["left"] == n_over, ps
    elif knob == "seed_quota":
        assert first["quota"] == 1 and first["grid"] == (n + 255) // 256 and first["left"] == n_over, ps
    elif knob == "seed_budget2":      # the second pass with the first one's budget: it leaves all of them to the third
        assert len(ps) == 3 and ps[1]["budget"] == SC.TRIP_BUDGET and ps[1]["left"] == n_over == ps[2]["n"], ps


# ------------------------------------------------------------------------------------------ the suffix-array look-ups
def test_sa_lookups_equal_the_recorded_bwt_sa(env):
    """the first min(x2, 50) ranks of every recorded interval (the option sets of seed_cases.SA_OPTSETS: the short set's are most of the
    text), every (parent, rank) once"""
    rec, dev = env["rec"], env["dev"]
    ranks = {0: set(), 1: set()}
    n_lists = 0
    for (optset, name, parent) in rec.key:
        if optset in SC.SA_OPTSETS:
            n_lists += 1
            for x0, _, x2, _ in rec.intervals(optset, name, parent):
                ranks[parent].update(range(int(x0), int(x0) + min(int(x2), 50)))
    assert n_lists == 2 * sum(len(SC.optset_cases(o)) for o in SC.SA_OPTSETS)
    jobs, want = [], []
    for parent in (0, 1):
        assert ranks[parent] == set(rec.sa[parent])      # the recording holds exactly these
        for k in sorted(ranks[parent]):
            jobs.append((k, parent, 0))
            want.append(rec.sa[parent][k])
    assert len(jobs) > 5000
    try:
        got = dev.sa(np.array(jobs, dtype=SA_DT))
    except RuntimeError as e:
        pytest.exit("tests/test_gpu_seed_recorded.py: %s" % e, returncode=3)
    bad = np.nonzero(got != np.array(want, np.uint64))[0]
    assert len(bad) == 0, "%d of %d positions differ; the first: rank %d parent %d -> %d, recorded %d" % (
        len(bad), len(jobs), jobs[bad[0]][0], jobs[bad[0]][1], got[bad[0]], want[bad[0]])
