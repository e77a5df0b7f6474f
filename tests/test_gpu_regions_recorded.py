"""The region kernels (csrc/hip/k_occ.hip, k_regions.hip, k_seedsw.hip, k_c2r.hip: SA intervals -> chains -> filtered chains -> regions, through the ladder of LDS and HBM stores)
against the reference's own regions, recorded: Device.regions over the designed strand searches of tests/regions_cases.py must equal
tests/golden/ref_regions.npz per strand search -- every region, every field, in order, frac_rep by its bits -- with the cases alone, scattered
among two thousand ordinary strand searches, under each routing setting of the library and under the option set that makes the seed filter run
for short reads.  Nothing may come back declined but the reads one base longer than the long tiers' rows, and those for their length only.

A regions batch takes the long reads' launches when its longest read exceeds RG_QCAP, and max_occ is an option of the whole call: the cases
run as three batches (short reads, long reads, the over-represented cases with their lowered max_occ).

tests/test_regions_recorded_cpu.py checks the recording's coverage of the table caps, and the host path and the Python restatement against it."""
import re
import time
import numpy as np
import pytest

import regions_cases as RC
from biscuit_amd.api import Index, Device, default_opt, SEED_DT

pytestmark = pytest.mark.gpu

READ_LENGTH_STATUS = -9      # rg_task's status 9: a read longer than the rows of the launch
T0 = time.time()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    rec = RC.load()
    assert int(rec.z["genome_crc"]) == RC.genome_crc() and int(rec.z["reads_crc"]) == RC.reads_crc()
    d = tmp_path_factory.mktemp("regions_idx")
    RC.write_fasta(str(d / "g.fa"))
    idx = Index.build(str(d / "g.fa"), str(d / "g"))
    dev = Device(0)
    dev.upload_index(idx)
    yield {"rec": rec, "idx": idx, "dev": dev}
    dev.close()
    idx.close()
    print("tests/test_gpu_regions_recorded.py: %.1f s from import to teardown" % (time.time() - T0))


def groups():
    """[(name, max_occ or None, [case])]"""
    cs = RC.cases()
    return [("short", None, [c for c in cs if not c["max_occ"] and not RC.long_group(c)]),
            ("long", None, [c for c in cs if not c["max_occ"] and RC.long_group(c)]),
            ("over", RC.OVER_MAX_OCC, [c for c in cs if c["max_occ"]])]


def ordinary(n, seed):
    """n reads of 150 bases from the unique part of the genome, every third reverse-complemented, with up to two substitutions"""
    bg = RC.genome()[0][0][1]
    r = RC.Ints(seed)
    out = []
    for k in range(n):
        at = r.below(len(bg) - 200)
        s = bg[at:at + 150].copy()
        for _ in range(k % 3):
            s[r.below(150)] = r.below(4)
        out.append(RC.revcomp(s) if k % 3 == 0 else s)
    return out


def run_group(env, optset, max_occ, cs, n_ordinary=0):
    """one regions batch: the cases' strand searches (parent 1 then 0 of each read), among 2 * n_ordinary others when asked -> the list of
    differences from the recording"""
    dev, rec = env["dev"], env["rec"]
    opt = default_opt()
    for k, v in dict(RC.OPTSETS)[optset].items():
        setattr(opt, k, v)
    if max_occ:
        opt.max_occ = max_occ
    reads = [(c["name"], c["seq"]) for c in cs] + [(None, s) for s in ordinary(n_ordinary, 77)]
    if n_ordinary:      # the cases scattered: a fixed permutation
        r = RC.Ints(5)
        keys = r.words(len(reads))
        reads = [reads[i] for i in np.argsort(keys, kind="stable")]
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
    buf = np.concatenate([s for _, s in reads])
    tasks = np.zeros(2 * len(reads), SEED_DT)
    for i, (_, s) in enumerate(reads):
        for k, parent in enumerate((1, 0)):
            tasks[2 * i + k] = (off[i], len(s), parent)
    try:
        dev.set_opt(opt)
        dev.set_reads(buf)
        regs, roff, rn = dev.regions(opt, tasks)
    except RuntimeError as e:      # an error of the device, not a difference: nothing more is started on it
        pytest.exit("tests/test_gpu_regions_recorded.py: %s" % e, returncode=3)
    bad = []
    for i, (name, s) in enumerate(reads):
        for k, parent in enumerate((1, 0)):
            t = 2 * i + k
            if name is None:
                if rn[t] < 0:
                    bad.append("an ordinary strand search came back declined (%d)" % rn[t])
                continue
            if len(s) > RC.DEFINES["RG_QCAP_LONG"]:
                if rn[t] != READ_LENGTH_STATUS:
                    bad.append("%s parent %d: a read of %d bases came back with %d, not declined for its length" % (name, parent, len(s), rn[t]))
                continue
            if rn[t] < 0:
                bad.append("%s parent %d: declined (%d); recorded counts %s" % (name, parent, rn[t], list(map(int, rec.counts(optset, name, parent)))))
                continue
            d = RC.same_regions(regs[roff[t]:roff[t] + rn[t]], rec.regions(optset, name, parent))
            if d:
                bad.append("%s parent %d: %s" % (name, parent, d))
    return bad


def run_all(env, optset="default", n_ordinary=0, which="all"):
    """which: "all", or one half of the comparison -- "answered": the regions of every strand search the device answered, "declined": that none
    but the reads too long for the rows came back declined"""
    bad, n = [], 0
    for gname, max_occ, cs in groups():
        bad += ["[%s] %s" % (gname, b) for b in run_group(env, optset, max_occ, cs, n_ordinary if gname == "short" else n_ordinary // 10)]
        n += 2 * len(cs)
    assert n == 2 * len(RC.cases())
    if which != "all":
        bad = [b for b in bad if (": declined (" in b) == (which == "declined")]
    assert not bad, "%d differences from the reference's regions over %d strand searches:\n%s" % (len(bad), n, "\n".join(bad[:25]))


def test_the_cases_alone(env):
    run_all(env)


def test_the_cases_among_two_thousand_ordinary_strand_searches(env):
    run_all(env, n_ordinary=1000)


@pytest.mark.parametrize("knob,value", [("regions_mid", 0), ("tier1c", 0), ("tier2_export", 1), ("tier2_export", 2), ("x4", 0), ("xl", 0), ("ext_pk", 0),
                                        ("pos_cap", 0), ("regions_quota", 1), ("c2r_quota", 1)])
def test_under_each_routing_setting(env, tune, knob, value):
    tune(knob, value)
    run_all(env)


def test_under_the_filter_active_option_set(env):
    """min_chain_weight = 5: mem_flt_chained_seeds runs for reads of 150 bases, every tier exports its chains and k_seedsw scores their seeds --
    the regions of every strand search the device answers (what it may decline is the next test's)"""
    run_all(env, optset="filter", which="answered")


def test_nothing_declined_under_the_filter_active_option_set(env):
    """With every tier exporting, the chains -> regions launches are the only makers of regions (shim.hip, run_tiers_exporting) and what
    outgrows the last of them is left to the caller: x1025 (a read of 200 bases over four families, 1025 regions a parent) came back with
    status -6 for both parents while that launch's workspace, RgC2rHL, held 1024 regions.  It holds one for every chain the last tier can
    export now; kx1152 is the same edge in a batch of kilobase reads."""
    run_all(env, optset="filter", which="declined")


# ------------------------------------------------------------------------------------------ which tier handed what on
HANDS_ON = re.compile(r"\[M::regions_batch\] (.+?) hands on: (\d+) for their intervals, (\d+) for their occurrences \(or a list too long\), (\d+) chains, "
                      r"(\d+) tied chain starts, (\d+) regions, (\d+) an interval to be walked further")
TIER_STORE = {"short": {"tier 1": "RgSmall", "tier 1b": "RgMid", "tier 1c": "RgMid2", "tier 2": "RgBig"},
              "long": {"tier 1b": "RgLongS", "tier 1c": "RgLongB"}}
COUNTING = ("tier 1b", "tier 1c")      # k_regions_mid counts what it hands on under phases=2; a tier without a line handed nothing on


def expected_hand_ons(rec, cs, store):
    """per reason, the recorded strand searches whose count exceeds that store's cap for it while fitting its other caps"""
    K = {k: i for i, k in enumerate(RC.COUNT_KEYS)}
    icap, scap, ccap, pcap = RC.STORES[store]
    n = {"intervals": 0, "occ": 0, "chains": 0, "tied": 0}
    for c in cs:
        if len(c["seq"]) > RC.DEFINES["RG_QCAP_LONG"]:
            continue
        for parent in (1, 0):
            x = rec.counts("default", c["name"], parent)
            over = {"intervals": x[K["intervals"]] > icap, "occ": x[K["occ"]] > scap, "chains": x[K["chains"]] > ccap or (pcap and x[K["records"]] > pcap)}
            for r in over:
                if over[r] and not any(over[o] for o in over if o != r):
                    n[r] += 1
            if x[K["tied"]] and not any(over.values()):
                n["tied"] += 1
    return n


def test_every_tier_hands_on_what_outgrows_it(env, tune, capfd):
    tune("phases", 2)
    for gname, max_occ, cs in groups():
        if gname == "over":
            continue
        capfd.readouterr()
        bad = run_group(env, "default", max_occ, cs)
        err = capfd.readouterr().err
        assert not bad, "\n".join(bad[:25])
        lines = {}
        for m in HANDS_ON.finditer(err):
            lines.setdefault(m.group(1), []).append([int(v) for v in m.groups()[1:]])
        print(gname, lines)
        assert "tier 3" not in lines and "tier 3 (exports)" not in lines, lines      # the last tier hands on nothing
        for tier, store in TIER_STORE[gname].items():
            if tier not in lines and tier not in COUNTING:
                continue
            got = [sum(v) for v in zip(*lines.get(tier, [[0] * 6]))]
            want = expected_hand_ons(env["rec"], cs, store)
            for reason, col in (("intervals", 0), ("occ", 1), ("chains", 2), ("tied", 3)):
                assert got[col] >= want[reason], (gname, tier, store, reason, got, want)
