"""The counters of extensions made ahead that the seed loop never reads (ctr_layout.hpp: CTR_X4W; DESIGN.md section 4, "Extensions ahead:
what is never read").  Under `phases` k_extl and k_ext4 run in their tallying instantiations, which leave the rows of every job beside the
export pool, and rg_c2r counts the jobs whose seed -- the first one it reaches in a chain's main list -- it skips as contained.

What is checked: the tallying instantiations give the regions of the default ones (the recorded reference lists, and bit for bit on reads with
indels, whose chains split at the read's own locus); the counts obey what follows from the loop itself (a job is unread only where a seed was
skipped, no more jobs are unread than finished, the first region's share is a share); and the sums over both kernels do not depend on which
kernel ran a job (`xl=0`: every job through k_ext4 -- a job's rows are the rows of its ksw_extend2 calls, whichever kernel makes them)."""
import re
import numpy as np
import pytest

import regions_cases as RC
import simdata
from biscuit_amd.api import Index, Device, default_opt, SEED_DT
from test_gpu_regions_recorded import env, run_group, groups      # noqa: F401  (env: the recorded cases' genome on the device)

pytestmark = pytest.mark.gpu

UNREAD = re.compile(r"\[M::regions_batch\] (k_ext4|k_extl): unread jobs (\d+) with (\d+) rows \([0-9.]+% of the kernel's rows\) \| of which inside the strand "
                    r"search's first region: (\d+) jobs, (\d+) rows")
EXT4 = re.compile(r"\[M::regions_batch\] k_ext4: (\d+) jobs, (\d+) rows in")
EXTL = re.compile(r"\[M::regions_batch\] k_extl: (\d+) jobs \((\d+) sent on to k_ext4\), (\d+) rows in")
LOOPS = re.compile(r"\[M::regions_batch\] seed loops \(mem_chain2region1\): (\d+) seeds reached, (\d+) skipped as contained, (\d+) took the extension made ahead")


def tally(err):
    """the reports of one or more regions batches, summed"""
    t = {"k_ext4": np.zeros(4, np.int64), "k_extl": np.zeros(4, np.int64), "jobs4": 0, "rows4": 0, "jobsl": 0, "sent_on": 0, "rowsl": 0, "skipped": 0, "taken": 0}
    for m in UNREAD.finditer(err):
        t[m.group(1)] += np.array([int(v) for v in m.groups()[1:]], np.int64)
    for m in EXT4.finditer(err):
        t["jobs4"] += int(m.group(1)); t["rows4"] += int(m.group(2))
    for m in EXTL.finditer(err):
        t["jobsl"] += int(m.group(1)); t["sent_on"] += int(m.group(2)); t["rowsl"] += int(m.group(3))
    for m in LOOPS.finditer(err):
        t["skipped"] += int(m.group(2)); t["taken"] += int(m.group(3))
    return t


def check_counts(t):
    for k, jobs, rows in (("k_ext4", t["jobs4"], t["rows4"]), ("k_extl", t["jobsl"] - t["sent_on"], t["rowsl"])):
        n, r, n0, r0 = (int(v) for v in t[k])
        assert 0 <= n0 <= n <= jobs and 0 <= r0 <= r <= rows, (k, t)
        assert (r == 0 or n > 0) and (r0 == 0 or n0 > 0), (k, t)
    assert int(t["k_ext4"][0] + t["k_extl"][0]) <= t["skipped"], t      # unread only where the loop skipped a seed
    # no more jobs are unread than were finished (a job k_extl sent on is finished by k_ext4)
    assert t["jobs4"] + t["jobsl"] - t["sent_on"] >= int(t["k_ext4"][0] + t["k_extl"][0]), t


def test_recorded_cases_under_the_tallying_kernels(env, tune, capfd):
    """the recorded region lists, cases among two thousand ordinary strand searches, with the counters on; the counts are consistent, and their
    sums over the two kernels are those of `xl=0`"""
    tune("phases", 1)
    sums, figures = [], []
    for xl in (1, 0):
        tune("xl", xl)
        capfd.readouterr()
        bad = []
        for gname, max_occ, cs in groups():
            if gname != "long":      # (chunks of long reads export without extensions ahead)
                bad += run_group(env, "default", max_occ, cs, 1000 if gname == "short" else 100)
        # (a report is printed before the batch's strand searches that were seeded again finish on the side stream: what they add shows in the
        # next report, so a batch of two ordinary reads closes the sums)
        bad += run_group(env, "default", None, [], 2)
        err = capfd.readouterr().err
        assert not bad, "\n".join(bad[:25])
        t = tally(err)
        figures.append("xl=%d: %s" % (xl, t))
        assert t["jobs4"] > 0 and (xl == 0) == (t["jobsl"] == 0), t
        check_counts(t)
        sums.append(t["k_ext4"] + t["k_extl"])
    print("\n".join(figures))
    assert (sums[0] == sums[1]).all(), sums


def test_reads_with_indels_unread_jobs_counted_and_regions_unchanged(tmp_path, tune, capfd):
    """reads with indels against a genome with repeat families: a chain split at the read's own locus has its best seed inside the first chain's
    region, so unread jobs exist; the regions are those of the default kernels bit for bit, and the sums over the two kernels are those of
    `xl=0` (every job through k_ext4)"""
    contigs = simdata.make_genome(300000, seed=11, n_contigs=2, repeat_frac=0.3)
    simdata.write_genome(str(tmp_path / "g.fa"), contigs)
    idx = Index.build(str(tmp_path / "g.fa"), str(tmp_path / "g"))
    dev = Device(0)
    try:
        dev.upload_index(idx)
        seqs = [s for _, s in simdata.make_single(contigs, 1500, 150, seed=5, sub=0.02, indel=0.02)]
        buf, off = simdata.read_buffer(seqs)
        tasks = np.zeros(2 * len(seqs), SEED_DT)
        for i, s in enumerate(seqs):
            for k, parent in enumerate((1, 0)):
                tasks[2 * i + k] = (off[i], len(s), parent)
        opt = default_opt()
        dev.set_opt(opt)
        dev.set_reads(buf)
        figures = []
        outs, sums = [], []
        for phases, xl in ((0, 1), (1, 1), (1, 0)):
            tune("phases", phases)
            tune("xl", xl)
            capfd.readouterr()
            regs, roff, rn = dev.regions(opt, tasks)
            outs.append([regs[roff[t]:roff[t] + rn[t]].tobytes() if rn[t] >= 0 else int(rn[t]) for t in range(len(tasks))])
            dev.regions(opt, tasks[:2])      # (closes the sums: what the side stream's strand searches add shows in the next report)
            err = capfd.readouterr().err
            if phases:
                t = tally(err)
                figures.append("xl=%d: %s" % (xl, t))
                assert (xl == 0) == (t["jobsl"] == 0), t
                check_counts(t)
                sums.append(t["k_ext4"] + t["k_extl"])
        print("\n".join(figures))
        assert outs[0] == outs[1] and outs[0] == outs[2]
        assert sums[0][0] > 0 and sums[0][1] > 0, sums      # unread jobs exist, and they ran rows
        assert (sums[0] == sums[1]).all(), sums             # the same jobs, rows and first-region shares whichever kernel ran them
    finally:
        dev.close()
        idx.close()
