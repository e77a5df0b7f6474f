"""-m gpu: the extensions' stopping rule (csrc/hip/ext_stop_rule.h, ext_stop.hpp) in every device form that applies it, through bsx_extend_batch
under the settings that pick the form -- ext4=1 (k_ext4<10> and <16>), ext4=2 (k_extl over the same jobs), ext4=4 (the wavefront forms of the
region kernels' inline extensions, packed 16-bit and, with ext_pk=0, 32-bit) -- with the switch ext_stop on and off, against the recorded
ksw_extend2 answers of the designed jobs (tests/ext_stop_cases.py: no reference is needed here); and at the regions level on a small genome:
region lists byte for byte the same with the switch on and off.  (ext4=3, ext_dp_win, runs every row: the rule is not built into it.)"""
import ctypes as C
import re
import numpy as np
import pytest
import ext_pk_cases as P
import ext_stop_cases as X
import simdata
import test_gpu_golden as G
from biscuit_amd.api import Device, EXT_DT, Index, SEED_DT, default_opt
from biscuit_amd import _lib as B

pytestmark = pytest.mark.gpu
FAM_EXT4, FAM_EXTL, FAM_TIER, FAM_C2R, FAM_WAVE = range(5)      # ext_stop.hpp


def stops(reset=False):
    """since the last reset: extensions stopped by the rule per launch family, those the rule would have stopped with the switch off, and the
    stops over all families"""
    c = (C.c_uint64 * 26)()
    B.check(B.lib().bsx_ext_stops(c, int(reset)), "bsx_ext_stops")
    return [int(c[5 * k]) for k in range(5)], [int(c[5 * k + 4]) for k in range(5)], int(c[25])


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """the designed jobs laid into a scratch genome, grouped by scoring set, with the recorded answers"""
    cases, want = X.load()
    tgt = np.concatenate([c[7] for c in cases]); toff = np.concatenate([[0], np.cumsum([len(c[7]) for c in cases])])
    qry = np.concatenate([c[6] for c in cases]); qoff = np.concatenate([[0], np.cumsum([len(c[6]) for c in cases])])
    idx, start = G._genome_of_targets(str(tmp_path_factory.mktemp("xs")), "xs", tgt, toff)
    assert (start >= 0).all()
    by_scoring = {}
    H = X.harness()
    for si in range(len(X.scorings())):
        a, b, gp, zd = X.scorings()[si]
        o = P.opt_of(a, b, gp, zd)
        ids = [k for k, c in enumerate(cases) if c[0] == si]
        jobs = np.zeros(len(ids), dtype=EXT_DT)
        fires = np.zeros(len(ids), bool)      # the scalar model of the rule (tests/host_ext_stop.cpp): the jobs it stops
        for j, k in enumerate(ids):
            _, fam, parent, w, eb, h0, q, t = cases[k]
            jobs[j] = (start[k], qoff[k], len(q), len(t), h0, w, eb, 1, 1, parent, 0)
            fires[j] = X.model(H, q, t, o.ctmat if parent else o.gamat, gp, w, eb, zd, h0, 1)[1][0] >= 0
        by_scoring[si] = (jobs, want[ids], fires)
    return idx, qry, by_scoring


@pytest.mark.parametrize("si", range(4))
def test_every_form_equals_the_recording_and_stops_the_same_jobs(designed, si, tune, capfd):
    idx, qry, by_scoring = designed
    jobs, want, fires = by_scoring[si]
    assert len(jobs) >= 200
    a, b, gp, zd = X.scorings()[si]
    dev = Device(0)
    try:
        dev.upload_index(idx)
        dev.set_reads(qry); dev.set_opt(P.opt_of(a, b, gp, zd))
        short = jobs["qlen"] <= 159      # k_ext4<10> takes a batch whose longest query fits ten slots
        counts = {}
        for on in (1, 0):
            tune("ext_stop", on)
            # (form, ext4, ext_pk, the jobs it gets, the family that counts it)
            for name, ext4, pk, sel, fam in (("k_ext4<10>", 1, 1, short, FAM_EXT4), ("k_ext4<16>", 1, 1, None, FAM_EXT4), ("k_extl", 2, 1, None, FAM_EXTL),
                                             ("wave packed", 4, 1, None, FAM_WAVE), ("wave 32-bit", 4, 0, None, FAM_WAVE)):
                tune("ext4", ext4); tune("ext_pk", pk)
                jj, ww = (jobs, want) if sel is None else (jobs[sel], want[sel])
                stops(reset=True)
                res = dev.extend(jj)
                got = np.stack([res[f] for f in X.FIELDS], 1)
                bad = np.nonzero((got != ww).any(1))[0]
                assert len(bad) == 0, (name, on, len(bad), jj[bad[:3]], got[bad[:3]], ww[bad[:3]])
                counts[name, on] = stops()
        print(counts)
        full = counts["k_ext4<16>", 1][0][FAM_EXT4]
        assert full == int(fires.sum()) and counts["k_ext4<10>", 1][0][FAM_EXT4] == int(fires[short].sum()) > 0, (counts, fires.sum())      # the model's jobs
        # the same jobs stop in every form that ran them all
        assert counts["wave packed", 1][0][FAM_WAVE] == full and counts["wave 32-bit", 1][0][FAM_WAVE] == full, counts
        # ext4=2: k_ext4 first (all jobs), then k_extl over the jobs it can hold -- it stops those, and no others
        assert counts["k_extl", 1][0][FAM_EXT4] == full and 0 < counts["k_extl", 1][0][FAM_EXTL] <= full, counts
        # k_extl exactly: of the jobs the model stops, it stops every one it holds -- a job it holds ends there, and only the rule ends these
        # early; the others it reports as left to k_ext4 (a band beyond its window, an ambiguous base)
        tune("ext_stop", 1); tune("ext4", 2); tune("ext_pk", 1)
        stops(reset=True); capfd.readouterr()
        res = dev.extend(jobs[fires])
        assert (np.stack([res[f] for f in X.FIELDS], 1) == want[fires]).all()
        left = re.findall(r"\[M::extl\] (\d+) jobs, (\d+) left to k_ext4", capfd.readouterr().err)
        assert len(left) == 1 and int(left[0][0]) == int(fires.sum()), left
        held = int(fires.sum()) - int(left[0][1])
        assert held > 0 and stops()[0][FAM_EXTL] == held, (stops(), left)
        # the switch off: nothing is stopped, and what would have been is what the switch on stopped, form by form
        for name in ("k_ext4<10>", "k_ext4<16>", "k_extl", "wave packed", "wave 32-bit"):
            assert counts[name, 0][2] == 0 and counts[name, 0][0] == [0] * 5, (name, counts)
            assert counts[name, 1][1] == [0] * 5 and counts[name, 0][1] == counts[name, 1][0], (name, counts)
    finally:
        dev.close()


def test_regions_are_the_same_with_the_switch_on_and_off(tmp_path, tune, capfd):
    """reads with indels against a genome with repeat families (the genome of tests/test_gpu_x4_unread.py's second test): the region lists
    with ext_stop on and off are the same bytes, and under phases the report counts stopped extensions"""
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
        outs, stopped = [], []
        for phases, on in ((0, 1), (0, 0), (1, 1), (1, 0)):
            tune("phases", phases); tune("ext_stop", on)
            stops(reset=True)
            capfd.readouterr()
            regs, roff, rn = dev.regions(opt, tasks)
            outs.append([regs[roff[t]:roff[t] + rn[t]].tobytes() if rn[t] >= 0 else int(rn[t]) for t in range(len(tasks))])
            dev.regions(opt, tasks[:2])      # (closes the report: what the side stream's strand searches add shows in the next one)
            err = capfd.readouterr().err
            stopped.append(stops()[2])
            if phases:
                assert ("ext_stop=%d k_ext4:" % on) in err, err[-2000:]
        assert outs[0] == outs[1] and outs[0] == outs[2] and outs[0] == outs[3]
        assert stopped[2] > 0, stopped            # counted under phases with the switch on
        assert stopped[0] == 0 and stopped[1] == 0 and stopped[3] == 0, stopped      # (without phases the region launches count nothing; off: none)
    finally:
        dev.close()
        idx.close()
