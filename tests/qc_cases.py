"""Shared by tests/test_qc_cpu.py (CPU suite) and tests/test_gpu_qc.py (-m gpu): the command lines run with --qc, the comparison of the files
written with tests/qc_model.py over the SAM, and the check that the inputs exercise what the rule distinguishes.  The data set is
bsconv_cases.make_data (N runs, contigs ending in C / starting with G, reads placed there).  Beside the cases the issue names, pe150_b1 (reads
of both bisulfite strands searched against one parent) is what puts records whose YD disagrees with their own conversions into the input."""
import os
import e2e_cases as E
import bsconv_cases as B
import qc_model as Q

CASES = ["pe150_b0", "se150", "long_1kb", "pe150_b1"]


def reads_of(d, args):
    """({(name, FLAG & 0xc0): read as sequenced}, paired) for a command line of e2e_cases"""
    fq = [a for a in args if a.endswith(".fq")]
    reads = {}
    for i, f in enumerate(fq):
        reads.update(Q.read_fastq(os.path.join(d, f), (0x40 if i == 0 else 0x80) if len(fq) == 2 else 0))
    return reads, len(fq) == 2


def read_files(prefix):
    return {s: open(prefix + s).read() for s in Q.SUFFIXES if os.path.exists(prefix + s)}


def run_qc(exe, opts, args, d, prefix, env=None):
    """the command line with --qc PREFIX -> (SAM without @PG, the files written)"""
    for s in Q.SUFFIXES:
        if os.path.exists(prefix + s):
            os.remove(prefix + s)
    sam, err = B.run(exe, ["--qc", prefix] + opts + args, d, env=env)
    return sam, read_files(prefix)


def check_files(got, sam, refs, reads, paired, what):
    """the files written must be the model's over `sam`, byte for byte -> the model's counters"""
    c = Q.process(sam, refs, reads)
    want = Q.files(c, paired)
    assert sorted(got) == sorted(want), (what, sorted(got))
    for s in want:
        assert got[s] == want[s], "%s: %s differs:\n got: %r\nwant: %r" % (what, s, got[s][:600], want[s][:600])
    return c


def assert_not_vacuous(counters):
    """over all the SAMs of a test together: the model itself must have met everything the rule distinguishes"""
    seen = {k: sum(c.seen[k] for c in counters) for k in counters[0].seen}
    for k in ("reverse", "read2", "yd_u", "below40", "q40", "S", "I", "D", "H", "pos_gt150"):
        assert seen[k] > 0, (k, seen)
    for k in range(2):              # both tables, converted and retained
        for s in range(2):
            assert sum(c.readpos[k][i][j][s] for c in counters for i in range(2) for j in range(Q.READ_LEN)) > 0, (k, s)
    off = {i for c in counters for i, v in enumerate(c.confusion) if v and i // 4 != i % 4}
    assert len(off) >= 2, off
