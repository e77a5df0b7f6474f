"""Shared by tests/test_cov_cpu.py (CPU suite) and tests/test_gpu_cov.py (-m gpu): the command lines run with --qc PREFIX --qc-cov, the GC BED
files made for bsconv_cases.make_data's genome, the comparison of the files written with tests/cov_model.py over the SAM, and the check that the
inputs exercise what the rule distinguishes."""
import gzip
import os
import bsconv_cases as B
import cov_model as V
import qc_cases as QC
import qc_model as Q


def write_beds(d, contigs):
    """top.bed (plain) and bot.bed.gz over the data set's contigs: overlapping intervals, one up to a contig's end, one over a contig's first
    bases, an empty one, extra columns, a comment, top and bottom overlapping each other -> (top path, bot path)"""
    names = [n for n, _ in contigs]
    lens = [len(g) for _, g in contigs]
    top = ["# top GC windows", "%s\t0\t1000\twin0\t0.7" % names[0], "%s\t500\t2500" % names[0], "%s\t%d\t%d" % (names[0], lens[0] - 777, lens[0]),
           "%s\t100\t100" % names[1], "%s 3000 20001 x" % names[1], ""]
    bot = ["track name=bot", "%s\t2000\t9000" % names[0], "%s\t0\t31" % names[-1], "%s\t31\t33" % names[-1], "%s\t%d\t%d" % (names[1], lens[1] // 2, lens[1] // 2 + 12345)]
    with open(d + "/top.bed", "w") as f:
        f.write("\n".join(top) + "\n")
    with gzip.open(d + "/bot.bed.gz", "wb") as f:
        f.write(("\n".join(bot) + "\n").encode())
    return d + "/top.bed", d + "/bot.bed.gz"


def read_files(prefix):
    return {s: open(prefix + s).read() for s in V.SUFFIXES if os.path.exists(prefix + s)}


def run_cov(exe, opts, args, d, prefix, env=None):
    """the command line with --qc PREFIX --qc-cov -> (SAM without @PG, the seven files of --qc, the coverage files)"""
    for s in V.SUFFIXES + Q.SUFFIXES:
        if os.path.exists(prefix + s):
            os.remove(prefix + s)
    sam, err = B.run(exe, ["--qc", prefix, "--qc-cov"] + opts + args, d, env=env)
    return sam, QC.read_files(prefix), read_files(prefix)


def check_files(got, sam, refs, top, bot, what):
    """the coverage files written must be the model's over `sam`, byte for byte -> the model's tables"""
    tabs = V.tables(sam, refs, None if top is None else V.read_bed(top), None if bot is None else V.read_bed(bot))
    want = V.files(tabs)
    assert sorted(got) == sorted(want) and len(want) == (13 if top else 5), (what, sorted(got))
    for s in want:
        assert got[s] == want[s], "%s: %s differs:\n got: %r\nwant: %r" % (what, s, got[s][:600], want[s][:600])
    return tabs


def assert_not_vacuous(all_tabs):
    """over all the tables of a test together: some depth >= 2, some CpG row, some q40 row that differs from its `all` row"""
    assert any(d >= 2 for tabs in all_tabs for d in tabs[0]), "no depth >= 2"
    assert any(d >= 1 and c > 0 for tabs in all_tabs for d, c in tabs[1].items()), "no covered CpG"
    assert any(tabs[2] != tabs[0] for tabs in all_tabs) and any(tabs[3] != tabs[1] for tabs in all_tabs), "q40 never differs from all"
    gc = [tabs for tabs in all_tabs if len(tabs) == 12]
    if gc:
        assert any(d >= 1 for tabs in gc for t in (4, 5, 8, 9) for d in tabs[t]), "nothing covered inside the masks"
