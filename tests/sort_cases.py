"""Shared by tests/test_sort_cpu.py (CPU suite) and tests/test_gpu_sort.py (-m gpu): the data of markdup_cases.make_data with N_STAR pairs added
whose reads both align nowhere (records with RNAME '*': the simulated data has none), the same genome under contig names whose name order is not
their index order (g2), two -H files, and the comparison of a `--sort` run with tests/sort_model.py's rewrite of the plain run of the same command
line.  Every run uses BSX_CHUNK_SIZE=40000 (x 4 threads: about 530 pairs a chunk), so that equal keys meet across chunks.

Counts found on the CPU checker's SAM with these seeds (test_sort_cpu.py asserts the bounds the issue sets), paired command line: 7 874 records in
8 chunks, 1 364 groups of equal keys (1 010 of them with members in different chunks), 176 unmapped records at their mate's position, 104
positions holding both strands, 80 records with RNAME '*'."""
import re
import numpy as np
import simdata
import bsconv_cases as B
import markdup_cases as MC
import sort_model as S

N_STAR = 40
CASES = MC.CASES
ENV = {"BSX_CHUNK_SIZE": "40000"}
NAMES2 = ["zeta", "alpha", "mid"]      # index order; name order: alpha, mid, zeta


def make_data(d, seed=91):
    contigs, origin = MC.make_data(d)
    junk = lambda n, a, b: ((a + b) * n)[:n]      # (no 19-mer of these two-letter repeats is in a random genome, under either conversion)
    for fq, both in (("m1.fq", 1), ("m2.fq", 1), ("mil.fq", 2)):
        recs = MC._read_fastq(d + "/" + fq)
        r2 = np.random.default_rng(seed + 1)      # the same places in m1 and m2
        for k in range(N_STAR):
            at = int(r2.integers(0, len(recs) // both + 1)) * both
            if fq == "mil.fq":      # between templates (a template is one record or two with one name)
                while 0 < at < len(recs) and recs[at][0] == recs[at - 1][0]:
                    at += 1
            l = len(recs[0][1])
            new = [("star%d" % k, junk(l, "A", "C") if fq != "m2.fq" else junk(l, "G", "T"), "I" * l)]
            if fq == "mil.fq":
                new.append(("star%d" % k, junk(l, "G", "T"), "I" * l))
            recs[at:at] = new
        MC._write_fastq(d + "/" + fq, recs)
    # the same genome, contigs renamed
    assert len(contigs) == len(NAMES2)
    simdata.write_genome(d + "/g2.fa", [(n, g) for n, (_, g) in zip(NAMES2, contigs)])
    from biscuit_amd.api import Index
    Index.build(d + "/g2.fa", d + "/g2").close()
    sq = ["@SQ\tSN:%s\tLN:%d" % (n, len(g)) for n, g in contigs]
    open(d + "/hdr_rev.txt", "w").write("\n".join(sq[::-1]) + "\n")
    open(d + "/hdr_hd.txt", "w").write("\n".join([sq[1], "@CO\tbefore", "@HD\tVN:1.5\tSO:unsorted\tGO:none", sq[0], sq[2], "@CO\tafter"]) + "\n")
    return contigs, origin


def run_pair(exe, opts, args, d, env=None, sort_opts=("--sort",)):
    """the command line without and with --sort -> (plain SAM, sorted SAM, stderr of the sorted run)"""
    e = dict(ENV)
    e.update(env or {})
    plain, _ = B.run(exe, list(opts) + list(args), d, env=e)
    got, err = B.run(exe, list(sort_opts) + ["-v", "3"] + list(opts) + list(args), d, env=e)
    return plain, got, err


def chunk_reads(err):
    """reads of every chunk, from the lines the command line prints at -v 3"""
    return [int(x) for x in re.findall(r"\[M::process\] read (\d+) sequences", err)]


def sort_counts(err):
    m = re.search(r"\[M::main_align\] sort: (\d+) runs, (\d+) records", err)
    assert m, err[-2000:]
    return int(m.group(1)), int(m.group(2))


def check_against_model(plain, got, what):
    want = S.process(plain)
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        i = next(i for i in range(min(len(g), len(w))) if g[i] != w[i])
        raise AssertionError("%s: line %d differs\n got: %s\nwant: %s" % (what, i, g[i][:300], w[i][:300]))


def census(plain, chunks):
    """what the data holds, on the plain SAM: (records, tie groups, tie groups over several chunks, unmapped at a mate's position, positions with
    both strands, records with RNAME '*').  chunks: reads per chunk of the run, chunk_reads() (the records of a read stay in its chunk)."""
    ends = np.cumsum(chunks)
    h, body = S.split(plain)
    rk = S.ranks(h)
    groups, order, chunk_of = {}, {}, []
    for l in body:
        f = l.split("\t")
        rid = (f[0], int(f[1]) & 0xc0)
        if rid not in order:
            order[rid] = len(order)
        chunk_of.append(int(np.searchsorted(ends, order[rid], side="right")))
    for i, l in enumerate(body):
        groups.setdefault(S.key(l, rk), []).append(chunk_of[i])
    ties = [g for g in groups.values() if len(g) > 1]
    unm = sum(1 for l in body if int(l.split("\t")[1]) & 4 and l.split("\t")[2] != "*")
    pos = {}
    for k in groups:
        if k[0] != S.NO_RANK:
            pos.setdefault(k[:2], set()).add(k[2])
    return (len(body), len(ties), sum(1 for g in ties if len(set(g)) > 1), unm, sum(1 for v in pos.values() if len(v) == 2),
            sum(1 for l in body if l.split("\t")[2] == "*"))
