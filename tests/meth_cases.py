"""Shared by tests/test_meth_cpu.py (CPU suite) and tests/test_gpu_meth.py (-m gpu): a data set like bsconv_cases.make_data's (N runs, contigs
ending in C / starting with G, reads placed there) whose FASTQs carry varying qualities -- low runs at either end of many reads and scattered
low bases, so that the quality floor of 20 decides columns and strand inference -- plus planted pairs that make cytosines uncallable (a read of
the other bisulfite strand showing T over a reference C, and A over a reference G); the command lines run with --qc PREFIX --qc-meth; the
comparison of the file written with tests/meth_model.py over the SAM; and the check that the inputs exercise what the rule distinguishes."""
import os
import numpy as np
import simdata
import bsconv_cases as B
import meth_model as M
import qc_cases as QC
import qc_model as Q


def write_fastq(path, recs, seed):
    """qualities 30..40, a run of 2..19 over the first 1..12 bases of half the reads and over the last 1..12 of half, 3 % of the other bases
    low; reads whose name starts with `plant` keep quality 40 throughout"""
    r = np.random.default_rng(seed)
    with open(path, "wb") as f:
        for name, seq in recs:
            n = len(seq)
            q = r.integers(30, 41, n)
            low = r.random(n) < 0.03
            q[low] = r.integers(2, 20, int(low.sum()))
            if r.random() < 0.5:
                q[:int(r.integers(1, 13))] = r.integers(2, 20)
            if r.random() < 0.5:
                q[n - int(r.integers(1, 13)):] = r.integers(2, 20)
            if name.startswith("plant"):
                q[:] = 40
            f.write(b"@" + name.encode() + b"\n" + simdata.BASES[seq].tobytes() + b"\n+\n" + bytes((q + 33).astype(np.uint8)) + b"\n")


def _convert(x):
    y = x.copy()
    y[y == 1] = 3                                                             # every C read as T
    return y


def planted_pairs(contigs, read_len):
    """per spot a fragment of 400 bases without N: a pair of the forward bisulfite strand over it, every C converted, and pairs of the other
    strand whose fragment has T at one reference C (a substitution, not a conversion) -> at that C: conv 1, opp_alt 1 or 2, uncallable.  The
    same for a reference G from the mirrored construction."""
    out = []
    for ci, (_, g) in enumerate(contigs):
        for s in range(3000, len(g) - 1000, 9000):
            f = g[s:s + 400]
            if (f == 4).any():
                continue
            for base in (1, 2):
                at = [p for p in range(30, 120) if f[p] == base]
                if not at:
                    continue
                p = at[0]
                fm = f.copy()
                fm[p] = 3 if base == 1 else 0
                own, opp = (f, simdata.revcomp(fm)) if base == 1 else (simdata.revcomp(f), fm)     # the cytosine's own strand, the other one
                for k, frag in enumerate([own, opp, opp]):
                    conv = _convert(frag)
                    out.append(("plant%d_%d_%d_%d" % (ci, s, base, k), conv[:read_len].copy(), simdata.revcomp(conv)[:read_len].copy()))
    return out


def write_dup_set(d, contigs, n=120, read_len=150, seed=77):
    """d1.fq / d2.fq: per fragment a pair with every C converted and, right behind it, a pair of the same fragment and strand with about half of
    them retained -- a duplicate by position whose columns differ, so that a file made with the duplicates differs from one made without --
    and a hundred ordinary pairs"""
    r = np.random.default_rng(seed)
    ps = []
    while len(ps) < 2 * n:
        ci = int(r.integers(0, len(contigs)))
        g = contigs[ci][1]
        s = int(r.integers(0, len(g) - 400))
        f = g[s:s + 400]
        if (f == 4).any():
            continue
        if r.random() < 0.5:
            f = simdata.revcomp(f)
        half = f.copy()
        half[(f == 1) & (r.random(400) < 0.5)] = 3
        for tag, conv in (("x", _convert(f)), ("y", half)):
            ps.append(("dup%d%s" % (len(ps) // 2, tag), conv[:read_len].copy(), simdata.revcomp(conv)[:read_len].copy()))
    ps += simdata.make_pairs(contigs, 100, read_len, seed + 1, sub=0.01, indel=0.006, pbat_frac=0.3)
    write_fastq(d + "/d1.fq", [(n_, a) for n_, a, b in ps], seed + 2)
    write_fastq(d + "/d2.fq", [(n_, b) for n_, a, b in ps], seed + 3)


def make_data(d, genome_bp=150000, n_pairs=300, n_long=24, seed=31):
    from biscuit_amd.api import Index
    contigs = B.make_genome(genome_bp, seed)
    simdata.write_genome(d + "/g.fa", contigs)
    Index.build(d + "/g.fa", d + "/g").close()
    ps = simdata.make_pairs(contigs, n_pairs, 150, seed + 1, sub=0.01, indel=0.006, pbat_frac=0.3, chimera_frac=0.06, bad_mate_frac=0.06, n_frac=0.03)
    ps += B.edge_pairs(contigs, 150, seed + 2)
    ps += planted_pairs(contigs, 150)
    write_fastq(d + "/b1.fq", [(n, a) for n, a, b in ps], seed + 3)
    write_fastq(d + "/b2.fq", [(n, b) for n, a, b in ps], seed + 4)
    write_fastq(d + "/long.fq", simdata.make_single(contigs, n_long, 1000, seed + 6), seed + 5)
    write_dup_set(d, contigs)
    return contigs


def run_meth(exe, opts, args, d, prefix, env=None):
    """the command line with --qc PREFIX --qc-meth -> (SAM without @PG, the seven files of --qc, the text of the table or None)"""
    for s in [M.SUFFIX] + Q.SUFFIXES:
        if os.path.exists(prefix + s):
            os.remove(prefix + s)
    sam, err = B.run(exe, ["--qc", prefix, "--qc-meth"] + opts + args, d, env=env)
    return sam, QC.read_files(prefix), open(prefix + M.SUFFIX).read() if os.path.exists(prefix + M.SUFFIX) else None


def check_file(got, sam, refs, what):
    """the file written must be the model's over `sam`, byte for byte -> the model's (K, S, uncallable sites, seen)"""
    want, K, S, unc, seen = M.process(sam, refs)
    assert got == want, "%s:\n got: %r\nwant: %r\nK %s S %s" % (what, got, want, K, S)
    return K, S, unc, seen


def assert_not_vacuous(results, record_filters=("unmapped", "mapq", "improper"), also=("counted", "inferred", "reverse", "S", "I", "D")):
    """over all the runs of a test together, on the model's side: no column of some file is -1, an uncallable site, a column dropped by each
    column rule, a record dropped by each record filter the data can produce, the strand of some record inferred, reverse records, S / I / D"""
    assert any(min(K[:4]) >= 20 for K, S, unc, seen in results), [K for K, S, unc, seen in results]
    assert any(unc > 0 for K, S, unc, seen in results), "no uncallable site"
    tot = {k: sum(seen[k] for K, S, unc, seen in results) for k in results[0][3]}
    for k in ("lowq", "end5", "end3", "hole", "overlap"):
        assert tot[k] > 0, (k, tot)
    for k in record_filters:
        assert tot[k] > 0, (k, tot)
    for k in also:
        assert tot[k] > 0, (k, tot)
