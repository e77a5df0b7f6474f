"""Shared by tests/test_markdup_cpu.py (CPU suite) and tests/test_gpu_markdup.py (-m gpu): the data of bsconv_cases.make_data (300 kbp genome,
3 000 pairs, 150 long reads) with templates added under new names at random places of the file, the command lines run with --markdup, and the
comparison with tests/markdup_model.py.

Added to b1.fq / b2.fq (-> m1.fq / m2.fq; mil.fq: the same interleaved, every fifth template a singleton; mlong.fq: the long reads, a third of
them twice):
  dx  exact copies of 300 pairs
  dc  copies of 150 pairs with the first 5-20 bases of read 1 replaced by random bases (the alignment soft-clips them: u5 must still match)
  du  two copies each of 60 pairs with read 2 replaced by an unalignable read (equal to each other, never to their original)
  ds  copies of 100 pairs with read 1 and read 2 exchanged (never equal to their original)
big1.fq / big2.fq: m1 / m2 twice, the second time under other names (-m gpu: enough units for several chunks of several slices).

Counts found on the CPU checker's SAM with these seeds (paired command line `-@ 4 g m1.fq m2.fq`; test_markdup_cpu.py asserts the bounds the
issue sets: at least 200 flagged, at least 20 of dx and of dc each, no ds equal to its original):
  3 872 templates, all 3 872 with a key, 475 flagged.  Added templates whose key equals their original's, the later of the two in the file
  being the one flagged: 298 of 300 dx, 117 of 150 dc, 0 of 100 ds; all 120 du equal their other copy (60 flagged) and none its original;
  99 of the 100 ds have both ends placed, like their original.  Single-end (m1.fq alone): 3 867 with a key, 537 flagged; interleaved:
  1 500 templates, 44 flagged."""
import re
import numpy as np
import simdata
import e2e_cases as E
import bsconv_cases as B
import markdup_model as M

N_EXACT, N_CLIP, N_UNAL, N_SWAP = 300, 150, 60, 100

CASES = [
    ("paired", ["-@", "4", "g", "m1.fq", "m2.fq"]),
    ("single_end", ["-@", "4", "g", "m1.fq"]),
    ("interleaved", ["-@", "4", "-p", "g", "mil.fq"]),
    ("secondary_M", ["-@", "4", "-M", "g", "m1.fq", "m2.fq"]),
    ("clipping", ["-@", "4", "-5", "3", "-3", "2", "-Y", "g", "m1.fq", "m2.fq"]),
    ("long_1kb", ["-@", "4", "g", "mlong.fq"]),
]


def _read_fastq(path):
    l = open(path).read().split("\n")
    return [(l[i][1:], l[i + 1], l[i + 3]) for i in range(0, len(l) - 3, 4)]


def _write_fastq(path, recs):
    with open(path, "w") as f:
        for n, s, q in recs:
            f.write("@%s\n%s\n+\n%s\n" % (n, s, q))


def make_data(d, seed=77):
    """-> (contigs, {added name: (kind, original name)})"""
    contigs = B.make_data(d, genome_bp=300000, n_pairs=3000, n_long=150)
    r1, r2 = _read_fastq(d + "/b1.fq"), _read_fastq(d + "/b2.fq")
    r = np.random.default_rng(seed)
    pick = r.permutation(3000)      # (the simulated pairs; the edge pairs behind them stay as they are)
    src = {"dx": pick[:N_EXACT], "dc": pick[N_EXACT:N_EXACT + N_CLIP], "du": pick[450:450 + N_UNAL], "ds": pick[510:510 + N_SWAP]}
    rnd = lambda n: "".join("ACGT"[int(x)] for x in r.integers(0, 4, n))
    added, origin = [], {}
    for kind in ("dx", "dc", "du", "ds"):
        for i in src[kind]:
            (n, s1, q1), (_, s2, q2) = r1[i], r2[i]
            for copy in range(2 if kind == "du" else 1):
                name = "%s%d_%s" % (kind, copy, n)
                if kind == "dc":
                    k = int(r.integers(5, 21))
                    rec = (name, rnd(k) + s1[k:], q1, s2, q2)
                elif kind == "du":
                    rec = (name, s1, q1, ("AC" * len(s2))[:len(s2)], q2)      # (no 19-mer of it is in a random genome)
                elif kind == "ds":
                    rec = (name, s2, q2, s1, q1)
                else:
                    rec = (name, s1, q1, s2, q2)
                added.append(rec)
                origin[name] = (kind, n)
    out = [(n, s1, q1, r2[i][1], r2[i][2]) for i, (n, s1, q1) in enumerate(r1)]
    for rec in added:
        out.insert(int(r.integers(0, len(out) + 1)), rec)
    _write_fastq(d + "/m1.fq", [(n, s1, q1) for n, s1, q1, s2, q2 in out])
    _write_fastq(d + "/m2.fq", [(n, s2, q2) for n, s1, q1, s2, q2 in out])
    il = []
    for i, (n, s1, q1, s2, q2) in enumerate(out[:1500]):
        il += [(n, s1, q1)] if i % 5 == 3 else [(n, s1, q1), (n, s2, q2)]
    _write_fastq(d + "/mil.fq", il)
    _write_fastq(d + "/big1.fq", [(n, s1, q1) for n, s1, q1, s2, q2 in out] + [("again_" + n, s1, q1) for n, s1, q1, s2, q2 in out])
    _write_fastq(d + "/big2.fq", [(n, s2, q2) for n, s1, q1, s2, q2 in out] + [("again_" + n, s2, q2) for n, s1, q1, s2, q2 in out])
    lg = _read_fastq(d + "/long.fq")
    for j in range(0, len(lg), 3):
        lg.insert(int(r.integers(0, len(lg) + 1)), ("dl_" + lg[j][0],) + lg[j][1:])
    _write_fastq(d + "/mlong.fq", lg)
    return contigs, origin


def stderr_counts(err):
    m = re.search(r"markdup: (\d+) templates, (\d+) with a placed end, (\d+) duplicates", err)
    assert m, err[-2000:]
    return tuple(int(x) for x in m.groups())


def check_against_model(plain, got, err, what):
    """`got` (a SAM written with --markdup) must be the model's rewrite of `plain` (the same command line without), and the counts on stderr the model's"""
    dups, want, n, n_keyed = M.process(plain)
    E.assert_same_sam(got.encode(), want.encode(), what)
    assert stderr_counts(err) == (n, n_keyed, len(dups)), (what, stderr_counts(err), (n, n_keyed, len(dups)))
    return dups


def by_kind(plain, dups, origin):
    """-> ({kind: added templates of that kind whose key equals their original's and of which the later one in the file is flagged}, swapped
    templates whose key equals their original's, swapped templates placed like their original)"""
    _, ts = M.templates(plain)
    key = {recs[0][0]: M.template_key(recs) for recs in ts}
    at = {recs[0][0]: i for i, recs in enumerate(ts)}
    n = {"dx": 0, "dc": 0, "du": 0, "ds": 0}
    for a, (kind, o) in origin.items():
        if kind == "du":      # equal to its other copy, never to the original (both of whose ends are placed)
            o = ("du1_" if a.startswith("du0_") else "du0_") + a[4:]
        if key[a] is not None and key[a] == key[o] and max(at[a], at[o]) in dups:
            n[kind] += 1
    sw = [(key.get(a), key.get(o)) for a, (kind, o) in origin.items() if kind == "ds"]
    both = lambda k: k is not None and k[0] is not None and k[1] is not None
    return n, sum(1 for a, o in sw if a is not None and a == o), sum(1 for a, o in sw if both(a) and both(o))
