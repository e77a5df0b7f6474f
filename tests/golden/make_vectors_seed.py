#!/usr/bin/env python3
"""Generates tests/golden/ref_seeds.npz: the interval lists the REAL reference makes of the designed strand searches of tests/seed_cases.py
-- mem_collect_intv's three passes (ref_collect.py) over the reference's own bwt_smem1a and bwt_seed_strategy1, through
oracle/_ref/libbiscuit_ref.so, on an index that this repository's builder wrote and the reference's bwt_restore_bwt / _sa read -- and what
the reference saw on the way (seed_cases.STAT_KEYS, and which pass-1 SMEMs pass 2 re-seeded), plus bwt_sa of the first min(x2, 50) ranks of
every recorded interval.

Every case is recorded for both parents under every option set of seed_cases.OPTSETS.  The file holds recorded results, counts and two
CRCs (genome, read buffer) only; a list equal to an earlier record's is stored as a reference to it.

    make -C oracle && python tests/golden/make_vectors_seed.py

prints the coverage table that tests/test_seed_recorded_cpu.py asserts from the file."""
import ctypes as C
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import oracle_lib  # noqa: E402
import seed_cases as SC  # noqa: E402
from ref_collect import collect_intv  # noqa: E402
from biscuit_amd.api import Index  # noqa: E402

R = oracle_lib.ref_lib()
assert R is not None, "oracle/_ref/libbiscuit_ref.so missing: run `make -C oracle`"
CAP = 8192      # entries of the buffer one bwt_smem1a call's list is copied to: more than the longest read has bases
LIMIT = 567348  # bytes: the largest fixture committed before this one (ref_vectors.npz)

d = tempfile.mkdtemp(prefix="bsx_seeds_")
SC.write_fasta(d + "/g.fa")
idx = Index.build(d + "/g.fa", d + "/g")
assert idx.l_pac == SC.l_pac()
idx.close()
H = {1: C.c_void_p(R.ref_bwt_load((d + "/g.par.bwt").encode(), (d + "/g.par.sa").encode())),
     0: C.c_void_p(R.ref_bwt_load((d + "/g.dau.bwt").encode(), (d + "/g.dau.sa").encode()))}

cases = SC.cases()
assert max(len(c["seq"]) for c in cases) < CAP
index_of = {c["name"]: i for i, c in enumerate(cases)}
rec, lists, resplit, resplit_len, resplit_x2 = [], [], [], [], []
for oi, (oname, _, _) in enumerate(SC.OPTSETS):
    o = SC.options(oname)
    for c in SC.optset_cases(oname):
        for parent in (1, 0):
            st = {}
            a = collect_intv(R, H, parent, SC.convert(c["seq"], parent), cap=CAP, stats=st, **o)
            for k in range(1, len(a)):      # records with equal info are identical: the order is defined
                assert a[k][3] != a[k - 1][3] or (a[k] == a[k - 1]).all(), (oname, c["name"], parent, k)
            p3 = st["pass3_x2"]
            rec.append((index_of[c["name"]], parent, oi, (len(a), st["pass1"], len(st["reseeded"]), st["pass3"], st["max_x2"], min(p3) if p3 else 0, max(p3 + [0]))))
            lists.append(a)
            resplit.append(np.array(st["reseeded"], np.int32))
            resplit_len += st["reseeded_len"]
            resplit_x2 += st["reseeded_x2"]

# a list equal to an earlier record's: stored once
same = np.full(len(rec), -1, np.int32)
seen = {}
for k, l in enumerate(lists):
    key = l.tobytes()
    if len(l) and key in seen:
        same[k] = seen[key]
    else:
        seen[key] = k
own = [lists[k] if same[k] < 0 else lists[k][:0] for k in range(len(rec))]
off = np.concatenate([[0], np.cumsum([len(l) for l in own])]).astype(np.int64)
roff = np.concatenate([[0], np.cumsum([len(l) for l in resplit])]).astype(np.int64)
alli = np.concatenate(own)

# bwt_sa of the ranks the chaining step would look up (capped like memchain.c:325), every rank once
sa = {}
for parent in (0, 1):
    ranks = set()
    for r_, l in zip(rec, lists):
        if r_[1] == parent and SC.OPTSETS[r_[2]][0] in SC.SA_OPTSETS:
            for x0, _, x2, _ in l:
                ranks.update(range(int(x0), int(x0) + min(int(x2), 50)))
    ranks = np.array(sorted(ranks), np.uint64)
    pos = np.zeros(len(ranks), np.uint64)
    R.ref_bwt_sa_batch(H[parent], C.c_int64(len(ranks)), ranks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p))
    sa[parent] = (ranks, pos)


def fits(a, dt):
    b = a.astype(dt)
    assert (b.astype(np.uint64) == a.astype(np.uint64)).all(), dt
    return b


out = {
    "genome_crc": np.uint32(SC.genome_crc()), "reads_crc": np.uint32(SC.reads_crc()),
    "names": np.array([c["name"] for c in cases]), "optsets": np.array([o[0] for o in SC.OPTSETS]),
    "rec_case": np.array([r_[0] for r_ in rec], np.int16), "rec_parent": np.array([r_[1] for r_ in rec], np.int8),
    "rec_opt": np.array([r_[2] for r_ in rec], np.int8), "rec_stat": np.array([r_[3] for r_ in rec], np.int32),
    "rec_same": same, "rec_off": off, "rec_roff": roff, "resplit": fits(np.concatenate(resplit), np.int16),
    "resplit_len": fits(np.array(resplit_len, np.int64), np.int16), "resplit_x2": fits(np.array(resplit_x2, np.int64), np.uint16),
    "x0": fits(alli[:, 0], np.uint32), "x1": fits(alli[:, 1], np.uint32), "x2": fits(alli[:, 2], np.uint32),
    "start": fits(alli[:, 3] >> np.uint64(32), np.uint16), "end": fits(alli[:, 3] & np.uint64(0xffffffff), np.uint16),
}
for parent in (0, 1):
    out["sa_rank_%d" % parent] = fits(sa[parent][0], np.uint32)
    out["sa_pos_%d" % parent] = fits(sa[parent][1], np.uint32)
path = os.path.join(HERE, "ref_seeds.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", len(rec), "strand searches,", sum(len(l) for l in lists), "intervals,", len(alli), "stored,",
      len(sa[0][0]) + len(sa[1][0]), "suffix-array positions")

# ------------------------------------------------------------------------------------------ the coverage table
rc = SC.load(path)
bad = 0
for edge, ok, what in SC.coverage(rc):
    print("%-4s %-34s %s" % ("ok" if ok else "MISS", edge, what))
    bad += not ok
print("case: parent 1 / parent 0 under the default option set (%s)" % ", ".join(SC.STAT_KEYS))
for c in cases:
    print("  %-12s len %4d  %s  %s" % (c["name"], len(c["seq"]), list(rc.stats("default", c["name"], 1).values()), list(rc.stats("default", c["name"], 0).values())))
assert not bad, "%d edges are not occupied" % bad
assert os.path.getsize(path) < LIMIT
