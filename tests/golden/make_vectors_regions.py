#!/usr/bin/env python3
"""Generates tests/golden/ref_regions.npz: the region lists the REAL reference makes of the designed strand searches of
tests/regions_cases.py -- mem_chain, mem_chain_flt, mem_flt_chained_seeds and mem_chain2region (lib/aln/memchain.c; together the body of
mem_align1_core, bwamem.c:183-208) called through ref_regions of oracle/ref_shim.c over an index that this repository's builder wrote and
the reference's bwa_idx_load read -- and what the reference saw on the way (regions_cases.COUNT_KEYS): intervals, occurrences visited,
their sum under max_occ, chains before the filter, chains of several seeds, chains after it, whether two chains shared a start.

Every case is recorded for both parents under every option set of regions_cases.OPTSETS (a case's own max_occ applies in all of them).
The file holds recorded results, counts and two CRCs (genome, read buffer) only; a list equal to an earlier record's is stored as a
reference to it.

    make -C oracle && python tests/golden/make_vectors_regions.py

prints the coverage table (which case sits at which cap, on which side) that tests/test_regions_recorded_cpu.py asserts from the file."""
import ctypes as C
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import regions_cases as RC  # noqa: E402
from biscuit_amd.api import Index, default_opt  # noqa: E402

R = oracle_lib.ref_lib()
assert R is not None and hasattr(R, "ref_regions"), "oracle/_ref/libbiscuit_ref.so missing or old: run `make -C oracle`"
R.ref_idx_load.restype = C.c_void_p
R.ref_idx_load.argtypes = [C.c_char_p]
R.ref_idx_free.argtypes = [C.c_void_p]
R.ref_regions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
CAP = 4096

d = tempfile.mkdtemp(prefix="bsx_regions_")
RC.write_fasta(d + "/g.fa")
idx = Index.build(d + "/g.fa", d + "/g")
idx.close()
h = R.ref_idx_load((d + "/g").encode())
assert h, "the reference could not load the index"
dflt = default_opt()

cases = RC.cases()
rec, lists = [], []
for oi, (oname, oset) in enumerate(RC.OPTSETS):
    for ci, c in enumerate(cases):
        for parent in (1, 0):
            regs = np.zeros((CAP, 12), np.int64)
            cnt = np.zeros(10, np.int64)
            seq = c["seq"]
            n = R.ref_regions(h, len(seq), seq.ctypes.data_as(C.c_void_p), parent, oset.get("min_seed_len", dflt.min_seed_len),
                              oset.get("min_chain_weight", dflt.min_chain_weight), c["max_occ"] or dflt.max_occ,
                              regs.ctypes.data_as(C.c_void_p), CAP, cnt.ctypes.data_as(C.c_void_p))
            assert 0 <= n <= CAP and cnt[0] == n
            rec.append((ci, parent, oi, cnt))
            lists.append(regs[:n].copy())
R.ref_idx_free(h)

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
off = np.zeros(len(rec) + 1, np.int64)
for k, l in enumerate(own):
    off[k + 1] = off[k] + len(l)
allr = np.concatenate(own)


def fits(a, dt):
    b = a.astype(dt)
    assert (b.astype(np.int64) == a).all(), dt
    return b


out = {
    "genome_crc": np.uint32(RC.genome_crc()), "reads_crc": np.uint32(RC.reads_crc()),
    "names": np.array([c["name"] for c in cases]), "optsets": np.array([o[0] for o in RC.OPTSETS]),
    "rec_case": np.array([r[0] for r in rec], np.int16), "rec_parent": np.array([r[1] for r in rec], np.int8),
    "rec_opt": np.array([r[2] for r in rec], np.int8), "rec_cnt": np.array([r[3] for r in rec], np.int32),
    "rec_same": same, "rec_off": off,
    "rb": allr[:, 0], "rlen": fits(allr[:, 1] - allr[:, 0], np.int32), "qb": fits(allr[:, 2], np.int16), "qe": fits(allr[:, 3], np.int16),
    "rid": fits(allr[:, 4], np.int8), "score": fits(allr[:, 5], np.int16), "truesc": fits(allr[:, 6], np.int16), "w": fits(allr[:, 7], np.int16),
    "seedcov": fits(allr[:, 8], np.int16), "seedlen0": fits(allr[:, 9], np.int16), "frac_rep": fits(allr[:, 10], np.uint32), "bss": fits(allr[:, 11], np.uint8),
}
path = os.path.join(HERE, "ref_regions.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", len(rec), "strand searches,", sum(len(l) for l in lists), "regions,", len(allr), "stored")
assert os.path.getsize(path) <= 567348

# ------------------------------------------------------------------------------------------ the coverage table
rc = RC.load(path)
print("%-10s %-8s %5s | %-8s %s | %-8s %s" % ("store", "count", "cap", "at", "parent 1, 0", "past", "parent 1, 0"))
for store, dim, at, past in RC.EDGES:
    k = RC.COUNT_KEYS.index(dim)
    a = [int(rc.counts("default", at, p)[k]) for p in (1, 0)]
    b = [int(rc.counts("default", past, p)[k]) for p in (1, 0)]
    print("%-10s %-8s %5d | %-8s %-11s | %-8s %s" % (store, dim, RC.edge_cap(store, dim), at, a, past, b))
print("case: parent 1 / parent 0 counts under the default option set (%s)" % ", ".join(RC.COUNT_KEYS))
for c in cases:
    print("  %-10s len %4d  %s  %s" % (c["name"], len(c["seq"]), list(map(int, rc.counts("default", c["name"], 1))), list(map(int, rc.counts("default", c["name"], 0)))))
