#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_ssw.npz: ksw_align2 inputs and the REAL reference's outputs at the shapes of the seed-SW filter
(mem_seed_sw, memchain.c:501-535): windows of up to 199 x 199, 16-bit mode, xtra = KSW_XSTART alone -- what k_swl16 (k_seedsw.hip: sixteen
jobs to a wavefront in packed 16-bit) and the 32-bit alignment of a seed without room in the job list have to score.  Same entry points and
array layout as make_vectors.py / make_vectors_long.py, under the key prefix ssw_, plus ssw_fam (a family id per vector, names in ssw_fams).

Targets are N-free and non-empty (the GPU tests lay them into a scratch genome): no vector is ever left out.

    make -C oracle && python tests/golden/make_vectors_ssw.py

prints the per-family counts that tests/ssw_cases.py holds as constants."""
import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import sw_model  # noqa: E402

R = oracle_lib.ref_lib()
assert R is not None, "oracle/_ref/libbiscuit_ref.so missing: run `make -C oracle`"
u8p, i8p = C.POINTER(C.c_uint8), C.POINTER(C.c_int8)
rng = np.random.default_rng(20261019)
XSTART = 0x80000

# scoring option sets: (a, b, (o_del, e_del, o_ins, e_ins)).  0..5: the gap settings of the other two files and their mirrors (insertions the
# cheaper side), 3 and 4 with gaps so cheap against b = 20 that adjacent gaps beat a mismatch; 6, 7: match scores that take 199 columns past
# 2^14; 8..10: the largest option sets ssw16_exact (ssw16_bound.h) admits -- 199 mx + 175 e + 2 oe + bias = 32767, 32766, 32766 -- with the
# matrix at the extremes of int8 (8), the gap extension (9) and the gap open (10) as large as the rest allows; mismatches cost as much as a
# match gives or more, so that a path that avoids a long gap by running on through unrelated bases loses
SC = [(1, 2, (6, 1, 6, 1)), (1, 4, (5, 2, 7, 1)), (2, 9, (2, 1, 3, 1)), (1, 20, (1, 1, 1, 1)), (2, 20, (3, 1, 2, 1)), (4, 20, (7, 1, 5, 2)),
      (127, 4, (6, 1, 6, 1)), (90, 20, (2, 1, 3, 1)),
      (127, 128, (1028, 30, 1028, 30)), (100, 100, (73, 10, 11, 72)), (127, 128, (3594, 1, 3594, 1))]
GUARD = (8, 9, 10)
# the nearest option sets the rule refuses: one more on the term each of 8..10 pushes
REFUSED = [(127, 128, (1029, 30, 1029, 30)), (100, 100, (73, 10, 11, 73)), (127, 128, (3595, 1, 3595, 1))]
ALL_SC = SC + REFUSED


def guard_lhs(a, b, gp):
    bias = max(b, 1)      # the matrices' most negative entry: -b, or the -1 of an N
    return 199 * a + 175 * max(gp[1], gp[3]) + 2 * max(gp[0] + gp[1], gp[2] + gp[3]) + bias


for s in GUARD:
    assert 32768 - 100 <= guard_lhs(*SC[s]) < 32768, (s, guard_lhs(*SC[s]))
for s in REFUSED:
    assert 32768 <= guard_lhs(*s) <= 32768 + 200, (s, guard_lhs(*s))

FAMS = ["stripes", "long_short", "score_low", "score_mid", "score_high", "ins_cross", "del_cross", "adjacent_gaps", "query_n", "guard", "guard_ins", "refused", "refused_ins"]


def P(a, t):
    return a.ctypes.data_as(t)


def mat(which, a, b):
    m = np.zeros(25, np.int8)
    R.ref_fill_scmat(which, a, b, P(m, i8p))
    return m


def ragged(lst, dt):
    off = np.zeros(len(lst) + 1, np.int64)
    for i, x in enumerate(lst):
        off[i + 1] = off[i] + len(x)
    return np.concatenate(lst).astype(dt), off


def bases(n):
    return rng.integers(0, 4, n).astype(np.uint8)


def subst(seq, p):
    s = seq.copy()
    hit = rng.random(len(s)) < p
    s[hit] = rng.integers(0, 4, int(hit.sum()))
    return s


def convert(q, which):
    """half of the read's C (which = 1) or G (2) as bisulfite conversion leaves them: T / A, which the strand's matrix scores as matches"""
    q = q.copy()
    hit = (q == (1 if which == 1 else 2)) & (rng.random(len(q)) < 0.5)
    q[hit] = 3 if which == 1 else 0
    return q


vec, n_which = [], [0]


def next_which():
    n_which[0] += 1
    return 1 + n_which[0] % 2


def rec(fam, si, q, t, which=None, need=None):
    """one recorded vector; need = "ins" / "del": the plain model must score lower with that kind of gap forbidden"""
    which = next_which() if which is None else which
    a, b, gp = ALL_SC[si]
    q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
    assert 1 <= len(q) <= 199 and 1 <= len(t) <= 199 and (t < 4).all() and (q < 5).all()
    m = mat(which, a, b)
    o = (C.c_int * 7)()
    q1, t1 = q.copy(), t.copy()
    R.ref_ksw_align2(len(q1), P(q1, u8p), len(t1), P(t1, u8p), P(m, i8p), gp[0], gp[1], gp[2], gp[3], XSTART, o)
    assert (q1 == q).all() and (t1 == t).all()
    assert sw_model.sw_score(q, t, m, *gp) == o[0], (fam, si, len(q), len(t), o[0])
    if need:
        lower = sw_model.sw_score(q, t, m, *gp, insertions=need != "ins", deletions=need != "del")
        if lower >= o[0]:
            return None
    vec.append((q, t, [a, b, which] + list(gp) + [XSTART], list(o), FAMS.index(fam), si))
    return o[0]


def pair(qlen, tlen, sub, which):
    """a query and a target that share min(qlen, tlen) bases, the shorter somewhere inside the longer"""
    if tlen >= qlen:
        t = bases(tlen)
        at = int(rng.integers(0, tlen - qlen + 1))
        q = subst(t[at:at + qlen], sub)
    else:
        q = bases(qlen)
        at = int(rng.integers(0, qlen - tlen + 1))
        t = q[at:at + tlen].copy()
        q = subst(q, sub)
    return convert(q, which), t


def tlen_free(lo, hi):
    while True:
        n = int(rng.integers(lo, hi + 1))
        if n % 8:
            return n


# ------------------------------------------------------------------------------------------ stripe counts
QLENS = sorted({1, 2, 7, 193, 199} | {8 * m + d for m in range(1, 25) for d in (-1, 0, 1)})
assert {(n + 7) // 8 for n in QLENS} == set(range(1, 26))
TEDGE = [1, 7, 8, 9, 15, 16, 17, 199]
for k, qlen in enumerate(QLENS):
    for j, tlen in enumerate((TEDGE[k % 8], tlen_free(max(1, qlen - 20), min(199, qlen + 30)))):
        w = next_which()
        q, t = pair(qlen, tlen, float(rng.choice([0, 0.03, 0.1])), w)
        rec("stripes", (2 * k + j) % 6, q, t, w)

# ------------------------------------------------------------------------------------------ the longest beside the shortest
for si in (0, 1, 6):
    for k in range(8):
        w = next_which()
        q, t = pair(199, 199, 0.02, w)
        rec("long_short", si, q, t, w)
        q = bases(1 + k)
        rec("long_short", si, q, q[k // 2:k // 2 + 1], w)

# ------------------------------------------------------------------------------------------ score range
for si in (6, 7):
    a = SC[si][0]
    for k in range(14):      # at or above 2^14: 199 matching columns, or nearly
        w = next_which()
        q, t = pair(199, 199, 0.0 if k % 3 else 0.01, w)
        s = rec("score_high", si, q, t, w)
        assert s >= 16384, (si, s)
    for k in range(14):      # below 256: one or two columns
        w = next_which()
        q, t = pair(1 + (k % 2 if 2 * a < 256 else 0), (1, 2, 9, 60, 199, 17, 33)[k % 7], 0.0, w)
        s = rec("score_low", si, q, t, w)
        assert s < 256, (si, s)
    for k in range(14):
        w = next_which()
        q, t = pair(int(rng.integers(4, 120)), tlen_free(4, 199), 0.02, w)
        s = rec("score_mid", si, q, t, w)
        assert 256 <= s < 16384, (si, s)

# ------------------------------------------------------------------------------------------ gaps that cross lanes
n_fallback = 0


def gap_job(fam, si, qlen, run, boundary, kind):
    """kind "ins": the query carries a run of `run` bases the target lacks, laid across column `boundary` (a lane's first column under the
    query's own stripe count); "del": the target carries it, at that column of the query"""
    global n_fallback
    lo, hi = 6, qlen - (run if kind == "ins" else 0) - 6
    start = min(max(boundary - run // 2 if kind == "ins" else boundary, lo), hi)
    if kind == "ins":
        assert start <= boundary < start + run, (qlen, run, boundary, start)
        q = bases(qlen)
        t = np.concatenate([q[:start], q[start + run:]])
    else:
        q = bases(qlen)
        t = np.concatenate([q[:start], bases(run), q[start:]])
    for s in (si, 6):      # where the flanks are too short for the gap to pay under these options: a = 127 against a gap of 6 + run
        if rec(fam, s, q, t, need=kind) is not None:
            n_fallback += s != si
            return
    raise AssertionError((fam, si, qlen, run, boundary, kind))


INS_SETS = [6, 7, 2, 5, 4]
n = 0
for qlen, runs in ((199, (1, 2, 24, 25, 26, 49, 50, 51, 60, 75)), (121, (1, 15, 16, 17, 32, 33, 40)), (64, (1, 8, 9, 16, 17, 24))):
    slen = (qlen + 7) // 8
    assert max(runs) > 2 * slen
    for run in runs:
        for k in (1, 4, 7):
            gap_job("ins_cross", INS_SETS[n % 5], qlen, run, k * slen, "ins")
            n += 1
for tlen, runs in ((199, (1, 25, 51, 75)), (121, (16, 33)), (64, (9, 17))):
    for run in runs:
        qlen = tlen - run
        slen = (qlen + 7) // 8
        for k in (1, 4, 7):
            gap_job("del_cross", INS_SETS[n % 5], qlen, run, k * slen, "del")
            n += 1

# ------------------------------------------------------------------------------------------ adjacent gaps instead of a mismatch
n_adj = 0
for k in range(36):
    si = (3, 4, 7)[k % 3]
    qlen = int(rng.integers(30, 200))
    w = next_which()
    t = bases(qlen)
    q = t.copy()
    for at in rng.choice(np.arange(5, qlen - 5), max(1, qlen // 15), replace=False):
        q[at] = (t[at] + 1) % 4      # (never a conversion the strand's matrix tolerates: those are C>T and G>A, + 2)
    a, b, gp = SC[si]
    m = mat(w, a, b)
    both = sw_model.sw_score(q, t, m, *gp)
    n_adj += both > max(sw_model.sw_score(q, t, m, *gp, insertions=False), sw_model.sw_score(q, t, m, *gp, deletions=False))
    rec("adjacent_gaps", si, q, t, w)
assert n_adj >= 24, n_adj      # the best path needs both kinds of gap

# ------------------------------------------------------------------------------------------ N in the query
for qlen in (199, 100, 33):
    slen = (qlen + 7) // 8
    for at in (0, qlen - 1, slen, 3 * slen, 7 * slen):
        if at >= qlen:
            at = (qlen - 1) // slen * slen      # the last lane's first column
        for w in (1, 2):
            q, t = pair(qlen, tlen_free(qlen, 199) if qlen < 199 else 199, 0.02, w)
            q[at] = 4
            rec("query_n", (0, 1, 2, 6)[(at + w) % 4], q, t, w)

# ------------------------------------------------------------------------------------------ at the guard, and just beyond it
# (the refused sets first: the file's last vector, whose target the layouts of tests/ssw_cases.py put at a strand's end, is one both forms score)
GUARD_INS_MIN = 8      # per option set: insertion jobs of 199 columns whose gap pays, the run across a lane's first column
n_guard_ins = {}
for fam, sets in (("refused", [len(SC) + k for k in range(len(REFUSED))]), ("guard", list(GUARD))):
    for si in sets:
        a, b, gp = ALL_SC[si]
        for w in (1, 2):
            q, t = pair(199, 199, 0.0, w)
            s = rec(fam, si, q, t, w)
            assert s == 199 * a
        # the long insertions: flanks long enough that the gap pays under these options (a flank of f matching columns is worth f a, the gap
        # costs o_ins + run e_ins), the run laid across column 25 k wherever such flanks leave room for that
        for run in (25, 51, 60):
            fmin = (gp[2] + run * gp[3]) // a + 6
            for k in (1, 2, 4, 6, 7):
                start = min(max(k * 25 - run // 2, fmin), 199 - run - fmin)
                if not start <= k * 25 < start + run:
                    continue
                q = bases(199)
                t = np.concatenate([q[:start], q[start + run:]])
                assert rec(fam + "_ins", si, q, t, need="ins") is not None, (si, run, k, start)
                n_guard_ins[si] = n_guard_ins.get(si, 0) + 1
        assert n_guard_ins[si] >= GUARD_INS_MIN, (si, n_guard_ins)
        for run in (25, 51):
            q = bases(199 - run)
            t = np.concatenate([q[:70], bases(run), q[70:]])
            assert rec(fam, si, q, t, need="del") is not None, (si, run)
        for k in range(10):
            w = next_which()
            q, t = pair(QLENS[int(rng.integers(0, len(QLENS)))], tlen_free(1, 199), 0.03, w)
            rec(fam, si, q, t, w)
if len(vec) % 2 == 0:      # an odd count: the last target lies on the forward strand in the first layout, on the reverse strand in the second
    q, t = pair(199, 199, 0.02, 1)
    rec("guard", GUARD[-1], q, t, 1)
assert len(vec) % 2 == 1 and vec[-1][5] in GUARD and vec[0][5] < len(SC)

out = {}
out["ssw_q"], out["ssw_qoff"] = ragged([e[0] for e in vec], np.uint8)
out["ssw_t"], out["ssw_toff"] = ragged([e[1] for e in vec], np.uint8)
out["ssw_par"] = np.array([e[2] for e in vec], np.int32)
out["ssw_out"] = np.array([e[3] for e in vec], np.int32)
out["ssw_fam"] = np.array([e[4] for e in vec], np.int32)
out["ssw_fams"] = np.array(FAMS)
path = os.path.join(HERE, "ref_vectors_ssw.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes,", len(vec), "vectors")
assert os.path.getsize(path) < 600 * 1000

# ------------------------------------------------------------------------------------------ the counts the tests hold as constants
fam = out["ssw_fam"]
print("FAMILY_COUNTS =", {f: int((fam == i).sum()) for i, f in enumerate(FAMS)})
sc = out["ssw_out"][:, 0]
def classes(s):
    return {"low": int((s < 256).sum()), "mid": int(((s >= 256) & (s < 16384)).sum()), "high": int((s >= 16384).sum())}


print("SCORE_CLASSES =", classes(sc))
print("SCORE_CLASSES_ADMITTED =", classes(sc[np.array([e[5] < len(SC) for e in vec])]))      # without the refused option sets
print("GUARD_INS (per option set, refused ones last) =", [n_guard_ins[s] for s in sorted(n_guard_ins)], ">=", GUARD_INS_MIN)
print("OPTION_SETS =", len({tuple(p[:2]) + tuple(p[3:7]) for p in out["ssw_par"].tolist()}), "| gap jobs moved to a = 127:", n_fallback,
      "| adjacent gaps needed:", n_adj, "| stripe counts:", len({(len(e[0]) + 7) // 8 for e in vec}))
