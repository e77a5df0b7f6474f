"""Designed ksw_extend2 jobs for the extensions' stopping rule (biscuit_amd/csrc/hip/ext_stop_rule.h), shared by its CPU and GPU tests, and
the recorded answers (tests/golden/ext_stop.npz, written by tests/golden/make_vectors_ext_stop.py from the reference's own ksw_extend2).

An extension that has reached the end of its query goes on for as many rows as its score takes to decay; the rule ends it on the first row
after which no result field can change.  The families plant what decides that row -- a clean run to the end, a peak before the end, an end
never reached, a later row that ties the to-the-end score and moves gtle, a first column that holds the largest potential, an ambiguous base,
a z-drop that fires first -- at the query lengths on the kernels' seams: k_ext4's 16-column slots and its 10 / 16 slot limit (159 / 160),
columns 64 and 128 of the wavefront forms, k_extl's window."""
import ctypes as C
import os
import subprocess
import numpy as np
from biscuit_amd.api import default_opt
import ext_pk_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_stop.npz")
QLENS = (1, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 255)
FAMILIES = ("clean", "peak", "never", "tie", "first_col", "n_in_query", "zdrop_first", "indel")
FIELDS = ("score", "qle", "tle", "gtle", "gscore", "max_off")


def scorings():
    """the scoring sets of ext_pk_cases (unequal gap penalties, a = 2, a z-drop of 12) and the defaults"""
    o = default_opt()
    return tuple(P.SCORINGS) + ((int(o.a), int(o.b), (int(o.o_del), int(o.e_del), int(o.o_ins), int(o.e_ins)), int(o.zdrop)),)


def harness():
    """tests/host_ext_stop.cpp: the scalar model of the loop with the rule (the rule is the kernels' own header)"""
    so = os.path.join(ROOT, "tests", "_build", "libhostextstop.so")
    src = os.path.join(ROOT, "tests", "host_ext_stop.cpp")
    deps = [src, os.path.join(ROOT, "biscuit_amd", "csrc", "hip", "ext_stop_rule.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + ROOT + "/biscuit_amd/csrc/hip", src, "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def model(H, q, t, mat, gp, w, eb, zd, h0, obey):
    """(the six fields, [fire row, rows run, rows on which PHI grew, rows with an H above an earlier PHI, evaluations, row that first reached the end, ties, last tying row])"""
    out, info = (C.c_int * 6)(), (C.c_int * 8)()
    rc = H.host_ext_stop(C.c_int(len(q)), _p(q), C.c_int(len(t)), _p(t), mat, C.c_int(gp[0]), C.c_int(gp[1]), C.c_int(gp[2]), C.c_int(gp[3]),
                         C.c_int(w), C.c_int(eb), C.c_int(zd), C.c_int(h0), C.c_int(obey), out, info)
    assert rc == 0
    return list(out), list(info)


def _tlen(qlen):
    """the target of the defaults: the query side plus cal_max_gap of it, 2 qlen - 5; at least a few rows past the end for the shortest queries"""
    return max(2 * qlen - 5, qlen + 8)


def _mismatch(rng, t):
    return ((t + 1 + rng.integers(0, 3, len(t))) % 4).astype(np.uint8)


def one_job(rng, qlen, family, a):
    """(query, target, h0, w) or None where the family has no job at this length"""
    tlen = _tlen(qlen)
    t = rng.integers(0, 4, tlen).astype(np.uint8)
    q = t[:qlen].copy()
    h0 = int(rng.integers(19, 60)) * a
    w = 100
    if family == "clean":
        pass
    elif family == "peak":                # mismatches in the last d bases: the score peaks d columns before the end
        d = min(int(rng.integers(7, 15)), qlen - 1)
        if d < 1:
            return None
        q[qlen - d:] = _mismatch(rng, t[qlen - d:qlen])
    elif family == "never":               # nothing matches beyond the first bases and the first row is zero beyond its first column
        if qlen < 15:
            return None                   # (the first row's band holds a query this short whole: column qlen - 1 is reached on row 0)
        t[2:] = rng.choice(np.array([1, 3], np.uint8), tlen - 2)    # G against C and T: a mismatch at every offset, under the plain and
        q[2:] = 2                                                   # under both three-letter matrices
        h0 = int(rng.integers(2, 5)) * a
    elif family == "first_col":           # a short query behind a long seed: eh[0].h, injected while beg == 0, holds the largest potential
        if qlen > 33:
            return None
        h0 = int(rng.integers(150, 250)) * a
    elif family == "n_in_query":
        q[int(rng.integers(0, qlen))] = 4
        if qlen > 70:
            q[int(rng.choice([63, 64, 65]))] = 4
    elif family == "zdrop_first":         # the second half does not match: where the z-drop is small it ends the extension before the rule can
        if qlen < 15:
            return None
        q[qlen // 2:] = _mismatch(rng, t[qlen // 2:qlen])
        h0 = int(rng.integers(30, 60)) * a
    elif family == "indel":               # a gap a few bases before the end: the end is reached off the diagonal, under a band that travels
        if qlen < 15:
            return None
        k, at = int(rng.integers(1, 4)), qlen - int(rng.integers(5, 12))
        if rng.random() < 0.5:
            q = np.concatenate([q[:at], rng.integers(0, 4, k).astype(np.uint8), q[at:]])[:qlen]
        else:
            q = np.concatenate([q[:at], t[at + k:at + k + qlen]])[:qlen]
        w = int(rng.choice([7, 14, 100]))
    else:
        raise ValueError(family)
    return q.astype(np.uint8), t, h0, w


def tie_jobs(rng, H, mat, gp, zd, a, want=12, tries=40000):
    """jobs in which a row after the one that first reached the end reaches it with h1 == gscore and moves gtle (ksw.c:451 updates on >=): a
    seeded search over short two-letter queries, where equal scores along different paths are common"""
    out = []
    for _ in range(tries):
        if len(out) >= want:
            break
        qlen = int(rng.choice([7, 15, 16, 17, 31, 32, 33]))
        t = rng.integers(0, 2, _tlen(qlen)).astype(np.uint8) * 3
        q = t[:qlen].copy()
        flip = rng.random(qlen) < 0.25
        q[flip] = 3 - q[flip]
        h0, w = int(rng.integers(8, 40)) * a, int(rng.choice([7, 100]))
        _, info = model(H, q, t, mat, gp, w, 5, zd, h0, 0)
        if info[6] > 0 and info[0] >= 0:
            out.append((q, t, h0, w))
    return out


def build(seed=20241021):
    """[(scoring index, family, parent, w, end_bonus, h0, query, target)]: a few hundred per scoring set.  The tie family comes out of a search
    with the model, so the list is made once, by the generator of the recorded answers, and the tests read it from there (load())"""
    rng = np.random.default_rng(seed)
    H = harness()
    out = []
    for si, (a, b, gp, zd) in enumerate(scorings()):
        o = P.opt_of(a, b, gp, zd)
        for qlen in QLENS:
            for fam in FAMILIES:
                if fam == "tie":
                    continue
                for parent in (0, 1):
                    j = one_job(rng, qlen, fam, a)
                    if j is not None:
                        q, t, h0, w = j
                        out.append((si, fam, parent, w, int(rng.integers(0, 6)), h0, q, t))
        for parent in (0, 1):
            for q, t, h0, w in tie_jobs(rng, H, o.ctmat if parent else o.gamat, gp, zd, a):
                out.append((si, "tie", parent, w, 5, h0, q, t))
    return out


def save(path, cases, answers):
    np.savez_compressed(path, si=np.array([c[0] for c in cases], np.int32), fam=np.array([FAMILIES.index(c[1]) for c in cases], np.int32),
                        par=np.array([[c[2], c[3], c[4], c[5]] for c in cases], np.int32),
                        q=np.concatenate([c[6] for c in cases]), qoff=np.concatenate([[0], np.cumsum([len(c[6]) for c in cases])]).astype(np.int64),
                        t=np.concatenate([c[7] for c in cases]), toff=np.concatenate([[0], np.cumsum([len(c[7]) for c in cases])]).astype(np.int64),
                        out=np.asarray(answers, np.int32))


def load(path=GOLDEN):
    """(cases as build() returns them, the recorded six fields per case)"""
    V = np.load(path)
    cases = []
    for k in range(len(V["si"])):
        parent, w, eb, h0 = [int(x) for x in V["par"][k]]
        cases.append((int(V["si"][k]), FAMILIES[int(V["fam"][k])], parent, w, eb, h0,
                      V["q"][V["qoff"][k]:V["qoff"][k + 1]], V["t"][V["toff"][k]:V["toff"][k + 1]]))
    return cases, V["out"]
