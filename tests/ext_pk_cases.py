"""Designed ksw_extend2 jobs for the packed 16-bit extension row (biscuit_amd/csrc/hip/ext_pk.hpp), shared by its CPU and GPU tests.

The row keeps entry 128 p + l of the reference's eh[] in the low half of lane l's registers and entry 128 p + 64 + l in the high half, so the
places where it can go wrong are the half seam (column 64), the slot seam (column 128), and for a 16-lane form columns 16 and 32: the band's
first and last column are carried across them by planted insertions and deletions and by narrow bands that travel down the diagonal."""
import ctypes as C
import numpy as np
from biscuit_amd.api import default_opt
from biscuit_amd import _lib as B

QLENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 126, 127, 128, 129, 191, 254, 255)
KINDS = ("clean", "ins", "del", "mismatch_run", "small_h0", "n_in_query")
# (a, b, (o_del, e_del, o_ins, e_ins), zdrop): the defaults' shape, unequal insertion and deletion penalties, a z-drop that stops extensions
SCORINGS = ((1, 2, (5, 2, 5, 2), 100), (2, 3, (5, 2, 4, 1), 100), (1, 4, (6, 1, 3, 3), 12))
WIDTHS = (100, 200, 7, 14)    # -w and twice it, for the default and for a band narrow enough to travel


def opt_of(a, b, gp, zdrop):
    o = default_opt()
    o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins, o.zdrop = a, b, gp[0], gp[1], gp[2], gp[3], zdrop
    B.lib().bsx_opt_fill_matrices(C.byref(o))
    return o


def one_job(rng, qlen, kind, a):
    """(query, target, h0): the query is the target's start with a few substitutions and what `kind` plants"""
    tlen = int(qlen * rng.uniform(1.0, 1.5)) + (1 if qlen < 4 else 0)
    t = rng.integers(0, 4, tlen + 8).astype(np.uint8)
    q = t[:qlen].copy()
    sub = rng.random(qlen) < 0.03
    q[sub] = rng.integers(0, 4, int(sub.sum()))
    h0 = int(rng.integers(19, 60)) * a
    # where the planted event sits: just before a seam, so that the band's edge crosses it in the rows that follow
    seams = [s for s in (16, 32, 64, 128) if s + 4 < qlen]
    at = int(rng.choice(seams)) - int(rng.integers(1, 6)) if seams else max(0, qlen // 2)
    k = int(rng.integers(1, 7))
    if kind == "ins" and qlen > 8:            # the query has k bases the target lacks: the alignment moves k columns to the right
        q = np.concatenate([q[:at], rng.integers(0, 4, k).astype(np.uint8), q[at:]])[:qlen]
    elif kind == "del" and qlen > 8:          # the query lacks k bases of the target: k columns to the left
        q = np.concatenate([q[:at], t[at + k:at + k + qlen]])[:qlen]
        if len(q) < qlen:
            q = np.concatenate([q, rng.integers(0, 4, qlen - len(q)).astype(np.uint8)])
    elif kind == "mismatch_run":              # nothing matches from `at` on: rows run empty (beg >= end) or the z-drop stops them
        q[at:] = (t[at:qlen] + 1 + rng.integers(0, 3, qlen - at)) % 4
    elif kind == "small_h0":                  # the first row is zero beyond a few columns
        h0 = int(rng.integers(1, 9))
    elif kind == "n_in_query":
        q[int(rng.integers(0, qlen))] = 4
        if qlen > 70:
            q[int(rng.choice([63, 64, 65]))] = 4
    return q.astype(np.uint8), t[:tlen], h0


def jobs(seed=20240611):
    """[(scoring index, parent, w, end_bonus, h0, query, target)], a few hundred per scoring set"""
    rng = np.random.default_rng(seed)
    out = []
    for si, (a, b, gp, zd) in enumerate(SCORINGS):
        for qlen in QLENS:
            for ki, kind in enumerate(KINDS):
                for parent in (0, 1):
                    w = WIDTHS[(ki + parent * 2 + qlen) % 4]      # every width with every kind and strand over the lengths
                    q, t, h0 = one_job(rng, qlen, kind, a)
                    out.append((si, parent, w, int(rng.integers(0, 6)), h0, q, t))
                    if kind in ("ins", "del"):                    # and the same event under the band of the other width class
                        out.append((si, parent, WIDTHS[(ki + parent * 2 + qlen + 2) % 4], 5, h0, q, t))
    return out
