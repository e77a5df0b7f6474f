"""The recorded seed-filter vectors (tests/golden/ref_vectors_ssw.npz, made by tests/golden/make_vectors_ssw.py) as job lists: which jobs share a
wavefront of k_swl16 (sixteen consecutive ones) and a lane's registers (2g and 2g + 1) is decided here, by the order of a list.  Shared by the CPU
restatement's test (tests/test_ssw16_host.py) and the GPU tests (tests/test_gpu_ssw.py).  An entry of a list is a vector's number, or FILLER:
an empty job (qlen = 0), what ssw_take leaves of a wave's block of job numbers."""
import ctypes as C
import os
import numpy as np
from biscuit_amd import _lib as B
from biscuit_amd.api import default_opt

HERE = os.path.dirname(os.path.abspath(__file__))
FILLER = -1
# what make_vectors_ssw.py prints: equalities, a vector that drops out of a comparison fails its test
FAMILY_COUNTS = {'stripes': 150, 'long_short': 48, 'score_low': 28, 'score_mid': 28, 'score_high': 28, 'ins_cross': 69, 'del_cross': 24,
                 'adjacent_gaps': 36, 'query_n': 30, 'guard': 42, 'guard_ins': 29, 'refused': 42, 'refused_ins': 29}
FAMILY_COUNTS_ADMITTED = dict(FAMILY_COUNTS, refused=0, refused_ins=0)      # what the packed kernel scores: not the option sets beyond its guard
SCORE_CLASSES = {'low': 267, 'mid': 220, 'high': 96}
SCORE_CLASSES_ADMITTED = {'low': 267, 'mid': 170, 'high': 75}
GUARD_INS_MIN = 8      # per option set at the guard or just beyond it: 199-column jobs whose best path needs the long insertion
NEEDS_INSERTION, NEEDS_DELETION = ("ins_cross", "guard_ins", "refused_ins"), ("del_cross",)
N_OPTION_SETS, N_REFUSED_SETS = 14, 3
ORDERINGS = ("as_generated", "shuffled", "long_short", "high_low", "matrices", "fillers")
LIST_LENGTHS = (1, 15, 16, 17, 31, 33)
TILED = 300007      # more than twice 16 jobs x 256 CUs x 32 waves, and no multiple of 16 (300 000 is one): the last wavefront is a partial one


class Vectors:
    def __init__(self):
        V = np.load(os.path.join(HERE, "golden", "ref_vectors_ssw.npz"))
        self.q, self.qoff, self.t, self.toff = V["ssw_q"], V["ssw_qoff"], V["ssw_t"], V["ssw_toff"]
        self.par, self.out, self.fam, self.fams = V["ssw_par"], V["ssw_out"], V["ssw_fam"], [str(x) for x in V["ssw_fams"]]
        self.n = len(self.par)
        self.qlen, self.tlen = np.diff(self.qoff).astype(np.int64), np.diff(self.toff).astype(np.int64)
        self.score = self.out[:, 0].astype(np.int64)
        self.use_ct = (self.par[:, 2] == 1).astype(np.uint8)
        assert (self.par[:, 7] == 0x80000).all() and (self.tlen > 0).all() and (self.t < 4).all()
        self.refused = (self.fam == self.fams.index("refused")) | (self.fam == self.fams.index("refused_ins"))

    def groups(self):
        """option set (a, b, o_del, e_del, o_ins, e_ins) -> its vectors, in file order"""
        g = {}
        for i in range(self.n):
            a, b, which, od, ed, oi, ei, xtra = [int(x) for x in self.par[i]]
            g.setdefault((a, b, od, ed, oi, ei), []).append(i)
        return g

    def family_counts(self, ids):
        ids = sorted(set(int(i) for i in ids if i != FILLER))
        return {f: int((self.fam[ids] == k).sum()) for k, f in enumerate(self.fams)} if ids else {f: 0 for f in self.fams}



def opt_of(key):
    """the library's options for an option set (a, b, o_del, e_del, o_ins, e_ins), its two strand matrices filled"""
    o = default_opt()
    o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins = key
    B.lib().bsx_opt_fill_matrices(C.byref(o))
    return o


def mats_of(key):
    o = opt_of(key)
    return np.array(list(o.ctmat), np.int8), np.array(list(o.gamat), np.int8)


def _interleave(a, b):
    out = []
    for k in range(max(len(a), len(b))):
        out += ([a[k]] if k < len(a) else []) + ([b[k]] if k < len(b) else [])
    return out


def orderings(V, ids, seed=1):
    """name -> list; every list holds each vector of ids exactly once"""
    ids = list(ids)
    rng = np.random.default_rng(1000 + seed)
    o = {"as_generated": ids, "shuffled": [ids[k] for k in rng.permutation(len(ids))]}
    # alternating long and short: the largest window beside the smallest, so that 199 x 199 shares a lane's registers with 1..8 x 1
    by_size = sorted(ids, key=lambda i: (-(V.qlen[i] + V.tlen[i]), i))
    half = (len(ids) + 1) // 2
    o["long_short"] = _interleave(by_size[:half], by_size[half:][::-1])
    # alternating high and low score, each way round in turn: (high, low), (low, high), ...
    by_score = sorted(ids, key=lambda i: (-V.score[i], i))
    hi, lo = by_score[:half], by_score[half:][::-1]
    hl = []
    for k in range(half):
        pair = [hi[k]] + ([lo[k]] if k < len(lo) else [])
        hl += pair[::-1] if k & 1 else pair
    o["high_low"] = hl
    o["matrices"] = _interleave([i for i in ids if not V.use_ct[i]], [i for i in ids if V.use_ct[i]])
    # empty jobs: beside every job of the first wavefront, a whole wavefront of them, then one after every third job
    f = []
    for i in ids[:8]:
        f += [i, FILLER]
    f += [FILLER] * 16
    for k, i in enumerate(ids[8:]):
        f += [i] + ([FILLER] if k % 3 == 2 else [])
    o["fillers"] = f
    for name, lst in o.items():
        assert sorted(x for x in lst if x != FILLER) == sorted(ids), name
    return o


def neighbours(lst):
    """the pairs that share a lane's registers: entries 2g and 2g + 1"""
    return [(lst[k], lst[k + 1]) for k in range(0, len(lst) - 1, 2)]


def layout(V, which):
    """the targets one behind the other in one contig.  which = 0: even vectors as recorded, odd ones reverse-complemented and addressed on the
    reverse strand; 1: the other way round.  Returns (genome, tpos per vector)"""
    parts, at, where = [], 0, []
    for i in range(V.n):
        t = V.t[V.toff[i]:V.toff[i + 1]]
        rev = (i & 1) != which
        parts.append((3 - t)[::-1] if rev else t)
        where.append((at, rev))
        at += len(t)
    l_pac = at
    tpos = np.array([2 * l_pac - s - int(V.tlen[i]) if rev else s for i, (s, rev) in enumerate(where)], np.int64)
    return np.concatenate(parts).astype(np.uint8), tpos


def score_classes(scores):
    s = np.asarray(scores)
    return {"low": int((s < 256).sum()), "mid": int(((s >= 256) & (s < 16384)).sum()), "high": int((s >= 16384).sum())}


def strand_ends(V, tpos, l_pac, ids):
    """the strand ends that the windows of the vectors in ids touch: ("start" | "end", 0 | 1 | 2) for a window that starts or ends at 0, l_pac, 2 l_pac"""
    ends = set()
    for i in set(ids) - {FILLER}:
        for what, p in (("start", int(tpos[i])), ("end", int(tpos[i] + V.tlen[i]))):
            if p % l_pac == 0:
                ends.add((what, p // l_pac))
    return ends


def padded_queries(V, ids):
    return {int((V.qlen[i] + 7) // 8 * 8) for i in ids if i != FILLER}
