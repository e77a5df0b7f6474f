"""Region lists made for mem_sort_deduplicate (mem_alnreg.c:112-202), shared by tests/test_dedup_cases_cpu.py (which qualifies them on the
host function and pins that function to oracle/backhalf.py) and tests/test_gpu_dedup.py (which hands them to k_dedup / k_dedup_long
through bsx_hook_regions_put).

A read is `per_read` lists of bsx_region_t; the function sees their concatenation.  Coordinates lie inside [0, 2 * l_pac).

Validity: every region has qe > qb and re > rb.  The host function marks a dead region by qe = qb while the kernels keep a mask, so a
region that ARRIVES degenerate would be treated differently by construction -- and mem_chain2region never makes one.

Families (FAMILIES): scattered, satellite, tied_ends, tied_scores, threshold, strands, concat; see each generator.  Lists whose
regions must not meet each other in the redundancy scan are laid on a grid of slots whose neighbours carry different `rid`s: the
genome of the tests' index is too short to put a thousand regions max_chain_gap apart, and the scan's reach test asks for equal rid
first (mem_alnreg.c:135).

model_dedup() is a restatement of the function in the form the wave kernel runs it (every earlier region of a p at once), with
klib's introsort from tools/dbg/parsort_model.py on the rank keys the kernel builds.  It returns the kept indices and counters of
what the list exercised; the tests count with it and with the host function, never with device output."""
import os
import sys
import numpy as np
from biscuit_amd import _lib as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "dbg"))
import parsort_model as PM   # noqa: E402

REGION_DT = np.dtype(B.Region)
LENGTHS = [0, 1, 2, 3, 16, 17, 18, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 1000, 1023, 1024, 1025, 1100]
FAMILIES = ("scattered", "satellite", "tied_ends", "tied_scores", "threshold", "strands", "concat")
OPTION_SETS = {"default": {}, "tight": {"mask_level_redun": 0.5, "max_chain_gap": 50, "w": 10}}
SHORT_CAP, CAP_A, CAP_B = 32, 256, 1024   # k_dedup; k_dedup_long<256>; k_dedup_long<1024>


def make_opt(name):
    from biscuit_amd.api import default_opt
    o = default_opt()
    for k, v in OPTION_SETS[name].items():
        setattr(o, k, v)
    return o


def size_class(n):
    return "short" if n <= SHORT_CAP else "A" if n <= CAP_A else "B" if n <= CAP_B else "over"


class Case:
    def __init__(self, name, family, lists, expect=None, group=None):
        self.name, self.family, self.lists, self.expect, self.group = name, family, lists, expect, group   # expect: "bail" / "nobail" / None
        self.per_read = len(lists)
        self.n = sum(len(x) for x in lists)

    def cat(self):
        return np.concatenate(self.lists) if self.lists else np.zeros(0, dtype=REGION_DT)

    @property
    def wide(self):   # a query start beyond what oracle/backhalf.py packs into its sort key (10 bits)
        c = self.cat()
        return bool(len(c)) and int(c["qb"].max()) >= 1024


def regs(rb, re, qb, qe, rid, score):
    a = np.zeros(len(rb), dtype=REGION_DT)
    a["rb"], a["re"], a["qb"], a["qe"], a["rid"], a["score"] = rb, re, qb, qe, rid, score
    a["truesc"] = a["score"]
    assert (a["qe"] > a["qb"]).all() and (a["re"] > a["rb"]).all() and (a["rb"] >= 0).all()
    return a


def one(rb, re, qb, qe, rid, score):
    return regs([rb], [re], [qb], [qe], [rid], [score])


def split(rng, a, per_read, how):
    """the list cut into per_read lists: "even", "head" (k + rest with a short first list), "tail", "empty" (some lists empty)"""
    n = len(a)
    if per_read == 1:
        return [a]
    if how == "head":
        cuts = sorted(min(n, c) for c in ([1] if per_read == 2 else [1, 2, 3]))
    elif how == "tail":
        cuts = sorted(max(0, n - c) for c in ([2] if per_read == 2 else [4, 2, 1]))
    elif how == "empty":
        cuts = [0] if per_read == 2 else sorted([0, n // 2, n // 2])
    else:
        cuts = sorted(int(x) for x in rng.integers(0, n + 1, per_read - 1))
    cuts = [0] + cuts + [n]
    return [a[cuts[i]:cuts[i + 1]] for i in range(per_read)]


def grid(n_slots, l_pac):
    """slot starts and their rids: far enough apart for a slot's content (< 190 bases), neighbours on different rids"""
    stride = min(400, (2 * l_pac - 1000) // max(1, n_slots))
    assert stride >= 200, "the index is too short for %d slots" % n_slots
    x = 500 + stride * np.arange(n_slots, dtype=np.int64)
    return x, (np.arange(n_slots) % 3).astype(np.int32), stride


# --------------------------------------------------------------------------------------------------------------------- families
def scattered(rng, n, l_pac, o):
    """one region a slot, all ends distinct, (score, qb) distinct: the scan's act mask is empty, both sorts rank without ties"""
    x, rid, stride = grid(n, l_pac)
    ln = rng.integers(30, 151, n)
    rb = x + rng.integers(0, stride - 190 + 1, n)
    k = rng.permutation(n)
    qb = k // 131 + rng.integers(0, 3, n) * 10
    a = regs(rb, rb + ln, qb, qb + ln + rng.integers(-2, 3, n), rid, 20 + k % 131)
    return a[rng.permutation(n)]


def satellite(rng, n, l_pac, o):
    """long regions nested around one locus, ends a base or two apart (a later end goes with an earlier start, so no pair is ever tested
    for a concatenation): every region is within reach of all earlier ones and covers them on the reference, the overlaps on the
    query lie around the mask_level_redun threshold, scores mixed"""
    mlr = float(o.mask_level_redun)
    L = 3000 if mlr > 0.9 else 600
    half = L // 2
    mid = int(rng.integers(half + 3000, l_pac - half - 3000)) + (l_pac if rng.random() < 0.5 else 0)
    re = mid + half + np.cumsum(rng.integers(1, 3, n))
    rb = mid - half - np.cumsum(rng.integers(0, 3, n))
    slack = int(L * (1 - mlr))                       # a shift of this much on the query is the threshold
    qb = 100 + rng.integers(0, 2 * slack, n)
    qlen = L - rng.integers(0, max(2, slack // 3), n)
    score = rng.choice([60, 80, 100, 100, 120, 150, 150, 200], n) if rng.random() < 0.5 else rng.integers(50, 300, n)
    a = regs(rb, re, qb, qb + qlen, np.zeros(n, np.int32), score)
    return a[rng.permutation(n)]


def tied_ends(rng, n, l_pac, o, frac=0.5, order="random"):
    """`frac` of the regions take the end of another one; input order random, ascending or descending by end"""
    x, rid, stride = grid(max(n, 1), l_pac)
    ln = rng.integers(30, 151, n)
    re = x[:n] + 160 + rng.integers(0, stride - 190 + 1, n)
    if n > 1:
        m = rng.random(n) < frac
        pool = max(1, int(n * (1 - frac)) if frac < 1 else int(rng.choice([2, 8, max(2, n // 10)])))
        src = rng.integers(0, min(pool, n), n)
        re = np.where(m, re[src], re)
        rid = np.where(m, rid[src], rid[:n])
    rb = re - ln
    qb = rng.integers(0, 50, n)
    a = regs(rb, re, qb, qb + ln + rng.integers(-2, 3, n), rid[:n], rng.integers(20, 150, n))
    if order == "random":
        return a[rng.permutation(n)]
    a = a[np.argsort(a["re"], kind="stable")]
    return a if order == "asc" else a[::-1].copy()


def tied_scores(rng, n, l_pac, o, identical=True, order="random"):
    """runs of equal score, equal (score, rb), fully equal (score, rb, qb) -- identical hits in runs of 2, 3 and 10 -- all with
    different ends; a run shares a slot.  Every region has a rid of its own: the redundancy scan, which would remove the copies
    before the second sort sees them, never starts (the pass over identical hits does not look at rid, mem_alnreg.c:183-189)"""
    x, rid, stride = grid(max(n, 1), l_pac)
    rb, re, qb, qe, rd, sc = [], [], [], [], [], []
    slot = 0
    scores = [int(s) for s in rng.choice(np.arange(30, 150), 6, replace=False)]
    while len(rb) < n:
        kind = int(rng.integers(0, 4 if identical else 3))
        run = min(n - len(rb), 1 if kind == 0 else int(rng.integers(2, 7)) if kind == 1 else int(rng.integers(2, 5)) if kind == 2 else int(rng.choice([2, 3, 10])))
        s = scores[int(rng.integers(0, len(scores)))]
        lens = rng.choice(np.arange(30, 151), run, replace=False)
        for k in range(run):
            sl = slot + (k if kind <= 1 else 0)
            b = int(x[sl]) + (int(rng.integers(0, 20)) if kind <= 1 else 7)
            q = int(rng.integers(0, 40)) if kind <= 1 else 5 + k if kind == 2 else 9
            rb.append(b); re.append(b + int(lens[k])); qb.append(q); qe.append(q + int(lens[k])); rd.append(int(rid[sl])); sc.append(s)
        slot += run if kind <= 1 else 1
    a = regs(rb, re, qb, qe, np.arange(len(rb), dtype=np.int32), sc)
    if order != "random" and n:   # scores monotone along the order by end: the second sort starts from a sorted list full of ties
        a = a[np.argsort(a["re"], kind="stable")]
        a["score"] = np.sort(a["score"])[::-1] if order == "desc" else np.sort(a["score"])
        a["truesc"] = a["score"]
    return a[rng.permutation(n)]


def strands(rng, n, l_pac, o):
    """forward regions (rb < l_pac) and reverse ones just behind l_pac on one rid, same-strand neighbours anti-collinear (no test for a
    concatenation passes among them), forward/reverse pairs collinear and within reach: only the l_pac rule keeps the read from the
    bail-out.  A few regions of another rid lie among them, and behind some of those a higher-scoring near copy of the next region:
    the rid break is what saves that region."""
    mlr, gap = float(o.mask_level_redun), int(o.max_chain_gap)
    ln = 60
    s = int(np.ceil(ln * (1 - mlr))) + 1             # neighbours this far apart are not redundant
    a_n = n // 2
    b_n = n - a_n
    t0 = min(100, max(0, (gap - 41) // s))           # forward region u from the boundary and reverse region k: on one diagonal when u + k = t0
    C = 40 + ln + (s + 1) * t0
    S = max(0, b_n - 1 - C)
    u = a_n - 1 - np.arange(a_n)
    k = np.arange(b_n)
    rb = np.concatenate([l_pac - 40 - ln - s * u, l_pac + s * k])
    qb = np.concatenate([u + S, C + S - k])
    score = rng.integers(40, 150, n)
    extra = []
    for c in (rng.permutation(np.arange(a_n + 1, n))[:n // 20] if n >= 8 else []):   # reverse region c: [near copy, stranger, c] in the order by end
        c = int(c)
        extra.append(one(rb[c] + ln - 1 - 30, rb[c] + ln - 1, 0, 30, 1, 50))                          # the stranger: rid 1, its end one below c's
        extra.append(one(rb[c] - 2, rb[c] - 2 + ln, qb[c], qb[c] + ln, 0, int(score[c]) + 10))     # the copy: two bases down, scores higher
    a = regs(rb, rb + ln, qb, qb + ln, np.zeros(n, np.int32), score)
    if extra and n - len(extra) > 0:
        a = np.concatenate([a[np.sort(rng.permutation(n)[:n - len(extra)])]] + extra)
    return a[rng.permutation(len(a))]


SPECIAL_RID = 3   # the placed regions of a grid list: on a rid of their own, so that no ordinary region meets them


def _grid_fill(rng, n, l_pac, special, where):
    """a scattered list of n regions with the regions of `special(x, rid)` at position `where` along the genome (they replace as many
    ordinary ones)"""
    sp = special(0, SPECIAL_RID)
    width = int(sp["re"].max()) + 300
    m = max(0, n - len(sp))
    stride = min(400, (2 * l_pac - 1500 - width) // max(1, m))
    assert stride >= 200, "the index is too short for %d slots" % m
    where = min(where, m)
    xs = 500 + stride * where
    if xs < l_pac < xs + width:
        where, xs = 0, 500
    sp = special(xs, SPECIAL_RID)
    i = np.arange(m, dtype=np.int64)
    x = 500 + stride * i + np.where(i >= where, width, 0)
    assert m == 0 or int(x.max()) + stride < 2 * l_pac
    ln = rng.integers(30, 151, m)
    rb = x + rng.integers(0, stride - 190 + 1, m)
    k = rng.permutation(m)
    qb = 20 + k // 131
    base = regs(rb, rb + ln, qb, qb + ln, (i % 3).astype(np.int32), 20 + k % 131)
    a = np.concatenate([base, sp])
    return a[rng.permutation(len(a))]


def concat_special(o, kind):
    """(x, rid) -> regions of one slot: "gap": a collinear pair a gap apart; "behind": q_c, K, p in end order -- K kills p before p
    meets q_c; "front": K, q_c, p -- p meets q_c first; "far": the pair with 70 regions between them in the order by end"""
    mlr, gap = float(o.mask_level_redun), int(o.max_chain_gap)
    d = int(100 * (1 - mlr)) + 10

    def f(x, rid):
        if kind == "gap":
            return np.concatenate([one(x, x + 40, 100, 140, rid, 70), one(x + 50, x + 90, 150, 190, rid, 60)])
        if kind == "far":
            g = min(110, gap - 5)
            fill = regs(x + 41 + np.arange(70) - 35, x + 41 + np.arange(70), np.full(70, 900), np.full(70, 935), np.full(70, rid), 30 + np.arange(70) % 7)
            return np.concatenate([one(x, x + 40, 100, 140, rid, 70), fill, one(x + 40 + g, x + 80 + g, 140 + g, 180 + g, rid, 60)])
        qc = one(x, x + 100, 200, 300, rid, 80)
        p = one(x + d, x + d + 100, 200 + d, 300 + d, rid, 70)
        if kind == "pair":
            return np.concatenate([qc, p])
        K = one(x + d, x + (101 if kind == "behind" else 99), 290, 300 + d, rid, 90)
        return np.concatenate([qc, K, p])
    return f


def threshold_specials(o):
    """-> [(group name, delta, special)]: for each comparison of the function a pair exactly on it (delta 0) and one unit to either side"""
    mlr, gap, w = float(o.mask_level_redun), int(o.max_chain_gap), int(o.w)
    out = []

    def add(name, make):
        for dlt in (-1, 0, 1):
            out.append((name, dlt, (lambda dd: lambda x, rid: make(x, rid, dd))(dlt)))
    for mr in (20, 40, 100, 160):
        t = int(round(mr * mlr))
        # q = [x, x+mr), p starts so that or_ = t + delta; the queries coincide; p scores lower: p goes iff or_ > mlr * mr
        add("or_%d" % mr, lambda x, rid, dd, mr=mr, t=t: np.concatenate([one(x, x + mr, 10, 10 + mr, rid, 90), one(x + mr - (t + dd), x + mr - (t + dd) + mr + 5, 10, 10 + mr, rid, 50)]))
        add("oq_%d" % mr, lambda x, rid, dd, mr=mr, t=t: np.concatenate([one(x, x + mr, 10, 10 + mr, rid, 90), one(x, x + mr + 2, 10 + mr - (t + dd), 10 + mr - (t + dd) + mr + 5, rid, 50)]))
    # reach: a collinear pair (q moved by 40 + max_chain_gap + delta on both axes) that puts rb_p on re_q + max_chain_gap: it bails iff p is within reach
    add("reach", lambda x, rid, dd: np.concatenate([one(x, x + 40, 10, 50, rid, 90), one(x + 40 + gap + dd, x + 80 + gap + dd, 50 + gap + dd, 90 + gap + dd, rid, 80)]))
    W1, W2 = w << 1, w << 2
    L1 = 15 * (W1 + 10)
    add("w1", lambda x, rid, dd: np.concatenate([one(x, x + L1, 10, 10 + L1, rid, 90), one(x + L1 + W1 + 10 + dd, x + 2 * L1 + W1 + 10 + dd, 20 + L1, 20 + 2 * L1, rid, 80)]))
    L2, oq2 = 20 * W2, W2 // 4
    add("w2", lambda x, rid, dd: np.concatenate([one(x, x + L2, 10, 10 + L2, rid, 90), one(x + L2 - (oq2 + W2 + dd), x + 2 * L2 - (oq2 + W2 + dd), 10 + L2 - oq2, 10 + 2 * L2 - oq2, rid, 80)]))
    # r on 0.05 (gap 20 over a span of 400, the queries touching) and on 0.1 (overlap 20 over a span of 200): in double r = 0.05 lies BELOW (double)0.05f
    add("r05", lambda x, rid, dd: np.concatenate([one(x, x + 190, 10, 200, rid, 90), one(x + 210 + dd, x + 400 + dd, 200, 390, rid, 80)]))
    add("r10", lambda x, rid, dd: np.concatenate([one(x, x + 110, 10, 120, rid, 90), one(x + 90 - dd, x + 200 - dd, 120, 230, rid, 80)]))
    return out


# --------------------------------------------------------------------------------------------------------------------- the set
_cache = {}


def cases(l_pac, optset):
    """the whole set for one option set: [Case]; seeded, the same on every call"""
    key = (int(l_pac), optset)
    if key in _cache:
        return _cache[key]
    o = make_opt(optset)
    rng = np.random.default_rng(20240 + (0 if optset == "default" else 1))
    lengths = LENGTHS + [int(v) for v in (rng.integers(35, 255, 3).tolist() + rng.integers(258, 1023, 3).tolist())]
    out = []
    hows = ["even", "head", "tail", "empty"]
    tick = [0]

    def put(family, name, a, expect=None, group=None, pr=None, how=None):
        t = tick[0]
        tick[0] += 1
        pr = pr or (1, 2, 4)[t % 3]
        how = how or hows[(t // 3) % 4]
        out.append(Case("%s/%s/n%d/pr%d%s" % (family, name, len(a), pr, how if pr > 1 else ""), family, split(rng, a, pr, how), expect, group))

    for n in lengths:
        for v in range(2):
            put("scattered", "v%d" % v, scattered(rng, n, l_pac, o))
            put("satellite", "v%d" % v, satellite(rng, n, l_pac, o))
            put("strands", "v%d" % v, strands(rng, n, l_pac, o))
        for order in ("random", "asc", "desc"):
            for frac in ((0.1, 1.0) if order == "random" else (0.5, 1.0)):
                put("tied_ends", "%s_f%d" % (order, int(frac * 100)), tied_ends(rng, n, l_pac, o, frac, order))
        put("tied_scores", "plain", tied_scores(rng, n, l_pac, o, identical=False))
        put("tied_scores", "ident", tied_scores(rng, n, l_pac, o, identical=True))
        put("tied_scores", "ident_%s" % ("asc", "desc")[n % 2], tied_scores(rng, n, l_pac, o, identical=True, order=("asc", "desc")[n % 2]))
    # the splits the size classes turn on
    for tot, cuts in ((33, [31]), (1024, [1]), (257, [1, 1, 255]), (32, [0]), (33, [16, 16, 16]), (1024, [256, 512, 768])):
        a = tied_ends(rng, tot, l_pac, o, 0.5, "random")
        c = [0] + cuts + [tot]
        out.append(Case("tied_ends/split_%s" % "+".join(str(c[i + 1] - c[i]) for i in range(len(c) - 1)), "tied_ends", [a[c[i]:c[i + 1]] for i in range(len(c) - 1)]))
    # threshold: every pair alone, in a list of the lane kernel's size and in one of the wave kernel's
    for name, dlt, sp in threshold_specials(o):
        for n in (2, 20, 40, 300):
            where = int(rng.integers(0, max(1, n)))
            a = sp(2000, 0) if n == 2 else _grid_fill(rng, n, l_pac, sp, where)
            out.append(Case("threshold/%s/d%+d/n%d" % (name, dlt, n), "threshold", split(rng, a, 1 + (n == 20), "even"), None, (name, dlt, n)))
    # concat
    for n in (2, 3, 17, 32, 33, 64, 65, 128, 200, 256, 257, 300, 513, 800, 1000, 1024):
        for kind in ("gap", "pair", "front", "far"):
            if n < (2 if kind in ("gap", "pair") else 3 if kind == "front" else 72):
                continue
            where = int(rng.integers(0, n))
            put("concat", kind, _grid_fill(rng, n, l_pac, concat_special(o, kind), where), expect="bail")
    for n in (3, 20, 33, 100, 257, 600, 1024):   # must NOT bail: filed with the threshold cases' family share
        where = int(rng.integers(0, n))
        put("concat", "behind", _grid_fill(rng, n, l_pac, concat_special(o, "behind"), where), expect="nobail")
    _cache[key] = out
    return out


# --------------------------------------------------------------------------------------------------------------------- the model
def _rank_less(cols):
    """number of rows strictly smaller in lexicographic order of the columns (first column most significant), per row"""
    n = len(cols[0])
    order = np.lexsort(tuple(reversed(cols)))
    rk = np.zeros(n, dtype=np.int64)
    if n == 0:
        return rk
    new = np.ones(n, dtype=bool)
    eq = np.ones(n - 1, dtype=bool)
    for c in cols:
        eq &= c[order][1:] == c[order][:-1]
    new[1:] = ~eq
    first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
    rk[order] = first
    return rk


def _klib_by_rank(rk, start, stats, which):
    """the order klib's introsort leaves the elements `start` (in that starting order) in, compared by rk alone: as the kernel gets it --
    by rank when no two are equal, else the wave-parallel sort on weights n - rk"""
    n = len(start)
    if len(np.unique(rk)) == n:
        out = np.empty(n, dtype=np.int64)
        out[rk] = start
        return out
    stats["tie%d" % which] = True
    a = [(int(n - rk[i]), i) for i in range(n)]
    if not PM.par_introsort(list(a)):
        stats["depth%d" % which] = True
    b = list(a)
    assert PM.par_introsort(a, comb=True) and PM.klib_introsort(b, comb=True) and a == b
    return np.array([start[i] for _, i in a], dtype=np.int64)


def model_dedup(c, o, l_pac):
    """mem_sort_deduplicate on the concatenated list c -> (kept indices in final order, or None for the bail-out; counters)"""
    st = {"tie1": False, "tie2": False, "depth1": False, "depth2": False, "act": 0, "walk_max": 0, "late_kill": 0, "early_q_late_p": 0, "late_bail": 0,
          "lpac_saved": 0, "rid_break": 0, "scan_dropped": 0, "ident_dropped": 0}
    n = len(c)
    if n <= 1:
        return list(range(n)), st
    rb, re, qb, qe, rid, sc = (c[f].astype(np.int64) for f in ("rb", "re", "qb", "qe", "rid", "score"))
    mlr, gap, w = np.float32(o.mask_level_redun), int(o.max_chain_gap), int(o.w)
    R05, R10 = float(np.float32(0.05)), float(np.float32(0.05) * np.float32(2))
    order = _klib_by_rank(_rank_less([re]), np.arange(n), st, 1)
    dead = np.zeros(n, dtype=bool)
    for a in range(1, n):
        p = order[a]
        q1 = order[a - 1]
        if not (rid[p] == rid[q1] and rb[p] < re[q1] + gap):
            continue
        st["act"] += 1
        qs = order[a - 1::-1]
        reach = (rid[qs] == rid[p]) & (rb[p] < re[qs] + gap)
        f = len(qs) if reach.all() else int(np.argmin(reach))
        if f < len(qs) and rid[qs[f]] != rid[p] and reach[f + 1:].any():
            st["rid_break"] += 1
        qs = qs[:f]
        live = ~dead[qs]
        or_ = re[qs] - rb[p]
        oq = np.where(qb[qs] < qb[p], qe[qs] - qb[p], qe[p] - qb[qs])
        mr = np.minimum(re[qs] - rb[qs], re[p] - rb[p])
        mq = np.minimum(qe[qs] - qb[qs], qe[p] - qb[p])
        red = live & (or_.astype(np.float32) > mlr * mr.astype(np.float32)) & (oq.astype(np.float32) > mlr * mq.astype(np.float32))
        kills = red & (sc[p] < sc[qs])
        k = int(np.argmax(kills)) if kills.any() else f
        cand = live & ~red & (rb[qs] < rb[p])
        cand[k:] = False
        ci = np.nonzero(cand)[0]
        if len(ci):
            q = qs[ci]
            ok = ~((qb[q] >= qb[p]) | (qe[q] >= qe[p]) | (re[q] >= re[p]))
            wv = np.abs((re[q] - rb[p]) - (qe[q] - qb[p]))
            r = np.abs((re[q] - rb[p]) / (re[p] - rb[q]).astype(np.float64) - (qe[q] - qb[p]) / np.where(ok, qe[p] - qb[q], 1).astype(np.float64))
            gapcase = (re[q] < rb[p]) | (qe[q] < qb[p])
            ok &= np.where(gapcase, ~((wv > w << 1) | (r >= R05)), ~((wv > w << 2) | (r >= R10)))
            lp = (rb[q] < l_pac) & (rb[p] >= l_pac)
            st["lpac_saved"] += int((ok & lp).sum())
            ok &= ~lp
            if ok.any():
                st["late_bail"] += int(ci[np.argmax(ok)] >= 64)
                return None, st
        st["walk_max"] = max(st["walk_max"], min(k + 1, f) if k < f else f)
        dead[qs[:k][red[:k]]] = True
        if k < f:
            dead[p] = True
            if k >= 64:
                st["late_kill"] += 1
                st["early_q_late_p"] += bool(red[:64].any())
    left = order[~dead[order]]
    st["scan_dropped"] = n - len(left)
    m = len(left)
    rk2 = _rank_less([-sc[left], rb[left], qb[left]])
    o2 = _klib_by_rank(rk2, left, st, 2) if m > 1 else left
    keep = [int(o2[0])] if m else []
    for i in range(1, m):
        x, y = o2[i], o2[i - 1]
        if not (sc[x] == sc[y] and rb[x] == rb[y] and qb[x] == qb[y]):
            keep.append(int(x))
    st["ident_dropped"] = m - len(keep)
    return keep, st


def host_dedup(L, o, idx, c):
    """bsx_hook_regs_sort_dedup on the concatenated list -> kept indices, or None for -1"""
    import ctypes as C
    L.bsx_hook_regs_sort_dedup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.bsx_hook_regs_sort_dedup.restype = C.c_int
    c = np.ascontiguousarray(c)
    keep = np.zeros(max(1, len(c)), dtype=np.int32)
    m = L.bsx_hook_regs_sort_dedup(C.byref(o), idx.h, c.ctypes.data_as(C.c_void_p), len(c), keep.ctypes.data_as(C.c_void_p))
    return None if m < 0 else [int(v) for v in keep[:m]]


_qual = {}


def qualified(idx, optset):
    """[(case, host result, model result, model counters)] for the whole set; computed once a session"""
    key = (int(idx.l_pac), optset)
    if key not in _qual:
        o = make_opt(optset)
        L = B.lib()
        rows = []
        for cs in cases(idx.l_pac, optset):
            c = cs.cat()
            mk, st = model_dedup(c, o, idx.l_pac)
            rows.append((cs, host_dedup(L, o, idx, c), mk, st))
        _qual[key] = rows
    return _qual[key]
