"""Designed strand searches for the seeding kernels (csrc/hip/k_seedt.hip, k_seed.hip over seed_tab.hpp and seed_core.hpp), shared by
tests/golden/make_vectors_seed.py (which records what the reference's own bwt_smem1a and bwt_seed_strategy1 make of them under
mem_collect_intv's three passes), tests/test_seed_recorded_cpu.py and tests/test_gpu_seed_recorded.py.

A genome and reads by construction, from the integer generator of tests/regions_cases.py (splitmix64), so that every case's place relative
to every branch of the seeding machines is known before a kernel runs.  The recording (tests/golden/ref_seeds.npz) holds a CRC of the
genome and of the read buffer: tests compare them before they compare anything else.

The genome (two contigs, about 60 kb, so that the table of k-mer intervals gets K = seed_tab_depth(2 * l_pac) = 8 levels):

* c1: EDGE unique bases (its base 0 is a read's), unique background, the exact-copy families f1 .. f21 -- R copies of a unit of UNIT bases,
  each followed by SPACER unique ones -- so that an interval's x2 sits on either side of split_width (10; 3 in the strict set) and of
  max_mem_intv (20), the extra copies of three units' cores (below), and unique bases up to the contig's end (the junction read's left half)
* c2: unique bases, a run of HOMO As, unique bases, the tandem array, unique bases, a run of Ns (the index builder replaces them), unique
  background, the second copies of its slots' cores, EDGE unique bases (the text's last base is a read's)

The tandem array has period 5 (ACGTT: period 5 under both conversions) and its copies have diverged: a substitution (one that survives both
conversions) every 20 to 34 bases.
A read cut from it is one SMEM and cheap.  A read of the pure period is what crosses the first seeding pass's budget: no stretch of it
longer than the array's longest intact run occurs anywhere, every shorter stretch occurs at a different number of places, so every start
gives dozens of intervals that each walk back a different way (the reads "inside young copies of a repeat family" of shim.hip's stage
4).  An array of exact copies would not do: the whole read would be one SMEM.

A read's pieces are cut from inside units or from unique sequence and meet at bases that differ under both conversions from what the
genome holds there, so an SMEM ends where its piece ends (regions_cases.join has the same rule).
"""
import zlib
import numpy as np

from regions_cases import Ints, _differs_both, _sub_both, revcomp, A_, C_, G_, T_

N_ = 4
UNIT, SPACER = 120, 40
EDGE = 200
BG1, BG2 = 18000, 14000
HOMO = 2500
TAN_UNIT = (A_, C_, G_, T_, T_)
TAN = 6000
N_RUN = 200
FAMILIES = [("f1", 1), ("f2", 2), ("f3", 3), ("f10", 10), ("f11", 11), ("f19", 19), ("f20", 20), ("f21", 21)]
# What pass 2 finds when it re-seeds an SMEM must be there to be found, or a strand search that skips the re-seeding returns the same list:
# bases CORE of the units of f3, f10 and f11 have CORE_EXTRA more copies of their own, and of every SLOT bases of bg2 (the stitched reads'
# pieces start at bases SLOT_START of a slot and have 28 and more: the core lies inside them) the bases SLOT_CORE have one more -- intervals with more occurrences than the SMEM
# around them, which only the re-seeding reports
CORE, CORE_EXTRA, CORE_FAMILIES = (32, 56), 3, ("f3", "f10", "f11")
SLOT, SLOT0, SLOTS, SLOT_START, SLOT_CORE = 60, 300, 225, (1, 8), (9, 28)

# (name, options that differ from the defaults, the cases it is recorded for: None = all)
STRICT = {"min_seed_len": 15, "split_width": 3, "max_mem_intv": 8, "split_factor": 1.2}
SHORT = {"min_seed_len": 6, "split_width": 30, "max_mem_intv": 50, "split_factor": 1.0}
NOP3_CASES = ("len150", "len193", "p2_f10_28", "p3_f19", "smem65", "tan150", "polyA", "nothing", "n_all")
SHORT_MAX_LEN, SHORT_ALSO = 257, ("len1025",)      # what the short set is recorded for: a read of 3000 bases has 5000 intervals under it
OPTSETS = [("default", {}, None), ("strict", STRICT, None), ("short", SHORT, "short reads"), ("nop3", {"max_mem_intv": 0}, NOP3_CASES)]
SA_OPTSETS = ("default", "strict", "nop3")      # whose intervals' suffix-array positions are recorded (the short set's are most of the text)
DEFAULTS = {"min_seed_len": 19, "split_factor": 1.5, "split_width": 10, "max_mem_intv": 20}

TRIP_BUDGET = 4096      # shim.hip, rg_plan: requests per 256 bases of read after which the first seeding pass hands a strand search on
SEEDT_WPT = 12          # k_seedt.hip: words of sixteen packed digits a lane holds in LDS; longer reads are read where they lie

_cache = {}


def options(optset):
    o = dict(DEFAULTS)
    o.update({n: v for n, v, _ in OPTSETS}[optset])
    return o


def split_len(o):
    return int(np.float32(o["min_seed_len"]) * np.float32(o["split_factor"]) + .499)      # (opt.split_factor is a float)


def tab_depth(n_symbols):
    """seed_tab_depth (seed_tab.hpp)"""
    k, p = 0, 3
    while k < 18 and p <= n_symbols // 8:
        k += 1
        p *= 3
    return 0 if k < 2 else k


def genome():
    """([(contig name, codes 0..4)], {name: its unit or stretch}, {name: (contig, offset)})"""
    if "g" in _cache:
        return _cache["g"]
    r = Ints(0x5EED2026)
    parts = {"c1": [], "c2": []}
    at = {}
    S = {}

    def put(contig, name, seq):
        at[name] = (contig, sum(len(p) for p in parts[contig]))
        S[name] = seq
        parts[contig].append(seq)

    put("c1", "edge0", r.bases(EDGE))
    put("c1", "bg1", r.bases(BG1))
    for name, n in FAMILIES:
        u = r.bases(UNIT)
        S[name] = u
        for k in range(n):
            parts["c1"] += [u, r.bases(SPACER)]
    def flanked(src, a, b):
        """src[a:b] between bases that differ from src[a - 1] and src[b] under both conversions, then a few unique ones"""
        f = r.bases(8)
        for at, other in ((0, int(src[a - 1])), (1, int(src[b]))):
            while not _differs_both(int(f[at]), other):
                f[at] = (f[at] + 1) % 4
        return np.concatenate([f[:1], src[a:b], f[1:]])

    put("c1", "cores", np.concatenate([flanked(S[fam], *CORE) for fam in CORE_FAMILIES for _ in range(CORE_EXTRA)]))
    put("c1", "tail1", r.bases(EDGE))
    put("c2", "head2", r.bases(EDGE))
    put("c2", "homo", np.full(HOMO, A_, np.uint8))
    put("c2", "sep1", _not_starting(r.bases(EDGE), A_))
    tan = np.tile(np.array(TAN_UNIT, np.uint8), TAN // 5)
    rt, k = Ints(0x7A4DE5), 7      # (a stream of its own: the array stays what it is when the rest of the genome changes)
    while k < len(tan):
        tan[k] = [b for b in range(4) if _differs_both(int(tan[k]), b)][rt.below(2)]      # a substitution that survives both conversions: no intact run is longer under one of them
        k += 20 + rt.below(15)
    put("c2", "tan", tan)
    put("c2", "sep2", r.bases(EDGE))
    put("c2", "nrun", np.full(N_RUN, N_, np.uint8))
    put("c2", "bg2", r.bases(BG2))
    put("c2", "echo", np.concatenate([flanked(S["bg2"], SLOT0 + SLOT * j + SLOT_CORE[0], SLOT0 + SLOT * j + SLOT_CORE[1]) for j in range(SLOTS)]))
    put("c2", "edge1", r.bases(EDGE))
    contigs = [(c, np.concatenate(parts[c])) for c in ("c1", "c2")]
    _cache["g"] = (contigs, S, at)
    return _cache["g"]


def _not_starting(seq, base):
    if seq[0] == base:
        seq[0] = (base + 1) % 4
    return seq


def l_pac():
    return sum(len(g) for _, g in genome()[0])


def K():
    """levels of the table of k-mer intervals the device builds for this genome"""
    return tab_depth(2 * l_pac())


def genome_crc():
    return zlib.crc32(b"".join(g.tobytes() for _, g in genome()[0])) & 0xffffffff


def write_fasta(path):
    with open(path, "wb") as f:
        for name, g in genome()[0]:
            f.write(b">" + name.encode() + b"\n")
            s = np.frombuffer(b"ACGTN", np.uint8)[g].tobytes()
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


# ------------------------------------------------------------------------------------------ reads
def with_n(seq, where):
    seq = seq.copy()
    for w in where:
        seq[w] = N_
    return seq


def stretches(seq, lens):
    """N-free stretches of the given lengths from the read's start on, one N between them; the rest of the read stays as it is"""
    seq, at = seq.copy(), 0
    for n in lens:
        at += n
        if at < len(seq):
            seq[at] = N_
        at += 1
    return seq


def _spans(window, m):
    """does a stretch of m bases of the window occur in the genome under either conversion?  (3 ** -19 times 240 kb of text, times the
    twenty stretches across each of a thousand junctions: a stitched read would hold a few SMEMs of chance)"""
    if "kmers" not in _cache:
        fwd = np.concatenate([g for _, g in genome()[0]])
        both = np.concatenate([fwd, np.full(1, N_, np.uint8), revcomp(fwd)])
        _cache["kmers"] = {}
        for parent in (0, 1):
            t = convert(both, parent).tobytes()
            _cache["kmers"][parent] = {t[i:i + m] for i in range(len(t) - m + 1)}
    for parent in (0, 1):
        w = convert(window, parent).tobytes()
        if any(w[i:i + m] in _cache["kmers"][parent] for i in range(len(w) - m + 1)):
            return True
    return False


def cases():
    """[dict(name, seq, budget)] in the order of the recording.  budget: None, or "over" / "under" for the strand searches whose requests
    tests/test_seed_recorded_cpu.py compares with the first pass's budget"""
    if "c" in _cache:
        return _cache["c"]
    contigs, S, at = genome()
    c1, c2 = contigs[0][1], contigs[1][1]
    bg1, bg2, tan = S["bg1"], S["bg2"], S["tan"]
    r = Ints(0xFACADE)
    k_tab = K()
    out = []

    def add(name, seq, rc=False, budget=None):
        assert all(c["name"] != name for c in out), name
        out.append({"name": name, "seq": np.ascontiguousarray(seq, np.uint8), "budget": budget})
        if rc:
            add(name + "_rc", revcomp(np.ascontiguousarray(seq, np.uint8)), budget=budget)

    # ---- lengths: unique sequence with a substitution every 64 bases or so (several SMEMs; pass 2 re-seeds the long ones)
    cur = 100
    for n in (18, 19, 20, 150, 191, 192, 193, 255, 256, 257, 1024, 1025, 3001):
        s = bg1[cur:cur + n].copy()
        for p in range(47, n - 20, 64):
            s = _sub_both(s, p)
        add("len%d" % n, s, rc=True, budget="under" if n >= 150 else None)
        cur += n + 30
    # ---- N placement (K from the genome's size)
    base200, base150 = bg2[1000:1200], bg2[2000:2150]
    for tag, base in (("a", base200), ("b", base150)):      # a: read where it lies (more than SEEDT_WPT * 16 bases); b: packed digits in LDS
        n = len(base)
        for w in (0, n - 1, 15, 16, 17, 31, 32, k_tab - 1, k_tab):      # (the first SMEM starts at base 0: the last two are x0 + K - 1, x0 + K)
            add("n%s_at%d" % (tag, w), with_n(base, [w]), rc=(w in (16, k_tab)))
        add("n%s_x0" % tag, with_n(base, [0, 1, 2 + k_tab - 1]))      # the first SMEM starts at base 2
        add("n%s_x0b" % tag, with_n(base, [0, 1, 2 + k_tab]))
        add("n%s_run" % tag, with_n(base, range(70, 82)), rc=True)
        add("n%s_st" % tag, stretches(base, (k_tab - 1, k_tab, k_tab + 1, 18, 19, 20)), rc=True)
        for e in (k_tab - 1, k_tab, k_tab + 1, 18, 19):      # the stretch at the read's end
            add("n%s_end%d" % (tag, e), with_n(base, [n - 1 - e]))
    add("n_all", np.full(150, N_, np.uint8))
    add("n_all200", np.full(200, N_, np.uint8))
    # ---- pass 2: an SMEM of split_len - 1 / split_len bases with x2 at split_width / one past it, between two substitutions
    for oname, fams in (("default", ("f10", "f11")), ("strict", ("f3", "f10"))):
        sl = split_len(options(oname))
        for fam in fams:
            for n in (sl - 1, sl):
                s = S[fam][10:110].copy()
                s = _sub_both(_sub_both(s, 20), 21 + n)
                add("p2%s_%s_%d" % ("" if oname == "default" else "s", fam, n), s, rc=(n == sl))
    # ---- pass 3: x2 around max_mem_intv
    for fam in ("f19", "f20", "f21", "f1", "f2"):
        add("p3_%s" % fam, S[fam][8:108], rc=(fam in ("f19", "f20")))
    nothing = Ints(0xDEAD).bases(150)
    add("nothing", nothing, rc=True)
    add("nothing250", Ints(0xBEEF).bases(250))
    # ---- many SMEMs: pieces of split_len and more unique bases; every fourth from f11 (x2 = 11: not re-seeded), so that the re-seeding
    # masks are not all ones
    sl = split_len(options("default"))

    def stitch(n_pieces, seed):
        """every fourth piece from f11, the others from the slots of bg2 one after the other: a slot without a start at which its piece can
        follow the piece before it is passed over"""
        rr, m = Ints(seed), options("default")["min_seed_len"]
        ps, end, slot = [], None, rr.below(8)      # end: (source, index behind the last piece's end)
        ends, fails = [], 0
        while len(ps) < n_pieces:
            k = len(ps)
            n = sl + (k % 3)
            if k % 4 == 3:
                src, st = S["f11"], 60 + rr.below(20)      # (behind the unit's core)
                last = UNIT - n - 3
            else:
                src, st, last = bg2, SLOT0 + SLOT * slot + SLOT_START[0], SLOT0 + SLOT * slot + SLOT_START[1]
                slot += 1
                assert slot <= SLOTS
            if k:
                pu, pe = end
                while st <= last and (not (_differs_both(int(pu[pe]), int(src[st])) and _differs_both(int(pu[pe - 1]), int(src[st - 1])))
                                      or _spans(np.concatenate([ps[-1][-(m - 1):], src[st:st + m - 1]]), m)):
                    st += 1
            if st > last:
                fails += 1
                if fails == 4:      # (the tail of the piece before matches somewhere by chance: whatever follows it would extend the match)
                    ps.pop()
                    end, fails = ends.pop(), 0
                continue
            ps.append(src[st:st + n])
            ends.append(end)
            end, fails = (src, st + n), 0
        return np.concatenate(ps)

    for n in (63, 64, 65, 127, 128, 129, 200):
        # (seeds at which no stretch across two pieces matches the bases the index builder puts in place of the genome's Ns: _spans cannot know them)
        add("smem%d" % n, stitch(n, (4000 if n == 200 else 3000) + n), rc=(n in (65, 129)), budget="under")
    # ---- low complexity
    add("polyA", np.full(150, A_, np.uint8), budget="under")
    add("polyT", np.full(150, T_, np.uint8), budget="under")
    add("polyC", np.full(150, C_, np.uint8), budget="under")
    add("tan150", tan[500:650], rc=True, budget="under")      # cut from the array: one SMEM and what lies inside it
    add("tan250", tan[400:650], budget="under")
    pure = np.tile(np.array(TAN_UNIT, np.uint8), 60)
    # the pure period matches the diverged copies piecewise, at thousands of places: past the first pass's budget all of them, the two
    # short ones within the second pass's eight budgets, the reads of 150 bases past those too (and with lists of 2863 intervals)
    add("tan60d", pure[:60], budget="over")
    add("tan80d", pure[:80], budget="over")
    add("tan150d", pure[:150], rc=True, budget="over")
    add("half", np.concatenate([c2[at["tan"][1] - 75:at["tan"][1]], tan[:75]]), rc=True, budget="under")      # half unique, half array
    add("halfA", np.concatenate([S["homo"][:75], S["sep1"][:75]]), budget="under")
    # ---- text edges
    add("edge_first", c1[:60], rc=True)
    add("edge_last", c2[-60:], rc=True)
    add("junction", np.concatenate([c1[-75:], c2[:75]]), rc=True)
    # ---- a dozen ordinary strand searches
    for k in range(12):
        a = 3000 + 900 * k + r.below(500)
        s = bg2[a:a + 150].copy()
        for _ in range(k % 4):
            p = r.below(150)
            s[p] = (s[p] + 2) % 4
        if k == 7:
            s[81] = N_
        add("ord%02d" % k, revcomp(s) if k % 2 else s, budget="under")
    _cache["c"] = out
    return out


def read_buffer(cs):
    off = np.zeros(len(cs) + 1, np.int64)
    for i, c in enumerate(cs):
        off[i + 1] = off[i] + len(c["seq"])
    return np.concatenate([c["seq"] for c in cs]), off


def reads_crc():
    return zlib.crc32(read_buffer(cases())[0].tobytes()) & 0xffffffff


def convert(seq, parent):
    """the read as the reference's seeding sees it: C>T for parent 1, G>A for parent 0"""
    s = seq.copy()
    if parent:
        s[s == C_] = T_
    else:
        s[s == G_] = A_
    return s


def optset_cases(optset):
    only = {n: c for n, _, c in OPTSETS}[optset]
    if only == "short reads":
        return [c for c in cases() if len(c["seq"]) <= SHORT_MAX_LEN or c["name"] in SHORT_ALSO]
    return [c for c in cases() if only is None or c["name"] in only]


# ------------------------------------------------------------------------------------------ the recording
STAT_KEYS = ("intervals", "pass1", "reseeded", "pass3", "max_x2", "p3_min_x2", "p3_max_x2")


class Recording:
    """tests/golden/ref_seeds.npz: per (option set, case, parent) the reference's interval list ordered by info, what it saw on the way
    (STAT_KEYS; resplit(): the indices of the pass-1 SMEMs that pass 2 re-seeded), and the suffix-array positions of the ranks the chaining
    step would look up"""

    def __init__(self, path):
        z = np.load(path)
        self.z = z
        self.names = [str(x) for x in z["names"]]
        self.optsets = [str(x) for x in z["optsets"]]
        self.key = {(self.optsets[int(o)], self.names[int(c)], int(p)): k for k, (o, c, p) in enumerate(zip(z["rec_opt"], z["rec_case"], z["rec_parent"]))}
        self.stat, self.same, self.off, self.roff = z["rec_stat"], z["rec_same"], z["rec_off"], z["rec_roff"]
        self.sa = {p: dict(zip(z["sa_rank_%d" % p].tolist(), z["sa_pos_%d" % p].tolist())) for p in (0, 1)}

    def stats(self, optset, name, parent):
        return dict(zip(STAT_KEYS, (int(v) for v in self.stat[self.key[(optset, name, parent)]])))

    def resplit(self, optset, name, parent):
        """[(index among pass 1's SMEMs, its length, its x2)] of the SMEMs pass 2 re-seeded"""
        k = self.key[(optset, name, parent)]
        a, b = int(self.roff[k]), int(self.roff[k + 1])
        return [(int(i), int(n), int(x)) for i, n, x in zip(self.z["resplit"][a:b], self.z["resplit_len"][a:b], self.z["resplit_x2"][a:b])]

    def intervals(self, optset, name, parent):
        """(n, 4) uint64: x0, x1, x2, info"""
        k = self.key[(optset, name, parent)]
        src = int(self.same[k]) if self.same[k] >= 0 else k
        a, b = int(self.off[src]), int(self.off[src + 1])
        z = self.z
        out = np.zeros((b - a, 4), np.uint64)
        out[:, 0], out[:, 1], out[:, 2] = z["x0"][a:b], z["x1"][a:b], z["x2"][a:b]
        out[:, 3] = (z["start"][a:b].astype(np.uint64) << np.uint64(32)) | z["end"][a:b].astype(np.uint64)
        assert len(out) == self.stat[k][0]
        return out


def load(path=None):
    import os
    return Recording(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_seeds.npz"))


def same_intervals(got, want):
    """list for list, field for field -> None, or a text naming the first difference"""
    if len(got) != len(want):
        return "%d intervals, recorded %d" % (len(got), len(want))
    if not (got == want).all():
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        return "interval %d of %d: %s, recorded %s" % (i, len(got), [int(v) for v in got[i]], [int(v) for v in want[i]])
    return None


# ------------------------------------------------------------------------------------------ which case sits at which edge, on which side
LENGTHS = (18, 19, 20, 191, 192, 193, 255, 256, 257, 1024, 1025, 3001)
SMEM_COUNTS = (63, 64, 65, 127, 128, 129, 200)


def coverage(rec):
    """[(edge, occupied, what the recording says)] for both parents of every case that was built for an edge; from the recording, the
    cases' own bases (whose CRC the recording holds) and the option sets"""
    by = {c["name"]: c for c in cases()}
    rows = []

    def row(edge, ok, what):
        rows.append((edge, bool(ok), what))

    def has(optset, name, parent, n, x2):
        a = rec.intervals(optset, name, parent)
        return bool((((a[:, 3] & np.uint64(0xffffffff)) - (a[:, 3] >> np.uint64(32)) == n) & (a[:, 2] == x2)).any())

    dflt = options("default")
    for n in LENGTHS:
        for name in ("len%d" % n, "len%d_rc" % n):
            st = [rec.stats("default", name, p) for p in (1, 0)]
            want = n >= dflt["min_seed_len"]
            row("length %d: %s" % (n, name), len(by[name]["seq"]) == n and all((s["intervals"] > 0) == want for s in st), "intervals %s" % [s["intervals"] for s in st])
    k_tab = K()
    for tag, n in (("a", 200), ("b", 150)):
        assert (n > SEEDT_WPT * 16) == (tag == "a")
        spots = [("n%s_at%d" % (tag, w), [w]) for w in (0, n - 1, 15, 16, 17, 31, 32, k_tab - 1, k_tab)]
        spots += [("n%s_x0" % tag, [0, 1, 2 + k_tab - 1]), ("n%s_x0b" % tag, [0, 1, 2 + k_tab]), ("n%s_run" % tag, list(range(70, 82)))]
        spots += [("n%s_end%d" % (tag, e), [n - 1 - e]) for e in (k_tab - 1, k_tab, k_tab + 1, 18, 19)]
        for name, where in spots:
            seq = by[name]["seq"]
            ok = len(seq) == n and sorted(np.nonzero(seq == N_)[0].tolist()) == where
            tot = 0
            for p in (1, 0):
                a = rec.intervals("default", name, p)
                st_, en_ = a[:, 3] >> np.uint64(32), a[:, 3] & np.uint64(0xffffffff)
                ok = ok and not any(((st_ <= w) & (w < en_)).any() for w in where)
                tot += len(a)
            row("N at %s of %d: %s" % (where if len(where) < 4 else "%d..%d" % (where[0], where[-1]), n, name), ok and tot > 0, "%d intervals, none across an N" % tot)
        name = "n%s_st" % tag
        seq = by[name]["seq"]
        gaps = np.diff(np.concatenate([[-1], np.nonzero(seq == N_)[0]])) - 1
        row("N-free stretches: %s" % name, gaps.tolist() == [k_tab - 1, k_tab, k_tab + 1, 18, 19, 20], "stretches %s, then %d bases" % (gaps.tolist(), n - 1 - int(np.nonzero(seq == N_)[0][-1])))
    for name in ("n_all", "n_all200"):
        row("all N: %s" % name, (by[name]["seq"] == N_).all() and all(rec.stats("default", name, p)["intervals"] == 0 for p in (1, 0)), "no interval")
    for oname, fams, tag in (("default", ("f10", "f11"), ""), ("strict", ("f3", "f10"), "s")):
        o = options(oname)
        sl = split_len(o)
        for fam in fams:
            x2 = dict(FAMILIES)[fam]
            for n in (sl - 1, sl):
                name = "p2%s_%s_%d" % (tag, fam, n)
                want = n >= sl and x2 <= o["split_width"]
                ok, got = True, []
                for p in (1, 0):
                    re_ = any(l == n and x == x2 for _, l, x in rec.resplit(oname, name, p))
                    got.append(re_)
                    a = rec.intervals(oname, name, p)
                    core = bool(((a[:, 2] == x2 + CORE_EXTRA) & ((a[:, 3] & np.uint64(0xffffffff)) - (a[:, 3] >> np.uint64(32)) < n)).any())
                    ok = ok and has(oname, name, p, n, x2) and re_ == want and core == want      # (what the re-seeding finds, and nothing else does)
                row("pass 2 [%s]: length %d (split_len %d), x2 %d (split_width %d)" % (oname, n, sl, x2, o["split_width"]), ok, "%s: re-seeded %s, expected %s" % (name, got, want))
    for fam, n3 in (("f19", True), ("f20", False), ("f21", False)):
        name = "p3_%s" % fam
        x2 = dict(FAMILIES)[fam]
        st = [rec.stats("default", name, p) for p in (1, 0)]
        ok = all(s["max_x2"] == x2 and ((s["pass3"] > 0 and s["p3_min_x2"] == s["p3_max_x2"] == x2) if n3 else s["pass3"] == 0) for s in st)
        row("pass 3: x2 %d against max_mem_intv %d" % (x2, dflt["max_mem_intv"]), ok, "%s: pass-3 seeds %s" % (name, [s["pass3"] for s in st]))
    row("nothing matches", all(rec.stats("default", "nothing", p)["intervals"] == 0 for p in (1, 0)), "nothing: no interval")
    for n in SMEM_COUNTS:
        name = "smem%d" % n
        for p in (1, 0):
            st = rec.stats("default", name, p)
            idx = [i for i, _, _ in rec.resplit("default", name, p)]
            ok = st["pass1"] == n
            for edge in (64, 128):      # re-seeded ones within eight places on both sides of the index, and one that is not
                if n > edge:
                    lo, hi = range(edge - 8, edge), range(edge, min(n, edge + 8))
                    ok = ok and any(i in idx for i in lo) and any(i in idx for i in hi) and any(i not in idx for i in lo)
            if n >= 129:
                ok = ok and max(idx) >= 128
            a = rec.intervals("default", name, p)      # every re-seeded piece of bg2 gives its slot's core: two occurrences
            ok = ok and int((a[:, 2] == 2).sum()) >= len(idx) - len([i for i in idx if i % 4 == 3])
            row("pass-1 SMEMs %d: %s parent %d" % (n, name, p), ok, "pass 1 left %d, %d re-seeded, the last at index %d" % (st["pass1"], len(idx), max(idx + [-1])))
    n3 = 0
    for name in NOP3_CASES:
        for p in (1, 0):
            row("max_mem_intv 0: %s parent %d" % (name, p), rec.stats("nop3", name, p)["pass3"] == 0, "no pass 3")
            n3 += rec.stats("default", name, p)["pass3"]
    row("max_mem_intv 0: the same cases have pass-3 seeds by default", n3 > 0, "%d" % n3)
    return rows
