"""Designed strand searches for the region kernels (csrc/hip/k_regions.hip and, past the tiers, k_seedsw.hip and k_c2r.hip), shared by tests/golden/make_vectors_regions.py (which records
what the reference's own mem_chain, mem_chain_flt, mem_flt_chained_seeds and mem_chain2region make of them), tests/test_regions_recorded_cpu.py
and tests/test_gpu_regions_recorded.py.

A genome and reads by construction, from an integer generator of this module (splitmix64; no library's random streams), so that every
case's place relative to every table cap of the region kernels is known before a kernel runs.  The recording (tests/golden/ref_regions.npz)
holds a CRC of the genome and of the read buffer: tests compare them before they compare anything else.

The building block is a family: R copies of one unit of UNIT bases, each followed by a spacer of SPACER unique bases (more than opt.w plus
the longest read of the short tiers, so that copies never chain together).

* a read cut exactly from the unit is one SMEM with R occurrences: R chains of one seed, R regions (mem_chain_flt keeps every overlapping
  chain of equal weight, memchain.c:430-457)
* the same read with one substitution: two seeds a copy -- 2 R occurrences, R chains of two seeds, R chain records
* reads that concatenate pieces of several families' units: the totals add up (pieces are cut from inside a unit, so what follows a piece
  in the genome is the same in every copy and an SMEM ends at the same base in all of them)
* truncated copies (families t64, t65, ta, tb: the unit's first LEAD + TRUNC bases only): the read's piece starts at base LEAD of the unit and
  carries a substitution at base LEAD + TRUNC, so its first seed is found at full and truncated copies alike; the truncated copies' chains
  weigh TRUNC against the full ones' piece length and mem_chain_flt drops them: more occurrences and chains than regions.  The reads of a
  kilobase use them to reach the long stores' occurrence caps with the regions, chains and chain records inside the other caps (k<N>);
  kx1152 is the plain construction -- 1152 occurrences, chains and regions -- past the 1024 regions that the long reads' last
  chains -> regions workspace held before it was given a region for every chain the last tier exports
* tied chain starts: a read that holds the same piece twice, further apart than opt.w, over a genome that holds it once a copy -- the second
  seed lands on the start of the chain the first one made and cannot join it
* over-represented intervals: max_occ lowered below R (OVER_MAX_OCC), the visiting rule of memchain.c:325-326: with a substitution the
  second interval's seeds join chains without starting any, so the walk goes on past max_occ

What binds where.  A tier counts occurrences as the sum over intervals of min(x[2], max_occ) and refuses more than SCAP; chains cannot
outnumber occurrences and SCAP == CCAP in every store, so "chains at CCAP" needs occurrences at SCAP (the x<N> cases: both at the cap, then
both one past it, where the occurrence test -- the earlier one -- binds); the m<N> cases put the occurrences alone one past the cap with
chains and chain records inside it.  Chain records (chains of several seeds) are at PCAP / PCAP + 1 in the s<N> cases with everything else
of that store inside its caps.

ICAP edges (65 intervals in a read of 150 bases) are not reached by any case here: intervals of one strand search are SMEMs of at least
min_seed_len bases, re-seeded SMEMs and the third pass's seeds, and a designed read whose 65 of them stay within the other caps of RgSmall
was not found (lowering min_seed_len multiplies chance seeds of the 3-letter alphabets with it, whose occurrences then bind first).  The
recorded interval counts are in the file; EDGES lists none for ICAP.

RgHuge's caps (4096 / 8192) are out of scope.
"""
import zlib
import numpy as np

# ------------------------------------------------------------------------------------------ the caps (rg_common.hpp, k_c2r.hip; the CPU test compares)
STORES = {      # ICAP, SCAP, CCAP, PCAP
    "RgSmall": (64, 128, 128, 32),
    "RgMid": (128, 256, 256, 64),
    "RgMid2": (256, 512, 512, 96),
    "RgLongS": (640, 1152, 1152, 160),
    "RgLongB": (768, 1536, 1536, 288),
    "RgBig": (512, 1024, 1024, 0),
}
DEFINES = {"RG_XREGS": 64, "RG_XSEEDS": 128, "RG_QCAP": 256, "RG_QCAP_LONG": 1024}
C2R = {"RgC2rB": (256, 256), "RgC2rH": (1024, 1024), "RgC2rHL": (1024, 8192)}      # seeds of a list, regions of a strand search

# ------------------------------------------------------------------------------------------ integers
M64 = (1 << 64) - 1


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class Ints:
    """splitmix64: state += golden ratio, output = mix(state); vectorised for runs of bases"""

    def __init__(self, seed):
        self.s = seed & M64

    def words(self, n):
        k = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(self.s)
        self.s = (self.s + n * 0x9E3779B97F4A7C15) & M64
        return _mix(k)

    def below(self, n):
        return int(self.words(1)[0] % np.uint64(n))

    def bases(self, n):
        w = self.words((n + 15) // 16)      # 16 bases a word, from its high bits down
        sh = (np.uint64(62) - np.uint64(2) * np.arange(16, dtype=np.uint64))
        return ((w[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)[:n]


# ------------------------------------------------------------------------------------------ the genome
UNIT, SPACER, TRUNC = 260, 400, 40
BACKGROUND = 300000
OVER_MAX_OCC = 50
# name -> copies; "a".."d": families of equal size for sums
FAMILIES = [("f20", 20), ("f32", 32), ("f33", 33), ("f64", 64), ("f65", 65), ("f96", 96), ("f97", 97), ("f128", 128), ("f129", 129),
            ("f255", 255), ("f256a", 256), ("f256b", 256), ("f256c", 256), ("f256d", 256), ("f257", 257)]
TRUNCATED = [("t64", 64, 64), ("t65", 65, 64), ("ta", 64, 384), ("tb", 64, 384)]      # full copies, truncated copies (interleaved)
LEAD = 20      # a read's piece of a unit starts here or later: what precedes it in the genome is the same in every copy, truncated ones included
A_, C_, G_, T_ = 0, 1, 2, 3

_cache = {}


def genome():
    """[(name, nt4 codes)]: "bg" = BACKGROUND unique bases, "fam" = every family, copy after copy; and {family: its unit}"""
    if "g" in _cache:
        return _cache["g"]
    r = Ints(0x20261019)
    bg = r.bases(BACKGROUND)
    parts, units = [r.bases(SPACER)], {}
    for name, n in FAMILIES:
        u = r.bases(UNIT)
        units[name] = u
        for _ in range(n):
            parts += [u, r.bases(SPACER)]
    for name, n_full, n_trunc in TRUNCATED:
        u = r.bases(UNIT)
        u[LEAD + TRUNC] = T_      # the read's substitution there is A: differs from T under both conversions; the truncated copies go on with T
        units[name] = u
        for k in range(max(n_full, n_trunc)):
            if k < n_full:
                parts += [u, r.bases(SPACER)]
            if k < n_trunc:
                parts += [u[:LEAD + TRUNC], np.array([T_], np.uint8), r.bases(SPACER)]
    fam = np.concatenate(parts)
    _cache["g"] = ([("bg", bg), ("fam", fam)], units)
    return _cache["g"]


def genome_crc():
    return zlib.crc32(b"".join(g.tobytes() for _, g in genome()[0])) & 0xffffffff


def write_fasta(path):
    with open(path, "wb") as f:
        for name, g in genome()[0]:
            f.write(b">" + name.encode() + b"\n")
            s = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


# ------------------------------------------------------------------------------------------ reads
def _sub(seq, at, to=None):
    seq = seq.copy()
    seq[at] = (seq[at] + 2) % 4 if to is None else to      # (+ 2: A<>G, C<>T -- one of the two conversions hides it, as it would a real one)
    return seq


def _differs_both(a, b):
    """bases that differ under the C>T and under the G>A conversion"""
    ct = lambda x: T_ if x == C_ else x
    ga = lambda x: A_ if x == G_ else x
    return ct(a) != ct(b) and ga(a) != ga(b)


def _sub_both(seq, at):
    """a substitution that survives both conversions"""
    seq = seq.copy()
    for to in (A_, T_, C_, G_):
        if _differs_both(int(seq[at]), to):
            seq[at] = to
            return seq
    raise AssertionError


def piece(units, fam, start, length, sub=None):
    p = units[fam][start:start + length]
    assert len(p) == length
    return p if sub is None else _sub_both(p, sub)


def revcomp(x):
    y = x[::-1].copy()
    m = y < 4
    y[m] = 3 - y[m]
    return y


def cases():
    """[dict(name, seq, max_occ (None: the default), expect)] -- expect: recorded counts under the default option set that the coverage test
    asserts for both parents (keys of COUNT_KEYS); the order is the order of the recording"""
    if "c" in _cache:
        return _cache["c"]
    contigs, U = genome()
    bg = contigs[0][1]
    r = Ints(0xC0FFEE)
    out = []

    def add(name, seq, max_occ=None, **expect):
        assert all(c["name"] != name for c in out), name
        out.append({"name": name, "seq": np.ascontiguousarray(seq, np.uint8), "max_occ": max_occ, "expect": expect})

    def cat(*ps):
        return np.concatenate(ps)

    def join(*specs, start0=20):
        """pieces (family, length[, substitution at]) of units behind each other.  Every piece after the first starts at the first base of
        its unit (from 20 on) at which no SMEM can run across the junction under either conversion: the base that follows the piece before
        it in the genome differs from this piece's first, and this unit's base before the piece from the last base of the piece before."""
        ps, prev = [], None
        for sp in specs:
            fam, n, sub = sp if len(sp) == 3 else (sp[0], sp[1], None)      # sub: its place in the piece, or "trunc": where the truncated copies end
            u, st = U[fam], start0
            if prev is not None:
                pu, pe = prev
                while not (_differs_both(int(pu[pe]), int(u[st])) and _differs_both(int(pu[pe - 1]), int(u[st - 1]))):
                    st += 1
            assert st + n <= UNIT - 20, (fam, st, n)
            ps.append(_sub(u[st:st + n], LEAD + TRUNC - st, A_) if sub == "trunc" else piece(U, fam, st, n, sub))
            prev = (u, st + n)
        return cat(*ps)

    def exact(fams, total_len, start=20):
        n = total_len // len(fams)
        assert n >= 25
        return join(*[(f, n) for f in fams], start0=start)

    def filler(n, before, after):
        """n bases found nowhere in the genome by design, whose ends keep the SMEMs of the pieces around them (before: (unit, end of the
        piece), after: (unit, start of the piece)) from running into them"""
        f = r.bases(n)
        for at, other in ((0, int(before[0][before[1]])), (n - 1, int(after[0][after[1] - 1]))):
            while not _differs_both(int(f[at]), other):
                f[at] = (f[at] + 1) % 4
        return f

    # ---- occurrences and chains together at a cap and one past it: reads cut exactly from units
    add("x64", exact(["f64"], 150), occ=64, chains=64, records=0, regions=64)                      # regions at RG_XREGS
    add("x65", exact(["f65"], 150), occ=65, chains=65, records=0, regions=65)
    add("x128", exact(["f128"], 150), occ=128, chains=128, records=0, regions=128)                 # RgSmall SCAP / CCAP
    add("x129", exact(["f129"], 150), occ=129, chains=129, records=0, regions=129)
    add("x256", exact(["f256a"], 150), occ=256, chains=256, records=0, regions=256)                # RgMid; regions at RgC2rB's
    add("x257", exact(["f257"], 150), occ=257, chains=257, records=0, regions=257)
    add("x512", exact(["f256a", "f256b"], 150), occ=512, chains=512, records=0, regions=512)       # RgMid2
    add("x513", exact(["f256a", "f257"], 150), occ=513, chains=513, records=0, regions=513)
    add("x1024", exact(["f255", "f256a", "f256b", "f257"], 200), occ=1024, chains=1024, records=0, regions=1024)      # RgBig; regions at RgC2rH's
    add("x1025", exact(["f256a", "f256b", "f256c", "f257"], 200, start=26), occ=1025, chains=1025, records=0, regions=1025)
    # ---- occurrences alone one past a cap (and at it): a piece with a substitution (two seeds a copy) beside exact pieces
    add("m128", join(("f32", 71, 35), ("f64", 79)), occ=128, chains=96, records=32)
    add("m129", join(("f32", 71, 35), ("f65", 79)), occ=129, chains=97, records=32)
    add("m256", join(("f64", 71, 35), ("f128", 79)), occ=256, chains=192, records=64)
    add("m257", join(("f64", 71, 35), ("f129", 79)), occ=257, chains=193, records=64)
    add("m512", join(("f96", 71, 35), ("f64", 60), ("f256a", 60)), occ=512, chains=416, records=96)
    add("m513", join(("f96", 71, 35), ("f64", 60), ("f257", 60)), occ=513, chains=417, records=96)
    add("m1025", join(("f128", 71, 35), ("f256a", 50), ("f256b", 50), ("f257", 50)),
        occ=1025, chains=897, records=128)
    # ---- chain records at PCAP and one past it
    for n in (32, 33, 64, 65, 96, 97):
        add("s%d" % n, piece(U, "f%d" % n, 20, 150, sub=75), occ=2 * n, chains=n, records=n, regions=n)
    # ---- more chains than regions: truncated copies
    add("t64", join(("t64", 150, "trunc")), occ=64 + 64 + 64, chains=128, records=64, regions=64)
    add("t65", join(("t65", 150, "trunc")), occ=65 + 64 + 65, chains=129, records=65, regions=65)
    # ---- tied chain starts
    u20, u128 = U["f20"], U["f128"]
    s30 = piece(U, "f20", 20, 30)
    add("tie_small", cat(s30, filler(115, (u20, 50), (u20, 20)), s30), tied=1)      # fewer than 128 occurrences
    two = piece(U, "f20", 20, 71, sub=35)
    add("tie_multi", cat(two, filler(115, (u20, 91), (u20, 20)), two[:35]), tied=1)      # the tie on a chain of two seeds
    s30b = piece(U, "f128", 20, 30)
    add("tie_mid", cat(s30b, filler(115, (u128, 50), (u128, 20)), s30b), tied=1)      # past RgSmall; inside RgMid but for the tie
    # ---- over-represented intervals: max_occ below the copies (and the same reads under the default, x64b / s64b)
    add("over_x64", exact(["f64"], 150, start=40), max_occ=OVER_MAX_OCC, over=1)
    add("over_s64", piece(U, "f64", 40, 150, sub=75), max_occ=OVER_MAX_OCC, over=2)
    add("x64b", exact(["f64"], 150, start=40), occ=64, chains=64, regions=64)
    add("s64b", piece(U, "f64", 40, 150, sub=75), occ=128, chains=64, records=64, regions=64)
    # ---- read lengths at the short tiers' row length
    for n in (255, 256, 257):
        add("len%d" % n, U["f20"][:n], occ=20, chains=20, regions=20)
    # ---- reads of a kilobase: unique sequence at the long tiers' row length, and the long stores' occurrence caps
    add("len1024", bg[100000:101024], regions=1)
    add("len1025", bg[110000:111025], regions=1)
    # (a truncated family's piece: 128 + 384 occurrences, 448 chains, 64 chain records, 64 regions)
    add("k1152", join(("ta", 200, "trunc"), ("f256a", 200), ("f256b", 200), ("f128", 200), start0=21), occ=1152, chains=1088, records=64, regions=704)      # RgLongS SCAP
    add("k1153", join(("ta", 200, "trunc"), ("f256a", 200), ("f257", 200), ("f128", 200), start0=21), occ=1153, chains=1089, records=64, regions=705)
    add("k1536", join(("ta", 200, "trunc"), ("tb", 200, "trunc"), ("f256a", 200), ("f256b", 200)), occ=1536, chains=1408, records=128, regions=640)      # RgLongB SCAP
    add("k1537", join(("ta", 200, "trunc"), ("tb", 200, "trunc"), ("f256a", 200), ("f257", 200)), occ=1537, chains=1409, records=128, regions=641)
    add("kx1152", exact(["f255", "f256a", "f256b", "f257", "f128"], 1000), regions=1152)
    # ---- two dozen ordinary strand searches: unique sequence, both strands, substitutions, an indel, an N
    for k in range(12):
        at = 5000 + 20000 * k + r.below(1000)
        s = bg[at:at + 150].copy()
        if k % 2:
            s = revcomp(s)
        for _ in range(k % 4):
            s = _sub(s, r.below(150))
        if k == 5:
            s = np.concatenate([s[:70], s[73:], bg[at + 150:at + 153] if not k % 2 else revcomp(bg[at - 3:at])])      # a deletion of three bases
        if k == 6:
            s = np.concatenate([s[:60], r.bases(2), s[60:148]])      # an insertion of two
        if k == 7:
            s[81] = 4      # an N
        assert len(s) == 150
        add("ord%02d" % k, s, regions_min=1)
    _cache["c"] = out
    return out


COUNT_KEYS = ("regions", "intervals", "visited", "occ", "chains", "records", "kept", "tied", "max_seeds", "over")
OPTSETS = [("default", {}), ("filter", {"min_chain_weight": 5})]


def long_group(case):
    """a regions batch takes the long reads' launches when its longest read exceeds RG_QCAP: such reads are run as a batch of their own"""
    return len(case["seq"]) > DEFINES["RG_QCAP"]


def read_buffer(cs):
    """the cases' reads behind each other -> (buffer, offsets)"""
    off = np.zeros(len(cs) + 1, np.int64)
    for i, c in enumerate(cs):
        off[i + 1] = off[i] + len(c["seq"])
    return np.concatenate([c["seq"] for c in cs]), off


def reads_crc():
    return zlib.crc32(read_buffer(cases())[0].tobytes()) & 0xffffffff


# ------------------------------------------------------------------------------------------ which case sits at which cap, on which side
# (store or launch, dimension, case at the cap, case one past it); asserted from the recording by tests/test_regions_recorded_cpu.py
EDGES = [
    ("RgSmall", "occ", "x128", "x129"), ("RgSmall", "chains", "x128", "x129"), ("RgSmall", "occ", "m128", "m129"), ("RgSmall", "records", "s32", "s33"),
    ("RgMid", "occ", "x256", "x257"), ("RgMid", "chains", "x256", "x257"), ("RgMid", "occ", "m256", "m257"), ("RgMid", "records", "s64", "s65"),
    ("RgMid2", "occ", "x512", "x513"), ("RgMid2", "chains", "x512", "x513"), ("RgMid2", "occ", "m512", "m513"), ("RgMid2", "records", "s96", "s97"),
    ("RgBig", "occ", "x1024", "x1025"), ("RgBig", "chains", "x1024", "x1025"), ("RgBig", "occ", "x1024", "m1025"),
    ("RgLongS", "occ", "k1152", "k1153"), ("RgLongB", "occ", "k1536", "k1537"),
    ("RG_XREGS", "regions", "x64", "x65"), ("RG_XREGS", "regions", "t64", "t65"), ("RgC2rB", "regions", "x256", "x257"), ("RgC2rH", "regions", "x1024", "x1025"),
]
_DIM = {"occ": 1, "chains": 2, "records": 3}


def edge_cap(store, dim):
    if store in STORES:
        return STORES[store][_DIM[dim]]
    if store in C2R:
        return C2R[store][1]
    return DEFINES[store]


# ------------------------------------------------------------------------------------------ the recording
REGION_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep", "bss", "parent")


class Recording:
    """tests/golden/ref_regions.npz: per (option set, case, parent) the reference's counts and its region list as an array of the layout
    of bsx_region_t (frac_rep from its recorded bits)"""

    def __init__(self, path):
        from biscuit_amd import _lib as B
        z = np.load(path)
        self.z = z
        self.names = [str(x) for x in z["names"]]
        self.optsets = [str(x) for x in z["optsets"]]
        self.dt = np.dtype(B.Region)
        self.key = {(self.optsets[int(o)], self.names[int(c)], int(p)): k for k, (o, c, p) in enumerate(zip(z["rec_opt"], z["rec_case"], z["rec_parent"]))}
        self.cnt = z["rec_cnt"]
        self.same, self.off = z["rec_same"], z["rec_off"]

    def counts(self, optset, name, parent):
        return self.cnt[self.key[(optset, name, parent)]]

    def regions(self, optset, name, parent):
        k = self.key[(optset, name, parent)]
        src = int(self.same[k]) if self.same[k] >= 0 else k
        a, b = int(self.off[src]), int(self.off[src + 1])
        z = self.z
        out = np.zeros(b - a, self.dt)
        out["rb"] = z["rb"][a:b]
        out["re"] = z["rb"][a:b] + z["rlen"][a:b]
        for f in ("qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "bss"):
            out[f] = z[f][a:b]
        out["frac_rep"] = z["frac_rep"][a:b].astype(np.uint32).view(np.float32)
        out["parent"] = parent
        assert len(out) == self.cnt[k][0]
        return out


def load(path=None):
    import os
    return Recording(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_regions.npz"))


def same_regions(got, want):
    """field for field, in order; frac_rep by its bits -> None, or a text naming the first difference"""
    if len(got) != len(want):
        return "%d regions, recorded %d" % (len(got), len(want))
    for f in REGION_FIELDS:
        a, b = got[f], want[f]
        if f == "frac_rep":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not (a == b).all():
            i = int(np.nonzero(a != b)[0][0])
            return "region %d of %d: %s = %r, recorded %r (got %r, recorded %r)" % (i, len(got), f, a[i], b[i], got[i], want[i])
    return None
