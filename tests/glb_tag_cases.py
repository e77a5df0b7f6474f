"""Designed global-alignment jobs for K6 (csrc/hip/k_global.hip), shared by tests/golden/make_vectors_glbtags.py (which records what the
reference's own bis_bwa_gen_cigar2, lib/aln/bwa.c:290-430, and the band-doubling loop of mem_alnreg_setSAM, mem_alnreg_format.c:63-77, make of
them), tests/test_glb_tags_recorded_cpu.py and tests/test_gpu_glb_tags_recorded.py.

A genome of three contigs and reads by construction, from the integer generator of tests/regions_cases.py (splitmix64), so that every job's
CIGAR and the places of its mismatches are known before a kernel runs.  The recording (tests/golden/ref_glb_tags.npz) holds a CRC of the
genome and of the read buffer: tests compare them before they compare anything else.

A job is designed in alignment order -- the order in which the reference and the kernel walk it: the target is the forward sequence of
[f, f + tlen) on a forward view and its complement on a reverse view (bwa.c:307-312 reverses the reverse strand's sequences), the read is the
designed query there, reversed on a reverse view.  The design is a list of operations:

    ("M", n, {"x": columns that mismatch under both scoring matrices, "n": columns that hold N, "ct": (a, b) every C of the target in these
              columns read as T, "ga": (a, b) every G read as A})
    ("D", n)      n target bases without a query base
    ("I", n)      n query bases without a target base, chosen to mismatch the target on both sides

With qlen == tlen, w0 = 0 and n_try = 1 the reference and the kernel take the no-gap branch (bwa.c:314-322): one M of the whole length whatever
the bases are -- the pattern cases.  Everything with gaps is a DP job; "cigar" in a case is then what the design expects of the reference, and
the generator asserts it of its own recording.

What the kernel does with a job (lane_global_batch, csrc/hip/shim.hip): the size class by query length and band (QCAP, BAND), and within the
first two classes the MD walk by the wave over target bases staged in LDS when tlen <= TCAP, by one lane otherwise.  size_class() restates
that rule for the coverage table; the CPU test holds the three tables against the source.
"""
import re
import zlib
import numpy as np

from regions_cases import Ints

# ------------------------------------------------------------------------------------------ the kernel's classes (shim.hip; the CPU test compares)
QCAP = (256, 1024, 16384, 0x7fffffff)
BAND = (256, 1024, 2048, 2048)
TCAP = (512, 2048, 0, 0)
CLASS_NAMES = ("q256", "q1024", "q16384", "hbm")

CONTIGS = (("g0", 160000), ("g1", 120000), ("g2", 50000))
L_PAC = sum(n for _, n in CONTIGS)
OPTSETS = [("default", {}), ("alt", {"a": 2, "b": 3, "o_del": 5, "o_ins": 7, "e_del": 2, "e_ins": 1})]      # -A 2 -B 3 -O 5,7 -E 2,1
EXITS = ("single", "truesc", "same_score", "w_max", "tries")      # how the loop of mem_alnreg_format.c:65-77 ended (single: n_try = 1)
VIEWS = ("F1", "F0", "R1", "R0")      # view (forward / reverse), parent
CIGAR_CAP = 32

# the table tests/golden/make_vectors_glbtags.py prints of its recording; the tests compare it with coverage() of the file, by equality
COVERAGE = {"class": [65, 13, 3, 2], "walk": {"staged": 76, "lane": 7}, "view": {"F1": 23, "F0": 18, "R1": 19, "R0": 23},
            "exit": {"single": 74, "truesc": 1, "same_score": 5, "w_max": 2, "tries": 1}, "optset": {"default": 76, "alt": 7},
            "md_deletions": 36, "longest_md": 1056, "class_with_deletion": [26, 6, 2, 1], "nogap": 36}

_cache = {}


def genome():
    if "g" not in _cache:
        r = Ints(0x20261020)
        _cache["g"] = [(name, r.bases(n)) for name, n in CONTIGS]
    return _cache["g"]


def forward():
    if "f" not in _cache:
        _cache["f"] = np.concatenate([g for _, g in genome()])
    return _cache["f"]


def genome_crc():
    return zlib.crc32(forward().tobytes()) & 0xffffffff


def write_fasta(path):
    with open(path, "wb") as f:
        for name, g in genome():
            f.write(b">" + name.encode() + b"\n")
            s = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


def contig_of(f):
    """index of the contig that holds forward coordinate f"""
    off = 0
    for i, (_, n) in enumerate(CONTIGS):
        if f < off + n:
            return i
        off += n
    raise AssertionError(f)


def _differs(q, r):
    """q against r is a mismatch under both matrices: different, and neither conversion"""
    return q != r and not (q == 3 and r == 1) and not (q == 0 and r == 2)


def design(f, ops, rev, ints):
    """-> (query in alignment order, tlen, the designed CIGAR as text), or None where a deletion would not stay where the design puts it"""
    tlen = sum(o[1] for o in ops if o[0] in "MD")
    assert contig_of(f) == contig_of(f + tlen - 1), (f, tlen)
    t = forward()[f:f + tlen]
    if rev:
        t = (3 - t).astype(np.uint8)
    q, y, dels = [], 0, []
    for o in ops:
        op, n = o[0], o[1]
        if op == "M":
            m = o[2] if len(o) > 2 else {}
            seg = t[y:y + n].copy()
            for key, frm, to in (("ct", 1, 3), ("ga", 2, 0)):
                if key in m:
                    a, b = m[key]
                    w = np.nonzero(t[y + a:y + b] == frm)[0] + a
                    seg[w] = to
            for c in m.get("x", ()):
                seg[c] = t[y + c] ^ 1      # A<>C, G<>T: a mismatch under both matrices
            for c in m.get("n", ()):
                seg[c] = 4
            q.append(seg)
            y += n
        elif op == "D":
            dels.append((sum(len(x) for x in q), y, n))
            y += n
        else:      # inserted bases that mismatch the target base before and the one after, so that the gap stays where it is put
            ins = ints.bases(n)
            others = [int(t[k]) for k in (y - 1, y) if 0 <= k < tlen]
            for at in (0, n - 1):
                b = int(ins[at])
                for _ in range(4):
                    if all(_differs(b, r) for r in others):
                        break
                    b = (b + 1) % 4
                ins[at] = b
            q.append(ins)
    qq = np.concatenate(q).astype(np.uint8)
    for x, y, n in dels:      # a deletion stays where it is put: the column before it cannot take the gap's last base (the traceback would
        # move the gap left), and a mismatching column behind it cannot take the gap's first base
        if x > 0 and not _differs(int(qq[x - 1]), int(t[y + n - 1])):
            return None
        if x < len(qq) and y + n < tlen and qq[x] != t[y + n] and not _differs(int(qq[x]), int(t[y])):
            return None
    merged = []
    for o in ops:
        if merged and merged[-1][0] == o[0]:
            merged[-1][1] += o[1]
        else:
            merged.append([o[0], o[1]])
    return qq, tlen, "".join("%d%s" % (n, op) for op, n in merged)


def runs(rs, closing):
    """one M whose mismatches follow match runs of the given lengths, then `closing` matches"""
    x, at = [], 0
    for r in rs:
        at += r
        x.append(at)
        at += 1
    return [("M", at + closing, {"x": x})]


def cases():
    """[dict(name, family, seq, rb, re, parent, rev, w0, n_try, truesc, optset, nogap, cigar (designed, or None), exit (expected), has)]
    in the order of the recording"""
    if "c" in _cache:
        return _cache["c"]
    out = []
    ints = Ints(0x61B7A65)
    state = {"f": 1000, "v": 0}

    def add(name, family, ops, view=None, w0=None, n_try=1, truesc=None, optset="default", cigar="design", exit_=None, f=None, has=()):
        assert all(c["name"] != name for c in out), name
        if view is None:      # the four (view, parent) pairs in turn
            view = VIEWS[state["v"] % 4]
            state["v"] += 1
        rev, parent = view[0] == "R", int(view[1])
        auto = f is None
        f = state["f"] if auto else f
        while True:      # the first place from f on at which the design's deletions stay put
            o = ops
            if callable(ops):      # a design that looks at the target first: ops(alignment-order target at f, parent)
                o = ops((3 - forward()[f:f + 4096]).astype(np.uint8) if rev else forward()[f:f + 4096], parent)
            d = design(f, o, rev, ints)
            if d is not None:
                break
            f += 1
        q, tlen, designed = d
        if auto:
            state["f"] = f + tlen + 317
        nogap = w0 is None
        if nogap:
            assert len(q) == tlen and n_try == 1
            w0 = 0
        rb, re_ = (2 * L_PAC - (f + tlen), 2 * L_PAC - f) if rev else (f, f + tlen)
        out.append({"name": name, "family": family, "seq": np.ascontiguousarray(q[::-1] if rev else q), "rb": rb, "re": re_, "parent": parent, "rev": rev,
                    "w0": w0, "n_try": n_try, "truesc": len(q) if truesc is None else truesc, "optset": optset, "nogap": nogap,
                    "cigar": designed if cigar == "design" else cigar, "exit": exit_ or ("single" if n_try == 1 else None), "has": tuple(has), "f": f})

    # ---- digit edges, staged walk: runs of 0, 1, 9, 10, 99, 100 before a mismatch with each of them as the closing count in turn
    small = [0, 1, 9, 10, 99, 100]
    for k, c in enumerate(small):
        add("dig_mm_close%d" % c, "digit", runs(small[k:] + small[:k], c))
    # ... before a deletion (the run starts behind a mismatch; run 0: the mismatch in the column just before the D)
    for k, u in enumerate(small[1:]):
        add("dig_del%d" % u, "digit", [("M", 20 + u, {"x": [19]}), ("D", 3), ("M", 30)], w0=10, optset="alt" if u in (9, 10) else "default")

    def conv_before_d(t, parent):
        """a conversion in the column just before a D ("...C0^..."): it scores as a match, so the gap cannot move across it for free (a plain
        mismatch there ties with the gap one column to the left, which the traceback prefers)"""
        want, alike = (1, 3) if parent else (2, 0)
        m = next(m for m in range(20, 200) if t[m - 1] == want and t[m + 2] not in (want, alike))
        return [("M", m, {"ct" if parent else "ga": (m - 1, m)}), ("D", 3), ("M", 30)]
    add("dig_del0_p1", "digit", conv_before_d, view="F1", w0=10, cigar=None, has=("0^",))
    add("dig_del0_p0", "digit", conv_before_d, view="R0", w0=10, cigar=None, has=("0^",))
    # ... 999 and 1000, staged in the second class (query <= 1024, target <= 2048)
    add("dig_mm999", "digit", runs([999], 9))
    add("dig_mm1000", "digit", runs([1000], 10))
    add("dig_close999", "digit", runs([0], 999))
    add("dig_close1000", "digit", runs([1], 1000))
    add("dig_del999", "digit", [("M", 999), ("D", 5), ("M", 20)], w0=10)
    add("dig_del1000", "digit", [("M", 1000), ("D", 5), ("M", 20)], w0=10)
    # ... 9999 and 10000 in the third class (one lane)
    add("dig_del10000", "digit", [("M", 10000), ("D", 4), ("M", 60)], view="F1", w0=10)
    add("dig_mm9999", "digit", runs([9999], 10), view="R0")
    # ... 99999 and 100000: rows in HBM, a band of a few columns
    add("dig_mm100000", "digit", runs([100000], 1), view="F1", w0=3, f=2000)
    add("dig_del99999", "digit", [("M", 99999), ("D", 2), ("M", 50)], view="R0", w0=3, f=170000)
    # ---- lane and block edges of the staged walk
    for view in VIEWS:
        add("lane_cols_" + view, "lane", [("M", 200, {"x": [0, 63, 64, 127, 199]})], view=view)
    for n in (63, 64, 65, 128):
        add("lane_len%d_last" % n, "lane", [("M", n, {"x": [n - 1]})])
    add("lane_runs_63_64_65_128", "lane", [("M", 63), ("I", 2), ("M", 64), ("D", 2), ("M", 65), ("I", 1), ("M", 128), ("D", 1), ("M", 40)], w0=10)
    add("lane_clean_block", "lane", [("M", 192, {"x": [10, 150]})])
    add("lane_full_block", "lane", [("M", 192, {"x": list(range(64, 128))})])
    add("lane_all256", "lane", [("M", 256, {"x": list(range(256))})])
    add("lane_all512", "lane", [("M", 512, {"x": list(range(512))})])
    # ---- runs across operations
    for view in VIEWS:
        add("ops_mim_" + view, "ops", [("M", 50), ("I", 3), ("M", 50)], view=view, w0=10)
    add("ops_mm_after_d", "ops", [("M", 40), ("D", 3), ("M", 40, {"x": [0]})], w0=10)
    for n in (1, 63, 64, 65, 200):
        add("ops_d%d" % n, "ops", [("M", 60), ("D", n), ("M", 60)], w0=10)
    add("ops_i_first", "ops", [("I", 3), ("M", 100)], w0=10)
    add("ops_i_last", "ops", [("M", 100), ("I", 3)], w0=10)
    add("ops_d_first", "ops", [("D", 10), ("M", 150)], w0=10)
    add("ops_d_first_alt", "ops", [("D", 10), ("M", 150, {"x": [70]})], w0=10, optset="alt")
    add("ops_d_last", "ops", [("M", 150), ("D", 10)], w0=10)
    add("ops_d_near_end", "ops", [("M", 140), ("D", 5), ("M", 10)], w0=10)
    # (I next to D is not reached: n substitutions cost n * b, an insertion and a deletion of n bases 2 * o + 2 * n * e, more under both option
    # sets, so no optimal alignment holds the pair; the nearest designed is ten columns apart)
    add("ops_i_near_d", "ops", [("M", 60), ("I", 5), ("M", 10), ("D", 8), ("M", 60)], w0=20)
    # ---- the same read across a long deletion on both sides of each class's target stage
    for qh, d in ((125, 262), (125, 263), (500, 1048), (500, 1049)):
        add("tcap_t%d" % (2 * qh + d), "tcap", [("M", qh), ("D", d), ("M", qh)], view="F1" if d % 2 == 0 else "R0", w0=10, cigar=None)
    # ---- views and parents: both kinds of conversion in one read; none (retained C and G); an N
    for view in VIEWS:
        add("view_conv_" + view, "view", [("M", 150, {"ct": (0, 150), "ga": (0, 150), "x": [75]})], view=view)
        add("view_ret_" + view, "view", [("M", 150)], view=view)
        add("view_n_" + view, "view", [("M", 150, {"n": [70], "ct": (0, 60)})], view=view)
        add("view_dp_" + view, "view", [("M", 70, {"ct": (0, 70)}), ("D", 4), ("M", 80, {"ga": (40, 80), "x": [33]})], view=view, w0=10,
            optset="alt" if view in ("F0", "R1") else "default")
    add("view_conv_alt", "view", [("M", 150, {"ct": (0, 150), "ga": (0, 150)})], view="R1", optset="alt")
    # ---- the retry loop (n_try = 3)
    big = 1 << 20
    add("try_first", "retry", [("M", 150, {"x": [40]})], w0=5, n_try=3, truesc=100, exit_="truesc")
    add("try_tries", "retry", [("M", 100), ("I", 30), ("M", 200), ("D", 30), ("M", 100)], w0=8, n_try=3, truesc=big, cigar=None, exit_="tries")
    add("try_same", "retry", [("M", 100), ("D", 40), ("M", 100)], w0=5, n_try=3, truesc=big, exit_="same_score")      # min_w = 43 on every try
    add("try_wmax_first", "retry", [("M", 100), ("D", 20), ("M", 100)], w0=400, n_try=3, truesc=big, exit_="w_max")
    add("try_wmax_capped", "retry", [("M", 400), ("I", 330), ("M", 400), ("D", 330), ("M", 300)], w0=200, n_try=3, truesc=big, cigar=None, exit_="w_max")
    add("try_changes", "retry", [("M", 60), ("I", 8), ("M", 60), ("D", 8), ("M", 60)], w0=5, n_try=3, truesc=big, cigar=None, has=("changes",))
    add("try_changes_alt", "retry", [("M", 60), ("I", 8), ("M", 60), ("D", 8), ("M", 60)], w0=5, n_try=3, truesc=big, cigar=None, optset="alt", has=("changes",))
    add("try_nogap", "retry", [("M", 150, {"x": [10, 11, 90]})], w0=0, n_try=3, truesc=big, exit_="same_score")
    add("try_last_wins", "retry", [("M", 80), ("D", 12), ("M", 80, {"x": [5]})], view="R0", w0=4, n_try=3, truesc=big, cigar=None)
    _cache["c"] = out
    return out


def ordinary(n, seed):
    """n jobs of 150 bases as the aligner makes them all day (no recording: the device's forms are compared with each other): both views and
    parents, a few substitutions, bisulfite conversions, every fourth with a short insertion; n_try = 3"""
    r, out = Ints(seed), []
    while len(out) < n:
        k = len(out)
        f = 500 + r.below(L_PAC - 1000)
        if contig_of(f) != contig_of(f + 200):
            continue
        rev, parent = VIEWS[k % 4][0] == "R", int(VIEWS[k % 4][1])
        m = {"x": sorted({r.below(150) for _ in range(k % 3)}), "ct" if parent else "ga": (0, 150)}
        ops = [("M", 150, m)] if k % 4 else [("M", 70, {"x": m["x"][:1] and [m["x"][0] % 70]}), ("I", 1 + k % 3), ("M", 80)]
        q, tlen, _ = design(f, ops, rev, r)
        rb, re_ = (2 * L_PAC - (f + tlen), 2 * L_PAC - f) if rev else (f, f + tlen)
        out.append({"name": None, "seq": np.ascontiguousarray(q[::-1] if rev else q), "rb": rb, "re": re_, "parent": parent, "rev": rev,
                    "w0": (0, 3, 10, 40)[(k // 2) % 4], "n_try": 3, "truesc": len(q) - r.below(30), "optset": None, "f": f})
    return out


def read_buffer(cs=None):
    cs = cases() if cs is None else cs
    off = np.zeros(len(cs) + 1, np.int64)
    for i, c in enumerate(cs):
        off[i + 1] = off[i] + len(c["seq"])
    return np.concatenate([c["seq"] for c in cs]), off


def reads_crc():
    return zlib.crc32(read_buffer()[0].tobytes()) & 0xffffffff


def set_opt(opt, optset):
    """the option set's fields into a bsx_opt_t, matrices refilled"""
    from biscuit_amd import _lib as B
    for k, v in dict(OPTSETS)[optset].items():
        setattr(opt, k, v)
    import ctypes
    B.lib().bsx_opt_fill_matrices(ctypes.byref(opt))
    return opt


def job_of(c, qoff, cigar_off, opt, want_cigar=1):
    """the device job of a case, as bsx_setsam_job makes it (csrc/host/sam.c): the view walked from its last base on a reverse view"""
    n, tlen = len(c["seq"]), c["re"] - c["rb"]
    if c["rev"]:
        return (c["re"] - 1, qoff + n - 1, n, tlen, c["w0"], opt.w << 2, c["truesc"], c["n_try"], cigar_off, CIGAR_CAP, -1, -1, c["parent"], want_cigar)
    return (c["rb"], qoff, n, tlen, c["w0"], opt.w << 2, c["truesc"], c["n_try"], cigar_off, CIGAR_CAP, 1, 1, c["parent"], want_cigar)


def size_class(c, opt):
    """lane_global_batch's rule (shim.hip) -> (class 0..3, walk: "staged" or "lane")"""
    qlen, tlen = len(c["seq"]), c["re"] - c["rb"]
    mat0 = opt.ctmat[0] if c["parent"] else opt.gamat[0]
    wtop = min(c["w0"] << (c["n_try"] - 1), opt.w << 2)
    dl = abs(tlen - qlen)
    max_ins = int(float(((qlen + 1) >> 1) * mat0 - opt.o_ins) / opt.e_ins + 1.)
    max_del = int(float(((qlen + 1) >> 1) * mat0 - opt.o_del) / opt.e_del + 1.)
    wk = max(min((max(max_ins, max_del, 1) + dl + 1) >> 1, wtop), dl + 3)
    band = min(qlen, 2 * wk + 1)
    k = 0
    while qlen > QCAP[k] or band > BAND[k]:
        k += 1
    return k, "staged" if tlen <= TCAP[k] else "lane"


# ------------------------------------------------------------------------------------------ reading a CIGAR and an MD
def cigar_text(words):
    return "".join("%d%s" % (int(w) >> 4, "MIDSH"[int(w) & 0xf]) for w in words)


MD_TOKEN = re.compile(rb"(\d+)(\^[ACGTN]+|[ACGTN]|$)")


def md_runs(md):
    """an MD string (bytes, without its NUL) -> [(run, "mm" | "del" | "end", deleted bases)], checked to cover the whole string"""
    out, at = [], 0
    while True:
        m = MD_TOKEN.match(md, at)
        assert m, (md[:80], at)
        what = m.group(2)
        out.append((int(m.group(1)), "end" if not what else "del" if what[:1] == b"^" else "mm", max(0, len(what) - 1) if what[:1] == b"^" else 0))
        at = m.end()
        if not what:
            assert at == len(md), (md[:80], at)
            return out


# ------------------------------------------------------------------------------------------ the recording
class Recording:
    """tests/golden/ref_glb_tags.npz: per case every try's (w, score), how the loop ended, and the last try's score, CIGAR, NM, ZC, ZR, bss_u, MD"""

    def __init__(self, path):
        z = np.load(path)
        self.z = z
        self.names = [str(x) for x in z["names"]]
        self.index = {n: i for i, n in enumerate(self.names)}

    def get(self, name):
        z, i = self.z, self.index[name]
        nt = int(z["n_tries"][i])
        return {"tries": [(int(z["try_w"][i][k]), int(z["try_score"][i][k])) for k in range(nt)], "exit": EXITS[int(z["exit"][i])],
                "score": int(z["score"][i]), "w": int(z["try_w"][i][nt - 1]), "cigar": z["cigar"][int(z["cigar_off"][i]):int(z["cigar_off"][i + 1])].astype(np.uint32),
                "NM": int(z["NM"][i]), "ZC": int(z["ZC"][i]), "ZR": int(z["ZR"][i]), "bss_u": int(z["bss_u"][i]),
                "md": z["md"][int(z["md_off"][i]):int(z["md_off"][i + 1])].tobytes()}      # without the NUL


def load(path=None):
    import os
    return Recording(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glb_tags.npz"))


def coverage(rec, opts):
    """the table the generator prints and the tests hold as constants; opts: {option set: bsx_opt_t}"""
    cs = cases()
    t = {"class": [0] * 4, "walk": {"staged": 0, "lane": 0}, "view": {v: 0 for v in VIEWS}, "exit": {e: 0 for e in EXITS},
         "optset": {o: 0 for o, _ in OPTSETS}, "md_deletions": 0, "longest_md": 0, "class_with_deletion": [0] * 4, "nogap": 0}
    for c in cs:
        r = rec.get(c["name"])
        k, walk = size_class(c, opts[c["optset"]])
        t["class"][k] += 1
        t["walk"][walk] += 1
        t["view"][("R" if c["rev"] else "F") + str(c["parent"])] += 1
        t["exit"][r["exit"]] += 1
        t["optset"][c["optset"]] += 1
        nd = sum(1 for _, kind, _ in md_runs(r["md"]) if kind == "del")
        t["md_deletions"] += nd
        t["class_with_deletion"][k] += nd > 0
        t["longest_md"] = max(t["longest_md"], len(r["md"]))
        t["nogap"] += c["nogap"]
    return t
