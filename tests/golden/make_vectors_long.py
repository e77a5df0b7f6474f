#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_long.npz: ksw_extend2 / ksw_align2 / ksw_global2 inputs and the REAL reference's outputs at the
shapes where the device dispatch changes kernel -- every query-length class, band class and HBM row scheme of lane_extend_batch /
lane_sw_batch / lane_global_batch (shim.hip) and the register window of ext_dp_win.  Same entry points and array layout as
make_vectors.py (which stays what it is, with its own random stream), under the key prefixes lext_ / lsw_ / lgl_.

Targets are N-free (the GPU tests lay them into a scratch genome, which cannot hold N); a few extension and local-alignment queries carry
an N.  Query and target are mutated copies of each other.

    make -C oracle && python tests/golden/make_vectors_long.py

prints the per-family and per-class counts that tests/test_gpu_golden.py holds as constants."""
import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simdata  # noqa: E402
import oracle_lib  # noqa: E402

R = oracle_lib.ref_lib()
assert R is not None, "oracle/_ref/libbiscuit_ref.so missing: run `make -C oracle`"
u8p, i8p = C.POINTER(C.c_uint8), C.POINTER(C.c_int8)
rng = np.random.default_rng(20261017)
XSTART, XSUBO, XBYTE = 0x80000, 0x40000, 0x10000


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
    return (np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)), off


def bases(n):
    return rng.integers(0, 4, n).astype(np.uint8)


def mutate(seq, sub, ind):
    return simdata.mutate(seq, rng, sub, ind)


def scoring(b_set=(2, 2, 4, 1)):
    return int(rng.choice([1, 1, 1, 2])), int(rng.choice(list(b_set))), int(rng.integers(1, 3))


EXT_GAPS = [[6, 1, 6, 1], [6, 1, 6, 1], [5, 2, 7, 1], [1, 1, 1, 1], [12, 2, 12, 2]]
SW_GAPS = [[6, 1, 6, 1], [6, 1, 6, 1], [5, 2, 7, 1], [1, 1, 1, 1], [2, 1, 3, 1]]
GL_GAPS = [[6, 1, 6, 1], [6, 1, 6, 1], [5, 2, 7, 1], [1, 1, 1, 1]]

# ------------------------------------------------------------------------------------------ extension
ext, ext_fam = [], {}


def ext_job(fam, qlen, w, sub, ind, h0=None, gp=None, sc=None, zd=None, eb=None, with_n=False):
    a, b, which = sc if sc else scoring()
    gp = [int(x) for x in (gp if gp else rng.choice(EXT_GAPS))]
    core = bases(qlen + int(rng.integers(0, 250)))
    q = core[:qlen].copy()
    t = mutate(core, sub, ind)
    if with_n:
        q[rng.integers(0, qlen)] = 4
    zd = int(rng.choice([100, 100, 20, 0])) if zd is None else zd
    eb = int(rng.choice([10, 5, 0])) if eb is None else eb
    h0 = int(rng.integers(1, 601)) if h0 is None else h0
    o = (C.c_int * 6)()
    R.ref_ksw_extend2(len(q), P(q, u8p), len(t), P(t, u8p), P(mat(which, a, b), i8p), gp[0], gp[1], gp[2], gp[3], w, eb, zd, h0, o)
    ext.append((q, t, [a, b, which] + gp + [w, eb, zd, h0], list(o)))
    ext_fam[fam] = ext_fam.get(fam, 0) + 1
    return list(o)


# 320 jobs of 256..1000 bases, bands of 201, 255 and 401 columns; 140 of them 5-10 % diverged with scoring under which they survive
n_div_alive = n_narrow = 0
for it in range(320):
    w = (100, 127, 200)[it % 3] if it % 16 else 127
    n_narrow += w <= 127
    if it % 16 < 7:
        o = ext_job("bulk", int(rng.integers(256, 1001)), w, float(rng.choice([0.05, 0.07, 0.1])), float(rng.choice([0, 0.01])),
                    sc=(int(rng.choice([1, 2])), int(rng.choice([1, 2])), int(rng.integers(1, 3))), zd=int(rng.choice([100, 0])))
        n_div_alive += o[2] > 200
    else:
        ext_job("bulk", int(rng.integers(256, 1001)), w, float(rng.choice([0, 0.02, 0.1, 0.3])), float(rng.choice([0, 0.01, 0.05])), with_n=it % 20 == 9)
assert n_narrow >= 150 and n_div_alive >= 100, (n_narrow, n_div_alive)
# class edges: x4_max_query(10) = 159 | 160, x4_max_query(16) = 255, QCAP 256 | 1024
for qlen in (159, 160, 161, 255, 256, 257, 1023, 1024, 1025):
    for w in (100, 100, 5):
        ext_job("class_edge", qlen, w, 0.02, 0.01)
# band edges: 255 | 257 and 511 | 513 columns (BAND[0], BAND[1]); once as drawn, once with cheap gaps and a high h0 so that the band stays wide
for w in (127, 128, 255, 256):
    ext_job("band_edge", int(rng.integers(690, 711)), w, 0.02, 0.01)
    ext_job("band_edge", int(rng.integers(690, 711)), w, 0.07, 0.01, h0=500, gp=[1, 1, 1, 1], sc=(1, 1, 1), zd=0)
for w in (300, 511):
    ext_job("band_edge", int(rng.integers(1490, 1511)), w, 0.02, 0.01)
    ext_job("band_edge", int(rng.integers(1490, 1511)), w, 0.07, 0.01, h0=500, gp=[1, 1, 1, 1], sc=(1, 1, 2), zd=0)
# the 16 384 class (k_extend<32>, rows in LDS)
for it in range(30):
    ext_job("q16384", int(rng.integers(1025, 4001)), int(rng.choice([100, 100, 200, 5])), float(rng.choice([0, 0.02, 0.07])), float(rng.choice([0, 0.005])), with_n=it == 7)
ext_job("q16384", 16384, 100, 0.02, 0.002, zd=100, sc=(1, 2, 1))
# rows in HBM: two true continuations and one that is drawn like the others
for it in range(3):
    o = ext_job("hbm", int(rng.integers(16385, 17501)), 100, 0.02, 0.002, zd=100 if it < 2 else None, sc=(1, int(rng.choice([2, 4])), 1 + it % 2) if it < 2 else None,
                gp=[6, 1, 6, 1] if it < 2 else None)
    assert it == 2 or o[0] > 5000, o
# a first row whose non-zero entries run past column 320 (the window's first five slots)
for it in range(10):
    ext_job("wide_first_row", int(rng.integers(420, 901)), (100, 127)[it % 2], float(rng.choice([0.02, 0.07])), 0.01, h0=int(rng.integers(400, 601)),
            gp=[[6, 1, 6, 1], [1, 1, 1, 1]][it % 2])
out = {}
out["lext_q"], out["lext_qoff"] = ragged([e[0] for e in ext], np.uint8)
out["lext_t"], out["lext_toff"] = ragged([e[1] for e in ext], np.uint8)
out["lext_par"] = np.array([e[2] for e in ext], np.int32)
out["lext_out"] = np.array([e[3] for e in ext], np.int32)

# ------------------------------------------------------------------------------------------ local alignment
sw, sw_fam = [], {}
n_planted = 0


def sw_job(fam, qlen, extra, sub, ind, xtra, plant=False, sc=None, with_n=False):
    global n_planted
    a, b, which = sc if sc else scoring((2, 2, 4, 1, 9, 20))
    gp = [int(x) for x in rng.choice(SW_GAPS)]
    q = bases(qlen)
    body = mutate(q, sub, ind)
    tail = bases(max(0, extra - (len(body) - qlen)))
    if plant:      # a second copy of half the query behind the first
        half = qlen // 2
        assert len(tail) >= half + 20, (qlen, extra)
        at = int(rng.integers(10, len(tail) - half - 9))
        tail[at:at + half] = q[:half]
        n_planted += 1
        head = bases(0)
    else:
        cut = int(rng.integers(0, len(tail) + 1))
        head, tail = tail[:cut], tail[cut:]
    t = np.concatenate([head, body, tail]).astype(np.uint8)
    if with_n:
        q[rng.integers(0, qlen)] = 4
    o = (C.c_int * 7)()
    q1, t1 = q.copy(), t.copy()
    R.ref_ksw_align2(len(q1), P(q1, u8p), len(t1), P(t1, u8p), P(mat(which, a, b), i8p), gp[0], gp[1], gp[2], gp[3], xtra, o)
    sw.append((q, t, [a, b, which] + gp + [xtra], list(o)))
    sw_fam[fam] = sw_fam.get(fam, 0) + 1
    return list(o)


def xtra16():
    x = XSTART | (XSUBO if rng.random() < 0.7 else 0) | int(rng.choice([19, 30, 10]))
    if rng.random() < 0.05:
        x &= ~XSTART
    return x


for it in range(40):
    qlen = int(rng.integers(257, 1025))
    plant = it % 3 == 0
    sw_job("q1024", qlen, qlen // 2 + int(rng.integers(40, 500)) if plant else int(rng.integers(0, 1101)), float(rng.choice([0, 0.02, 0.1, 0.3])),
           float(rng.choice([0, 0.01, 0.05])), xtra16(), plant, with_n=it == 5)
for it in range(40):
    plant = it % 3 == 0
    qlen = int(rng.integers(1025, 2001 if plant else 3073))
    sw_job("q3072", qlen, 1100 if plant else int(rng.integers(0, 1101)), float(rng.choice([0, 0.02, 0.1])), float(rng.choice([0, 0.01, 0.05])), xtra16(), plant,
           with_n=it == 5)
for qlen in (255, 256, 257, 1023, 1024, 1025, 3071, 3072):      # (the query is padded to a multiple of 8 columns)
    sw_job("class_edge", qlen, int(rng.integers(100, 1101)), 0.02, 0.01, XSTART | XSUBO | 19)
assert n_planted * 4 >= 88
# byte mode at the stripe-count edges of k_swl, with and without the start pass
for qlen in (15, 16, 17, 31, 32, 33, 240, 241, 255, 256):
    for xs in (XSTART, 0):
        sw_job("byte_edge", qlen, int(rng.integers(50, 600)), 0.1, 0.01, xs | XSUBO | XBYTE | 10, sc=(1, int(rng.choice([2, 4])), int(rng.integers(1, 3))))
# byte mode that reaches 255: whatever ksw_align2 answers then
n_sat = 0
for it in range(10):
    o = sw_job("byte_saturated", int(rng.integers(150, 251)), int(rng.integers(50, 600)), 0.005, 0.0, (XSTART if it % 2 == 0 else 0) | XSUBO | XBYTE | 19,
               sc=(2, int(rng.choice([2, 4, 1])), int(rng.integers(1, 3))))
    n_sat += o[0] == 255
assert n_sat == 10, n_sat
out["lsw_q"], out["lsw_qoff"] = ragged([e[0] for e in sw], np.uint8)
out["lsw_t"], out["lsw_toff"] = ragged([e[1] for e in sw], np.uint8)
out["lsw_par"] = np.array([e[2] for e in sw], np.int32)
out["lsw_out"] = np.array([e[3] for e in sw], np.int32)

# ------------------------------------------------------------------------------------------ global alignment
gl, gl_fam = [], {}
CIG_CAP = 1 << 16


def w_limit(lq, lt, a, gp):
    """the widest band bis_bwa_gen_cigar2 (bwa.c:325-333) leaves as it is -- the rule of test_global_kernel_vs_reference_vectors"""
    max_ins = int(float(((lq + 1) >> 1) * a - gp[2]) / gp[3] + 1.)
    max_del = int(float(((lq + 1) >> 1) * a - gp[0]) / gp[1] + 1.)
    return (max(max_ins, max_del, 1) + abs(lt - lq) + 1) >> 1


def gl_job(fam, q, t, w, wc, a, b, which, gp):
    d = abs(len(t) - len(q))
    assert d + 3 <= w <= w_limit(len(q), len(t), a, gp), (fam, len(q), len(t), w, w_limit(len(q), len(t), a, gp))
    cg = (C.c_uint32 * CIG_CAP)(); n = C.c_int()
    s = R.ref_ksw_global2(len(q), P(q, u8p), len(t), P(t, u8p), P(mat(which, a, b), i8p), gp[0], gp[1], gp[2], gp[3], w, wc, C.byref(n), cg, CIG_CAP)
    assert n.value <= CIG_CAP
    gl.append((q, t, [a, b, which] + gp + [w, wc], s, np.array(cg[:n.value], np.uint32)))
    gl_fam[fam] = gl_fam.get(fam, 0) + 1
    return n.value


def gl_drawn(fam, n, sub, ind, w=None, wc=None, by_query=False, a=None):
    """target of n bases and its mutated copy as the query (by_query: the other way round, for an exact query length)"""
    a_, b, which = scoring()
    a = a_ if a is None else a
    gp = [int(x) for x in rng.choice(GL_GAPS)]
    x = bases(n)
    y = mutate(x, sub, ind)
    q, t = (x, y) if by_query else (y, x)
    d = abs(len(t) - len(q))
    if w is None:
        w = min(d + int(rng.choice([3, 5, 20, 100, 400])), w_limit(len(q), len(t), a, gp))
    return gl_job(fam, q, t, w, int(rng.random() < 0.8) if wc is None else wc, a, b, which, gp)


for it in range(60):
    gl_drawn("t1024", int(rng.integers(300, 1025)), float(rng.choice([0, 0.02, 0.1])), float(rng.choice([0, 0.01, 0.05])))
for it in range(40):
    gl_drawn("t3000", int(rng.integers(1025, 3001)), float(rng.choice([0, 0.02, 0.1])), float(rng.choice([0, 0.01, 0.03])))
for qlen in (255, 256, 257, 1023, 1024, 1025):
    gl_drawn("class_edge", qlen, 0.02, 0.01, wc=1, by_query=True)
# band edges of BAND = {256, 1024, 2048}: 255 | 257, 1023 | 1025 and 2001 columns
for w in (127, 128):
    gl_drawn("band_edge", 600, 0.05, 0.01, w=w, wc=1, by_query=True)
for w in (511, 512):
    gl_drawn("band_edge", 2200, 0.05, 0.005, w=w, wc=1, by_query=True)
gl_drawn("band_edge", 4100, 0.05, 0.003, w=1000, wc=1, by_query=True, a=1)
# the last LDS class at its limit, and rows in HBM: indels at 0.2 %, dozens of CIGAR operations
for qlen in (16384, int(rng.integers(16385, 17501)), int(rng.integers(16385, 17501))):
    a_, b, which = scoring()
    q = bases(qlen)
    t = mutate(q, 0.02, 0.002)
    n_ops = gl_job("q16384" if qlen <= 16384 else "hbm", q, t, max(100, abs(len(t) - qlen) + 3), 1, a_, b, which, [6, 1, 6, 1])
    assert n_ops >= 24, n_ops
assert all((e[0] < 4).all() for e in gl)
out["lgl_q"], out["lgl_qoff"] = ragged([e[0] for e in gl], np.uint8)
out["lgl_t"], out["lgl_toff"] = ragged([e[1] for e in gl], np.uint8)
out["lgl_par"] = np.array([e[2] for e in gl], np.int32)
out["lgl_score"] = np.array([e[3] for e in gl], np.int32)
out["lgl_cigar"], out["lgl_coff"] = ragged([e[4] for e in gl], np.uint32)
assert all((e[1] < 4).all() for e in ext + sw + gl), "targets are N-free"

path = os.path.join(HERE, "ref_vectors_long.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 600 * 1000

# ------------------------------------------------------------------------------------------ the counts the tests hold as constants
print("families: ext", ext_fam, "sw", sw_fam, "gl", gl_fam)
print("ext: diverged and alive", n_div_alive, "| sw: planted", n_planted, "score2 > 0:", sum(e[3][3] > 0 for e in sw), "| gl: with CIGAR", sum(e[2][8] for e in gl))
for name in ("ref_vectors.npz", "ref_vectors_long.npz"):
    V = np.load(os.path.join(HERE, name))
    p = "l" if "long" in name else ""
    qo, to = V[p + "ext_qoff"], V[p + "ext_toff"]
    ok = [i for i in range(len(qo) - 1) if to[i + 1] > to[i] and not (V[p + "ext_t"][to[i]:to[i + 1]] > 3).any()]
    ql = np.diff(qo)[ok]
    w = V[p + "ext_par"][ok, 7]
    band = np.minimum(ql, 2 * w + 1)
    cls = {}      # (class by query length, class by band columns): the kernel class is the larger of the two (shim.hip, lane_extend_batch)
    for q_, b_ in zip(ql, band):
        k = (int(sum(q_ > x for x in (256, 1024, 16384))), int(sum(b_ > x for x in (256, 512))))
        assert b_ <= 2048
        cls[k] = cls.get(k, 0) + 1
    print(name, "ext: wavefront", len(ok), "by (query, band) class", dict(sorted(cls.items())), "window", int((2 * w + 1 <= 256).sum()), "quarter/lane", int((ql <= 255).sum()))
    qo, to = V[p + "sw_qoff"], V[p + "sw_toff"]
    ok = [i for i in range(len(qo) - 1) if to[i + 1] > to[i] and not (V[p + "sw_t"][to[i]:to[i + 1]] > 3).any()]
    cls = {}
    for i in ok:
        byte = bool(V[p + "sw_par"][i, 7] & XBYTE)
        pad = 16 if byte else 8
        Q = (int(qo[i + 1] - qo[i]) + pad - 1) // pad * pad
        c = "swl" if byte and Q <= 256 else 256 if Q <= 256 else 1024 if Q <= 1024 else 3072
        cls[c] = cls.get(c, 0) + 1
    print(name, "sw:", len(ok), "by class", cls)
    qo, to = V[p + "gl_qoff"], V[p + "gl_toff"]
    cls, n_cig = {}, 0
    for i in range(len(qo) - 1):
        q_, t_ = V[p + "gl_q"][qo[i]:qo[i + 1]], V[p + "gl_t"][to[i]:to[i + 1]]
        a, b, which, od, ed, oi, ei, w, wc = [int(x) for x in V[p + "gl_par"][i]]
        if len(t_) == 0 or (t_ > 3).any() or (q_ > 3).any() or w > w_limit(len(q_), len(t_), a, [od, ed, oi, ei]):
            continue
        band = min(len(q_), 2 * w + 1)
        c = 0
        while len(q_) > (256, 1024, 16384, 1 << 31)[c] or band > (256, 1024, 2048, 2048)[c]:
            c += 1
        cls[c] = cls.get(c, 0) + 1
        n_cig += wc
    print(name, "gl:", sum(cls.values()), "by class", dict(sorted(cls.items())), "with CIGAR", n_cig)
