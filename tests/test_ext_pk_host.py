"""CPU: the packed 16-bit extension row (csrc/hip/ext_pk.hpp) as a scalar restatement over int16_t halves (tests/host_ext_pk.cpp: the same
masks, scan identity, carries and guard -- the guard is the kernels' own header) against the oracle's ksw_extend2, with every intermediate
range-checked: a job the guard admits never leaves 16 bits, jobs right below its threshold included."""
import ctypes as C
import os
import subprocess
import numpy as np
import ext_pk_cases as X
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _harness():
    so = os.path.join(ROOT, "tests", "_build", "libhostextpk.so")
    src = os.path.join(ROOT, "tests", "host_ext_pk.cpp")
    deps = [src, os.path.join(ROOT, "biscuit_amd", "csrc", "hip", "ext_pk_bound.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + ROOT + "/biscuit_amd/csrc/hip", src, "-o", so])
    H = C.CDLL(so)
    H.host_ext_pk_guard.argtypes = [C.c_int] * 6 + [C.c_longlong, C.c_int]
    return H


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(H, fn, q, t, mat, gp, w, eb, zd, h0, rng_out=None):
    out = (C.c_int * 6)()
    args = [C.c_int(len(q)), _p(q), C.c_int(len(t)), _p(t), mat, C.c_int(gp[0]), C.c_int(gp[1]), C.c_int(gp[2]), C.c_int(gp[3]), C.c_int(w), C.c_int(eb),
            C.c_int(zd), C.c_int(h0), out]
    rc = fn(*(args + ([rng_out] if rng_out is not None else [])))
    return rc, list(out)


def _references():
    """the oracle's ksw_extend2 (oracle/port.c) and, where it has been built, the reference's own (oracle/_ref)"""
    refs = [oracle_lib.port_lib().oracle_extend1]
    R = oracle_lib.ref_lib()
    if R is not None:
        refs.append(R.ref_ksw_extend2)
    return refs


def test_designed_jobs_equal_oracle_and_stay_in_16_bits():
    H, refs = _harness(), _references()
    n = 0
    for si, parent, w, eb, h0, q, t in X.jobs():
        a, b, gp, zd = X.SCORINGS[si]
        o = X.opt_of(a, b, gp, zd)
        mat = o.ctmat if parent else o.gamat
        rng = (C.c_longlong * 3)()
        rc, got = _run(H, H.host_ext_pk, q, t, mat, gp, w, eb, zd, h0, rng)
        assert rc == 0, (si, len(q), h0)
        assert rng[2] == 0 and -32768 <= rng[0] and rng[1] <= 32767, (si, len(q), list(rng))
        for ref in refs:
            _, want = _run(H, ref, q, t, mat, gp, w, eb, zd, h0)
            assert got == want, (si, parent, w, eb, h0, len(q), len(t), got, want)
        n += 1
    assert n == 3 * len(X.QLENS) * 16, n      # every length x (six kinds + the two gap kinds again under the other band) x both strands, per scoring set


def test_random_jobs_at_the_guards_threshold():
    """scoring sets with a large match score and gap extension, h0 the largest the guard admits for the query: the row's largest intermediates
    sit at 32767; one more and the guard must refuse"""
    H, refs = _harness(), _references()
    rng = np.random.default_rng(77)
    n = 0
    for it in range(2000):
        qlen = int(rng.choice(X.QLENS)) if it % 2 else int(rng.integers(1, 256))
        a, b, ei = int(rng.integers(20, 120)), int(rng.integers(1, 128)), int(rng.integers(1, 20))
        gp = (int(rng.integers(0, 40)), int(rng.integers(1, 20)), int(rng.integers(0, 40)), ei)
        o = X.opt_of(a, b, gp, 100)
        parent = it & 1
        mat = o.ctmat if parent else o.gamat
        mx, mn = max(max(mat), 0), min(min(mat), 0)
        h0 = 32767 - max(255 * ei, mx) - qlen * mx
        if h0 < 1:
            continue
        assert H.host_ext_pk_guard(mx, mn, gp[0], gp[1], gp[2], gp[3], h0 + qlen * mx, qlen) == 1
        assert H.host_ext_pk_guard(mx, mn, gp[0], gp[1], gp[2], gp[3], h0 + 1 + qlen * mx, qlen) == 0
        q, t, _ = X.one_job(rng, qlen, X.KINDS[it % len(X.KINDS)], a)
        r3 = (C.c_longlong * 3)()
        w, zd, eb = (100, 200, 7, 14)[it % 4], 100, 5
        rc, got = _run(H, H.host_ext_pk, q, t, mat, gp, w, eb, zd, h0, r3)
        assert rc == 0 and r3[2] == 0 and -32768 <= r3[0] and r3[1] <= 32767, (it, qlen, h0, list(r3))
        for ref in refs:
            _, want = _run(H, ref, q, t, mat, gp, w, eb, zd, h0)
            assert got == want, (it, qlen, h0, a, b, gp, got, want)
        n += 1
    assert n >= 1200, n


def test_guard_refuses_what_does_not_fit():
    H = _harness()
    g = H.host_ext_pk_guard
    assert g(1, -2, 5, 2, 5, 2, 19 + 150, 150) == 1           # the defaults
    assert g(1, -2, 5, 2, 5, 2, 150, 256) == 0                # a query the two packed slots cannot hold
    assert g(1, -2, 5, 0, 5, 2, 150, 150) == 0                # (a gap extension of zero divides by zero in the band clamp anyway)
    assert g(1, -2, 40000, 2, 5, 2, 150, 150) == 0            # a penalty that does not fit a half
    assert g(1, -2, 30000, 2, 30000, 2, 150, 150) == 1 and g(1, -128, 32700, 2, 5, 2, 150, 150) == 0   # M - oe_del would pass -32768
    assert g(100, -4, 5, 2, 5, 28, 25500, 155) == 1 and g(100, -4, 5, 2, 5, 29, 25500, 155) == 0
