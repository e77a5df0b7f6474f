"""CPU: the packed 16-bit seed-filter alignment (k_swl16, csrc/hip/k_seedsw.hip) as a lane-by-lane scalar restatement (tests/host_ssw16.cpp:
8 lanes x 2 halves a job pair, the wave's shared stripe and row counts, the biased byte profile, the closed form of the lazy-F loop; the guard
is the kernel's own header) against the scores recorded from the reference's ksw_align2, under every ordering of tests/ssw_cases.py, with every
16-bit value range-checked: no option set the guard admits leaves [0, 32767]."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ssw_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _harness():
    so = os.path.join(ROOT, "tests", "_build", "libhostssw16.so")
    src = os.path.join(ROOT, "tests", "host_ssw16.cpp")
    deps = [src, os.path.join(ROOT, "biscuit_amd", "csrc", "hip", "ssw16_bound.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + ROOT + "/biscuit_amd/csrc/hip", src, "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(H, V, key, lst):
    """the list through the restatement: (return code, score per entry, [lo, hi, bad])"""
    ct, ga = S.mats_of(key)
    ids = np.array(lst, np.int64)
    real = ids != S.FILLER
    safe = np.where(real, ids, 0)
    qlen = np.where(real, V.qlen[safe], 0).astype(np.int32); tlen = np.where(real, V.tlen[safe], 0).astype(np.int32)
    qoff = np.ascontiguousarray(V.qoff[safe], np.int64); toff = np.ascontiguousarray(V.toff[safe], np.int64)
    use_ct = np.ascontiguousarray(V.use_ct[safe], np.uint8)
    q, t = np.ascontiguousarray(V.q, np.uint8), np.ascontiguousarray(V.t, np.uint8)
    scores = np.full(len(ids), -7, np.int32)
    rng = (C.c_longlong * 3)()
    rc = H.host_ssw16(C.c_int(len(ids)), _p(qlen), _p(tlen), _p(qoff), _p(toff), _p(use_ct), _p(q), _p(t), _p(ct), _p(ga),
                      C.c_int(key[2]), C.c_int(key[3]), C.c_int(key[4]), C.c_int(key[5]), _p(scores), rng)
    return rc, scores, list(rng)


@pytest.fixture(scope="module")
def V():
    return S.Vectors()


@pytest.mark.parametrize("ordering", S.ORDERINGS)
def test_restatement_equals_recorded_and_stays_in_15_bits(V, ordering):
    H = _harness()
    seen, n_refused, top = [], 0, 0
    for key, ids in V.groups().items():
        lst = S.orderings(V, ids)[ordering]
        rc, scores, rng = _run(H, V, key, lst)
        if V.refused[ids[0]]:
            assert rc == -2, key      # the nearest option sets beyond the guard
            n_refused += 1
            continue
        assert rc == 0, key
        assert rng[2] == 0 and 0 <= rng[0] and rng[1] <= 32767, (key, rng)
        top = max(top, rng[1])
        want = np.array([V.score[i] if i != S.FILLER else 0 for i in lst])
        bad = np.nonzero(scores != want)[0]
        assert len(bad) == 0, (key, [(lst[k], int(scores[k]), int(want[k])) for k in bad[:5]])
        seen += [i for i in lst if i != S.FILLER]
    assert n_refused == S.N_REFUSED_SETS
    assert V.family_counts(seen) == S.FAMILY_COUNTS_ADMITTED
    assert S.score_classes(V.score[sorted(set(seen))]) == S.SCORE_CLASSES_ADMITTED
    assert top > 32767 - 500, top      # the option sets at the guard bring the largest value formed to the top of the range


@pytest.mark.parametrize("n", S.LIST_LENGTHS)
def test_short_lists(V, n):
    """lists that end inside a wavefront, at its end, and one job into the next"""
    H = _harness()
    m = 0
    for key, ids in V.groups().items():
        if V.refused[ids[0]] or len(ids) < n:
            continue
        lst = S.orderings(V, ids)["shuffled"][:n]
        rc, scores, rng = _run(H, V, key, lst)
        assert rc == 0 and rng[2] == 0
        assert (scores == V.score[lst]).all(), (key, n)
        m += 1
    assert m >= 8      # (of the 11 admitted option sets, three hold fewer than 31 vectors)


def test_orderings_put_the_right_jobs_side_by_side(V):
    """what the orderings are for, checked on the file itself: the pairs that share a lane's registers"""
    G = V.groups()
    big = lambda i: i != S.FILLER and V.qlen[i] == 199 and V.tlen[i] == 199
    small = lambda i: i != S.FILLER and V.qlen[i] <= 8 and V.tlen[i] == 1
    hi = lambda i: i != S.FILLER and V.score[i] >= 16384
    lo = lambda i: i != S.FILLER and V.score[i] < 256
    n_ls = n_hl = n_lh = n_hh = n_m = n_f = 0
    for key, ids in G.items():
        o = S.orderings(V, ids)
        n_ls += sum(big(a) and small(b) for a, b in S.neighbours(o["long_short"]))
        n_hl += sum(hi(a) and lo(b) for a, b in S.neighbours(o["high_low"]))
        n_lh += sum(lo(a) and hi(b) for a, b in S.neighbours(o["high_low"]))
        n_hh += sum(hi(a) and hi(b) for a, b in S.neighbours(o["as_generated"]))
        n_m += sum(V.use_ct[a] != V.use_ct[b] for a, b in S.neighbours(o["matrices"]))
        f = o["fillers"]
        n_f += all(x == S.FILLER for x in f[16:32]) and sum((a == S.FILLER) != (b == S.FILLER) for a, b in S.neighbours(f)) >= 8
    assert n_ls >= 16 and n_hl >= 10 and n_lh >= 10 and n_hh >= 20 and n_m >= 200 and n_f == len(G), (n_ls, n_hl, n_lh, n_hh, n_m, n_f)
    # the two layouts put windows at both ends of both strands
    for which in (0, 1):
        g, tpos = S.layout(V, which)
        l_pac = len(g)
        admitted = [i for i in range(V.n) if not V.refused[i]]      # (windows of vectors that both forms score)
        assert S.strand_ends(V, tpos, l_pac, admitted) == ({("start", 0), ("end", 1)} if which == 0 else {("start", 1), ("end", 2)})
        for i in (0, 1, V.n - 2, V.n - 1):      # what a kernel reads at tpos + k is the recorded target
            t = V.t[V.toff[i]:V.toff[i + 1]]
            read = [int(g[p]) if p < l_pac else 3 - int(g[2 * l_pac - 1 - p]) for p in range(int(tpos[i]), int(tpos[i]) + len(t))]
            assert read == [int(x) for x in t]
    assert {120, 128, 136, 184, 192, 200} <= S.padded_queries(V, range(V.n))      # both sides of the sw_pass<2|3|4> edges


def test_empty_target_beside_other_jobs(V):
    """a query against a target of no bases scores 0 and leaves its neighbours' scores alone"""
    H = _harness()
    key, ids = next((k, v) for k, v in V.groups().items() if not V.refused[v[0]])
    lst = ids[:19]
    keep = V.tlen.copy()
    try:
        for k in (0, 3, 18):
            V.tlen[lst[k]] = 0
        rc, scores, rng = _run(H, V, key, lst)
    finally:
        V.tlen[:] = keep
    assert rc == 0 and rng[2] == 0
    assert [int(x) for x in scores] == [0 if k in (0, 3, 18) else int(V.score[lst[k]]) for k in range(19)]


def test_guard_at_its_limit():
    g = _harness().host_ssw16_guard
    assert g(1, -2, 6, 1, 6, 1) == 1                                              # the defaults
    assert g(127, -128, 1028, 30, 1028, 30) == 1 and g(127, -128, 1029, 30, 1029, 30) == 0
    assert g(100, -100, 73, 10, 11, 72) == 1 and g(100, -100, 73, 10, 11, 73) == 0
    assert g(127, -128, 3594, 1, 3594, 1) == 1 and g(127, -128, 3595, 1, 3595, 1) == 0
    assert g(1, -2, 6, 1, 40000, 1) == 0 and g(1, -2, -1, 1, 6, 1) == 0            # a penalty no half holds; a negative one
    assert g(165, -2, 6, 1, 6, 1) == 0                                            # -A 165: 199 columns pass 2^15


def test_stand_alone_program_runs_clean(tmp_path):
    """the same file as a program of its own (the form a sanitizer build runs): random jobs, empty ones among them, against a plain Smith-Waterman"""
    exe = str(tmp_path / "host_ssw16")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DHOST_SSW16_MAIN", "-I" + ROOT + "/biscuit_amd/csrc/hip", os.path.join(ROOT, "tests", "host_ssw16.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
