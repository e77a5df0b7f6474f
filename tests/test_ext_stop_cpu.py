"""CPU: the extensions' stopping rule (biscuit_amd/csrc/hip/ext_stop_rule.h, the header the kernels include) in a scalar model of the loop
(tests/host_ext_stop.cpp) against the recorded ksw_extend2 answers of the designed jobs (tests/ext_stop_cases.py), against the oracle's
extension (oracle/port.c) and, where oracle/_ref is built, against the reference's own function on 20 000 seeded random jobs.  With the rule
not obeyed the model evaluates PHI after every row and executes the proof: PHI never grows, and no later row holds an H above it."""
import ctypes as C
import numpy as np
import ext_pk_cases as P
import ext_stop_cases as X
import oracle_lib


def _ref_call(fn, q, t, mat, gp, w, eb, zd, h0):
    out = (C.c_int * 6)()
    fn(C.c_int(len(q)), X._p(q), C.c_int(len(t)), X._p(t), mat, C.c_int(gp[0]), C.c_int(gp[1]), C.c_int(gp[2]), C.c_int(gp[3]), C.c_int(w), C.c_int(eb),
       C.c_int(zd), C.c_int(h0), out)
    return list(out)


def test_designed_jobs_equal_the_recording_and_the_proof_holds():
    H = X.harness()
    port = oracle_lib.port_lib().oracle_extend1
    cases, want = X.load()
    opts = [P.opt_of(a, b, gp, zd) for a, b, gp, zd in X.scorings()]
    fired = {f: [0, 0] for f in X.FAMILIES}
    per_scoring = [0] * len(opts)
    n_peak_windows = 0
    for k, (si, fam, parent, w, eb, h0, q, t) in enumerate(cases):
        a, b, gp, zd = X.scorings()[si]
        mat = opts[si].ctmat if parent else opts[si].gamat
        got, info = X.model(H, q, t, mat, gp, w, eb, zd, h0, 1)          # the rule obeyed
        free, chk = X.model(H, q, t, mat, gp, w, eb, zd, h0, 0)          # every row run, the proof checked
        key = (k, si, fam, parent, w, eb, h0, len(q), len(t))
        assert got == [int(x) for x in want[k]], (key, got, want[k])
        assert free == got, (key, free, got)
        assert got == _ref_call(port, q, t, mat, gp, w, eb, zd, h0), key
        assert chk[2] == 0, ("PHI grew", key, chk)
        assert chk[3] == 0, ("an H above an earlier PHI", key, chk)
        assert chk[0] == info[0], key                                     # the same row with and without obeying
        early = info[0] >= 0
        assert early == (info[1] < chk[1]), (key, info, chk)                # a stop always saves at least the next row
        fired[fam][0] += 1
        fired[fam][1] += int(early and info[1] < chk[1])
        per_scoring[si] += 1
        if fam == "clean":
            # fires within two rows of the row on which the diagonal reaches the end, qlen - 1, and rows are saved
            assert early and 0 <= info[0] - (len(q) - 1) <= 2 and info[1] < chk[1], (key, info, chk)
        if fam == "first_col":
            # the first column's potential, h0 - o_del - e_del (i + 1) + qlen mx, is below G = h0 + qlen a from row 0 on (mx == a): as clean
            assert early and 0 <= info[0] - (len(q) - 1) <= 2, (key, info, chk)
        if fam == "peak":
            # The last d bases mismatch on the diagonal: the score peaks at P = h0 + (qlen - d) a in column qlen - d - 1, and the diagonal
            # reaches the end on row qlen - 1 with a score of at least P - d bmax (bmax: the largest mismatch penalty), if that is positive, so
            # the final gscore G is at least that.  No stop before the row that set G (gtle - 1; an insertion path may reach the last column
            # before the diagonal does, with more).  On a row i >= qlen every cell lies i - j >= i - qlen + 1 rows below the
            # diagonal, i.e. behind a deletion at least that long, so PHI <= P + d mx - o_del - e_del (i - qlen + 1) whatever the target's
            # later rows match by chance; that is below G once i - qlen + 1 > (d (mx + bmax) - o_del) / e_del.  (With the defaults' shape,
            # d (1 + b) - 6 rows after the end: the issue's "about d - 6" per unit of loss.)  Checked where the z-drop cannot end the job first.
            qlen = len(q)
            d = 0
            while d < qlen and q[qlen - 1 - d] != t[qlen - 1 - d]:
                d += 1
            m44 = np.array(list(mat), np.int8).reshape(5, 5)[:4, :4]
            mx, bmax = int(m44.max()), -int(m44.min())
            assert d >= 1 and mx == a, key
            upper = qlen + max(0, (d * (mx + bmax) - gp[0]) // gp[1])
            if h0 + (qlen - d) * a - d * bmax > 0 and upper + 1 < len(t) and zd >= 100:
                assert early and got[3] - 1 <= info[0] <= upper, (key, d, upper, info, chk)
                n_peak_windows += 1
        if fam == "never":
            assert not early, (key, info, got)
        if fam == "tie":
            assert chk[6] > 0 and early, (key, chk)
            assert info[0] >= chk[7], ("the rule fired before the last row that tied gscore and moved gtle", key, info, chk)
    assert all(n >= 200 for n in per_scoring), per_scoring
    assert fired["clean"][1] == fired["clean"][0] and fired["never"][1] == 0, fired
    assert n_peak_windows >= 60, n_peak_windows
    assert fired["peak"][1] > 0 and fired["first_col"][1] > 0 and fired["indel"][1] > 0 and fired["n_in_query"][1] > 0, fired


def test_random_jobs_against_the_reference():
    """20 000 seeded random jobs against the reference's own ksw_extend2 where oracle/_ref is built (else against the oracle's restatement)"""
    H = X.harness()
    R = oracle_lib.ref_lib()
    ref = R.ref_ksw_extend2 if R is not None else oracle_lib.port_lib().oracle_extend1
    rng = np.random.default_rng(4242)
    opts = [P.opt_of(a, b, gp, zd) for a, b, gp, zd in X.scorings()]
    n_fired = 0
    for it in range(20000):
        si = it % len(opts)
        a, b, gp, zd = X.scorings()[si]
        qlen = int(rng.integers(1, 200)) if it % 3 else int(rng.choice(X.QLENS))
        tlen = int(qlen * rng.uniform(0.6, 2.2)) + 1
        alphabet = 2 if it % 5 == 0 else 4
        t = (rng.integers(0, alphabet, tlen) * (3 if alphabet == 2 else 1)).astype(np.uint8)
        q = np.resize(t, qlen).copy() if tlen < qlen else t[:qlen].copy()
        sub = rng.random(qlen) < rng.choice([0.0, 0.03, 0.15, 0.5])
        q[sub] = rng.integers(0, 4, int(sub.sum()))
        if it % 7 == 0 and qlen > 10:       # a gap
            at, k = int(rng.integers(1, qlen - 1)), int(rng.integers(1, 6))
            q = (np.concatenate([q[:at], rng.integers(0, 4, k).astype(np.uint8), q[at:]])[:qlen] if it % 2 else np.resize(np.concatenate([q[:at], q[at + k:]]), qlen)).astype(np.uint8)
        if it % 11 == 0:
            q[int(rng.integers(0, qlen))] = 4
        h0 = int(rng.integers(1, 300)) if it % 4 == 0 else int(rng.integers(19, 60)) * a
        w, eb, parent = int(rng.choice([100, 200, 7, 14, 1])), int(rng.integers(0, 6)), it & 1
        mat = opts[si].ctmat if parent else opts[si].gamat
        got, info = X.model(H, q, t, mat, gp, w, eb, zd, h0, 1)
        free, chk = X.model(H, q, t, mat, gp, w, eb, zd, h0, 0)
        want = _ref_call(ref, q, t, mat, gp, w, eb, zd, h0)
        assert got == want and free == want, (it, si, parent, w, eb, h0, qlen, tlen, got, free, want)
        assert chk[2] == 0 and chk[3] == 0 and chk[0] == info[0], (it, chk, info)
        n_fired += info[0] >= 0
    assert n_fired > 2000, n_fired
