"""CPU: the plain int64 Smith-Waterman of tests/sw_model.py equals the score recorded from the reference's ksw_align2 on every vector of
tests/golden/ref_vectors_ssw.npz and on the 16-bit-mode vectors of ref_vectors.npz (both matrices, every gap setting of the two files): the
reference the seed filter's kernels are held to is the plain operation, not a restatement of ksw's striping."""
import os
import numpy as np
import ssw_cases as S
import sw_model

HERE = os.path.dirname(os.path.abspath(__file__))


def test_model_equals_recorded_seed_filter_vectors():
    V = S.Vectors()
    n = 0
    for key, ids in V.groups().items():
        ct, ga = S.mats_of(key)
        for i in ids:
            q, t = V.q[V.qoff[i]:V.qoff[i + 1]], V.t[V.toff[i]:V.toff[i + 1]]
            got = sw_model.sw_score(q, t, ct if V.use_ct[i] else ga, *key[2:])
            assert got == V.score[i], (key, i, got, int(V.score[i]))
            n += 1
    assert n == V.n == sum(S.FAMILY_COUNTS.values())
    assert V.family_counts(range(V.n)) == S.FAMILY_COUNTS
    sc = V.score
    assert {"low": int((sc < 256).sum()), "mid": int(((sc >= 256) & (sc < 16384)).sum()), "high": int((sc >= 16384).sum())} == S.SCORE_CLASSES
    assert len(V.groups()) == S.N_OPTION_SETS
    assert {int((x + 7) // 8) for x in V.qlen} == set(range(1, 26))      # every stripe count


def test_gap_families_need_their_gaps():
    """the vectors of the gap families score lower when that kind of gap is forbidden: their best path crosses the lanes with it.  At the guard
    and just beyond it, every option set has at least GUARD_INS_MIN such insertion jobs of 199 columns"""
    V = S.Vectors()
    n, per_set = {}, {}
    for key, ids in V.groups().items():
        ct, ga = S.mats_of(key)
        for i in ids:
            fam = V.fams[V.fam[i]]
            if fam not in S.NEEDS_INSERTION + S.NEEDS_DELETION:
                continue
            q, t = V.q[V.qoff[i]:V.qoff[i + 1]], V.t[V.toff[i]:V.toff[i + 1]]
            ins = fam in S.NEEDS_INSERTION
            without = sw_model.sw_score(q, t, ct if V.use_ct[i] else ga, *key[2:], insertions=not ins, deletions=ins)
            assert without < V.score[i], (key, i, fam)
            n[fam] = n.get(fam, 0) + 1
            if fam != "ins_cross" and ins:
                assert len(q) == 199
                per_set[key] = per_set.get(key, 0) + 1
    assert n == {f: S.FAMILY_COUNTS[f] for f in S.NEEDS_INSERTION + S.NEEDS_DELETION}
    assert len(per_set) == 2 * S.N_REFUSED_SETS and min(per_set.values()) >= S.GUARD_INS_MIN, per_set


def test_model_equals_recorded_16_bit_vectors_of_the_first_file():
    V = np.load(os.path.join(HERE, "golden", "ref_vectors.npz"))
    qo, to, par = V["sw_qoff"], V["sw_toff"], V["sw_par"]
    n = 0
    for i in range(len(par)):
        a, b, which, od, ed, oi, ei, xtra = [int(x) for x in par[i]]
        if xtra & 0x10000:      # KSW_XBYTE: the byte kernel saturates
            continue
        o = S.opt_of((a, b, od, ed, oi, ei))
        mat = np.array(list({0: o.mat, 1: o.ctmat, 2: o.gamat}[which]), np.int8)
        got = sw_model.sw_score(V["sw_q"][qo[i]:qo[i + 1]], V["sw_t"][to[i]:to[i + 1]], mat, od, ed, oi, ei)
        assert got == int(V["sw_out"][i][0]), (i, got, V["sw_out"][i])
        n += 1
    assert n == 184
