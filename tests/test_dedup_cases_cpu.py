"""CPU: the lists of tests/dedup_cases.py do what their families are for, and the oracle the GPU tests hold the kernels to -- the host's
bsx_regs_sort_dedup through bsx_hook_regs_sort_dedup -- is itself pinned on them: to the module's restatement (model_dedup, every list), to
oracle/backhalf.sort_dedup over the reference's own introsort (a sample: every family, every size class, lists of 1024 regions), and the
wave-parallel sort's model to klib's at the lengths the wave kernel really runs it at (257 .. 1024).  Counted with the host function
and tools/dbg/parsort_model.py only."""
import collections
import ctypes as C
import os
import random
import sys
import numpy as np
import pytest
import dedup_cases as DC
from oracle_lib import ref_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools", "dbg"))
import backhalf        # noqa: E402
import parsort_model as M   # noqa: E402


def family_counts(rows):
    fam = collections.defaultdict(collections.Counter)
    for cs, host, model, st in rows:
        F, cl = fam[cs.family], DC.size_class(cs.n)
        F["reads"] += 1
        F["regions"] += cs.n
        F["bail"] += host is None
        F["class_" + cl] += 1
        for k in ("tie1", "tie2", "depth1", "depth2"):
            F[k + "_" + cl] += bool(st[k])
        F["no_act"] += st["act"] == 0
        F["multi_group"] += st["walk_max"] >= 64
        for k in ("late_kill", "early_q_late_p", "late_bail", "lpac_saved", "rid_break", "scan_dropped", "ident_dropped"):
            F[k] += st[k] > 0
        if host is not None:
            F["dropped"] += len(host) < cs.n
    return fam


@pytest.mark.parametrize("optset", list(DC.OPTION_SETS))
def test_families_do_what_they_are_for(small_index, optset):
    rows = DC.qualified(small_index, optset)
    fam = family_counts(rows)
    for f in DC.FAMILIES:
        print(optset, f, dict(sorted(fam[f].items())))
    lengths = set(cs.n for cs, _, _, _ in rows)
    assert set(DC.LENGTHS) <= lengths, sorted(set(DC.LENGTHS) - lengths)
    assert set(cs.per_read for cs, _, _, _ in rows) == {1, 2, 4}
    assert any(any(len(x) == 0 for x in cs.lists) and cs.n > 32 for cs, _, _, _ in rows)      # empty lists inside a long read
    assert {(31, 2), (1, 1023)} <= set(tuple(len(x) for x in cs.lists) for cs, _, _, _ in rows)
    two_l_pac = 2 * small_index.l_pac
    for cs, host, model, st in rows:
        c = cs.cat()
        assert ((c["qe"] > c["qb"]) & (c["re"] > c["rb"]) & (c["rb"] >= 0) & (c["re"] <= two_l_pac)).all(), cs.name
        assert host == model, cs.name          # the host function and the restatement: same kept indices in the same order, or both bail
        if cs.expect:
            assert (host is None) == (cs.expect == "bail"), cs.name
    S, T, E, X, R, K = (fam[f] for f in ("scattered", "satellite", "tied_ends", "tied_scores", "strands", "concat"))
    # scattered: nobody within anybody's reach, no ties: only the sorts run, by rank
    assert S["no_act"] == S["reads"] and S["bail"] == 0 and not any(S[k + "_" + cl] for k in ("tie1", "tie2") for cl in ("short", "A", "B"))
    assert S["class_A"] > 5 and S["class_B"] > 5
    # satellite: scans over several groups of 64, kills there, and q's killed in the first group before p dies in a later one
    assert T["multi_group"] > 10 and T["late_kill"] > 5 and T["early_q_late_p"] > 5 and T["scan_dropped"] > 20
    # tied ends: in every long class, and klib's depth limit on the rank keys in both
    assert E["tie1_A"] > 20 and E["tie1_B"] > 20 and E["depth1_A"] > 3 and E["depth1_B"] > 3 and E["tie1_short"] > 10
    # tied scores: the second sort's tie path in both long classes, its depth limit, and the identical-hit pass
    assert X["tie2_A"] > 5 and X["tie2_B"] > 5 and X["depth2_A"] > 0 and X["depth2_B"] > 0 and X["ident_dropped"] > 20
    assert 0 < X["tie2_A"] < X["class_A"] and 0 < X["tie2_B"] < X["class_B"]      # and lists of equal scores that rank without a tie
    # strands: pairs only the l_pac rule keeps from the bail-out; rid breaks with regions of p's rid behind them
    assert R["lpac_saved"] > 20 and R["rid_break"] > 20
    # concat: every list meant to bail does, the ones behind a killing q do not; some bail in the second group of 64
    assert K["bail"] > 30 and K["late_bail"] > 3 and K["bail"] < K["reads"]
    for f in DC.FAMILIES:
        if f not in ("concat", "threshold"):
            assert fam[f]["bail"] * 4 <= fam[f]["reads"], (f, fam[f]["bail"])
    assert sum(F["dropped"] for F in fam.values()) > 200
    # threshold: across delta -1, 0, +1 the host's outcome changes exactly once, at every size the pair is embedded in
    g = collections.defaultdict(dict)
    for cs, host, _, _ in rows:
        if cs.family == "threshold":
            g[(cs.group[0], cs.group[2])][cs.group[1]] = None if host is None else len(host)
    assert len(g) >= 52 and all(("reach", n) in g for n in (2, 20, 40, 300))
    for key, v in g.items():
        assert (v[-1] != v[0]) + (v[0] != v[1]) == 1, (key, v)
    for name in ("r05", "r10"):      # r = 0.05 exactly lies below (double)0.05f: the pair on the value is still handed to the alignment
        assert g[(name, 2)][0] is None and g[(name, 2)][1] is not None


def _sample(rows):
    """lists for the comparison with oracle/backhalf.py: per family one of each size class (the small ones of a class where the restatement's
    scan is quadratic), and lists of 1024 regions from the families whose scans are short"""
    seen, out = set(), []
    for cs, host, _, st in sorted(rows, key=lambda r: r[0].n):
        if cs.wide or cs.n > DC.CAP_B or cs.n < 2:
            continue
        key = (cs.family, DC.size_class(cs.n), cs.n == 1024 and cs.family in ("scattered", "tied_ends", "tied_scores"), st["tie1"] or st["tie2"], min(cs.n, 640) // 64)
        if key not in seen:
            seen.add(key)
            out.append((cs, host))
    return out


def test_host_function_against_backhalf_on_a_sample(small_index):
    R = ref_lib()
    if R is None:
        pytest.skip("oracle/_ref is not built")
    R.ref_introsort_kv.argtypes = [C.c_int64, C.c_void_p]

    def klib_order(keys):
        kv = np.zeros((len(keys), 2), dtype=np.int64)
        kv[:, 0] = keys
        kv[:, 1] = np.arange(len(keys))
        if len(keys):
            R.ref_introsort_kv(len(keys), kv.ctypes.data_as(C.c_void_p))
        return [int(x) for x in kv[:, 1]]
    n_1024 = 0
    fams = collections.defaultdict(set)
    for optset in DC.OPTION_SETS:
        o = DC.make_opt(optset)
        od = {"mask_level_redun": o.mask_level_redun, "max_chain_gap": o.max_chain_gap, "w": o.w}
        for cs, host in _sample(DC.qualified(small_index, optset)):
            c = cs.cat()
            regs = [{f: int(r[f]) for f in ("rb", "re", "qb", "qe", "rid", "score")} for r in c]
            want = backhalf.sort_dedup(od, small_index.l_pac, regs, klib_order)
            assert want == host, (optset, cs.name)      # the same kept indices in the same order, or None <=> -1
            fams[cs.family].add(DC.size_class(cs.n))
            n_1024 += cs.n == 1024
    print({f: sorted(v) for f, v in fams.items()}, n_1024)
    assert set(fams) == set(DC.FAMILIES) and n_1024 >= 4
    for f in DC.FAMILIES:
        assert {"A", "B"} <= fams[f], (f, fams[f])


KERNEL_LENGTHS = [257, 511, 512, 513, 1000, 1023, 1024]


def _keys(rnd, n, kind):
    if kind == 0:
        w = [rnd.randint(1, 4) for _ in range(n)]
    elif kind == 1:
        w = [rnd.randint(1, n // 2) for _ in range(n)]                       # dense ranks, half of them tied
    elif kind == 2:
        w = [rnd.randint(1, n) if rnd.random() < 0.9 else 7 for _ in range(n)]
    elif kind == 3:
        w = [5] * n
    else:
        w = sorted((rnd.randint(1, rnd.choice([8, 30, n // 4])) for _ in range(n)), reverse=kind == 4)   # pre-sorted either way
    return w


def test_sort_model_at_the_wave_kernels_lengths():
    """rg_introsort_par's construction (every partition at once, the closing rank) against sequential klib and, when built, the reference's
    own template, on 257 .. 1024 keys (tests/test_parsort_model.py stops at the chain filter's 256)"""
    R = ref_lib()
    if R is not None:
        R.ref_introsort_kv_desc.argtypes = [C.c_int64, C.c_void_p]
    rnd = random.Random(41)
    n_comb = collections.Counter()
    for n in KERNEL_LENGTHS:
        for kind in (0, 1, 2, 3, 4, 5, 4, 5):
            w = _keys(rnd, n, kind)
            a = [(w[i], i) for i in range(n)]
            b, c = list(a), list(a)
            if not M.par_introsort(list(a)):
                n_comb[n] += 1
                assert not M.klib_introsort(list(a))
            assert M.klib_introsort(a, comb=True) and M.par_introsort(b, comb=True)
            assert a == b, (n, kind)
            if R is not None:
                kv = np.array(c, dtype=np.int64)
                R.ref_introsort_kv_desc(n, kv.ctypes.data_as(C.c_void_p))
                assert [x[1] for x in b] == kv[:, 1].tolist(), (n, kind)
    print(dict(n_comb))
    assert all(n_comb[n] > 0 for n in KERNEL_LENGTHS), dict(n_comb)   # the depth limit (comb sort by one lane) at every length
