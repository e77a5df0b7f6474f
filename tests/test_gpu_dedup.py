"""GPU: C5 on the device -- k_dedup (a lane per read) and k_dedup_long<256> / <1024> (a wavefront per read), csrc/hip/k_dedup.hip -- on the
lists of tests/dedup_cases.py, handed over through bsx_hook_regions_put, against mem_sort_deduplicate as the host runs it
(bsx_hook_regs_sort_dedup; tests/test_dedup_cases_cpu.py pins that function and qualifies the lists).  Read by read: the number kept, the
indices in order, and out_n == -1 exactly when the host function needs a concatenation score; the documented refusals; the hook's errors."""
import collections
import ctypes as C
import re
import numpy as np
import pytest
import dedup_cases as DC
from biscuit_amd import _lib as B

pytestmark = pytest.mark.gpu
E_ARG = -2


def flat(reads):
    """reads: lists of region arrays (one list of arrays per read, all of one per_read) -> regs, off, cnt as bsx_hook_regions_put takes them"""
    parts, off, cnt, at = [], [], [], 0
    for lists in reads:
        for a in lists:
            off.append(at)
            cnt.append(len(a))
            parts.append(a)
            at += len(a)
    regs = np.concatenate(parts) if parts else np.zeros(0, dtype=DC.REGION_DT)
    return regs, np.array(off, dtype=np.int64), np.array(cnt, dtype=np.int32)


def kept(i, out_n, out_idx, long_off, pool):
    m = int(out_n[i])
    if m < 0:
        return None
    if long_off[i] < 0:
        return [int(v) for v in out_idx[i, :m]]
    return [int(v) for v in pool[int(long_off[i]):int(long_off[i]) + m]]


_runs = {}


def run_set(device, small_index, optset):
    """the whole case set of one option set through bsx_hook_regions_put + bsx_regions_dedup2, one call per per_read -> {case name: (kept or None, long_off)}"""
    if optset not in _runs:
        o = DC.make_opt(optset)
        rows = DC.qualified(small_index, optset)
        got = {}
        for pr in (1, 2, 4):
            sel = [cs for cs, _, _, _ in rows if cs.per_read == pr]
            regs, off, cnt = flat([cs.lists for cs in sel])
            device.put_regions(regs, off, cnt)
            out_n, out_idx, long_off, pool = device.dedup2(o, len(sel), pr)
            for i, cs in enumerate(sel):
                got[cs.name] = (kept(i, out_n, out_idx, long_off, pool), int(long_off[i]))
        _runs[optset] = got
    return _runs[optset]


@pytest.mark.parametrize("optset", list(DC.OPTION_SETS))
def test_dedup2_against_host_function(small_index, device, tune, optset):
    rows = DC.qualified(small_index, optset)
    got = run_set(device, small_index, optset)
    seen = collections.Counter()
    bad = []
    for cs, host, model, st in rows:
        g, loff = got[cs.name]
        cl = DC.size_class(cs.n)
        if cl == "over":
            ok = g is None and loff == -1
        else:
            # complete, per_read <= 4, <= 1024 regions, query coordinates <= 0xffff: -1 exactly when the host returns -1, else the same indices in order
            assert int(cs.cat()["qe"].max(initial=0)) <= 0xffff
            ok = g == host and (loff >= 0) == (cl != "short" and host is not None)
        if not ok:
            bad.append((cs.name, None if g is None else g[:12], None if host is None else host[:12], loff))
        seen["class_" + cl] += 1
        seen["bail_" + cl] += host is None
        for k in ("tie1", "tie2", "depth1", "depth2"):
            seen[k + "_" + cl] += bool(st[k])
        seen["multi_group_" + cl] += st["walk_max"] >= 64
        seen["late_kill"] += st["late_kill"] > 0
        seen["early_q_late_p"] += st["early_q_late_p"] > 0
        seen["late_bail"] += st["late_bail"] > 0
    print(optset, dict(sorted(seen.items())))
    assert not bad, (len(bad), bad[:6], dict(seen))
    # what was compared, counted on the host function and the model alone
    for cl in ("short", "A", "B"):
        assert seen["class_" + cl] > 100 and seen["bail_" + cl] > 5, dict(seen)
    for cl in ("A", "B"):
        assert seen["tie1_" + cl] > 20 and seen["tie2_" + cl] > 5 and seen["depth1_" + cl] > 3 and seen["depth2_" + cl] > 0 and seen["multi_group_" + cl] > 5, dict(seen)
    assert seen["class_over"] > 10 and seen["late_kill"] > 10 and seen["early_q_late_p"] > 10 and seen["late_bail"] > 3, dict(seen)


def test_size_classes_go_to_their_kernels(small_index, device, tune, capfd):
    """the wave kernels' lists as the library reports them (the `phases` setting): the reads of 33 .. 256 regions in the first, 257 .. 1024 in the second"""
    rows = DC.qualified(small_index, "default")
    tune("phases", "1")
    got = collections.Counter()
    for pr in (1, 2, 4):
        sel = [cs for cs, _, _, _ in rows if cs.per_read == pr]
        regs, off, cnt = flat([cs.lists for cs in sel])
        device.put_regions(regs, off, cnt)
        capfd.readouterr()
        device.dedup2(DC.make_opt("default"), len(sel), pr)
        err = capfd.readouterr().err
        m = re.search(r"a wavefront per read: (\d+) reads of up to 256 regions, (\d+) of up to (\d+)", err)
        assert m and int(m.group(3)) == DC.CAP_B, err[-500:]
        got["A"] += int(m.group(1))
        got["B"] += int(m.group(2))
    want = collections.Counter(DC.size_class(cs.n) for cs, _, _, _ in rows)
    assert want["A"] > 100 and want["B"] > 100 and sum(cs.n == 256 for cs, _, _, _ in rows) > 5 and sum(cs.n == 257 for cs, _, _, _ in rows) > 5
    assert (got["A"], got["B"]) == (want["A"], want["B"])


def _pick(rows, n_lo, n_hi, per_read, k=6):
    out = [r for r in rows if n_lo <= r[0].n <= n_hi and r[0].per_read == per_read and r[1] is not None and all(len(x) for x in r[0].lists)]
    assert len(out) >= 2
    return out[:k]


def test_refusals(small_index, device, tune, capfd):
    o = DC.make_opt("default")
    rows = DC.qualified(small_index, "default")
    L = B.lib()
    # --- a strand search the device did not finish (count -1), in a short and in a long read, first or last of the read's lists
    sel = _pick(rows, 4, 32, 2) + _pick(rows, 33, 256, 2) + _pick(rows, 257, 1024, 2)
    regs, off, cnt = flat([cs.lists for cs, _, _, _ in sel])
    for t in range(len(sel)):
        cnt[2 * t + t % 2] = -1
    device.put_regions(regs, off, cnt)
    tune("phases", "1")
    capfd.readouterr()
    out_n, out_idx, long_off, pool = device.dedup2(o, len(sel), 2)
    err = capfd.readouterr().err
    tune("phases", None)
    assert (out_n == -1).all() and (long_off == -1).all(), (out_n, long_off)
    m = re.search(r"a wavefront per read: (\d+) reads of up to 256 regions, (\d+) of up to", err)   # and none of them was listed for the wave kernels
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0), err[-500:]
    # --- five lists a read
    five = [r for r in rows if r[0].per_read == 1][:40]
    five = [five[i:i + 5] for i in range(0, 40, 5)]
    regs, off, cnt = flat([[cs.lists[0] for cs, _, _, _ in grp] for grp in five])
    device.put_regions(regs, off, cnt)
    out_n, out_idx, long_off, pool = device.dedup2(o, len(five), 5)
    assert (out_n == -1).all() and (long_off == -1).all()
    # --- more regions than the wave kernel holds
    over = [r for r in rows if r[0].n in (1025, 1100) and r[0].per_read == 2]
    assert len(over) >= 4 and {1025, 1100} == set(r[0].n for r in over)
    regs, off, cnt = flat([cs.lists for cs, _, _, _ in over])
    device.put_regions(regs, off, cnt)
    out_n, out_idx, long_off, pool = device.dedup2(o, len(over), 2)
    assert (out_n == -1).all() and (long_off == -1).all()
    # --- a query end beyond 16 bits: refused in a long list, processed in a short one
    wide = DC.one(5000, 5100, 69900, 70000, 7, 77)
    cs_long = _pick(rows, 40, 200, 1, 1)[0][0]
    cs_short = _pick(rows, 8, 31, 1, 1)[0][0]
    reads = [[np.concatenate([cs_long.lists[0][:20], wide, cs_long.lists[0][20:]])], [np.concatenate([cs_short.lists[0][:3], wide, cs_short.lists[0][3:]])],
             [np.concatenate([wide, wide])]]
    regs, off, cnt = flat(reads)
    device.put_regions(regs, off, cnt)
    out_n, out_idx, long_off, pool = device.dedup2(o, 3, 1)
    assert out_n[0] == -1 and long_off[0] == -1
    for i in (1, 2):
        assert kept(i, out_n, out_idx, long_off, pool) == DC.host_dedup(L, o, small_index, reads[i][0]) and long_off[i] == -1, i
    # --- the wave kernels switched off, and the entry point without them: long reads are the caller's, short ones as before
    mixed = _pick(rows, 2, 32, 2, 20) + _pick(rows, 33, 1024, 2, 20)
    regs, off, cnt = flat([cs.lists for cs, _, _, _ in mixed])
    device.put_regions(regs, off, cnt)
    tune("long_dedup", "0")
    r_off = device.dedup2(o, len(mixed), 2)
    tune("long_dedup", None)
    n1, i1 = device.dedup(o, len(mixed), 2)
    for i, (cs, host, _, _) in enumerate(mixed):
        if cs.n > 32:
            assert r_off[0][i] == -1 and r_off[2][i] == -1 and n1[i] == -1, cs.name
        else:
            assert kept(i, r_off[0], r_off[1], r_off[2], r_off[3]) == host and r_off[2][i] == -1, cs.name
            assert [int(v) for v in i1[i, :n1[i]]] == host, cs.name


def test_regions_put_arguments(small_index, device):
    L = B.lib()
    f = L.bsx_hook_regions_put
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    regs = DC.scattered(np.random.default_rng(1), 10, small_index.l_pac, DC.make_opt("default"))
    off = np.array([0, 4], dtype=np.int64)
    cnt = np.array([4, 6], dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert f(None, 2, p(regs), 10, p(off), p(cnt)) == -1          # BSX_E_NODEVICE
    from biscuit_amd.api import Device
    bare = Device(0)
    assert f(bare.h, 2, p(regs), 10, p(off), p(cnt)) == -1        # no index uploaded
    bare.close()
    for args in ((2, None, 10, p(off), p(cnt)), (2, p(regs), 10, None, p(cnt)), (2, p(regs), 10, p(off), None)):
        assert f(device.h, *args) == E_ARG
    cnt_bad = np.array([4, 7], dtype=np.int32)
    assert f(device.h, 2, p(regs), 10, p(off), p(cnt_bad)) == E_ARG      # off + cnt > n_regs
    off_bad = np.array([0, 11], dtype=np.int64)
    assert f(device.h, 2, p(regs), 10, p(off_bad), p(cnt)) == E_ARG
    cnt_open = np.array([4, -1], dtype=np.int32)
    assert f(device.h, 2, p(regs), 10, p(off_bad), p(cnt_open)) == 0     # an unfinished strand search: its offset is not looked at
    assert f(device.h, 2, p(regs), 10, p(off), p(cnt)) == 0
    o = DC.make_opt("default")
    out_n = np.zeros(4, dtype=np.int32)
    out_idx = np.zeros(4 * L.bsx_regions_dedup_cap(), dtype=np.uint8)
    L.bsx_regions_dedup.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    assert L.bsx_regions_dedup(device.h, C.byref(o), 2, 2, p(out_n), p(out_idx)) == E_ARG    # 4 strand searches asked for, 2 put
    assert L.bsx_regions_dedup(device.h, C.byref(o), 3, 1, p(out_n), p(out_idx)) == E_ARG
    assert L.bsx_regions_dedup(device.h, C.byref(o), 1, 2, p(out_n), p(out_idx)) == 0
    assert [int(v) for v in out_idx[:out_n[0]]] == DC.host_dedup(L, o, small_index, regs)
