"""-m gpu: the per-cytosine methylation BED on the device.  (a) bsx_meth_sites (k_msite.hip) on the three-contig, three-tile genome of
tests/test_gpu_meth.py with two CpGs added (one across the tile boundary at 3 T, one whose G is the second last base of contig t1): counters
planted with designed jobs through bsx_meth_batch, the records of every type, coverage floor and merge mode against a plain walk of the rule in
this file, and their lines (bsx_meth_bed_line) against tests/methbed_model.py; windows, ranges, refused arguments, a second extraction after more
jobs; (b) the HIP command line with --meth-bed against the model over the SAM it wrote and against the CPU checker's file, SAM and QC files
unchanged, also with --markdup and with a --bsconv filter; (c) the records of a stream against the process's and the model's.  Every comparison
is exact."""
import ctypes as C
import os
import numpy as np
import pytest
import simdata
import e2e_cases as E
import meth_cases as MC
import meth_model as M
import methbed_cases as MBC
import methbed_model as MB
import qc_model as Q
import test_gpu_meth as TM

pytestmark = pytest.mark.gpu
HIP = os.path.join(E.ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(E.ROOT, "oracle", "oracle_align")
CG, CHG, CHH, CN, SIDE_C, SIDE_G = 0, 1, 2, 3, 4, 8
ONE = [(3, "S"), (1, "M"), (3, "S")]                                          # the only column has q1 = 4 of 7
MODES = [(t, k, m) for t in ("cg", "ch", "c") for k in (1, 3) for m in (False, True) if not (m and t != "cg")]


# ------------------------------------------------------------------ (a) the kernels against a plain walk of the rule
def _plant(g, p, ret, conv, opp_alt=0):
    """one-column jobs that add exactly (ret, conv, 0, opp_alt) at the C or G at p"""
    own, other = (0, 1) if g[p] == 1 else (1, 0)                              # the strand tag that counts at this base, and the other one
    same, alt = (1, 3) if g[p] == 1 else (2, 0)
    mk = lambda b, tag: TM.Job(p, ONE, [0, 0, 0, b, 0, 0, 0], tag=tag)
    return [mk(same, own)] * ret + [mk(alt, own)] * conv + [mk(alt, other)] * opp_alt


def _class(g, start_of, f):
    """pileup's CX of the C or G at f: g = the genome with 4 at every N, start_of[f] = the start of f's contig and end_of it in start_of[f][1]"""
    lo, hi = start_of[f]
    if f - 2 < lo or f + 2 >= hi or (g[f - 2:f + 3] == 4).any():
        return CN
    n1, n2 = (g[f + 1], g[f + 2]) if g[f] == 1 else (3 - g[f - 1], 3 - g[f - 2])
    return CG if n1 == 2 else CHG if n2 == 2 else CHH


def _walk_sites(g, start_of, cnt, typ, k, merge, f_lo=0, f_hi=None):
    """the rule of include/bsx.h (bsx_meth_site_t) -> [(fpos, ret_c, n_c, ret_g, n_g, flags)]"""
    f_hi = len(g) if f_hi is None else f_hi
    kept = {}
    for f in np.flatnonzero(cnt[:, 0] + cnt[:, 1] > 0):
        ret, conv, oref, oalt = (int(x) for x in cnt[f])
        if g[f] not in (1, 2) or (oalt != 0 and not 20 * oalt < ret + oref):
            continue
        cls = _class(g, start_of, f)
        if cls in {"cg": (CG,), "ch": (CHG, CHH), "c": (CG, CHG, CHH, CN)}[typ] and ret + conv >= k:
            kept[int(f)] = (g[f] == 2, ret, ret + conv, cls)
    out = []
    for f in sorted(kept):
        isg, ret, n, cls = kept[f]
        if not merge:
            rec = (f, 0, 0, ret, n, cls | SIDE_G) if isg else (f, ret, n, 0, 0, cls | SIDE_C)
        elif not isg:
            gg = kept.get(f + 1)
            rec = (f, ret, n, gg[1], gg[2], CG | SIDE_C | SIDE_G) if gg is not None and gg[0] else (f, ret, n, 0, 0, CG | SIDE_C)
        elif f - 1 in kept and not kept[f - 1][0]:
            continue
        else:
            rec = (f, 0, 0, ret, n, cls | SIDE_G)
        if f_lo <= f < f_hi:
            out.append(rec)
    return out


def _tuples(recs):
    assert (recs["pad"] == 0).all()
    return [tuple(int(r[k]) for k in ("fpos", "ret_c", "n_c", "ret_g", "n_g", "flags")) for r in recs]


def _lines(recs, contigs, typ, k, merge):
    """the device's records as the library's formatter prints them"""
    from biscuit_amd import _lib as L_
    f = L_.lib().bsx_meth_bed_line
    f.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]
    f.restype = C.c_size_t
    opt = L_.MethSiteOpt(L_.METH_TYPES[typ], int(merge), k, 0)
    buf = C.create_string_buffer(256)
    out, at, ci = [], 0, 0
    offs = np.cumsum([0] + [len(c) for _, c in contigs])
    for i in range(len(recs)):
        ci = int(np.searchsorted(offs, int(recs["fpos"][i]), side="right")) - 1
        r = recs[i:i + 1]
        n = f(buf, contigs[ci][0].encode(), int(offs[ci]), C.byref(opt), r.ctypes.data_as(C.c_void_p))
        out.append(buf.raw[:n].decode())
    return out


def _model_lines(contigs, cnt, typ, k, merge):
    refs = {name: "".join("ACGTN"[b] for b in c) for name, c in contigs}
    per, at = {}, 0
    for name, c in contigs:
        per[name] = cnt[at:at + len(c)].tolist()
        at += len(c)
    return MB.bed_lines(per, refs, list(refs), typ, k, merge)[0]


N3 = 8400


def _genome(T):
    """the genome of tests/test_gpu_meth.py with a CpG whose G is the second last base of t1, a CpG across the tile boundary at 3 T, and a fourth
    contig t3 = (CG) x 4200 from 3 T + 33 on: whole tiles of nothing but cytosines, CpGs across the boundaries at 4 T and 5 T"""
    import test_gpu_cov as TC
    contigs = [(n, c.copy()) for n, c in TC._genome(T)]
    t1, t2 = contigs[1][1], contigs[2][1]
    t1[34], t1[35] = 1, 2                                                     # C three from t1's end, G two from it
    at = 3 * T - 1 - (T + 38)                                                 # t2 starts at T + 38
    t2[at - 2:at + 4] = (0, 3, 1, 2, 3, 0)                                    # A T C G T A with the C at 3 T - 1, the last position of tile 2
    return contigs + [("t3", np.tile(np.array([1, 2], np.uint8), N3 // 2))]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device
    d = str(tmp_path_factory.mktemp("methbed_k"))
    T = L_.COV_TILE
    contigs = _genome(T)
    simdata.write_genome(d + "/k.fa", contigs)
    Index.build(d + "/k.fa", d + "/k").close()
    idx = Index(d + "/k")
    dev = Device(0)
    dev.upload_index(idx)
    g = np.concatenate([c for _, c in contigs])
    start_of, at = [], 0
    for _, c in contigs:
        start_of += [(at, at + len(c))] * len(c)
        at += len(c)
    assert idx.l_pac == len(g) == 3 * T + 33 + N3 and g[3 * T - 1] == 1 and g[3 * T] == 2 and g[4 * T - 1] == 1 and g[4 * T] == 2
    yield dev, contigs, T, g, start_of
    dev.close()
    idx.close()


def _first_jobs(g, T):
    """tile 0: the CpG at the genome's first two bases, thirty cytosines inside, a C without its G and a G without its C, the C at the tile's last position; tile 1: nothing; tile 2: every C and G
    (reads over the whole tile, three of the strand that counts at C, one of the other), with them the CpG across the boundary at 3 T; all of t3
    likewise"""
    r = np.random.default_rng(17)
    jobs = _plant(g, 0, 2, 1) + _plant(g, 1, 1, 3) + _plant(g, T - 1, 3, 0)
    inside = [p for p in range(200, 1000) if g[p] in (1, 2)][:30]
    for p in inside:
        jobs += _plant(g, p, int(r.integers(0, 4)), int(r.integers(1, 3)))
    lone = [p for p in range(1000, 1100) if g[p] == 1 and g[p + 1] == 2]      # CpGs of which only the C, only the G is covered
    jobs += _plant(g, lone[0], 1, 2) + _plant(g, lone[1] + 1, 4, 0)
    seq = np.where(g[2 * T - 10:3 * T + 10] == 4, 0, g[2 * T - 10:3 * T + 10])
    jobs += [TM.Job(2 * T - 10, [(T + 20, "M")], seq, tag=0)] * 3 + [TM.Job(2 * T - 10, [(T + 20, "M")], seq, tag=1)]
    t3 = 3 * T + 33
    ops = [(3, "S"), (N3, "M"), (3, "S")]                                     # every column of t3 counts
    seq = np.concatenate([[0, 0, 0], g[t3:t3 + N3], [0, 0, 0]])
    jobs += [TM.Job(t3, ops, seq, tag=0)] * 3 + [TM.Job(t3, ops, seq, tag=1)]
    return jobs


def _more_jobs(g, T, start_of):
    """the contig edges, the N holes, a deep CpG, an uncallable C beside a callable G, a tie of the beta"""
    jobs = []
    L = 3 * T + 33                                                            # t2's end
    for p in (T + 1 + 34, T + 1 + 35, T + 37, T + 38, L - 2, L - 1):          # t1's late CpG, t1's last C and t2's first G, t2's last CpG
        jobs += _plant(g, p, 2, 1)
    t2 = T + 38
    for k in (0, 1, 2):                                                       # C N G
        jobs += _plant(g, t2 + 100 + 37 * k, 1, 1) + _plant(g, t2 + 100 + 37 * k + 2, 3, 0)
    jobs += _plant(g, 2 * T - 11, 1, 0)                                       # the C before the N run
    two_away = [p for p in range(t2 + 90, t2 + 1600) if g[p] in (1, 2) and (g[p - 2:p + 3] == 4).sum() == 1 and g[p - 1] != 4 and g[p + 1] != 4][:6]
    assert len(two_away) >= 2
    for p in two_away:
        jobs += _plant(g, p, 3, 1)
    cpgs = [p for p in range(1100, T - 200) if g[p] == 1 and g[p + 1] == 2 and _class(g, start_of, p) == CG and _class(g, start_of, p + 1) == CG]
    assert len(cpgs) >= 4
    jobs += _plant(g, cpgs[0], 501, 500) + _plant(g, cpgs[0] + 1, 1, 1499)    # mergecg's count is 500 + 2, not 501 + 1
    jobs += _plant(g, cpgs[1], 0, 1, opp_alt=1) + _plant(g, cpgs[1] + 1, 2, 0)
    jobs += _plant(g, cpgs[2], 1, 15) + _plant(g, cpgs[3] + 1, 3, 13)         # 0.0625 -> 0.062, 0.1875 -> 0.188
    return jobs, cpgs, two_away


def _check_all(dev, contigs, T, g, start_of, cnt, what):
    L = len(g)
    seen = {}
    for typ, k, merge in MODES:
        want = _walk_sites(g, start_of, cnt, typ, k, merge)
        recs = dev.meth_sites(0, L, typ, k, merge)
        assert _tuples(recs) == want, (what, typ, k, merge)
        small_buf = dev.meth_sites(0, L, typ, k, merge, cap=T)               # the smallest buffer
        assert small_buf.tobytes() == recs.tobytes(), (what, typ, k, merge)
        assert _lines(recs, contigs, typ, k, merge) == _model_lines(contigs, cnt, typ, k, merge), (what, typ, k, merge)
        seen[(typ, k, merge)] = want
    return seen


def test_designed_places_every_type_floor_and_merge_mode(small):
    dev, contigs, T, g, start_of = small
    L = len(g)
    dev.meth_reset()
    assert len(dev.meth_sites(0, L)) == 0                                     # no state yet
    jobs = _first_jobs(g, T)
    cnt = TM._walk(g, jobs)
    TM._run(dev, jobs)
    TM._same_counters(dev, cnt, "first jobs")
    seen = _check_all(dev, contigs, T, g, start_of, cnt, "first jobs")
    every = seen[("c", 1, False)]
    at = [w[0] for w in every]
    assert at[0] == 0 and T - 1 in at and 3 * T in at                         # the first and the last position of a tile
    assert not [f for f in at if T <= f < 2 * T] and [f for f in at if f < T] and [f for f in at if 2 * T <= f < 3 * T]      # an empty tile between two
    assert sorted(f for f in at if 2 * T <= f < 3 * T) == [int(f) for f in np.flatnonzero((g[2 * T:3 * T] == 1) | (g[2 * T:3 * T] == 2)) + 2 * T]      # every C and G of tile 2
    merged = {w[0]: w for w in seen[("cg", 1, True)]}
    assert merged[3 * T - 1] == (3 * T - 1, 3, 3, 1, 1, CG | SIDE_C | SIDE_G) and 3 * T not in merged      # joined across the tile boundary
    assert {w[0]: w for w in seen[("cg", 3, True)]}[3 * T - 1] == (3 * T - 1, 3, 3, 0, 0, CG | SIDE_C)      # the G does not pass the floor
    kinds = {w[5] & (SIDE_C | SIDE_G) for w in merged.values()}
    assert kinds == {SIDE_C, SIDE_G, SIDE_C | SIDE_G}
    # the same CpG across a boundary of the caller's loop, and ranges that begin and end inside tiles
    for typ, k, merge in (("cg", 1, True), ("cg", 1, False), ("c", 1, False)):
        for lo, hi in ((0, 3 * T), (3 * T, L), (5, T - 1), (T - 1, T), (2 * T + 7, 3 * T - 1), (3 * T - 1, 3 * T + 1), (700, 700)):
            recs, f_next = dev.meth_sites_window(lo, hi, typ, k, merge)
            assert f_next == hi and _tuples(recs) == _walk_sites(g, start_of, cnt, typ, k, merge, lo, hi), (typ, merge, lo, hi)
    a, _ = dev.meth_sites_window(0, 3 * T, "cg", 1, True)
    b, _ = dev.meth_sites_window(3 * T, L, "cg", 1, True)
    assert int(a["fpos"][-1]) == 3 * T - 1 and int(a["flags"][-1]) == CG | SIDE_C | SIDE_G and (b["fpos"] > 3 * T).all()
    # a buffer of one tile stops where the next tile no longer fits: every position of tile 4 is a site
    for lo, stop in ((0, 3 * T), (3 * T, 4 * T), (4 * T, 5 * T), (5 * T, L)):
        recs, f_next = dev.meth_sites_window(lo, L, "cg", 1, False, cap=T)
        assert f_next == stop and _tuples(recs) == _walk_sites(g, start_of, cnt, "cg", 1, False, lo, stop), (lo, stop, f_next)
    assert len(dev.meth_sites_window(4 * T, L, "cg", 1, False, cap=T)[0]) == T
    recs, f_next = dev.meth_sites_window(0, L, "cg", 1, True, cap=T)          # merged, the buffer ends between the C at 4 T - 1 and its G
    assert f_next == 4 * T and _tuples(recs[-1:]) == [(4 * T - 1, 3, 3, 1, 1, CG | SIDE_C | SIDE_G)]
    assert int(dev.meth_sites_window(4 * T, L, "cg", 1, True, cap=T)[0]["fpos"][0]) == 4 * T + 1
    # more jobs: a second extraction reflects them
    more, cpgs, two_away = _more_jobs(g, T, start_of)
    TM._run(dev, more)
    cnt = cnt + TM._walk(g, more)
    TM._same_counters(dev, cnt, "more jobs")
    seen = _check_all(dev, contigs, T, g, start_of, cnt, "more jobs")
    every = {w[0]: w for w in seen[("c", 1, False)]}
    cg = {w[0]: w for w in seen[("cg", 1, False)]}
    merged = {w[0]: w for w in seen[("cg", 1, True)]}
    assert T + 35 in cg and T + 36 not in cg and every[T + 36][5] == CN | SIDE_G      # t1's late CpG: the C has its five bases, the G lacks one
    assert merged[T + 35] == (T + 35, 2, 3, 0, 0, CG | SIDE_C)
    for p in (T + 37, T + 38, 3 * T + 31, 3 * T + 32, T + 38 + 100, T + 38 + 102, 2 * T - 11, 2 * T + 10):      # contig ends and holes: CN, in no cg file
        assert every[p][5] & 3 == CN and p not in cg, p
    for p in two_away:
        assert every[p][5] & 3 == CN and p not in cg, p
    assert merged[cpgs[0]] == (cpgs[0], 501, 1001, 1, 1500, CG | SIDE_C | SIDE_G)
    line = _lines(dev.meth_sites(cpgs[0], cpgs[0] + 1, "cg", 1, True), contigs, "cg", 1, True)
    assert line == ["t0\t%d\t%d\t0.201\t2501\tC:0.500:1001,G:0.001:1500\n" % (cpgs[0], cpgs[0] + 2)]      # (500 + 2) / 2501
    assert cpgs[1] not in every and merged[cpgs[1] + 1] == (cpgs[1] + 1, 0, 0, 2, 2, CG | SIDE_G)      # the uncallable C leaves its G alone
    assert _lines(dev.meth_sites(cpgs[2], cpgs[2] + 1, "cg", 3, False), contigs, "cg", 3, False) == ["t0\t%d\t%d\t0.062\t16\n" % (cpgs[2], cpgs[2] + 1)]
    assert _lines(dev.meth_sites(cpgs[3] + 1, cpgs[3] + 2, "cg", 3, False), contigs, "cg", 3, False) == ["t0\t%d\t%d\t0.188\t16\n" % (cpgs[3] + 1, cpgs[3] + 2)]
    dev.meth_reset()


def test_a_buffer_below_a_tile_is_refused_and_nothing_is_written(small):
    from biscuit_amd import _lib as L_
    dev, contigs, T, g, start_of = small
    L = len(g)
    dev.meth_reset()
    TM._run(dev, _plant(g, 0, 2, 1))
    f = L_.lib().bsx_meth_sites
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    out = np.full(T * 8, 0x5a5a5a5a, np.uint32)
    n, f_next = C.c_int64(-7), C.c_int64(-7)
    opt = L_.MethSiteOpt(L_.METH_TYPES["c"], 0, 1, 0)
    assert f(dev.h, C.byref(opt), 0, L, out.ctypes.data_as(C.c_void_p), T - 1, C.byref(n), C.byref(f_next)) == -2      # BSX_E_ARG
    assert (out == 0x5a5a5a5a).all() and n.value == -7 and f_next.value == -7
    for bad in (dict(f_lo=-1), dict(f_hi=L + 1), dict(f_lo=9, f_hi=8), dict(min_cov=0), dict(typ="c", merge=True)):
        kw = dict(f_lo=0, f_hi=L, typ="cg", min_cov=1, merge=False)
        kw.update(bad)
        with pytest.raises(L_.BsxError) as e:
            dev.meth_sites_window(**kw)
        assert "(-2)" in str(e.value), bad
    recs, f_next = dev.meth_sites_window(0, L, "c", 1, False, cap=T)
    assert f_next == L and _tuples(recs) == [(0, 2, 3, 0, 0, CN | SIDE_C)]
    dev.meth_reset()


# ------------------------------------------------------------------ (b) the command line
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("methbed_gpu"))
    MC.make_data(d)
    return d, Q.read_fasta(d + "/g.fa")


def test_hip_command_line_file_equals_model_and_cpu_checker(data):
    d, refs = data
    modes = {m: (o, a) for m, o, a in MBC.MODES}
    by_mode = {m: [] for m in modes}
    plan = (("pe150_b0", [], dict(E.CASES_CORE)["pe150_b0"], ("cg", "ch", "c", "k3", "merge"), ("c", "merge")),
            ("markdup", ["--markdup"], ["-@", "4", "g", "d1.fq", "d2.fq"], ("merge",), ("merge",)),
            ("filtered", ["--bsconv-max-cph", "3"], dict(E.CASES_CORE)["pe150_b0"], ("c",), ("c",)))
    beds = {}
    for case, opts, args, hip_modes, cpu_modes in plan:
        plain, files0, table = MC.run_meth(HIP, opts, args, d, d + "/p_" + case)
        files0[M.SUFFIX] = table
        for mode in hip_modes:
            sam, files, bed = MBC.run_bed(HIP, opts + modes[mode][0], args, d, d + "/hip_%s_%s" % (case, mode))
            assert sam == plain and files == files0, (case, mode)
            made_of = MBC.check_bed(bed, sam, refs, case, **modes[mode][1])
            assert made_of
            if case == "pe150_b0":                                            # (every mode runs on this one: their line counts compare)
                by_mode[mode] += made_of
            beds[(case, mode)] = bed
            if mode in cpu_modes:
                csam, cfiles, cbed = MBC.run_bed(CPU, opts + modes[mode][0], args, d, d + "/cpu_%s_%s" % (case, mode))
                E.assert_same_sam(sam.encode(), csam.encode(), case)
                assert bed == cbed and files == cfiles, (case, mode)
    assert beds[("markdup", "merge")] != beds[("pe150_b0", "merge")] and beds[("filtered", "c")] != beds[("pe150_b0", "c")]
    MBC.assert_not_vacuous(by_mode)


# ------------------------------------------------------------------ (c) a stream
def test_stream_records_equal_the_process_records_and_the_model(data):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device, default_opt
    d, refs = data
    L = L_.lib()
    idx = Index(d + "/g")
    dev = Device(0)
    dev.upload_index(idx)
    opt = default_opt()
    opt.n_threads = 4
    opt.flag |= 0x10 | 0x2
    L.bsx_sim_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]
    L.bsx_sim_free_reads.argtypes = [C.c_void_p, C.c_int64]
    L.bsx_stream_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.bsx_stream_push.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.bsx_stream_flush.argtypes = [C.c_void_p]
    L.bsx_stream_close.argtypes = [C.c_void_p]
    L.bsx_stream_close.restype = None
    L.bsx_stream_set_qc.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_set_qc_meth.argtypes = [C.c_void_p, C.c_int]
    sites_args = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bsx_stream_qc_meth_sites.argtypes = [C.c_void_p] + sites_args
    L.bsx_process_qc_meth_sites.argtypes = sites_args
    mopt = L_.MethSiteOpt(L_.METH_TYPES["cg"], 1, 1, 0)

    def all_sites(call):
        parts, lo = [], 0
        while lo < idx.l_pac:
            out = np.zeros(2 * L_.COV_TILE, dtype=np.dtype(L_.MethSite))
            n, nxt = C.c_int64(-1), C.c_int64(-1)
            L_.check(call(C.byref(mopt), lo, idx.l_pac, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), C.byref(nxt)), "sites")
            assert nxt.value > lo
            parts.append(out[:n.value].copy())
            lo = nxt.value
        return np.concatenate(parts)

    n_pairs, chunks, got = 1000, [], []
    try:
        for how in ("stream", "process"):
            ch = []
            for k in range(2):
                p = C.c_void_p()
                L_.check(L.bsx_sim_pairs(idx.h, n_pairs, 150, 900 + k, 200, 500, 0.01, 0.2, C.byref(p)), "sim_pairs")
                ch.append(p)
            chunks += ch
            s = C.c_void_p()
            L_.check(L.bsx_stream_open(dev.h, C.byref(opt), idx.h, None, C.byref(s)), "stream_open")
            if how == "stream":
                out1 = np.zeros(L_.COV_TILE, dtype=np.dtype(L_.MethSite))
                n, nxt = C.c_int64(), C.c_int64()
                assert L.bsx_stream_qc_meth_sites(s, C.byref(mopt), 0, idx.l_pac, out1.ctypes.data_as(C.c_void_p), len(out1), C.byref(n), C.byref(nxt)) == -2      # not switched on
                L_.check(L.bsx_stream_set_qc(s, 1), "set_qc")
                L_.check(L.bsx_stream_set_qc_meth(s, 1), "set_qc_meth")
                assert len(all_sites(lambda *a: L.bsx_stream_qc_meth_sites(s, *a))) == 0      # no chunk yet
            else:
                L_.check(L.bsx_process_set_qc(1), "process_set_qc")
                L_.check(L.bsx_process_set_qc_meth(1), "process_set_qc_meth")
            for k in range(2):
                L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, ch[k]), "push")
            L_.check(L.bsx_stream_flush(s), "flush")
            got.append(all_sites((lambda *a: L.bsx_stream_qc_meth_sites(s, *a)) if how == "stream" else L.bsx_process_qc_meth_sites))
            L.bsx_stream_close(s)
            if how == "process":
                L.bsx_process_set_qc_meth(0)
                L.bsx_process_set_qc(0)
        text = ""
        for k in range(2):
            rd = C.cast(chunks[k], C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        assert len(got[0]) > 100 and got[0].tobytes() == got[1].tobytes()
        contigs = [(name, np.array(["ACGTN".index(b) for b in seq.upper()], np.uint8)) for name, seq in refs.items()]
        want, made_of, seen = MB.process(text, refs, "cg", 1, True)
        assert "".join(_lines(got[0], contigs, "cg", 1, True)) == want
        assert {(w[2], w[3]) for w in made_of} == {(True, True), (True, False), (False, True)}
    finally:
        L.bsx_process_set_qc_meth(0)
        L.bsx_process_set_qc(0)
        for ch in chunks:
            L.bsx_sim_free_reads(ch, 2 * n_pairs)
        dev.close()
        idx.close()
