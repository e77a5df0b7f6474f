"""Global alignment with its tags against the reference's own, recorded (tests/golden/ref_glb_tags.npz: bis_bwa_gen_cigar2 of lib/aln/bwa.c
through oracle/ref_shim.c, inside the band-doubling loop of mem_alnreg_format.c:65-77, on the designed jobs of tests/glb_tag_cases.py) -- the
parts that need no GPU:

* the recording is the cases' (CRCs), covers what the cases are named for (the table of counts by equality, every digit, lane, operation and
  stage edge on both of its sides) and, where the reference library is built, equals a fresh call for every case
* the class tables of glb_tag_cases against lane_global_batch's (csrc/hip/shim.hip)
* the host's own walk -- bsx_setsam_finish without tags (csrc/host/sam.c), the path of backends that return none -- through
  bsx_hook_setsam_finish: MD, NM and the CIGAR after a leading or trailing deletion is squeezed out
* the CPU restatement of the kernel's first half and retry loop (oracle/port.c: global_batch): score, CIGAR and the last try's bandwidth

tests/test_gpu_glb_tags_recorded.py holds the device's side."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest

import oracle_lib
import glb_tag_cases as GC
from biscuit_amd import _lib as B
from biscuit_amd.api import Index, default_opt, GLB_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec():
    r = GC.load()
    assert int(r.z["genome_crc"]) == GC.genome_crc(), "the genome of glb_tag_cases is not the recorded one: run tests/golden/make_vectors_glbtags.py"
    assert int(r.z["reads_crc"]) == GC.reads_crc(), "the reads of glb_tag_cases are not the recorded ones"
    assert r.names == [c["name"] for c in GC.cases()]
    return r


@pytest.fixture(scope="module")
def opts():
    return {o: GC.set_opt(default_opt(), o) for o, _ in GC.OPTSETS}


@pytest.fixture(scope="module")
def index_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("glbtags_idx")
    GC.write_fasta(str(d / "g.fa"))
    idx = Index.build(str(d / "g.fa"), str(d / "g"))
    assert idx.l_pac == GC.L_PAC
    idx.close()
    return str(d / "g")


# ------------------------------------------------------------------------------------------ the tables and the coverage
def test_the_class_tables_are_the_shims():
    src = open(os.path.join(ROOT, "biscuit_amd", "csrc", "hip", "shim.hip")).read()
    body = src[src.index("static int lane_global_batch("):]
    for name, want in (("QCAP", GC.QCAP), ("BAND", GC.BAND), ("TCAP", GC.TCAP)):
        m = re.search(r"\b%s\[4\] = \{([^}]*)\}" % name, body)
        assert m, name
        assert tuple(int(x, 0) for x in m.group(1).split(",")) == want, (name, m.group(1))


def test_the_coverage_table(rec, opts):
    assert GC.coverage(rec, opts) == GC.COVERAGE
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_glb_tags.npz")) <= 567348      # tests/golden/ref_vectors.npz


def test_every_edge_is_present_on_both_sides(rec, opts):
    cs = GC.cases()
    info = {}
    for c in cs:
        r = rec.get(c["name"])
        k, walk = GC.size_class(c, opts[c["optset"]])
        info[c["name"]] = (c, r, k, walk, GC.md_runs(r["md"]), GC.cigar_text(r["cigar"]))
        # what the MD must always be: the target columns of the M runs and of the inner deletions, and NM's gaps
        runs = info[c["name"]][4]
        ops = [(int(w) & 0xf, int(w) >> 4) for w in r["cigar"]]
        inner = [(op, n) for i, (op, n) in enumerate(ops) if not (op == 2 and i in (0, len(ops) - 1))]
        assert sum(u for u, _, _ in runs) + sum(1 for _, kind, _ in runs if kind == "mm") == sum(n for op, n in ops if op == 0), c["name"]
        assert sorted(d for _, kind, d in runs if kind == "del") == sorted(n for op, n in inner if op == 2), c["name"]
        assert r["NM"] + r["ZC"] == sum(1 for _, kind, _ in runs if kind == "mm") + sum(n for op, n in inner if op in (1, 2)), c["name"]
        assert r["bss_u"] == int(r["ZC"] == 0), c["name"]

    def seen(walk, klass=None):
        return {(u, kind) for c, r, k, w, runs, _ in info.values() if w == walk and klass in (None, k) for u, kind, _ in runs}
    # ---- digit edges: every run length at which the decimal grows, in each of the three places, in the staged walk
    staged = seen("staged")
    for u in (0, 1, 9, 10, 99, 100, 999, 1000):
        for kind in ("mm", "del", "end"):
            assert (u, kind) in staged, (u, kind)
    assert {(9999, "mm"), (10000, "del")} <= seen("lane", 2)
    assert {(100000, "mm"), (99999, "del")} <= seen("lane", 3)
    assert all(len(info[n][0]["seq"]) > 100000 and info[n][2] == 3 for n in ("dig_mm100000", "dig_del99999"))
    # ---- lane and block edges
    for v in GC.VIEWS:
        c, r, k, walk, runs, text = info["lane_cols_" + v]
        assert walk == "staged" and [u for u, _, _ in runs] == [0, 62, 0, 62, 71, 0] and text == "200M"      # columns 0, 63, 64, 127 and 199
    for n in (63, 64, 65, 128):
        c, r, k, walk, runs, text = info["lane_len%d_last" % n]
        assert walk == "staged" and text == "%dM" % n and [(u, kind) for u, kind, _ in runs] == [(n - 1, "mm"), (0, "end")]
    assert info["lane_runs_63_64_65_128"][5] == "63M2I64M2D65M1I128M1D40M" and info["lane_runs_63_64_65_128"][3] == "staged"
    assert [(u, kind) for u, kind, _ in info["lane_clean_block"][4]] == [(10, "mm"), (139, "mm"), (41, "end")]      # columns 10 and 150: block 64..127 is clean
    assert [u for u, _, _ in info["lane_full_block"][4]] == [64] + [0] * 63 + [64]
    for name, n, k in (("lane_all256", 256, 0), ("lane_all512", 512, 1)):
        assert info[name][2:4] == (k, "staged") and len(info[name][1]["md"]) == 2 * n + 1 and info[name][1]["NM"] == n
    # ---- runs across operations
    for v in GC.VIEWS:
        assert info["ops_mim_" + v][5] == "50M3I50M" and info["ops_mim_" + v][1]["md"] == b"100" and info["ops_mim_" + v][1]["NM"] == 3
    assert any((0, "del", 3) in info[n][4] for n in ("dig_del0_p1", "dig_del0_p0"))      # a mismatch in the column before a D
    runs = info["ops_mm_after_d"][4]
    assert [(u, kind) for u, kind, _ in runs] == [(40, "del"), (0, "mm"), (39, "end")]      # ... and in the column behind it
    for n in (1, 63, 64, 65, 200):
        assert info["ops_d%d" % n][5] == "60M%dD60M" % n and info["ops_d%d" % n][3] == "staged"
    assert info["ops_i_first"][5] == "3I100M" and info["ops_i_last"][5] == "100M3I"
    for name, text, md, nm in (("ops_d_first", "10D150M", b"150", 0), ("ops_d_last", "150M10D", b"150", 0), ("ops_d_first_alt", "10D150M", None, 1)):
        assert info[name][5] == text and info[name][1]["NM"] == nm and md in (None, info[name][1]["md"])      # skipped in MD and NM
    assert info["ops_d_near_end"][5] == "140M5D10M"
    # ---- both walks on both sides of each stage
    for name, k, walk, tlen in (("tcap_t512", 0, "staged", 512), ("tcap_t513", 0, "lane", 513), ("tcap_t2048", 1, "staged", 2048), ("tcap_t2049", 1, "lane", 2049)):
        c, r = info[name][0], info[name][1]
        assert info[name][2:4] == (k, walk) and c["re"] - c["rb"] == tlen == GC.TCAP[k] + (walk == "lane"), name
        assert any(kind == "del" and d > 200 for _, kind, d in info[name][4]), name
    # ---- views and parents: every family in all four; conversions of both kinds in one read, each parent counting its own
    for fam in ("digit", "lane", "ops", "view"):
        assert {("R" if c["rev"] else "F") + str(c["parent"]) for c in cs if c["family"] == fam} == set(GC.VIEWS), fam
    assert {("R" if c["rev"] else "F") + str(c["parent"]) for c in cs if c["family"] in ("retry", "tcap")} == set(GC.VIEWS)
    for v in GC.VIEWS:
        r = info["view_conv_" + v][1]
        assert r["ZC"] > 10 and r["NM"] > 10 and r["bss_u"] == 0 and r["ZR"] == 0, v
        r = info["view_ret_" + v][1]
        assert (r["ZC"], r["NM"], r["bss_u"]) == (0, 0, 1) and r["ZR"] > 10, v
        r = info["view_n_" + v][1]
        cols, at = [], 0      # the columns of the MD's mismatches: the N of column 70 is one of them, and counted in NM
        for u, kind, _ in info["view_n_" + v][4]:
            at += u
            cols.append(at)
            at += 1
        assert 70 in cols[:-1] and r["NM"] >= 1 and int(info["view_n_" + v][0]["seq"][79 if v[0] == "R" else 70]) == 4, v
        assert any(kind == "del" for _, kind, _ in info["view_dp_" + v][4]), v
    assert {info["view_n_" + v][1]["bss_u"] for v in GC.VIEWS} == {0, 1}
    # ---- the retry loop: every way out, a try that changes the alignment, the no-gap branch inside the loop
    assert {info[c["name"]][1]["exit"] for c in cs if c["n_try"] == 3} == {"truesc", "same_score", "w_max", "tries"}
    assert info["try_first"][1]["tries"] == [(5, 147)]
    assert len(info["try_wmax_capped"][1]["tries"]) == 2 and info["try_wmax_capped"][1]["tries"][1][0] == 400
    for name in ("try_changes", "try_changes_alt", "try_tries"):
        t = info[name][1]["tries"]
        assert len(t) == 3 and t[0][1] < t[1][1], name
    assert info["try_nogap"][1]["tries"] == [(0, 141), (0, 141)] and info["try_nogap"][5] == "150M"
    # ---- both option sets in DP and in pattern jobs; a deletion in the MD in every size class
    assert {c["nogap"] for c in cs if c["optset"] == "alt"} == {True, False}
    assert all(n > 0 for n in GC.COVERAGE["class_with_deletion"])


# ------------------------------------------------------------------------------------------ the recording against a fresh call
def test_the_recording_equals_a_fresh_call(rec, index_base):
    R = oracle_lib.ref_lib()
    if R is None or not hasattr(R, "ref_gen_cigar2"):
        pytest.skip("oracle/_ref is not built")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_vectors_glbtags as MV
    rows = MV.record(MV.ref_handle(), index_base)
    assert len(rows) == len(GC.cases())
    for c, (tries, how, r) in zip(GC.cases(), rows):
        want = rec.get(c["name"])
        got = dict(r, tries=tries, exit=how, w=tries[-1][0])
        for f in ("tries", "exit", "score", "NM", "ZC", "ZR", "bss_u", "md", "w"):
            assert got[f] == want[f], (c["name"], f, got[f], want[f])
        assert (got["cigar"] == want["cigar"]).all(), c["name"]


# ------------------------------------------------------------------------------------------ the host's own walk
class HookReg(C.Structure):      # bsx_hook_reg_t (csrc/host/hook_types.h)
    _fields_ = [("rb", C.c_int64), ("re", C.c_int64)] + [(k, C.c_int32) for k in
                ("qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp", "is_alt")] + \
               [("hash", C.c_uint64), ("flag", C.c_int32), ("mapq", C.c_int32), ("frac_rep", C.c_float), ("bss", C.c_uint8), ("parent", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("pos", C.c_int32), ("n_cigar", C.c_int32), ("NM", C.c_int32), ("bss_u", C.c_int32), ("is_rev", C.c_uint32), ("ZC", C.c_uint32), ("ZR", C.c_uint32),
                ("pad2", C.c_uint32), ("cigar", C.c_void_p)]


def test_host_walk_equals_the_recording(rec, index_base):
    idx = Index(index_base)
    L = B.lib()
    L.bsx_hook_setsam_finish.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    opt = default_opt()
    starts = np.concatenate([[0], np.cumsum([n for _, n in GC.CONTIGS])])
    n_squeezed = 0
    for c in GC.cases():
        want = rec.get(c["name"])
        seq = c["seq"].copy()
        rd = B.Read()
        rd.l_seq = len(seq)
        rd.seq = seq.ctypes.data_as(C.POINTER(C.c_uint8))
        h = HookReg()
        h.rb, h.re, h.qb, h.qe, h.rid, h.parent = c["rb"], c["re"], 0, len(seq), GC.contig_of(c["f"]), c["parent"]
        cg = want["cigar"].copy()
        out = (C.c_int * 3)()
        oc = np.zeros(GC.CIGAR_CAP, np.uint32)
        omd = C.create_string_buffer(len(want["md"]) + 64)
        n = L.bsx_hook_setsam_finish(C.byref(opt), idx.h, C.byref(rd), C.byref(h), cg.ctypes.data_as(C.c_void_p), len(cg), None, None, out,
                                     oc.ctypes.data_as(C.c_void_p), GC.CIGAR_CAP, omd, len(want["md"]) + 64)
        # what mem_alnreg_setSAM leaves of the CIGAR (mem_alnreg_format.c:86-96): a leading deletion moves the position, else a trailing one is dropped
        ops, lead = list(want["cigar"]), 0
        if ops[0] & 0xf == 2:
            lead = int(ops.pop(0)) >> 4
            n_squeezed += 1
        elif ops[-1] & 0xf == 2:
            ops.pop()
            n_squeezed += 1
        assert n == len(ops) and list(oc[:n]) == ops, (c["name"], GC.cigar_text(oc[:max(n, 0)]))
        assert omd.value == want["md"] and out[2] == want["NM"] and out[1] == int(c["rev"]), (c["name"], omd.value[:80], want["md"][:80], out[2], want["NM"])
        assert out[0] == c["f"] - starts[GC.contig_of(c["f"])] + lead, (c["name"], out[0])
    assert n_squeezed >= 3
    idx.close()


# ------------------------------------------------------------------------------------------ the CPU restatement of the kernel's first half
def test_port_global_equals_the_recording(rec, index_base, opts):
    idx = Index(index_base)
    port = oracle_lib.Port(idx, n_threads=4)
    cs = GC.cases()
    buf, off = GC.read_buffer(cs)
    n = 0
    for oname, _ in GC.OPTSETS:
        sel = [i for i, c in enumerate(cs) if c["optset"] == oname]
        jobs = np.array([GC.job_of(cs[i], int(off[i]), k * GC.CIGAR_CAP, opts[oname]) for k, i in enumerate(sel)], dtype=GLB_DT)
        port.set_opt(opts[oname])
        port.set_reads(buf)
        res, pool = port.global_(jobs, len(sel) * GC.CIGAR_CAP)
        for k, i in enumerate(sel):
            want = rec.get(cs[i]["name"])
            got = pool[k * GC.CIGAR_CAP:k * GC.CIGAR_CAP + max(0, int(res[k]["n_cigar"]))]
            assert (int(res[k]["score"]), int(res[k]["n_cigar"]), int(res[k]["w_used"])) == (want["score"], len(want["cigar"]), want["w"]), (cs[i]["name"], res[k], want)
            assert (got == want["cigar"]).all(), (cs[i]["name"], GC.cigar_text(got), GC.cigar_text(want["cigar"]))
            n += 1
    assert n == len(cs)
    idx.close()
