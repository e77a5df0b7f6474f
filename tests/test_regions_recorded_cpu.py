"""Regions per strand search against the reference's own, recorded (tests/golden/ref_regions.npz: mem_chain, mem_chain_flt,
mem_flt_chained_seeds and mem_chain2region of lib/aln/memchain.c through oracle/ref_shim.c, on the designed strand searches of
tests/regions_cases.py) -- the parts that need no GPU:

* the front half's host path, which every strand search the device declines takes (bsx_hook_front_regions, csrc/host/pipeline.c: seeding and
  SA look-ups through the batch seams, bsx_chain_build / bsx_chain_filter, the seed filter, the extension rounds), over the CPU restatement
  of the kernels (oracle/port.c): list for list, field for field, in order, frac_rep by its bits
* the Python restatement (oracle/e2e.align1_core), on the cases it gets through in seconds
* the cap table of regions_cases against the typedefs and #defines of rg_common.hpp and k_c2r.hip, and the coverage table -- which case sits at which cap
  and on which side -- against the recorded counts, so that a case that drifts off its edge fails here instead of testing nothing

tests/test_gpu_regions_recorded.py holds the device's side."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest

import oracle_lib
import regions_cases as RC
from biscuit_amd import _lib as B
from biscuit_amd.api import Index, default_opt, SEED_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_MAX_OCC = 300      # the Python restatement extends a chain in milliseconds: a thousand chains are no unit test


@pytest.fixture(scope="module")
def rec():
    r = RC.load()
    assert int(r.z["genome_crc"]) == RC.genome_crc(), "the genome of regions_cases is not the recorded one: run tests/golden/make_vectors_regions.py"
    assert int(r.z["reads_crc"]) == RC.reads_crc(), "the reads of regions_cases are not the recorded ones"
    assert r.names == [c["name"] for c in RC.cases()] and r.optsets == [o[0] for o in RC.OPTSETS]
    return r


@pytest.fixture(scope="module")
def index_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("regions_idx")
    RC.write_fasta(str(d / "g.fa"))
    Index.build(str(d / "g.fa"), str(d / "g")).close()
    return str(d / "g")


def set_opt(opt, oset, max_occ):
    for k, v in oset.items():
        setattr(opt, k, v)
    if max_occ:
        opt.max_occ = max_occ


def batches():
    """the cases by max_occ (an option of the whole call): [(max_occ or None, [case])]"""
    cs = RC.cases()
    return [(m, [c for c in cs if c["max_occ"] == m]) for m in sorted({c["max_occ"] for c in cs}, key=lambda x: x or 0)]


def tasks_of(cs):
    buf, off = RC.read_buffer(cs)
    tasks = np.zeros(2 * len(cs), SEED_DT)
    for i, c in enumerate(cs):
        for k, parent in enumerate((1, 0)):
            tasks[2 * i + k] = (off[i], len(c["seq"]), parent)
    return buf, tasks


# ------------------------------------------------------------------------------------------ the host path
def front_regions(be, opt, idx, buf, tasks):
    f = B.lib().bsx_hook_front_regions
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    n = len(tasks)
    dt = np.dtype(B.Region)
    off, cnt = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32)
    cap = 1 << 15
    out = np.zeros(cap, dt)
    B.check(f(C.byref(be), C.byref(opt), idx.h, buf.ctypes.data_as(C.c_void_p), buf.size, n, tasks.ctypes.data_as(C.c_void_p),
              out.ctypes.data_as(C.c_void_p), cap, off.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)), "bsx_hook_front_regions")
    return out, off, cnt


@pytest.mark.parametrize("optset", [o[0] for o in RC.OPTSETS])
def test_host_path_equals_the_recording(rec, index_base, optset):
    idx = Index(index_base)
    port = oracle_lib.Port(idx, n_threads=4)
    be = port.backend()
    bad, n = [], 0
    for max_occ, cs in batches():
        opt = default_opt()
        opt.n_threads = 4
        set_opt(opt, dict(RC.OPTSETS)[optset], max_occ)
        buf, tasks = tasks_of(cs)
        out, off, cnt = front_regions(be, opt, idx, buf, tasks)
        for i, c in enumerate(cs):
            for k, parent in enumerate((1, 0)):
                t = 2 * i + k
                d = RC.same_regions(out[off[t]:off[t] + cnt[t]], rec.regions(optset, c["name"], parent))
                n += 1
                if d:
                    bad.append("%s parent %d: %s" % (c["name"], parent, d))
    assert n == 2 * len(RC.cases())
    assert not bad, "%d of %d strand searches differ from the reference's regions:\n%s" % (len(bad), n, "\n".join(bad[:20]))
    idx.close()


# ------------------------------------------------------------------------------------------ the Python restatement
def test_python_restatement_equals_the_recording(rec, index_base):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import e2e
    idx = e2e.Index(index_base)
    bad, n = [], 0
    for optset, oset in RC.OPTSETS:
        for c in RC.cases():
            if max(int(rec.counts("default", c["name"], p)[RC.COUNT_KEYS.index("visited")]) for p in (1, 0)) > E2E_MAX_OCC:
                continue
            if optset != "default" and len(c["seq"]) > 300:
                continue      # (the seed filter runs for reads of a kilobase under the default options already)
            opt = e2e.opt_init()
            opt.update(oset)
            e2e.fill_mats(opt)
            if c["max_occ"]:
                opt["max_occ"] = c["max_occ"]
            for parent in (1, 0):
                s = dict(name=c["name"], comment="", seq=c["seq"].copy(), l_seq=len(c["seq"]), bisseq=[None, None], clip5=0, clip3=0)
                regs = []
                e2e.align1_core(opt, idx, s, regs, parent)
                got = np.zeros(len(regs), np.dtype(B.Region))
                for i, r in enumerate(regs):
                    for f in RC.REGION_FIELDS:
                        got[i][f] = r[f]
                d = RC.same_regions(got, rec.regions(optset, c["name"], parent))
                n += 1
                if d:
                    bad.append("%s %s parent %d: %s" % (optset, c["name"], parent, d))
    assert n >= 100, n
    assert not bad, "%d of %d strand searches differ from the reference's regions:\n%s" % (len(bad), n, "\n".join(bad[:20]))


# ------------------------------------------------------------------------------------------ the caps and the coverage
def test_the_cap_table_is_the_headers():
    # the stores and the capacities every region unit reads, then the workspaces of the chains -> regions launches
    src = "".join(open(os.path.join(ROOT, "biscuit_amd", "csrc", "hip", f)).read() for f in ("rg_common.hpp", "k_c2r.hip"))
    for name, (icap, scap, ccap, pcap) in RC.STORES.items():
        m = re.search(r"^typedef RgStore<([^>]*)> %s;" % name, src, re.M)
        assert m, name
        a = [x.strip() for x in m.group(1).split(",")]
        assert [int(a[0]), int(a[1]), int(a[2])] == [icap, scap, ccap], (name, a)
        assert (int(a[7]) if len(a) > 7 else 0) == pcap, (name, a)
    for name, v in RC.DEFINES.items():
        m = re.search(r"^#define %s (\d+)\b" % name, src, re.M)
        assert m and int(m.group(1)) == v, name
    for name, (xseeds, xregs) in RC.C2R.items():
        m = re.search(r"^typedef RgC2rH?T<([^>]*)> %s;" % name, src, re.M)
        assert m, name
        a = [x.strip() for x in m.group(1).split(",")]
        assert [int(a[2]), int(a[3])] == [xseeds, xregs], (name, a)
    m = re.search(r"^typedef RgC2rT<RG_QCAP, RG_WIN, RG_XSEEDS> RgC2r;", src, re.M)
    assert m      # the first chains -> regions launch: RG_XSEEDS seeds a list, RG_XREGS regions (the template's default)
    assert re.search(r"^template <int \w+, int \w+, int \w+, int \w+ = RG_XREGS, bool \w+ = true>\nstruct RgC2rT \{", src, re.M)


def test_every_case_sits_where_the_table_says(rec):
    K = {k: i for i, k in enumerate(RC.COUNT_KEYS)}

    def fits(cnt, store, but=()):
        icap, scap, ccap, pcap = RC.STORES[store]
        lim = {"intervals": icap, "occ": scap, "chains": ccap, "records": pcap if pcap else 1 << 30}
        return all(cnt[K[d]] <= v for d, v in lim.items() if d not in but)

    for store, dim, at, past in RC.EDGES:
        cap = RC.edge_cap(store, dim)
        a = [rec.counts("default", at, p) for p in (1, 0)]
        b = [rec.counts("default", past, p) for p in (1, 0)]
        if store in RC.STORES:
            # at the cap with every other count of that store inside its caps; one past it likewise -- but that in a case of one-seed chains
            # alone occurrences and chains pass the cap together (SCAP == CCAP; the occurrence test comes first and binds)
            assert any(c[K[dim]] == cap and fits(c, store) for c in a), (store, dim, at, [list(c) for c in a])
            assert any(c[K[dim]] == cap + 1 and fits(c, store, but=("occ", "chains") if c[K["occ"]] == c[K["chains"]] else (dim,)) for c in b), (store, dim, past, [list(c) for c in b])
        else:
            assert any(c[K[dim]] == cap for c in a) and any(c[K[dim]] == cap + 1 for c in b), (store, dim, at, past)
    # what each case was designed to show, for at least one parent in full; ties and over-represented intervals for both
    for c in RC.cases():
        cnts = [rec.counts("default", c["name"], p) for p in (1, 0)]
        exact = {k: v for k, v in c["expect"].items() if k in K and k not in ("tied", "over")}
        assert any(all(x[K[k]] == v for k, v in exact.items()) for x in cnts), (c["name"], exact, [list(x) for x in cnts])
        for k in ("tied", "over"):
            if k in c["expect"]:
                assert all(x[K[k]] == c["expect"][k] for x in cnts), (c["name"], k, [list(x) for x in cnts])
        if "regions_min" in c["expect"]:
            assert all(x[0] >= c["expect"]["regions_min"] for x in cnts), c["name"]
    # the over-represented cases walk on past max_occ (memchain.c:325-326): more occurrences visited than the capped sum in one of them
    assert any(rec.counts("default", n, 1)[K["visited"]] > rec.counts("default", n, 1)[K["occ"]] for n in ("over_x64", "over_s64"))
    # three tied starts: one below RgSmall's occurrences, one on a chain of several seeds
    ties = [c["name"] for c in RC.cases() if c["expect"].get("tied")]
    assert len(ties) >= 3
    assert any(max(rec.counts("default", n, p)[K["occ"]] for p in (1, 0)) < 128 for n in ties)
    assert any(min(rec.counts("default", n, p)[K["records"]] for p in (1, 0)) >= 20 for n in ties)
    # read lengths at the rows' ends
    assert {255, 256, 257, 1024, 1025} <= {len(c["seq"]) for c in RC.cases()}
    assert sum(c["name"].startswith("ord") for c in RC.cases()) * 2 >= 24
    # the filter-active option set differs from the default where it should: mem_flt_chained_seeds runs for reads of 150 bases
    assert dict(RC.OPTSETS)["filter"] == {"min_chain_weight": 5}


def test_the_recording_is_a_small_fixture():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_regions.npz")) <= 567348      # tests/golden/ref_vectors.npz
