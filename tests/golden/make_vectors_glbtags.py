#!/usr/bin/env python3
"""Generates tests/golden/ref_glb_tags.npz: what the REAL reference makes of the designed global-alignment jobs of tests/glb_tag_cases.py --
bis_bwa_gen_cigar2 (lib/aln/bwa.c:290-430: the band set-up, ksw_global2, then NM / MD / ZC / ZR / bss_u from the CIGAR) called through
ref_gen_cigar2 of oracle/ref_shim.c over an index that this repository's builder wrote and the reference's bwa_idx_load read, both strand
views of it.  The eight lines of the band-doubling loop around that call (mem_alnreg_format.c:65-77; mem_alnreg_format.c itself does not
build here) are restated below: every try's (w, score) is recorded, how the loop ended, and the last try's outputs.

The file holds recorded results and two CRCs (genome, read buffer) only.

    make -C oracle && python tests/golden/make_vectors_glbtags.py

prints the coverage table that tests/test_glb_tags_recorded_cpu.py and tests/test_gpu_glb_tags_recorded.py hold as constants, and asserts of
its own recording what every case is named for."""
import ctypes as C
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import glb_tag_cases as GC  # noqa: E402
from biscuit_amd.api import Index, default_opt  # noqa: E402


def ref_handle():
    """-> (library, load(prefix) -> handle)"""
    R = oracle_lib.ref_lib()
    assert R is not None and hasattr(R, "ref_gen_cigar2"), "oracle/_ref/libbiscuit_ref.so missing or old: run `make -C oracle`"
    R.ref_idx_load.restype = C.c_void_p
    R.ref_idx_load.argtypes = [C.c_char_p]
    R.ref_idx_free.argtypes = [C.c_void_p]
    R.ref_gen_cigar2.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    return R


def ref_matrix(R, opt, parent):
    """the reference's own scoring matrix for a parent (bwa_fill_scmat_ct / _ga), which the option set's must equal"""
    m = (C.c_int8 * 25)()
    R.ref_fill_scmat(1 if parent else 2, opt.a, opt.b, m)
    assert list(m) == list(opt.ctmat if parent else opt.gamat)
    return m


def gen_cigar2(R, h, opt, c, w):
    """one call of the reference for a case at bandwidth w -> dict(score, cigar, NM, ZC, ZR, bss_u, md without its NUL)"""
    seq = c["seq"].copy()      # (the reference reverses the query in place and back)
    out = np.zeros(7, np.int64)
    cg = np.zeros(GC.CIGAR_CAP, np.uint32)
    md_cap = 2 * (c["re"] - c["rb"]) + 64
    md = C.create_string_buffer(md_cap)
    rc = R.ref_gen_cigar2(h, ref_matrix(R, opt, c["parent"]), opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, w, len(seq), seq.ctypes.data_as(C.c_void_p),
                          c["rb"], c["re"], c["parent"], out.ctypes.data_as(C.c_void_p), cg.ctypes.data_as(C.c_void_p), GC.CIGAR_CAP, md, md_cap)
    assert rc == 0 and (seq == c["seq"]).all(), c["name"]
    n = int(out[1])
    assert n > 0 and 0 <= out[6] < md_cap - 1, (c["name"], out)      # (an earlier try's CIGAR may outgrow the cap: only the last one's is kept)
    return {"score": int(out[0]), "n_cigar": n, "cigar": cg[:min(n, GC.CIGAR_CAP)].copy(), "NM": int(out[2]), "ZC": int(out[3]), "ZR": int(out[4]), "bss_u": int(out[5]), "md": md.raw[:int(out[6])]}


def set_sam_loop(R, h, opt, c):
    """mem_alnreg_format.c:65-77 around the real function -> ([(w, score) of every try], how it ended, the last try's outputs)"""
    w, last_sc, tries = c["w0"], -(1 << 30), []
    if c["n_try"] == 1:      # the jobs that are one call of the function, at their own bandwidth
        r = gen_cigar2(R, h, opt, c, w)
        return [(w, r["score"])], "single", r
    how = "tries"
    for _ in range(3):
        w = min(w, opt.w << 2)
        r = gen_cigar2(R, h, opt, c, w)
        tries.append((w, r["score"]))
        if r["score"] == last_sc:
            how = "same_score"
            break
        if w == opt.w << 2:
            how = "w_max"
            break
        if r["score"] >= c["truesc"] - opt.a:
            how = "truesc"
            break
        w <<= 1
        last_sc = r["score"]
    return tries, how, r


def record(R, base):
    h = R.ref_idx_load(base.encode())
    assert h, "the reference could not load the index"
    opts = {o: GC.set_opt(default_opt(), o) for o, _ in GC.OPTSETS}
    rows = []
    for c in GC.cases():
        tries, how, r = set_sam_loop(R, h, opts[c["optset"]], c)
        assert r["n_cigar"] <= GC.CIGAR_CAP, (c["name"], r["n_cigar"])
        rows.append((tries, how, r))
    R.ref_idx_free(h)
    return rows


def main():
    R = ref_handle()
    d = tempfile.mkdtemp(prefix="bsx_glbtags_")
    GC.write_fasta(d + "/g.fa")
    idx = Index.build(d + "/g.fa", d + "/g")
    assert idx.l_pac == GC.L_PAC
    idx.close()
    rows = record(R, d + "/g")
    cases = GC.cases()
    coff = np.concatenate([[0], np.cumsum([len(r["cigar"]) for _, _, r in rows])]).astype(np.int64)
    moff = np.concatenate([[0], np.cumsum([len(r["md"]) for _, _, r in rows])]).astype(np.int64)
    tw, ts = np.zeros((len(rows), 3), np.int32), np.zeros((len(rows), 3), np.int32)
    for i, (tries, _, _) in enumerate(rows):
        for k, (w, s) in enumerate(tries):
            tw[i, k], ts[i, k] = w, s
    out = {
        "genome_crc": np.uint32(GC.genome_crc()), "reads_crc": np.uint32(GC.reads_crc()), "names": np.array([c["name"] for c in cases]),
        "n_tries": np.array([len(t) for t, _, _ in rows], np.int8), "try_w": tw, "try_score": ts, "exit": np.array([GC.EXITS.index(h) for _, h, _ in rows], np.int8),
        "score": np.array([r["score"] for _, _, r in rows], np.int32), "cigar_off": coff, "cigar": np.concatenate([r["cigar"] for _, _, r in rows]).astype(np.uint32),
        "NM": np.array([r["NM"] for _, _, r in rows], np.int32), "ZC": np.array([r["ZC"] for _, _, r in rows], np.int32),
        "ZR": np.array([r["ZR"] for _, _, r in rows], np.int32), "bss_u": np.array([r["bss_u"] for _, _, r in rows], np.int8),
        "md_off": moff, "md": np.frombuffer(b"".join(r["md"] for _, _, r in rows), np.uint8),
    }
    path = os.path.join(HERE, "ref_glb_tags.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(rows), "jobs")
    assert os.path.getsize(path) <= 567348

    # ------------------------------------------------------------------------------------------ what every case is named for
    rec = GC.load(path)
    bad = []
    for c in cases:
        r = rec.get(c["name"])
        text = GC.cigar_text(r["cigar"])
        if c["cigar"] is not None:
            bad += [] if text == c["cigar"] else [(c["name"], text, c["cigar"])]
        if c["exit"] is not None:
            bad += [] if r["exit"] == c["exit"] else [(c["name"], r["exit"], r["tries"])]
        if "0^" in c["has"]:
            bad += [] if (0, "del", 3) in GC.md_runs(r["md"]) else [(c["name"], text, r["md"])]
        if "changes" in c["has"]:
            bad += [] if len(r["tries"]) >= 2 and len({s for _, s in r["tries"]}) >= 2 else [(c["name"], r["tries"])]
    assert not bad, "cases that are not what they are named for:\n" + "\n".join(map(str, bad))
    opts = {o: GC.set_opt(default_opt(), o) for o, _ in GC.OPTSETS}
    t = GC.coverage(rec, opts)
    print("jobs per size class (%s): %s" % (", ".join(GC.CLASS_NAMES), t["class"]))
    print("jobs per walk:", t["walk"])
    print("jobs per view x parent:", t["view"])
    print("jobs per loop exit:", t["exit"])
    print("jobs per option set:", t["optset"])
    print("jobs of the no-gap branch:", t["nogap"])
    print("deletions written into an MD: %d; jobs with one, per size class: %s" % (t["md_deletions"], t["class_with_deletion"]))
    print("the longest MD: %d bytes" % t["longest_md"])
    print("COVERAGE =", t)
    for c in cases:
        r = rec.get(c["name"])
        k, walk = GC.size_class(c, opts[c["optset"]])
        md = r["md"].decode()
        print("  %-24s %s%d %-7s %-6s %-6s q %6d t %6d tries %-28s %-10s score %6d NM %3d ZC %3d ZR %3d u %d  %s  %s" % (
            c["name"], "R" if c["rev"] else "F", c["parent"], c["optset"], GC.CLASS_NAMES[k], walk, len(c["seq"]), c["re"] - c["rb"], r["tries"], r["exit"],
            r["score"], r["NM"], r["ZC"], r["ZR"], r["bss_u"], GC.cigar_text(r["cigar"]), md if len(md) <= 60 else md[:40] + "..." + md[-12:]))


if __name__ == "__main__":
    main()
