"""K6 (csrc/hip/k_global.hip: banded global alignment with traceback inside the band-doubling loop, then NM / MD / ZC / ZR / bss_u from the
CIGAR) against the reference's own bis_bwa_gen_cigar2, recorded: the designed jobs of tests/glb_tag_cases.py through Device.global_tags,
Device.global_tags_ctx (the k_global<NC, true> instantiation) and Device.global_ must equal tests/golden/ref_glb_tags.npz job for job --
score, CIGAR, the last try's bandwidth, NM, ZC, ZR, bss_u, the MD's length and its bytes with the NUL -- with the cases alone in list order
and in a fixed permutation among a few hundred ordinary jobs of 150 bases, some of which ask for no CIGAR.  None is left out and none may
come back without a CIGAR.

The scoring options belong to the whole call, so each option set of the cases is a batch; the two jobs of a hundred kilobases (rows in HBM,
one lane walking the MD) are a batch of their own when the cases run alone, and its time is printed.

tests/test_glb_tags_recorded_cpu.py checks the recording's coverage, and the host's walk and the CPU restatement against it."""
import time
import numpy as np
import pytest

import glb_tag_cases as GC
from biscuit_amd.api import Index, Device, default_opt, GLB_DT

pytestmark = pytest.mark.gpu

T0 = time.time()
FORMS = ("tags", "ctx", "plain")
PAIR = ("dig_mm100000", "dig_del99999")


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    rec = GC.load()
    assert int(rec.z["genome_crc"]) == GC.genome_crc() and int(rec.z["reads_crc"]) == GC.reads_crc()
    assert rec.names == [c["name"] for c in GC.cases()]
    d = tmp_path_factory.mktemp("glbtags_idx")
    GC.write_fasta(str(d / "g.fa"))
    idx = Index.build(str(d / "g.fa"), str(d / "g"))
    assert idx.l_pac == GC.L_PAC
    dev = Device(0)
    dev.upload_index(idx)
    opts = {o: GC.set_opt(default_opt(), o) for o, _ in GC.OPTSETS}
    yield {"rec": rec, "idx": idx, "dev": dev, "opts": opts}
    dev.close()
    idx.close()
    print("tests/test_gpu_glb_tags_recorded.py: %.1f s from import to teardown" % (time.time() - T0))


def run_batch(env, form, optset, cs, want):
    """one batch of the form over the jobs of cs (case dicts; want[i]: whether job i asks for a CIGAR) -> (jobs, res, pool, tags or None, mds or None)"""
    dev = env["dev"]
    buf, off = GC.read_buffer(cs)
    jobs = np.array([GC.job_of(c, int(off[i]), i * GC.CIGAR_CAP, env["opts"][optset], want[i]) for i, c in enumerate(cs)], dtype=GLB_DT)
    try:
        dev.set_opt(env["opts"][optset])
        dev.set_reads(buf)
        if form == "tags":
            res, pool, tags, mds = dev.global_tags(jobs, len(cs) * GC.CIGAR_CAP)
        elif form == "ctx":
            res, pool, tags, mds, ctx = dev.global_tags_ctx(jobs, len(cs) * GC.CIGAR_CAP)
            assert ctx.shape == (len(cs), 2, 5, 2)
        else:
            (res, pool), tags, mds = dev.global_(jobs, len(cs) * GC.CIGAR_CAP), None, None
    except RuntimeError as e:      # an error of the device, not a difference: nothing more is started on it
        pytest.exit("tests/test_gpu_glb_tags_recorded.py: %s" % e, returncode=3)
    return jobs, res, pool, tags, mds


def differences(env, cs, want, jobs, res, pool, tags, mds):
    """-> (differences from the recording over the recorded jobs of the batch, how many were compared)"""
    rec, bad, n = env["rec"], [], 0
    for i, c in enumerate(cs):
        o = i * GC.CIGAR_CAP
        if not want[i]:
            if int(res[i]["n_cigar"]) != 0 or (tags is not None and (int(tags[i]["l_md"]) != -1 or mds[i] is not None)):
                bad.append("job %d asked for no CIGAR: n_cigar %d, l_md %s" % (i, res[i]["n_cigar"], None if tags is None else tags[i]["l_md"]))
            continue
        if c["name"] is None:
            continue
        w = rec.get(c["name"])
        n += 1
        nc = int(res[i]["n_cigar"])
        if nc <= 0:
            bad.append("%s: came back without a CIGAR (n_cigar %d)" % (c["name"], nc))
            continue
        got = {"score": int(res[i]["score"]), "n_cigar": nc, "w_used": int(res[i]["w_used"]), "cigar": GC.cigar_text(pool[o:o + nc])}
        exp = {"score": w["score"], "n_cigar": len(w["cigar"]), "w_used": w["w"], "cigar": GC.cigar_text(w["cigar"])}
        if tags is not None:
            got.update({f: int(tags[i][f]) for f in ("NM", "ZC", "ZR", "bss_u", "l_md")}, md=mds[i])
            exp.update({f: w[f] for f in ("NM", "ZC", "ZR", "bss_u")}, l_md=len(w["md"]), md=w["md"] + b"\0")
        for f in exp:
            if got[f] != exp[f]:
                show = (lambda v: v if not isinstance(v, (bytes, str)) or len(v) <= 64 else v[:40] + v[-20:])
                bad.append("%s: %s = %r, recorded %r" % (c["name"], f, show(got[f]), show(exp[f])))
    return bad, n


def packed(want, tags):
    """the MD strings are packed through one cursor: the [md_off, md_off + l_md] spans of the jobs with a CIGAR tile the pool's used part without
    a gap or an overlap (so they are disjoint and inside it), and a job without a CIGAR has none"""
    spans = sorted((int(tags[i]["md_off"]), int(tags[i]["l_md"]) + 1) for i in range(len(want)) if want[i])
    assert all(int(tags[i]["l_md"]) == -1 for i in range(len(want)) if not want[i])
    at = 0
    for off, n in spans:
        assert off == at and n >= 2, (off, at, n)
        at += n


def batches(pair_apart):
    cs = GC.cases()
    out = [(o, [c for c in cs if c["optset"] == o and not (pair_apart and c["name"] in PAIR)]) for o, _ in GC.OPTSETS]
    return out + ([("default", [c for c in cs if c["name"] in PAIR])] if pair_apart else [])


def same_forms(want, first, other):
    """the forms agree job for job: res, the CIGAR words in use and, where both have them, the tags and the MD bytes"""
    res, pool, tags, mds = first
    ores, opool, otags, omds = other
    assert (res == ores).all(), np.nonzero(res != ores)[0][:5]
    for i in range(len(want)):
        n = max(0, int(res[i]["n_cigar"]))
        assert (pool[i * GC.CIGAR_CAP:i * GC.CIGAR_CAP + n] == opool[i * GC.CIGAR_CAP:i * GC.CIGAR_CAP + n]).all(), i
    if tags is not None and otags is not None:
        assert omds == mds
        for f in ("NM", "ZC", "ZR", "bss_u", "l_md"):
            assert (tags[f][np.array(want) == 1] == otags[f][np.array(want) == 1]).all(), f


def test_the_cases_alone(env):
    """in list order, through the three forms; the _ctx form's res, CIGARs, tags and MD are the plain form's and the recording's"""
    n = {f: 0 for f in FORMS}
    bad = []
    for k, (optset, cs) in enumerate(batches(True)):
        want, outs = [1] * len(cs), {}
        for form in FORMS:
            t = time.time()
            out = run_batch(env, form, optset, cs, want)
            if k == 2:
                print("tests/test_gpu_glb_tags_recorded.py: the two jobs of a hundred kilobases through %s: %.2f s" % (form, time.time() - t))
            b, m = differences(env, cs, want, *out)
            bad += ["[%s, %s] %s" % (optset, form, x) for x in b]
            n[form] += m
            if out[3] is not None:
                packed(want, out[3])
            outs[form] = out[1:]
        if not bad:
            same_forms(want, outs["tags"], outs["ctx"])
            same_forms(want, outs["tags"], outs["plain"])
    assert all(v == len(GC.cases()) == sum(GC.COVERAGE["class"]) for v in n.values()), n
    assert not bad, "%d differences from the reference over %s jobs:\n%s" % (len(bad), n, "\n".join(bad[:30]))


def test_the_cases_among_ordinary_jobs(env):
    """a fixed permutation of the cases among a few hundred ordinary jobs of 150 bases, every fifth of which asks for no CIGAR"""
    n = {f: 0 for f in FORMS}
    bad = []
    for k, (optset, cs) in enumerate(batches(False)):
        others = GC.ordinary(300 if optset == "default" else 60, 91 + k)
        allc = cs + others
        want = [1] * len(cs) + [int(i % 5 != 0) for i in range(len(others))]
        for i, c in enumerate(others):      # (a job that asks for no CIGAR is one try, as the pipeline makes it)
            if not want[len(cs) + i]:
                c["n_try"] = 1
        perm = np.argsort(GC.Ints(7 + k).words(len(allc)), kind="stable")
        allc, want = [allc[i] for i in perm], [want[i] for i in perm]
        outs = {}
        for form in FORMS:
            jobs, res, pool, tags, mds = run_batch(env, form, optset, allc, want)
            b, m = differences(env, allc, want, jobs, res, pool, tags, mds)
            bad += ["[%s, %s] %s" % (optset, form, x) for x in b]
            n[form] += m
            if tags is not None:
                packed(want, tags)
                assert all(mds[i] is not None and mds[i][-1:] == b"\0" and len(mds[i]) == int(tags[i]["l_md"]) + 1 for i in range(len(allc)) if want[i])
            assert (res["n_cigar"][np.array(want) == 1] > 0).all() and (res["n_cigar"][np.array(want) == 0] == 0).all()
            outs[form] = (res, pool, tags, mds)
        if not bad:      # the forms agree on the ordinary jobs too
            same_forms(want, outs["tags"], outs["ctx"])
            same_forms(want, outs["tags"], outs["plain"])
    assert all(v == len(GC.cases()) for v in n.values()), n
    assert not bad, "%d differences from the reference over %s jobs:\n%s" % (len(bad), n, "\n".join(bad[:30]))
