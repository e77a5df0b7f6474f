"""-m gpu: the state of every output pass is torn down by bsx_device_close.  One device handle runs a batch of each of the six passes (column
counts, coverage with both masks, conversion counters, duplicate templates, two sorted runs, BAM records and BGZF members), so that every
state struct of the device holds memory (and the sort and the BAM writer their streams) when the handle is closed; a new handle in the same
process starts from nothing (no slot of the key table, no run) and gives the same tables, flags, permutations, schedule and bytes again."""
import numpy as np
import pytest
import simdata
import test_bam_model as TB
import test_gpu_bam as GB
import test_gpu_cov as TC
import test_gpu_markdup as GM
import test_gpu_meth as TM

pytestmark = pytest.mark.gpu
L_GENOME = 4000


def _inputs():
    from biscuit_amd import _lib as L_
    r = np.random.default_rng(21)
    g = r.integers(0, 4, L_GENOME).astype(np.uint8)
    g[100:104] = 4                                                            # an N run under the first job
    shapes = [(90, [(60, "M")]), (700, [(4, "S"), (30, "M"), (2, "I"), (20, "M"), (3, "D"), (25, "M")]), (1500, [(75, "M"), (5, "H")]),
              (L_GENOME - 50, [(50, "M")]), (0, [(40, "M"), (1, "D"), (40, "M")]), (720, [(80, "M")])]
    jobs = [TM._make(r, g, fpos, ops, rev=bool(i & 1), read2=bool(i & 2), tag=i % 3) for i, (fpos, ops) in enumerate(shapes)]
    meth, meth_pool, buf = TM._arrays(jobs)
    # the same records as column-count jobs (their CIGARs are in the conversion pool) and as coverage jobs
    qc = np.array([(j["fpos"], j["roff"], 0, j["rlen"], j["cig_off"], j["n_cigar"], j["flags"] | L_.QC_STRAND | L_.QC_CINREAD | L_.QC_BSCONV) for j in meth],
                  dtype=np.dtype(L_.QcJob))
    cov, cov_pool = TC._job_arrays([(fpos, ops, bool(i & 1)) for i, (fpos, ops) in enumerate(shapes)])
    keys = np.array([[GM.end(1, 100 + 7 * (i % 5)), GM.end(1, 400 + 7 * (i % 5), 1)] for i in range(12)], np.uint64)      # five templates, twelve times
    sort_keys = [np.array([L_.sort_key(i % 3, int(p), i & 1) for i, p in enumerate(r.integers(0, L_GENOME, n))], np.uint64) for n in (9, 14)]
    text = b"".join(GB.line(i) + b"\n" for i in range(7))
    return dict(g=g, buf=buf, meth=meth, meth_pool=meth_pool, qc=qc, cov=cov, cov_pool=cov_pool, keys=keys, sort_keys=sort_keys, text=text,
                top=[(10, 300), (1490, 1600)], bot=[(650, 800)])


def _round(dev, x):
    """one batch of every pass -> what each gives back, as a flat list of arrays and bytes"""
    out = []
    dev.set_reads(x["buf"])
    dev.qc_batch(x["qc"], x["meth_pool"])
    out += list(dev.qc_read())
    dev.cov_batch(x["cov"], x["cov_pool"])
    dev.cov_set_mask(0, x["top"])
    dev.cov_set_mask(1, x["bot"])
    out += dev.cov_tables()
    dev.meth_batch(x["meth"], x["meth_pool"])
    out += [dev.meth_read(0, L_GENOME)] + list(dev.meth_tables())
    sites = dev.meth_sites(0, L_GENOME, "c")
    out += [sites]
    out += [dev.markdup_batch(x["keys"][:5], 0), dev.markdup_batch(x["keys"][5:], 5)]
    out += [dev.sort_run(k) for k in x["sort_keys"]] + [dev.sort_schedule()]
    body, bad, why = dev.bam_encode(TB.HDR, x["text"])
    assert (bad, why) == (-1, 0)
    out += [body, dev.bgzf_deflate(body)]
    return out, len(sites)


def test_every_pass_gives_the_same_again_on_a_new_handle_after_close(tmp_path):
    from biscuit_amd.api import Index, Device
    x = _inputs()
    d = str(tmp_path)
    simdata.write_genome(d + "/g.fa", [("g0", x["g"][:2500]), ("g1", x["g"][2500:])])
    Index.build(d + "/g.fa", d + "/g").close()
    idx = Index(d + "/g")
    assert idx.l_pac == L_GENOME
    rounds = []
    try:
        for k in range(2):
            dev = Device(0)
            try:
                dev.upload_index(idx)
                assert dev.markdup_table() == (0, 0) and dev.sort_info() == (0, 0), k      # nothing of the handle closed before
                got, n_sites = _round(dev, x)
                slots, used = dev.markdup_table()
                assert slots > 0 and used == 5 and dev.sort_info() == (2, 23)                  # the states are there when the handle is closed
                rounds.append(got)
            finally:
                dev.close()
        # not vacuous: column counts, depths, masks, counters, sites, duplicates, both runs and the bytes
        one = rounds[0]
        readpos, conv, confusion = one[0], one[1], one[2]
        assert readpos.sum() > 0 and confusion.sum() > 0
        cov = one[3:15]
        assert all(int(t[1:].sum()) > 0 for t in (cov[0], cov[4], cov[8])) and int(cov[0].sum()) == L_GENOME
        assert one[15].sum() > 0 and n_sites > 0
        assert one[19].tolist() == [0] * 5 and one[20].tolist() == [1] * 7
        for perm, keys in zip(one[21:23], x["sort_keys"]):
            assert (perm == np.argsort(keys, kind="stable")).all()
        assert len(one[23]) == 23 and sorted(set(one[23].tolist())) == [0, 1]
        assert len(one[24]) > 0 and one[25][:4] == b"\x1f\x8b\x08\x04"
        assert len(rounds[1]) == len(one) == 26
        for i, (a, b) in enumerate(zip(one, rounds[1])):
            assert (a == b) if isinstance(a, bytes) else (a.shape == b.shape and (a == b).all()), i
    finally:
        idx.close()
