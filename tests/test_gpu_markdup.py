"""-m gpu: duplicate marking on the device.  (1) Device.markdup_batch (k_markdup.hip) against a Python dict on designed key lists: one batch and
several, a small first table that has to grow, claim words cut to 8 bits so that different keys meet in a slot; (2) the HIP command line with
--markdup over several chunks of several slices against the CPU checker (whose table is the host's), the model and its own plain run; (3) with
--qc and with a bsconv filter; (4) the totals of two streams of one process."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import e2e_cases as E
import bsconv_cases as B
import qc_cases as QC
import qc_model as Q
import markdup_cases as MC
import markdup_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(ROOT, "oracle", "oracle_align")
SIZES = [1, 63, 64, 65, 4096]
M64 = (1 << 64) - 1
ONES = np.uint64(M64)


# ---------------------------------------------------------------------------------------------- (1) the batch seam
def end(contig, u5, rev=0, yd=0):
    from biscuit_amd import _lib as L_
    return L_.MD_PLACED | (L_.MD_REVERSE if rev else 0) | (L_.MD_YD if yd else 0) | (contig & 0xfffffff) << 33 | ((u5 + L_.MD_U5_BIAS) & 0x1ffffffff)


def key_lists(n):
    """{name: uint64[n, 2]}: what the table must tell apart, and what it must not"""
    r = np.random.default_rng(1000 + n)
    i = np.arange(n, dtype=np.uint64)
    base = np.array([end(3, 123456, 0, 1), end(3, 123700, 1, 1)], np.uint64)
    out = {"all_equal": np.tile(base, (n, 1))}      # (at 64 and more: a whole wave contending for one slot)
    out["all_distinct"] = np.stack([np.uint64(end(1, 1000)) + i, np.full(n, end(1, 5000, 1), np.uint64)], 1)
    out["high_word_only"] = np.stack([np.full(n, base[0]), np.uint64(end(2, 77, 1)) + (i % np.uint64(max(1, n // 2)))], 1)      # every key twice (n >= 2)
    bit = np.stack([np.full(n, base[0]), np.full(n, base[1])], 1)
    for k in range(n):      # one bit of the 128 flipped, the same bit again 61 keys later
        b = (k % 61) * 2 + 1
        bit[k, b // 64] ^= np.uint64(1 << (b % 64))
    out["one_bit"] = bit
    placed = np.tile(base, (n, 1))      # read 2 placed / not placed (only the placed bit differs), in a random order
    placed[r.random(n) < 0.5, 1] &= np.uint64(~(1 << 63) & M64)
    out["placed_bit"] = placed
    mixed = np.stack([np.uint64(end(5, 40000)) + r.integers(0, max(2, n // 3), n).astype(np.uint64), np.full(n, end(5, 40300, 1), np.uint64)], 1)
    mixed[r.random(n) < 0.25] = ONES      # no placed end: skipped
    out["all_ones_mixed"] = mixed
    return out


def by_dict(keys):
    seen, out = set(), np.zeros(len(keys), np.uint8)
    for k, (a, b) in enumerate(keys.tolist()):
        if a == M64 and b == M64:
            continue
        out[k] = (a, b) in seen
        seen.add((a, b))
    return out


def md_hash(a, b, salt, bits):
    """bsx_markdup_hash (csrc/host/markdup_hash.h) restated"""
    def mix(x):
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & M64
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & M64
        return x ^ x >> 31
    h = mix(mix(a ^ (salt * 0x9E3779B97F4A7C15 & M64)) ^ b)
    if bits < 64:
        h &= (1 << bits) - 1
    return h or 1


def in_batches(dev, keys, step):
    dev.markdup_reset()
    return np.concatenate([dev.markdup_batch(keys[a:a + step], a) for a in range(0, len(keys), step)])


@pytest.fixture(scope="module")
def dev():
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Device
    d = Device(0)
    yield d
    L_.tune("markdup_slots", None)
    L_.tune("markdup_hash_bits", None)
    d.close()


@pytest.mark.parametrize("n", SIZES)
def test_batch_flags_equal_a_dict_in_one_batch_and_in_several(dev, n):
    for name, keys in key_lists(n).items():
        want = by_dict(keys)
        dev.markdup_reset()
        one = dev.markdup_batch(keys, 0)
        assert (one == want).all(), (name, n, np.flatnonzero(one != want)[:10].tolist())
        for step in (1, 64, 37):
            got = in_batches(dev, keys, step)
            assert (got == one).all(), (name, n, step, np.flatnonzero(got != one)[:10].tolist())
        again = dev.markdup_batch(keys, n)      # everything with a key is in the table now
        assert (again == (keys != ONES).any(1)).all(), (name, n)
    if n >= 64:
        assert by_dict(key_lists(n)["all_equal"]).sum() == n - 1 and by_dict(key_lists(n)["all_distinct"]).sum() == 0


@pytest.mark.parametrize("n", SIZES)
def test_a_small_first_table_grows_and_keeps_every_key(dev, n):
    from biscuit_amd import _lib as L_
    L_.tune("markdup_slots", 64)
    try:
        for name, keys in key_lists(n).items():
            want, n_keys = by_dict(keys), len({tuple(k) for k in keys.tolist() if tuple(k) != (M64, M64)})
            # in batches of 64 (one doubling at a time); as one batch (the first table is made large enough); one key, then the rest as one
            # batch (several doublings in one call, every slot moved each time, and the batch's keys looked up in what was moved)
            for how in ("by 64", "one batch", "one key, then the rest"):
                dev.markdup_reset()
                if how == "by 64":
                    got = in_batches(dev, keys, 64)
                elif how == "one batch":
                    got = dev.markdup_batch(keys, 0)
                else:
                    got = np.concatenate([dev.markdup_batch(keys[:1], 0), dev.markdup_batch(keys[1:], 1)])
                    if n > 65:
                        assert dev.markdup_table()[0] >= 64 << 4, (name, dev.markdup_table())      # room is made for every key of the batch, equal or not
                assert (got == want).all(), (name, n, how, np.flatnonzero(got != want)[:10].tolist())
                slots, used = dev.markdup_table()
                assert used == n_keys and used * 2 <= slots, (name, n, how, slots, used)
                if n == 4096 and name == "all_distinct" and how == "by 64":
                    assert slots >= 64 << 4, slots      # 64 -> 128 -> ... : at least four growths, each moving every slot
                assert (dev.markdup_batch(keys, n) == (keys != ONES).any(1)).all(), (name, n, how)      # nothing was lost on the way: duplicates after growth
    finally:
        L_.tune("markdup_slots", None)
        dev.markdup_reset()


@pytest.mark.parametrize("n", [63, 64, 65])
def test_keys_that_share_a_claim_word_take_the_next_salt(dev, n):
    from biscuit_amd import _lib as L_
    L = L_.lib()
    L.bsx_markdup_hash.restype = C.c_uint64
    L.bsx_markdup_hash.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    for name in ("all_distinct", "one_bit", "all_ones_mixed"):
        keys = key_lists(n)[name]
        for k in keys[:5]:
            kk = L_.MarkdupKey((C.c_uint64 * 2)(int(k[0]), int(k[1])))
            assert L.bsx_markdup_hash(C.byref(kk), 3, 8) == md_hash(int(k[0]), int(k[1]), 3, 8)
        by_hash = {}
        for a, b in keys.tolist():
            if (a, b) != (M64, M64):
                by_hash.setdefault(md_hash(a, b, 0, 8), set()).add((a, b))
        if name != "all_ones_mixed":      # the input itself must make a second salt round necessary
            assert any(len(v) > 1 for v in by_hash.values()), (name, n)
        L_.tune("markdup_hash_bits", 8)
        try:
            want = by_dict(keys)
            dev.markdup_reset()
            assert (dev.markdup_batch(keys, 0) == want).all(), (name, n)
            assert (in_batches(dev, keys, 37) == want).all(), (name, n)
        finally:
            L_.tune("markdup_hash_bits", None)
            dev.markdup_reset()


# ---------------------------------------------------------------------------------------------- (2), (3) the command line
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("markdup_gpu"))
    contigs, origin = MC.make_data(d)
    return d, origin, Q.read_fasta(d + "/g.fa")


BIG = ["-@", "4", "g", "big1.fq", "big2.fq"]
BIG_ENV = {"BSX_CHUNK_SIZE": "175000"}      # x 4 threads = 700 000 bases: 2 333 pairs a chunk, three full chunks and a rest, two slices each
_RUNS = {}


def run(exe, d, opts, args, env=None):
    key = (exe, d, tuple(opts), tuple(args), tuple(sorted((env or {}).items())))
    if key not in _RUNS:
        _RUNS[key] = B.run(exe, list(opts) + list(args), d, env=env)
    return _RUNS[key]


def test_command_line_over_chunks_and_slices_equals_cpu_checker_and_model(data):
    d, origin, refs = data
    plain, err0 = run(HIP, d, [], BIG, BIG_ENV)
    chunks = [int(x) for x in re.findall(r"\[M::process\] read (\d+) sequences", err0)]
    assert sum(1 for c in chunks if c >= 2 * 2048) >= 3, chunks
    got, err = run(HIP, d, ["--markdup"], BIG, BIG_ENV)
    dups = MC.check_against_model(plain, got, err, "hip big")
    assert len(dups) >= 3000      # everything placed in the second half of the file, and the copies in the first
    want, _ = run(CPU, d, ["--markdup"], BIG, BIG_ENV)
    E.assert_same_sam(got.encode(), want.encode(), "hip against the CPU checker")
    for a, b in zip(plain.split("\n"), got.split("\n")):      # apart from the flag column: the plain run
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:1] + fa[2:] == fb[:1] + fb[2:], a[:200]


def test_command_line_gives_the_same_bytes_again_and_with_overlapping_back_halves(data):
    d, origin, refs = data
    got, _ = run(HIP, d, ["--markdup"], BIG, BIG_ENV)
    again, _ = B.run(HIP, ["--markdup"] + BIG, d, env=BIG_ENV)
    assert again == got
    over, _ = B.run(HIP, ["--markdup"] + BIG, d, env=dict(BIG_ENV, BSX_TUNE="stream_whole_chunk=2"))
    assert over == got


@pytest.mark.parametrize("case", ["paired", "single_end", "interleaved", "clipping"])
def test_command_line_cases_equal_the_model(data, case):
    d, origin, refs = data
    args = dict(MC.CASES)[case]
    plain, _ = run(HIP, d, [], args)
    got, err = run(HIP, d, ["--markdup"], args)
    assert len(MC.check_against_model(plain, got, err, case)) >= 20


def test_with_qc_the_duplicate_table_is_the_models_over_the_marked_sam(data):
    d, origin, refs = data
    args = dict(MC.CASES)["paired"]
    sam, files = QC.run_qc(HIP, ["--markdup"], args, d, d + "/hip_md")
    only, _ = run(HIP, d, ["--markdup"], args)
    assert sam == only
    reads, paired = QC.reads_of(d, args)
    c = QC.check_files(files, sam, refs, reads, paired, "hip --qc --markdup")
    assert c.all_dup >= 200 and 0 < c.q40_dup <= c.all_dup
    csam, cfiles = QC.run_qc(CPU, ["--markdup"], args, d, d + "/cpu_md")
    assert cfiles == files and csam == sam


def test_with_a_bsconv_filter_the_flags_are_those_of_the_unfiltered_decision(data):
    d, origin, refs = data
    args = dict(MC.CASES)["paired"]
    full, _ = B.run(HIP, ["--markdup", "--bsconv"] + args, d)
    kept, err = B.run(HIP, ["--markdup", "--bsconv-max-cph", "1"] + args, d)
    fl, kl = full.split("\n"), kept.split("\n")
    assert 0 < len(kl) < len(fl)
    it = iter(fl)
    assert all(any(k == f for f in it) for k in kl)
    plain, _ = run(HIP, d, [], args)
    dups, _, n, n_keyed = M.process(plain)
    assert MC.stderr_counts(err) == (n, n_keyed, len(dups))
    ckept, _ = B.run(CPU, ["--markdup", "--bsconv-max-cph", "1"] + args, d)
    E.assert_same_sam(kept.encode(), ckept.encode(), "filtered, hip against the CPU checker")


# ---------------------------------------------------------------------------------------------- (4) streams
def test_two_streams_of_one_process_each_count_their_own(data):
    from biscuit_amd import _lib as L_
    from biscuit_amd.api import Index, Device, default_opt
    d, origin, refs = data
    L = L_.lib()
    idx = Index(d + "/g")
    dv = Device(0)
    dv.upload_index(idx)
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
    L.bsx_stream_set_markdup.argtypes = [C.c_void_p, C.c_int]
    L.bsx_stream_markdup_totals.argtypes = [C.c_void_p, C.c_void_p]
    n_pairs, made, streams = 2500, [], []      # (two slices a chunk)

    def one_stream(seeds):
        """chunks simulated from `seeds` (a seed again: the same pairs again) through a stream of their own -> (stream, SAM text)"""
        chunks = []
        for sd in seeds:
            p = C.c_void_p()
            L_.check(L.bsx_sim_pairs(idx.h, n_pairs, 150, sd, 200, 500, 0.01, 0.2, C.byref(p)), "sim_pairs")
            chunks.append(p)
            made.append(p)
        s = C.c_void_p()
        L_.check(L.bsx_stream_open(dv.h, C.byref(opt), idx.h, None, C.byref(s)), "stream_open")
        streams.append(s)
        L_.check(L.bsx_stream_set_markdup(s, 1), "set_markdup")
        for k, p in enumerate(chunks):
            L_.check(L.bsx_stream_push(s, 2 * n_pairs * k, 2 * n_pairs, p), "push")
        L_.check(L.bsx_stream_flush(s), "flush")
        text = ""
        for p in chunks:
            rd = C.cast(p, C.POINTER(L_.Read))
            text += "".join(C.string_at(rd[i].sam).decode() for i in range(2 * n_pairs))
        return s, text

    def totals(s):
        t = L_.MarkdupTotals()
        L_.check(L.bsx_stream_markdup_totals(s, C.byref(t)), "totals")
        return t.n_templates, t.n_keyed, t.n_dup

    try:
        got = []
        for seeds in ((900, 901, 900), (902, 902)):
            s, text = one_stream(seeds)
            # the model over the text with the flags taken off again must put them back where they are
            plain = "\n".join("\t".join(f[:1] + [str(int(f[1]) & ~0x400)] + f[2:]) for f in (l.split("\t") for l in text.split("\n") if l)) + "\n"
            dups, want, n, n_keyed = M.process(plain)
            assert want == text
            got.append((s, (n, n_keyed, len(dups))))
            assert totals(s) == (n, n_keyed, len(dups)) and n == len(seeds) * n_pairs and len(dups) >= n_pairs * 9 // 10
        assert got[0][1] != got[1][1]
        for s, want in got:      # the first stream's totals are still its own after the second ran
            assert totals(s) == want
    finally:
        for s in streams:
            L.bsx_stream_close(s)
        for p in made:
            L.bsx_sim_free_reads(p, 2 * n_pairs)
        dv.close()
        idx.close()
