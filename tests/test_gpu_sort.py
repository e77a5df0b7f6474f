"""-m gpu: coordinate order on the device.  (1) Device.sort_run (k_sort.hip) against np.argsort(kind="stable") on designed key lists at every
size where the code takes another path (one workgroup in LDS up to SORT_TILE keys, tiled passes over HBM beyond); (2) Device.sort_schedule over
several runs against the stable argsort of their concatenation; (3) the HIP command line with --sort against tests/sort_model.py's rewrite of
its own plain run, the CPU checker's --sort output and the same run read back through one-byte buffers, and the QC tables with and without;
(4) sort_run and sort_schedule at sizes where k_sort_scan2, one workgroup over the scan blocks' totals, takes a second and a third step."""
import os
import numpy as np
import pytest
import bsconv_cases as B
import qc_cases as QC
import sort_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(ROOT, "oracle", "oracle_align")


def T():
    from biscuit_amd.api import SORT_TILE
    return SORT_TILE


def sizes():
    t = T()
    return [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, 100003]


def key_lists(n):
    """{name: uint64[n]}"""
    from biscuit_amd import _lib as L_
    r = np.random.default_rng(2000 + n)
    i = np.arange(n, dtype=np.uint64)
    out = {"all_equal": np.full(n, L_.sort_key(2, 123456, 1), np.uint64)}
    out["sorted"] = np.uint64(L_.sort_key(1, 1000, 0)) + i * np.uint64(3)
    out["reversed"] = out["sorted"][::-1].copy()
    out["random64"] = r.integers(0, 1 << 64, n, dtype=np.uint64)
    out["bit0_only"] = np.uint64(L_.sort_key(0, 777, 0)) | r.integers(0, 2, n).astype(np.uint64)
    out["top_byte_only"] = np.uint64(0x00123456789abcde) | (r.integers(0, 256, n).astype(np.uint64) << np.uint64(56))
    out["two_values"] = np.where(i % np.uint64(2) == 0, np.uint64(L_.sort_key(1, 500, 0)), np.uint64(L_.sort_key(0, 900, 1)))      # one bucket takes half a tile
    q = r.integers(0, 1 << 40, n, dtype=np.uint64)
    q[r.random(n) < 0.25] = np.uint64((1 << 64) - 1)
    out["all_ones_at_a_quarter"] = q
    rank = r.integers(0, 3, n)
    rank = np.where(r.random(n) < 0.05, L_.SORT_NO_RANK, rank).astype(np.uint64)
    pos = r.integers(1, max(2, n // 3 + 2), n).astype(np.uint64)      # about three records a position: ties, and both strands
    out["genomic"] = rank << np.uint64(32) | pos << np.uint64(1) | r.integers(0, 2, n).astype(np.uint64)
    return out


@pytest.fixture(scope="module")
def dev():
    from biscuit_amd.api import Device
    d = Device(0)
    yield d
    d.close()


def test_the_key_macro_and_the_tile_are_the_headers():
    import re
    from biscuit_amd import _lib as L_
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert int(re.search(r"#define BSX_SORT_TILE (\d+)", hdr).group(1)) == T() == L_.SORT_TILE
    assert L_.sort_key(L_.SORT_NO_RANK, (1 << 31) - 1, 1) == (1 << 64) - 1 and L_.sort_key(1, 5, 0) == (1 << 32) + 10


@pytest.mark.parametrize("n", range(11))
def test_sort_run_is_the_stable_argsort(dev, n):
    n = sizes()[n]
    dev.sort_reset()
    runs = keys_total = 0
    for name, keys in key_lists(n).items():
        want = np.argsort(keys, kind="stable")
        got = dev.sort_run(keys)
        assert got.dtype == np.uint32 and len(got) == n
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, n, bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist())
        if name == "all_equal":
            assert (got == np.arange(n)).all()
        runs += n > 0
        keys_total += n
        assert dev.sort_info() == (runs, keys_total), (name, n)      # n == 0 adds no run
    dev.sort_reset()
    assert dev.sort_info() == (0, 0)


RUN_SIZES = lambda: [[1, 65, T() + 1, 2, 64], [100003, T()]]


@pytest.mark.parametrize("which", [0, 1])
def test_schedule_is_the_stable_argsort_of_the_concatenation_as_run_ids(dev, which):
    cuts = RUN_SIZES()[which]
    n = sum(cuts)
    run_id = np.repeat(np.arange(len(cuts)), cuts)
    for series in range(2):      # a second series on the same device after a reset
        for name, keys in key_lists(n).items():
            dev.sort_reset()
            assert dev.sort_schedule().size == 0
            at, runs = 0, []
            for c in cuts:
                k = keys[at:at + c]
                perm = dev.sort_run(k)
                assert (perm == np.argsort(k, kind="stable")).all(), (name, c)
                runs.append(k[perm])
                at += c
            assert dev.sort_info() == (len(cuts), n)
            cat = np.concatenate(runs)
            want = run_id[np.argsort(cat, kind="stable")]
            got = dev.sort_schedule()
            bad = np.flatnonzero(got != want)
            assert len(got) == n and len(bad) == 0, (name, cuts, bad[:10].tolist())
            if name == "all_equal":
                assert (np.diff(got.astype(np.int64)) >= 0).all() and (got == run_id).all()
            # following the schedule with one cursor per run gives the sorted concatenation
            merged = np.empty(n, np.uint64)
            order = np.argsort(got, kind="stable")      # output positions of run 0, then of run 1, ...
            merged[order] = cat
            assert (merged == np.sort(cat, kind="stable")).all(), name
            assert dev.sort_info() == (len(cuts), n)      # the runs stay
            assert (dev.sort_schedule() == got).all()
    dev.sort_reset()
    assert dev.sort_info() == (0, 0)


# ---------------------------------------------------------------------------------------------- past one step of k_sort_scan2
# k_sort_scan2 is one workgroup that takes 256 scan blocks (2048 tiles, 4 194 304 keys) a step and carries the sum between steps: 2049 tiles are
# the first size with a second step, 4100 tiles make three.  Every run of the command line's --sort ends in one bsx_sort_schedule over all
# records of the run, so a real library is past these sizes within its first few chunks.
BIG = lambda: [T() * T() + 1, 2 * T() * T() + 3 * T() + 7]
BIG_CASES = [(0, name) for name in ("genomic", "random64", "two_values", "top_byte_only", "all_equal", "reversed")] + [(1, "genomic"), (1, "random64")]
_big_lists = {}


def big_keys(n, name):
    if n not in _big_lists:      # (one size at a time: nine lists of 4 or 8 M keys)
        _big_lists.clear()
        _big_lists[n] = key_lists(n)
    return _big_lists[n][name]


def test_the_large_sizes_pass_one_two_scan_steps():
    from biscuit_amd.api import SORT_TILE
    blocks = [(-(-n // SORT_TILE) * 256 + 2047) // 2048 for n in BIG()]      # sort_n_scan_blocks
    assert SORT_TILE == 2048 and blocks == [257, 513] and [-(-b // 256) for b in blocks] == [2, 3]


@pytest.mark.parametrize("which,name", BIG_CASES)
def test_sort_run_past_one_scan_step_is_the_stable_argsort(dev, which, name):
    n = BIG()[which]
    keys = big_keys(n, name)
    dev.sort_reset()
    want = np.argsort(keys, kind="stable")
    got = dev.sort_run(keys)
    bad = np.flatnonzero(got != want)
    assert len(got) == n and len(bad) == 0, (name, n, len(bad), bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist())
    assert dev.sort_info() == (1, n)
    dev.sort_reset()


@pytest.mark.parametrize("name", ["genomic", "random64", "two_values"])
def test_schedule_of_chunk_sized_runs_whose_total_passes_one_scan_step(dev, name):
    """four runs of about 1.1 M keys, a chunk's worth each: every run takes the tiled passes within one scan step, their concatenation -- sorted
    with the run ids as the payload, not the index -- takes two"""
    cuts = [1100003, 1048576, 1100001, 1150000]
    n = sum(cuts)
    assert max(cuts) <= T() * T() < n and min(cuts) > T()
    keys = big_keys(n, name)
    run_id = np.repeat(np.arange(len(cuts)), cuts)
    dev.sort_reset()
    at, runs = 0, []
    for c in cuts:
        k = keys[at:at + c]
        perm = dev.sort_run(k)
        runs.append(k[perm])
        at += c
    cat = np.concatenate(runs)
    order = np.argsort(cat, kind="stable")
    got = dev.sort_schedule()
    want = run_id[order]
    bad = np.flatnonzero(got != want)
    assert len(got) == n and len(bad) == 0, (name, len(bad), bad[:10].tolist())
    assert dev.sort_info() == (len(cuts), n)
    merged = np.empty(n, np.uint64)      # following the schedule with one cursor per run gives the sorted concatenation
    merged[np.argsort(got, kind="stable")] = cat
    assert (merged == cat[order]).all(), name
    dev.sort_reset()
    assert dev.sort_info() == (0, 0)


# ---------------------------------------------------------------------------------------------- (3) the command line
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sort_gpu"))
    SC.make_data(d)
    return d


@pytest.mark.parametrize("case", ["paired", "single_end", "interleaved", "long_1kb"])
def test_command_line_equals_the_model_the_cpu_checker_and_one_byte_buffers(data, case, tmp_path):
    d = data
    args = dict(SC.CASES)[case]
    tmp = str(tmp_path)
    plain, got, err = SC.run_pair(HIP, [], args, d, sort_opts=("--sort", "--sort-tmp", tmp))
    SC.check_against_model(plain, got, "hip " + case)
    runs, records = SC.sort_counts(err)
    assert records == len(SC.S.split(plain)[1]) and runs == len(SC.chunk_reads(err)) and runs >= (5 if case == "paired" else 2), (runs, records)
    want, _ = B.run(CPU, ["--sort"] + args, d, env=SC.ENV)
    assert got == want, case + ": hip --sort against the CPU checker's"
    tiny, _ = B.run(HIP, ["--sort"] + args, d, env=dict(SC.ENV, BSX_TUNE="sort_buf_bytes=1"))
    assert tiny == got, case + ": one-byte buffers"
    assert os.listdir(tmp) == []


def test_with_markdup_and_qc_the_tables_are_unchanged_by_sort(data):
    d = data
    args = dict(SC.CASES)["paired"]
    sam0, files0 = QC.run_qc(HIP, ["--markdup"], args, d, d + "/qc_plain", env=SC.ENV)
    sam1, files1 = QC.run_qc(HIP, ["--markdup", "--sort"], args, d, d + "/qc_sorted", env=SC.ENV)
    assert files0 == files1 and len(files0) >= 6
    SC.check_against_model(sam0, sam1, "hip --markdup --qc --sort")
    assert any(int(l.split("\t")[1]) & 0x400 for l in sam1.split("\n") if l and l[0] != "@")
