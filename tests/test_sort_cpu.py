"""CPU: `--sort` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the device seam, i.e. the
host's own merge sort in sortout.c) on tests/sort_cases.py: every sorted SAM against tests/sort_model.py's rewrite of the plain run's SAM, byte
for byte; what the data must hold; the refusals; the option off; the temporary directory afterwards.  The -m gpu counterpart
(tests/test_gpu_sort.py) puts k_sort.hip on the other side."""
import os
import resource
import subprocess
import time
import pytest
import bsconv_cases as B
import sort_cases as SC
import sort_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sort"))
    SC.make_data(d)
    return d


_RUNS = {}


def pair(d, opts, args, env=None, sort_opts=("--sort",)):
    key = (d, tuple(opts), tuple(args), tuple(sorted((env or {}).items())), tuple(sort_opts))
    if key not in _RUNS:
        _RUNS[key] = SC.run_pair(CPU, opts, args, d, env=env, sort_opts=sort_opts)
    return _RUNS[key]


@pytest.mark.parametrize("case", [c for c, _ in SC.CASES])
def test_sorted_sam_is_the_models_rewrite_of_the_plain_sam(data, case):
    args = dict(SC.CASES)[case]
    plain, got, err = pair(data, [], args)
    SC.check_against_model(plain, got, case)
    runs, records = SC.sort_counts(err)
    assert records == len(S.split(plain)[1]) and runs == len(SC.chunk_reads(err)), (runs, records)
    assert got.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ\t")


def test_the_data_holds_what_the_rule_is_about(data):
    plain, got, err = pair(data, [], dict(SC.CASES)["paired"])
    chunks = SC.chunk_reads(err)
    n, ties, ties_across, unmapped_placed, both_strands, star = SC.census(plain, chunks)
    print("sort cases:", len(chunks), "chunks;", n, ties, ties_across, unmapped_placed, both_strands, star)
    assert len(chunks) >= 5 and ties_across >= 100 and unmapped_placed >= 100 and both_strands >= 20 and star >= 20


def test_with_markdup_with_a_bsconv_filter_and_through_one_byte_buffers(data):
    args = dict(SC.CASES)["paired"]
    plain, got, _ = pair(data, ["--markdup"], args)
    SC.check_against_model(plain, got, "--markdup")
    assert sum(1 for l in S.split(got)[1] if int(l.split("\t")[1]) & 0x400) >= 200
    plain_f, got_f, _ = pair(data, ["--bsconv-max-cph", "1"], args)
    SC.check_against_model(plain_f, got_f, "bsconv filter")
    assert 0 < len(S.split(got_f)[1]) < len(S.split(pair(data, [], args)[0])[1]) and "\tZN:Z:" in got_f
    _, want, _ = pair(data, [], args)
    tiny, _ = B.run(CPU, ["--sort"] + args, data, env=dict(SC.ENV, BSX_TUNE="sort_buf_bytes=1"))
    assert tiny == want


def test_contig_names_out_of_name_order_and_a_users_sq_order(data):
    args = ["-@", "4", "g2", "m1.fq", "m2.fq"]
    plain, got, _ = pair(data, [], args)
    h, body = S.split(got)
    assert [l.split("\t")[1] for l in h if l.startswith("@SQ")] == ["SN:alpha", "SN:mid", "SN:zeta"]      # name order: not index order (zeta, alpha, mid)
    SC.check_against_model(plain, got, "g2")
    names = [l.split("\t")[2] for l in body]
    first = {n: names.index(n) for n in ("alpha", "mid", "zeta", "*")}
    assert first["alpha"] < first["mid"] < first["zeta"] < first["*"]
    for hdr, lead in (("hdr_rev.txt", "@HD\tVN:1.6\tSO:coordinate\n@SQ\t"), ("hdr_hd.txt", "@HD\tVN:1.5\tSO:coordinate\tGO:none\n@SQ\t")):
        args = ["-@", "4", "-H", hdr, "g", "m1.fq", "m2.fq"]
        plain, got, _ = pair(data, [], args)
        SC.check_against_model(plain, got, hdr)
        assert got.startswith(lead) and got.count("@HD") == 1
        h, body = S.split(got)
        sq = [l.split("\t")[1][3:] for l in h if l.startswith("@SQ")]
        names = [l.split("\t")[2] for l in body]
        at = [names.index(n) for n in sq]
        assert at == sorted(at) and sq != sorted(sq), (hdr, sq, at)      # the user's order, which is not name order


def test_option_off_changes_nothing(data):
    args = dict(SC.CASES)["paired"]
    plain, got, _ = pair(data, [], args)
    golden, err = B.run(CPU, ["-v", "3"] + args, data, env=SC.ENV)
    assert golden == plain and "sort" not in err and "@HD" not in plain
    assert sorted(S.split(plain)[1]) == sorted(S.split(got)[1]) and S.split(plain)[1] != S.split(got)[1]


def run_raw(d, argv, env=None, **kw):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID")}
    e.update(SC.ENV)
    e.update(env or {})
    return subprocess.run([CPU] + argv, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


def test_refused_with_several_ranks_before_connecting(data):
    e = dict(RANK="1", WORLD_SIZE="2", LOCAL_RANK="1", LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=data + "/never", BSX_TUNE="gather_transport=socket")
    t0 = time.time()
    for opt in (["--sort"], ["--sort-tmp", data, "--sort"], ["--sort-t", data, "--sort"]):      # (getopt_long takes unambiguous abbreviations)
        p = run_raw(data, opt + dict(SC.CASES)["paired"], env=e)
        assert p.returncode == 1 and b"--sort" in p.stderr and b"WORLD_SIZE" in p.stderr and p.stdout == b"", opt
    assert time.time() - t0 < 30 and not os.path.exists(data + "/never")


def test_a_bad_temporary_directory_and_sort_tmp_alone_are_refused_before_aligning(data, tmp_path):
    args = dict(SC.CASES)["paired"]
    locked = tmp_path / "locked"
    locked.mkdir()
    a_file = tmp_path / "file"
    a_file.write_text("x")
    bad = [str(tmp_path / "missing"), str(a_file)]
    if os.geteuid() != 0:      # (root writes into a directory without the write bit)
        locked.chmod(0o500)
        bad.append(str(locked))
    for where in bad:
        p = run_raw(data, ["-v", "3", "--sort", "--sort-tmp", where] + args)
        assert p.returncode == 1 and p.stdout == b"" and b"--sort" in p.stderr and where.encode() in p.stderr, where
        assert b"[M::process] read" not in p.stderr, "aligned before the directory was looked at"
    p = run_raw(data, ["-v", "3", "--sort-tmp", str(tmp_path)] + args)
    assert p.returncode == 1 and p.stdout == b"" and b"--sort-tmp" in p.stderr and b"needs --sort" in p.stderr and b"[M::process] read" not in p.stderr


def test_the_temporary_directory_is_empty_after_a_run_and_after_a_write_error(data, tmp_path):
    args = dict(SC.CASES)["paired"]
    tmp = tmp_path / "t"
    tmp.mkdir()
    _, want, _ = pair(data, [], args)
    _, got, _ = SC.run_pair(CPU, [], args, data, sort_opts=("--sort", "--sort-tmp", str(tmp)))
    assert got == want and os.listdir(str(tmp)) == []
    # a file size limit of 256 KB: the temporary file (about 2.5 MB) cannot be completed; stdout and stderr are pipes, which have no size
    p = run_raw(data, ["--sort", "--sort-tmp", str(tmp)] + args, preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_FSIZE, (1 << 18, 1 << 18)))
    assert p.returncode == 1, p.returncode
    assert p.stdout == b"", "output after a failed write"      # not even the header: nothing that looks complete
    assert b"temporary file" in p.stderr and b"failed" in p.stderr, p.stderr[-1000:]
    assert os.listdir(str(tmp)) == []
