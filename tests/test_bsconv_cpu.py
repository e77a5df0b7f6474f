"""CPU: `--bsconv` and its filters through the command line over the CPU restatement of the kernels (oracle_align: the backend without the
device seam, i.e. the host walk of sam.c), against tests/bsconv_model.py applied to the plain run's SAM.  The -m gpu counterpart
(tests/test_gpu_bsconv.py) puts the HIP path, whose counts come from k_global, on the other side."""
import os
import subprocess
import pytest
import e2e_cases as E
import bsconv_cases as B
import bsconv_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bsconv"))
    B.make_data(d)
    refs = M.read_fasta(d + "/g.fa")
    assert any(s.endswith("C") for s in refs.values()) and sum(s.count("N") for s in refs.values()) > 100
    plain = {name: B.run(CPU, args, d)[0] for name, args in E.CASES_CORE}
    return d, refs, plain


@pytest.mark.parametrize("case", [c[0] for c in E.CASES_CORE])
def test_annotate_equals_plain_plus_model(data, case):
    d, refs, plain = data
    args = dict(E.CASES_CORE)[case]
    got, err = B.run(CPU, ["--bsconv"] + args, d)
    tot, n, nf = B.check_against_model(plain[case], got, err, refs, M.Conf(), case)
    assert nf == 0 and sum(tot) > 0
    # nothing dropped, unmapped lines unchanged, every other line = the plain line + one last field
    gl, pl = got.split("\n"), plain[case].split("\n")
    assert len(gl) == len(pl)
    n_zn = 0
    for a, b in zip(gl, pl):
        if a != b:
            assert a.startswith(b + "\tZN:Z:CA_R") and not int(b.split("\t")[1]) & 4
            n_zn += 1
        else:
            assert not a or a[0] == "@" or int(a.split("\t")[1]) & 4
    assert n_zn > 20


@pytest.mark.parametrize("case", ["pe150_b0", "long_1kb", "pe150_all_softclip"])
@pytest.mark.parametrize("fi", range(len(B.FILTERS)))
@pytest.mark.parametrize("show", [False, True])
def test_filters_keep_the_models_records(data, case, fi, show):
    d, refs, plain = data
    args = dict(E.CASES_CORE)[case]
    opts, kw = B.FILTERS[fi]
    got, err = B.run(CPU, opts + (["--bsconv-show-filtered"] if show else []) + args, d)
    tot, n, nf = B.check_against_model(plain[case], got, err, refs, M.Conf(show_filtered=show, **kw), "%s %s" % (case, " ".join(opts)))
    if case == "pe150_b0":
        assert 0 < nf < n      # the setting filters something and keeps something


def test_plain_run_says_nothing_about_bsconv(data):
    d, refs, plain = data
    got, err = B.run(CPU, dict(E.CASES_CORE)["pe150_b0"], d)
    assert got == plain["pe150_b0"] and "bsconv" not in err and "ZN:Z" not in got


def test_two_processes_give_the_same_records_and_totals(data):
    """the ranks path: every rank's totals added on rank 0"""
    d, refs, plain = data
    args = ["--bsconv-max-cph", "1", "-@", "1", "g", "b1.fq", "b2.fq"]
    env = {"BSX_CHUNK_SIZE": "20000"}
    one, err1 = B.run(CPU, args, d, env=env)
    base = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID", "BSX_TUNE"):
        base.pop(k, None)
    procs = []
    for r in range(2):
        e = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=d + "/rdv", BSX_TUNE="gather_transport=socket")
        procs.append(subprocess.Popen([CPU] + args, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = [p.communicate(timeout=900) for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][1].decode()[-3000:])
    assert E.strip_pg(outs[0][0]).decode() == one and outs[1][0] == b""
    assert B.stderr_counts(outs[0][1].decode()) == B.stderr_counts(err1) and b"[M::bsconv]" not in outs[1][1]
    assert err1.count("sequences (") >= 2      # more than one chunk, so both ranks had work
