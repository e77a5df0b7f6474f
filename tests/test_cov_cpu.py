"""CPU: `--qc PREFIX --qc-cov` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the device seam,
i.e. the host statement of the depth rule in cov.c), on the cases tests/test_qc_cpu.py uses, with and without the GC BED files (one plain, one
gzip): the thirteen (five) files against tests/cov_model.py over the SAM written, the SAM and the seven files of --qc against the runs without
the option; the option errors.  The -m gpu counterpart (tests/test_gpu_cov.py) puts k_cov on the other side."""
import os
import subprocess
import pytest
import e2e_cases as E
import bsconv_cases as B
import cov_cases as CV
import cov_model as V
import qc_cases as QC
import qc_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cov"))
    contigs = B.make_data(d)
    top, bot = CV.write_beds(d, contigs)
    return d, Q.read_fasta(d + "/g.fa"), top, bot


def test_files_equal_the_model_sam_and_qc_files_are_unchanged(data):
    d, refs, top, bot = data
    seen = []
    for case, args in E.CASES_CORE:
        plain, _ = B.run(CPU, args, d)
        qsam, qfiles = QC.run_qc(CPU, [], args, d, d + "/q_" + case)
        assert sorted(os.path.basename(f) for f in os.listdir(d) if f.startswith("q_" + case + "_")) == sorted("q_" + case + s for s in qfiles)      # --qc alone: its own files only
        sam, files7, cov = CV.run_cov(CPU, [], args, d, d + "/c_" + case)
        assert sam == plain == qsam and files7 == qfiles, case
        seen.append(CV.check_files(cov, sam, refs, None, None, case))
        sam, files7, cov = CV.run_cov(CPU, ["--qc-topgc", top, "--qc-botgc", bot], args, d, d + "/g_" + case)
        assert sam == plain and files7 == qfiles, case
        seen.append(CV.check_files(cov, sam, refs, top, bot, case + " gc"))
    CV.assert_not_vacuous(seen)


def test_qc_alone_still_lists_seven_files(data):
    d, refs, top, bot = data
    sam, files = QC.run_qc(CPU, [], dict(E.CASES_CORE)["pe150_b0"], d, d + "/seven")
    assert len(files) == 7 and sorted(f for f in os.listdir(d) if f.startswith("seven")) == sorted("seven" + s for s in Q.SUFFIXES)


def test_with_a_bsconv_filter_only_the_kept_records_count(data):
    d, refs, top, bot = data
    args = dict(E.CASES_CORE)["pe150_b0"]
    sam, _, cov = CV.run_cov(CPU, ["--bsconv-max-cph", "3"], args, d, d + "/flt")
    plain, _, cov0 = CV.run_cov(CPU, [], args, d, d + "/noflt")
    assert sam.count("\n") < plain.count("\n") and cov != cov0
    CV.check_files(cov, sam, refs, None, None, "filtered")


def _fails(args, d, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([CPU] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
    assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stderr.decode()[-1000:])
    return p.stderr.decode()


def test_option_errors(data):
    d, refs, top, bot = data
    args = dict(E.CASES_CORE)["se150"]
    before = sorted(os.listdir(d))
    assert "--qc-cov writes its tables beside those of --qc: it needs --qc PREFIX" in _fails(["--qc-cov"] + args, d)
    assert "--qc-topgc and --qc-botgc belong to --qc-cov" in _fails(["--qc", d + "/e1", "--qc-topgc", top, "--qc-botgc", bot] + args, d)
    assert "--qc-topgc and --qc-botgc must be given together" in _fails(["--qc", d + "/e2", "--qc-cov", "--qc-topgc", top] + args, d)
    assert "--qc-topgc and --qc-botgc must be given together" in _fails(["--qc", d + "/e2", "--qc-cov", "--qc-botgc", bot] + args, d)
    for world_args in (["--qc", d + "/e3", "--qc-cov"], ["--qc", d + "/e3", "--qc-co"]):
        err = _fails(world_args + args, d, env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "LOCAL_WORLD_SIZE": "2", "BSX_GATHER_ID": d + "/never"})
        assert "--qc-cov keeps the depth of the whole input on one device: it cannot run with WORLD_SIZE > 1" in err
    with open(d + "/bad.bed", "w") as f:
        f.write("nosuchcontig\t1\t2\n")
    assert "contig nosuchcontig is not in the index" in _fails(["--qc", d + "/e4", "--qc-cov", "--qc-topgc", d + "/bad.bed", "--qc-botgc", bot] + args, d)
    assert "cannot read" in _fails(["--qc", d + "/e5", "--qc-cov", "--qc-topgc", d + "/none.bed", "--qc-botgc", bot] + args, d)
    assert sorted(os.listdir(d)) == sorted(before + ["bad.bed"])      # nothing written, no rendezvous file opened


def test_an_input_without_reads_writes_tables_without_rows(data):
    """the declared deviation: no chunk reaches a backend, so no depth state is made and the files have their titles only"""
    d, refs, top, bot = data
    open(d + "/none.fq", "w").close()
    sam, files7, cov = CV.run_cov(CPU, ["--qc-topgc", top, "--qc-botgc", bot], ["-@", "1", "g", "none.fq"], d, d + "/none")
    assert all(l.startswith("@") for l in sam.split("\n") if l) and len(cov) == 13
    assert cov["_cv_table.txt"] == "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
    for i, name in enumerate(V.NAMES):
        assert cov["_covdist_%s_table.txt" % name] == "BISCUITqc Depth Distribution - %s\ndepth\tcount\n" % V.TITLES[i]
    sam, files7, cov = CV.run_cov(CPU, [], ["-@", "1", "g", "none.fq"], d, d + "/none4")
    assert len(cov) == 5
