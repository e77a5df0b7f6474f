"""CPU: `--qc PREFIX --qc-meth` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the device
seam, i.e. the host statement of the rule in meth.c), on the cases of e2e_cases.CASES_CORE over meth_cases.make_data's reads (varying qualities,
planted uncallable cytosines): PREFIX_totalBaseConversionRate.txt against tests/meth_model.py over the SAM written, the SAM and the seven files of
--qc against the runs without the option; with a --bsconv filter and with --markdup; the option errors.  The -m gpu counterpart
(tests/test_gpu_meth.py) puts k_meth on the other side."""
import os
import subprocess
import pytest
import e2e_cases as E
import bsconv_cases as B
import meth_cases as MC
import meth_model as M
import qc_cases as QC
import qc_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("meth"))
    MC.make_data(d)
    return d, Q.read_fasta(d + "/g.fa")


def test_file_equals_the_model_sam_and_qc_files_are_unchanged(data):
    d, refs = data
    seen = []
    for case, args in E.CASES_CORE:
        plain, _ = B.run(CPU, args, d)
        qsam, qfiles = QC.run_qc(CPU, [], args, d, d + "/q_" + case)
        assert sorted(os.path.basename(f) for f in os.listdir(d) if f.startswith("q_" + case + "_")) == sorted("q_" + case + s for s in qfiles)      # --qc alone: its own files only
        sam, files7, got = MC.run_meth(CPU, [], args, d, d + "/m_" + case)
        assert sam == plain == qsam and files7 == qfiles, case
        assert sorted(f for f in os.listdir(d) if f.startswith("m_" + case + "_")) == sorted("m_" + case + s for s in list(qfiles) + [M.SUFFIX])
        seen.append(MC.check_file(got, sam, refs, case))
    MC.assert_not_vacuous(seen, record_filters=("unmapped", "secondary", "mapq", "improper", "as"))


def test_with_a_bsconv_filter_only_the_kept_records_count(data):
    d, refs = data
    args = dict(E.CASES_CORE)["pe150_b0"]
    sam, _, got = MC.run_meth(CPU, ["--bsconv-max-cph", "3"], args, d, d + "/flt")
    plain, _, got0 = MC.run_meth(CPU, [], args, d, d + "/noflt")
    assert sam.count("\n") < plain.count("\n") and got != got0
    MC.check_file(got, sam, refs, "filtered")


def test_with_markdup_the_duplicates_do_not_count(data):
    d, refs = data
    args = ["-@", "4", "g", "d1.fq", "d2.fq"]                                  # meth_cases.write_dup_set: duplicates by position whose columns differ
    sam, _, got = MC.run_meth(CPU, ["--markdup"], args, d, d + "/md")
    only, _ = B.run(CPU, ["--markdup"] + args, d)
    nodup, _, got0 = MC.run_meth(CPU, [], args, d, d + "/nomd")
    assert sam == only and got != got0
    K, S, unc, seen = MC.check_file(got, sam, refs, "markdup")
    assert seen["dup"] > 0 and seen["counted"] > 0
    MC.check_file(got0, nodup, refs, "the same reads without --markdup")


def test_with_qc_cov_both_sets_of_files_are_written(data):
    d, refs = data
    args = dict(E.CASES_CORE)["se150"]
    sam, _, got = MC.run_meth(CPU, ["--qc-cov"], args, d, d + "/both")
    MC.check_file(got, sam, refs, "with --qc-cov")
    assert os.path.exists(d + "/both_cv_table.txt") and os.path.exists(d + "/both_covdist_all_base_table.txt")


def _fails(args, d, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([CPU] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
    assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stderr.decode()[-1000:])
    return p.stderr.decode()


def test_option_errors(data):
    d, refs = data
    args = dict(E.CASES_CORE)["se150"]
    before = sorted(os.listdir(d))
    assert "--qc-meth writes its table beside those of --qc: it needs --qc PREFIX" in _fails(["--qc-meth"] + args, d)
    for world_args in (["--qc", d + "/e3", "--qc-meth"], ["--qc", d + "/e3", "--qc-m"], ["--qc", d + "/e3", "--qc-met"]):
        err = _fails(world_args + args, d, env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "LOCAL_WORLD_SIZE": "2", "BSX_GATHER_ID": d + "/never"})
        assert "--qc-meth keeps the counts of every cytosine of the whole input on one device: it cannot run with WORLD_SIZE > 1" in err
    assert sorted(os.listdir(d)) == before                                    # nothing written, no rendezvous file opened


def test_the_abbreviation_is_taken(data):
    d, refs = data
    args = dict(E.CASES_CORE)["se150"]
    sam, _ = B.run(CPU, ["--qc", d + "/abbr", "--qc-m"] + args, d)
    MC.check_file(open(d + "/abbr" + M.SUFFIX).read(), sam, refs, "--qc-m")


def test_an_input_without_reads_gives_minus_one_four_times(data):
    d, refs = data
    open(d + "/none.fq", "w").close()
    sam, files7, got = MC.run_meth(CPU, [], ["-@", "1", "g", "none.fq"], d, d + "/none")
    assert all(l.startswith("@") for l in sam.split("\n") if l)
    assert got == M.TITLE + "CA\tCC\tCG\tCT\n-1\t-1\t-1\t-1\n"
