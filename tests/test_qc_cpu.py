"""CPU: `--qc PREFIX` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the device seam,
i.e. the host walk of qc.c), on the cases tests/test_bsconv_cpu.py uses: the files against tests/qc_model.py over the SAM written, the SAM
against the run without the option.  The -m gpu counterpart (tests/test_gpu_qc.py) puts k_qc on the other side."""
import os
import subprocess
import pytest
import e2e_cases as E
import bsconv_cases as B
import qc_cases as QC
import qc_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("qc"))
    B.make_data(d)
    return d, Q.read_fasta(d + "/g.fa")


def test_files_equal_the_model_and_sam_is_unchanged(data):
    d, refs = data
    counters = []
    for case, args in E.CASES_CORE:
        plain, _ = B.run(CPU, args, d)
        sam, files = QC.run_qc(CPU, [], args, d, d + "/cpu_" + case)
        assert sam == plain, case
        reads, paired = QC.reads_of(d, args)
        assert ("_isize_table.txt" in files) == paired
        counters.append(QC.check_files(files, sam, refs, reads, paired, case))
    QC.assert_not_vacuous(counters)


def test_with_a_bsconv_filter_only_the_kept_records_count(data):
    d, refs = data
    args = dict(E.CASES_CORE)["pe150_b0"]
    sam, files = QC.run_qc(CPU, ["--bsconv-max-cph", "3"], args, d, d + "/cpu_flt")
    plain, files0 = QC.run_qc(CPU, [], args, d, d + "/cpu_noflt")
    assert sam.count("\n") < plain.count("\n")
    reads, paired = QC.reads_of(d, args)
    c = QC.check_files(files, sam, refs, reads, paired, "filtered")
    assert c.all_tot == sum(1 for l in sam.split("\n") if l and l[0] != "@") and files["_dup_report.txt"] != files0["_dup_report.txt"]


def test_plain_run_writes_no_files_and_unknown_prefix_directory_fails(data):
    d, refs = data
    before = sorted(os.listdir(d))
    B.run(CPU, dict(E.CASES_CORE)["se150"], d)
    assert sorted(os.listdir(d)) == before
    p = subprocess.run([CPU, "--qc", d + "/no/such/dir/x"] + dict(E.CASES_CORE)["se150"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"cannot write" in p.stderr


def test_two_processes_write_the_one_process_files(data):
    """the ranks path: every rank's counters added up, rank 0 writes"""
    d, refs = data
    args = ["-@", "1", "g", "b1.fq", "b2.fq"]
    env = {"BSX_CHUNK_SIZE": "20000"}
    one, files1 = QC.run_qc(CPU, [], args, d, d + "/one", env=env)
    base = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID", "BSX_TUNE"):
        base.pop(k, None)
    procs = []
    for r in range(2):
        e = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=d + "/rdvq", BSX_TUNE="gather_transport=socket")
        procs.append(subprocess.Popen([CPU, "--qc", d + "/two"] + args, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = [p.communicate(timeout=900) for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][1].decode()[-3000:])
    assert E.strip_pg(outs[0][0]).decode() == one and outs[1][0] == b""
    assert QC.read_files(d + "/two") == files1 and len(files1) == 7
