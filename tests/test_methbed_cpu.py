"""CPU: `--qc PREFIX --qc-meth --meth-bed FILE` through the command line over the CPU restatement of the kernels (oracle_align: the backend
without the device seam, i.e. the host statement of the rule in meth.c), on the cases of e2e_cases.CASES_CORE over meth_cases.make_data's reads:
the file against tests/methbed_model.py over the SAM written for every type, a coverage floor and merge mode; the SAM and every QC file against
the run without the option; the option errors; an input without reads.  The -m gpu counterpart (tests/test_gpu_methbed.py) puts k_msite on the
other side."""
import os
import subprocess
import pytest
import e2e_cases as E
import meth_cases as MC
import methbed_cases as MBC
import qc_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("methbed"))
    MC.make_data(d)
    return d, Q.read_fasta(d + "/g.fa")


def test_file_equals_the_model_sam_and_qc_files_are_unchanged(data):
    d, refs = data
    by_mode = {m: [] for m, _, _ in MBC.MODES}
    for case, args in E.CASES_CORE:
        plain, files0, table = MC.run_meth(CPU, [], args, d, d + "/p_" + case)
        files0[MC.M.SUFFIX] = table
        for mode, opts, model_args in MBC.MODES:
            prefix = d + "/b_%s_%s" % (case, mode)
            sam, files, bed = MBC.run_bed(CPU, opts, args, d, prefix)
            assert sam == plain and files == files0, (case, mode)
            base = os.path.basename(prefix)
            assert sorted(f for f in os.listdir(d) if f.startswith(base + "_") or f.startswith(base + ".")) == sorted([base + s for s in files] + [base + ".bed"])
            by_mode[mode] += MBC.check_bed(bed, sam, refs, case, **model_args)
    MBC.assert_not_vacuous(by_mode)


def test_with_a_header_the_contigs_follow_its_sq_lines(data):
    d, refs = data
    names = list(refs)
    assert len(names) >= 3
    hdr = d + "/hdr.txt"
    with open(hdr, "w") as f:                                                  # the last contig first, the first one without a line
        for n in [names[-1]] + names[1:-1]:
            f.write("@SQ\tSN:%s\tLN:%d\n" % (n, len(refs[n])))
    args = ["-@", "4", "-H", hdr, "g", "b1.fq"]
    sam, _, bed = MBC.run_bed(CPU, ["--meth-type", "c"], args, d, d + "/hd")
    MBC.check_bed(bed, sam, refs, "-H", typ="c", min_cov=1, merge=False)
    seen = []
    for l in bed.split("\n")[:-1]:
        if not seen or seen[-1] != l.split("\t")[0]:
            seen.append(l.split("\t")[0])
    assert seen == [n for n in [names[-1]] + names[1:-1] + [names[0]] if n in seen] and len(seen) >= 3, seen


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
    qc, bed = ["--qc", d + "/e1", "--qc-meth"], ["--meth-bed", d + "/e1.bed"]
    assert "--meth-bed lists the cytosines --qc-meth counts: it needs --qc PREFIX --qc-meth" in _fails(bed + args, d)
    assert "it needs --qc PREFIX --qc-meth" in _fails(["--qc", d + "/e1"] + bed + args, d)
    for lone in (["--meth-type", "c"], ["--meth-min-cov", "2"], ["--meth-merge"]):
        assert "--meth-type, --meth-min-cov and --meth-merge belong to --meth-bed FILE" in _fails(qc + lone + args, d)
    for k in ("0", "-1", "x", "2x", ""):
        assert "--meth-min-cov %s: an integer of at least 1" % k in _fails(qc + bed + ["--meth-min-cov", k] + args, d)
    assert "--meth-type cpg: cg, ch or c" in _fails(qc + bed + ["--meth-type", "cpg"] + args, d)
    for t in ("ch", "c"):
        assert "--meth-merge joins the two cytosines of a CpG: it needs --meth-type cg" in _fails(qc + bed + ["--meth-merge", "--meth-type", t] + args, d)
    err = _fails(qc + bed + args, d, env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "LOCAL_WORLD_SIZE": "2", "BSX_GATHER_ID": d + "/never"})
    assert "it cannot run with WORLD_SIZE > 1" in err
    assert sorted(os.listdir(d)) == before                                    # nothing written


def test_an_input_without_reads_gives_an_empty_file(data):
    d, refs = data
    open(d + "/none.fq", "w").close()
    for opts in ([], ["--meth-merge"]):
        sam, files, bed = MBC.run_bed(CPU, opts, ["-@", "1", "g", "none.fq"], d, d + "/none")
        assert all(l.startswith("@") for l in sam.split("\n") if l) and bed == ""
