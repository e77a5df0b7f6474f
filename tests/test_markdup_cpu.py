"""CPU: `--markdup` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the device seam, i.e.
the host table of markdup.c) on tests/markdup_cases.py: the SAM against tests/markdup_model.py's rewrite of the plain run's SAM, byte for byte,
the counts on stderr, the BISCUITqc duplicate table, a bsconv filter, and the refusal with several ranks.  The -m gpu counterpart
(tests/test_gpu_markdup.py) puts k_markdup.hip on the other side."""
import os
import subprocess
import time
import pytest
import e2e_cases as E
import bsconv_cases as B
import qc_cases as QC
import qc_model as Q
import markdup_cases as MC
import markdup_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("markdup"))
    contigs, origin = MC.make_data(d)
    return d, origin, Q.read_fasta(d + "/g.fa")


_RUNS = {}


def run(d, opts, args, env=None):
    """a command line of the CPU checker, run once per module -> (SAM, stderr)"""
    key = (d, tuple(opts), tuple(args), tuple(sorted((env or {}).items())))
    if key not in _RUNS:
        _RUNS[key] = B.run(CPU, list(opts) + list(args), d, env=env)
    return _RUNS[key]


@pytest.mark.parametrize("case", [c for c, _ in MC.CASES])
def test_sam_is_the_models_rewrite_of_the_plain_sam(data, case):
    d, origin, refs = data
    args = dict(MC.CASES)[case]
    plain, _ = run(d, [], args)
    got, err = run(d, ["--markdup"], args)
    dups = MC.check_against_model(plain, got, err, case)
    assert len(dups) >= 20, (case, len(dups))
    if case == "paired":      # what the issue requires of the data
        n, swapped_equal, swapped_placed = MC.by_kind(plain, dups, origin)
        print("markdup cases:", MC.stderr_counts(err), n, swapped_equal, swapped_placed)
        assert len(dups) >= 200 and n["dx"] >= 20 and n["dc"] >= 20 and n["du"] >= 20, (len(dups), n)
        assert swapped_equal == 0 and swapped_placed >= 20, (swapped_equal, swapped_placed)


def test_ordinals_run_on_over_chunks(data):
    d, origin, refs = data
    args, env = dict(MC.CASES)["paired"], {"BSX_CHUNK_SIZE": "40000"}      # x 4 threads: about 530 pairs a chunk
    plain, err0 = B.run(CPU, args, d, env=env)
    assert err0.count("[M::process] read ") >= 5
    got, err = B.run(CPU, ["--markdup"] + args, d, env=env)
    assert len(MC.check_against_model(plain, got, err, "chunks")) >= 200


def test_option_off_changes_nothing_and_on_changes_only_flags(data):
    d, origin, refs = data
    args = dict(MC.CASES)["paired"]
    plain, err = run(d, [], args)
    assert "markdup" not in err and not any(int(l.split("\t")[1]) & 0x400 for l in plain.split("\n") if l and l[0] != "@")
    got, _ = run(d, ["--markdup"], args)
    for a, b in zip(plain.split("\n"), got.split("\n")):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:1] + fa[2:] == fb[:1] + fb[2:], a[:200]


def test_qc_duplicate_table_counts_the_marked_records(data):
    d, origin, refs = data
    for case in ("paired", "single_end"):
        args = dict(MC.CASES)[case]
        sam, files = QC.run_qc(CPU, ["--markdup"], args, d, d + "/qc_" + case)
        only, _ = run(d, ["--markdup"], args)
        assert sam == only, case
        reads, paired = QC.reads_of(d, args)
        c = QC.check_files(files, sam, refs, reads, paired, case)
        assert c.all_dup >= 200 and 0 < c.q40_dup <= c.all_dup, (c.all_dup, c.q40_dup)
        assert ("Number of duplicate reads:\t%d\n" % c.all_dup) in files["_dup_report.txt"]


def test_with_a_bsconv_filter_the_flags_are_those_of_the_unfiltered_decision(data):
    d, origin, refs = data
    args = dict(MC.CASES)["paired"]
    full, _ = B.run(CPU, ["--markdup", "--bsconv"] + args, d)                   # annotated, nothing dropped
    kept, err = B.run(CPU, ["--markdup", "--bsconv-max-cph", "1"] + args, d)
    fl, kl = full.split("\n"), kept.split("\n")
    assert 0 < len(kl) < len(fl)
    it = iter(fl)
    assert all(any(k == f for f in it) for k in kl), "the filtered SAM is not the marked SAM with records left out"
    plain, _ = run(d, [], args)
    dups, _, n, n_keyed = M.process(plain)
    assert MC.stderr_counts(err) == (n, n_keyed, len(dups))
    # a template whose records were all dropped still holds its key: some marked template left in the output has no earlier equal template there
    _, ts = M.templates(plain)
    first = {}
    for i, recs in enumerate(ts):
        first.setdefault(M.template_key(recs), i)
    names_kept = {l.split("\t")[0] for l in kl if l and l[0] != "@"}
    orphans = [i for i in dups if ts[i][0][0] in names_kept and ts[first[M.template_key(ts[i])]][0][0] not in names_kept]
    assert len(orphans) >= 1, len(orphans)      # (copies share their original's retention, so most are dropped or kept together: one instance is what the clause needs)


def test_refused_with_several_ranks_before_connecting(data):
    d, origin, refs = data
    e = dict(os.environ, RANK="1", WORLD_SIZE="2", LOCAL_RANK="1", LOCAL_WORLD_SIZE="2", BSX_GATHER_ID=d + "/never", BSX_TUNE="gather_transport=socket")
    t0 = time.time()
    for opt in ("--markdup", "--markd"):      # (getopt_long takes unambiguous abbreviations)
        p = subprocess.run([CPU, opt] + dict(MC.CASES)["paired"], cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 1 and b"--markdup" in p.stderr and b"WORLD_SIZE" in p.stderr and p.stdout == b"", opt
    assert time.time() - t0 < 30 and not os.path.exists(d + "/never")      # (rank 1 alone would wait for rank 0 at the rendezvous)
