"""Shared by tests/test_methbed_cpu.py (CPU suite) and tests/test_gpu_methbed.py (-m gpu): the command lines run with --qc PREFIX --qc-meth
--meth-bed FILE over meth_cases.make_data's reads, the comparison of the file written with tests/methbed_model.py over the SAM, and the check
that the inputs exercise what the rule distinguishes."""
import os
import bsconv_cases as B
import meth_model as M
import methbed_model as MB
import qc_cases as QC
import qc_model as Q

# name -> (options, the model's arguments)
MODES = [("cg", [], dict(typ="cg", min_cov=1, merge=False)),
         ("ch", ["--meth-type", "ch"], dict(typ="ch", min_cov=1, merge=False)),
         ("c", ["--meth-type", "c"], dict(typ="c", min_cov=1, merge=False)),
         ("k3", ["--meth-min-cov", "3"], dict(typ="cg", min_cov=3, merge=False)),
         ("merge", ["--meth-merge"], dict(typ="cg", min_cov=1, merge=True))]


def run_bed(exe, opts, args, d, prefix, env=None):
    """the command line with --qc PREFIX --qc-meth --meth-bed PREFIX.bed -> (SAM without @PG, the files of --qc and --qc-meth, the BED text)"""
    for s in [M.SUFFIX, ".bed"] + Q.SUFFIXES:
        if os.path.exists(prefix + s):
            os.remove(prefix + s)
    sam, err = B.run(exe, ["--qc", prefix, "--qc-meth", "--meth-bed", prefix + ".bed"] + opts + args, d, env=env)
    files = QC.read_files(prefix)
    files[M.SUFFIX] = open(prefix + M.SUFFIX).read()
    return sam, files, open(prefix + ".bed").read()


def check_bed(got, sam, refs, what, **model_args):
    """the file written must be the model's over `sam`, byte for byte -> what the model's lines are made of"""
    want, made_of, seen = MB.process(sam, refs, **model_args)
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("%s %s: %d lines against the model's %d; line %d: got %r, want %r" % (what, model_args, len(g), len(w), k, g[k:k + 1], w[k:k + 1]))
    return made_of


def assert_not_vacuous(by_mode):
    """by_mode: mode name -> what the lines of all its runs are made of.  Every type yields lines of each of its classes; the coverage filter
    drops some; merge mode yields joined lines, C-only lines and G-only lines"""
    classes = {m: {w[4] for w in by_mode[m]} for m in by_mode}
    assert classes["cg"] == {"CG"} and classes["ch"] == {"CHG", "CHH"} and classes["c"] >= {"CG", "CHG", "CHH"}, classes
    assert any(w[2] for w in by_mode["cg"]) and any(w[3] for w in by_mode["cg"])                      # Cs and Gs
    assert 0 < len(by_mode["k3"]) < len(by_mode["cg"])
    kinds = {(w[2], w[3]) for w in by_mode["merge"]}
    assert kinds == {(True, True), (True, False), (False, True)}, kinds
    assert len(by_mode["merge"]) < len(by_mode["cg"])
