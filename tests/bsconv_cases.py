"""Shared by tests/test_bsconv_cpu.py (CPU suite) and tests/test_gpu_bsconv.py (-m gpu): a data set whose genome has N runs, a contig
that ends in a C and one that starts with a G, reads placed at those spots, the command lines of tests/e2e_cases.py with the --bsconv
options, and the comparison with tests/bsconv_model.py."""
import re
import subprocess
import os
import numpy as np
import simdata
import e2e_cases as E
import bsconv_model as M

FILTERS = [
    (["--bsconv-max-cph", "1"], dict(max_cph=1)),
    (["--bsconv-max-cph-frac", "0.02", "--bsconv-filter-u"], dict(max_cph_frac=0.02, filter_u=True)),
    (["--bsconv-max-cpy", "0", "--bsconv-max-cpa", "1", "--bsconv-max-cpc", "3", "--bsconv-max-cpt", "2", "--bsconv-max-cpy-frac", "0.5"],
     dict(max_cpy=0, max_cpa=1, max_cpc=3, max_cpt=2, max_cpy_frac=0.5)),
]


def make_genome(genome_bp, seed, n_contigs=3):
    contigs = simdata.make_genome(genome_bp, seed=seed, n_contigs=n_contigs)      # (one long N run already)
    r = np.random.default_rng(seed + 100)
    for _, g in contigs:
        for _ in range(6):                                                        # short N runs, reads span them
            at = int(r.integers(1000, len(g) - 1000))
            g[at:at + int(r.integers(1, 25))] = 4
        g[-1] = 1                                                                 # ends in a C ...
        g[-3:-1] = (1, 2)                                                         # ... after a CpG
        g[0] = 2                                                                  # starts with a G
        g[1:4] = (2, 1, 1)
    return contigs


def edge_pairs(contigs, read_len, seed):
    """pairs whose first read starts at the first base of a contig, or whose fragment ends at its last, or sits right before / after an N run"""
    r = np.random.default_rng(seed)
    out = []
    for ci, (_, g) in enumerate(contigs):
        spots = [0, len(g) - 400]
        isn = np.flatnonzero(g == 4)
        for s in isn[np.flatnonzero(np.diff(np.concatenate([[-10], isn])) > 1)][:8]:      # first base of every N run
            spots += [max(0, int(s) - 400), max(0, int(s) - read_len - 2), min(len(g) - 400, int(s) - 30)]
        for e in isn[np.flatnonzero(np.diff(np.concatenate([isn, [10 ** 9]])) > 1)][:8]:   # last base of every N run
            spots += [min(len(g) - 400, int(e) + 1), min(len(g) - 400, int(e) + 2)]
        for s in spots:
            for flip in (0, 1):
                f = g[s:s + 400].copy()
                if flip:
                    f = simdata.revcomp(f)
                conv = simdata.bisulfite(f, r, other_ret=0.05)
                out.append(("e%d_%d_%d" % (ci, len(out), flip), conv[:read_len].copy(), simdata.revcomp(conv)[:read_len].copy()))
    return out


def make_data(d, genome_bp=150000, n_pairs=300, n_long=24, seed=31):
    from biscuit_amd.api import Index
    contigs = make_genome(genome_bp, seed)
    simdata.write_genome(d + "/g.fa", contigs)
    Index.build(d + "/g.fa", d + "/g").close()
    ps = simdata.make_pairs(contigs, n_pairs, 150, seed + 1, sub=0.01, indel=0.006, pbat_frac=0.3, chimera_frac=0.06, bad_mate_frac=0.06, n_frac=0.03)
    ps += edge_pairs(contigs, 150, seed + 2)
    simdata.write_fastq(d + "/b1.fq", [(n, a) for n, a, b in ps])
    simdata.write_fastq(d + "/b2.fq", [(n, b) for n, a, b in ps])
    simdata.write_fastq(d + "/long.fq", simdata.make_single(contigs, n_long, 1000, seed + 6))
    return contigs


def run(exe, args, cwd, env=None, timeout=1800):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)
    assert p.returncode == 0, (args, p.stderr.decode()[-3000:])
    return E.strip_pg(p.stdout).decode(), p.stderr.decode()


def stderr_counts(err):
    """([M::bsconv] processed N, M remain) and the eight totals"""
    m = re.search(r"\[M::bsconv\] processed (\d+), (\d+) remain", err)
    t = re.search(r"\[M::bsconv\] CpA_R (\d+) CpA_C (\d+) CpC_R (\d+) CpC_C (\d+) CpG_R (\d+) CpG_C (\d+) CpT_R (\d+) CpT_C (\d+)", err)
    assert m and t, err[-2000:]
    return int(m.group(1)), int(m.group(2)), [int(x) for x in t.groups()]


def check_against_model(plain, got, err, refs, conf, what):
    """`got` (the product's SAM under the options conf stands for) must be the model applied to `plain` (its SAM without them)"""
    want, tot, n, nf = M.process(plain, refs, conf)
    E.assert_same_sam(got.encode(), want.encode(), what)
    assert stderr_counts(err) == (n, n - nf, tot), (what, stderr_counts(err), (n, n - nf, tot))
    return tot, n, nf
