"""Cases and fast references that take the table passes of k_cov.hip and k_meth.hip past one trip per workgroup, shared by
tests/test_tables_scale_cpu.py and tests/test_gpu_tables_scale.py.  Everything is numpy and a function of n_cu (the device's compute units,
Device.n_cu) and T (_lib.COV_TILE), because every threshold of those passes is a multiple of n_cu:

  k_cov_scan                      1024 tiles a step, `run` carried between steps
  k_cov_walk<true>                grid 4 n_cu: the LDS histograms kept over the tiles t, t + 4 n_cu, t + 8 n_cu of a workgroup
  k_cov_sums, k_cov_walk<false>   grid 8 n_cu (`vmax` kept over tiles)
  k_meth_walk                     grid 8 n_cu (K[] / S[] kept in registers, flushed on `since` or on the last trip)
  k_cov_paint                     grid 8 n_cu, a workgroup per interval
  k_cov_add                       a sweep of 8 n_cu x 256 jobs
  k_meth_add                      a sweep of 8 n_cu x 4 jobs

The genome has 8 n_cu + 5 tiles, the last one partial: L = (8 n_cu + 4) T + 33.  The boundaries that matter are g T for g in G = {4 n_cu,
8 n_cu} (the first tile of a workgroup's second trip under either grid) and {1024, 2048} where those are below the tile count (the steps of
k_cov_scan); at 256 compute units the two sets are the same.  What tests/test_gpu_cov.py's genome plants around T is planted at each of them.
A CpG whose C ends tile g - 1 and a contig junction C | G at the same place exclude one another, so the three things sit on three
consecutive tile boundaries, all of them inside the later trips and the later scan step:

  g T          a CpG whose C is the last base of tile g - 1
  (g + 1) T    a contig ends here with C | G across the junction: no CpG, and a CN context for both bases
  (g + 2) T    an N run of 20 across the boundary, C before it and G after it
  tile g + 3   C N G triplets
  tiles b and b + 8 n_cu for b in 0..4: C N G triplets, so that both hold CN sites; the last tile, b = 4, has 33 bases and begins
               C A C C C G C T C N G: a cytosine of every context

and a CpG on the genome's first two and last two bases.

The job counts scale with the sweeps they have to pass: n_cov_bulk(n_cu) one-run coverage jobs (606 208 at 256 compute units, 524 288 being
one sweep of k_cov_add) and n_meth(n_cu) conversion records (10 240 at 256; 8192 being one sweep of k_meth_add).

The references are exact integers.  Coverage: np.add.at over the event arrays, cumsum, minimum for the CpGs, bincount per table and mask.
Conversion: the column rule of include/bsx.h over flat arrays of columns (tests/test_gpu_meth.py's _walk is the same rule column by column;
the CPU test compares the two), and tests/meth_model.py's context, callable_site and milli applied only at positions whose counters are not
zero.  The fault models at the end recompute an expectation as a pass that forgot its later trips would: the CPU test asserts that each of
them changes a table, so that a pass on the device cannot be vacuous."""
import numpy as np
import meth_model as M

SCAN_STEP = 1024           # tiles a step of k_cov_scan
LDS_BINS_MAX = 512         # COV_LDS_BINS_MAX
TRIPLET_AT, N_TRIPLETS = 1000, 8


def n_cov_bulk(n_cu):
    return 8 * n_cu * 256 + 8 * n_cu * 40


def n_meth(n_cu):
    return max(8 * n_cu * 5, 640)


def cov_sweep(n_cu):
    return 8 * n_cu * 256


def meth_sweep(n_cu):
    return 8 * n_cu * 4


class Cases:
    pass


# ------------------------------------------------------------------------------------------ the genome
def _genome(c, r):
    n_cu, T = c.n_cu, c.T
    c.n_tiles = 8 * n_cu + 5
    c.L = L = (8 * n_cu + 4) * T + 33
    c.G = sorted(set([4 * n_cu, 8 * n_cu] + [s for s in (SCAN_STEP, 2 * SCAN_STEP) if s < c.n_tiles]))
    g = r.integers(0, 4, L).astype(np.uint8)
    g[0], g[1] = 1, 2
    g[L - 2], g[L - 1] = 1, 2
    c.special = list(range(5)) + [8 * n_cu + b for b in range(5)]              # tiles b and b + 8 n_cu: one workgroup of a grid of 8 n_cu
    c.cpg_at, c.junctions, c.n_runs, c.triplet_tiles = [], [], [], sorted(set([x + 3 for x in c.G] + c.special[:-1]))
    c.last_tile = (c.n_tiles - 1) * T                                           # 33 bases: CA, CC, CC, CG, CT and CN by design
    g[c.last_tile:c.last_tile + 11] = (1, 0, 1, 1, 1, 2, 1, 3, 1, 4, 2)
    for x in c.G:
        p = x * T
        g[p - 1], g[p] = 1, 2
        c.cpg_at.append(p - 1)
        p = (x + 1) * T
        g[p - 1], g[p] = 1, 2
        c.junctions.append(p)
        p = (x + 2) * T
        g[p - 10:p + 10] = 4
        g[p - 11], g[p + 10] = 1, 2
        c.n_runs.append(p)
    for t in c.triplet_tiles:
        for k in range(N_TRIPLETS):
            p = t * T + TRIPLET_AT + 37 * k
            g[p:p + 3] = (1, 4, 2)
    c.g = g
    cuts = [0] + c.junctions + [L]
    c.contigs = [("s%d" % i, g[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    c.ctg_off = np.array(cuts, np.int64)
    c.boundaries = sorted(set([x * T for x in c.G] + c.junctions + c.n_runs))


# ------------------------------------------------------------------------------------------ coverage jobs and masks
def _designed_cov(T, L, at):
    """tests/test_gpu_cov.py's _designed, its tile boundary moved to `at`"""
    return [(at - 10, [(11, "M")], True), (at + 60, [(5, "S"), (10, "M"), (2, "I"), (3, "M"), (4, "D"), (6, "M"), (3, "H")], True),
            (at - 1, [(1, "M")], False), (at - 1, [(1, "M")], True), (at, [(1, "M")], False), (at - 40, [(90, "M")], True),
            (at + 90, [(130, "M"), (1, "D"), (7, "M")], False)]


def _cov(c, r):
    n_cu, T, L = c.n_cu, c.T, c.L
    n = n_cov_bulk(n_cu)
    ln = r.integers(1, 151, n)
    c.bulk_len = ln.astype(np.int64)
    c.bulk_fpos = (r.random(n) * (L - ln + 1)).astype(np.int64)
    c.bulk_q40 = (np.arange(n) & 1) == 0
    c.pile_a, c.pile_b = (4 * n_cu + 1) * T + 100, (8 * n_cu + 1) * T + 100      # a second-trip tile of either grid
    c.pile_a_n, c.pile_b_n = LDS_BINS_MAX + 88, LDS_BINS_MAX + 188
    jobs = [(T + 5, [(L - 7 - (T + 5), "M")], True)]                             # from tile 1 into the last tile
    jobs += [(0, [(50, "M")], True), (L - 30, [(30, "M")], False), (0, [(1, "M")], False), (L - 1, [(1, "M")], True)]
    for at in c.boundaries:
        jobs += _designed_cov(T, L, at)
    jobs += [(c.pile_a, [(100, "M")], k < 200) for k in range(c.pile_a_n)]
    jobs += [(c.pile_b, [(100, "M")], k < 300) for k in range(c.pile_b_n)]
    c.cov_designed = jobs
    # the masks: 100-base windows, more than 8 n_cu of them each
    masks = []
    for w in range(2):
        n_iv = 8 * n_cu + 40
        s = np.sort((r.random(n_iv) * (L - 100)).astype(np.int64))
        iv = [(int(x), int(x) + 100) for x in s]
        for k in range(0, 8 * n_cu, 16):                                        # pairs that abut inside one 32-bit word
            a = max(iv[k][0], 128) | 7
            iv[k], iv[k + 1] = (a - 100, a), (a, a + 100)
        # the later ones: longer than three tiles, over both piles, inside the last tile and up to the genome's end, at every boundary
        tail = [((4 * n_cu + 2) * T + 17 + 64 * w, (4 * n_cu + 5) * T + 50 + 64 * w), (c.pile_a - 30 + 50 * w, c.pile_a + 70 + 50 * w),
                (c.pile_b - 30 + 50 * w, c.pile_b + 70 + 50 * w), (c.last_tile + 3 + w, c.last_tile + 9 + w), (L - 20 - 25 * w, L)]
        tail += [(at - 3 + 2 * w, at + 2 + w) for at in c.boundaries]
        iv[len(iv) - len(tail):] = tail
        masks.append(iv)
    c.top, c.bot = masks
    assert all(0 <= b <= e <= L for m in masks for b, e in m) and all(any(e == L for b, e in m) for m in masks)


def cov_job_list(c, lo=0, hi=None):
    """every coverage job in tests/test_gpu_cov.py's list form, in the order of cov_arrays (the bulk first)"""
    bulk = [(int(f), [(int(n), "M")], bool(q)) for f, n, q in zip(c.bulk_fpos, c.bulk_len, c.bulk_q40)]
    return (bulk + c.cov_designed)[lo:hi]


def cov_arrays(c):
    """-> (_lib.QcJob array, pool): the bulk jobs (one CIGAR word each), then the designed ones"""
    from biscuit_amd import _lib as L_
    flags = L_.QC_COV | L_.QC_STRAND
    n = len(c.bulk_fpos)
    pool = [(c.bulk_len.astype(np.uint32) << np.uint32(4))]
    a = np.zeros(n + len(c.cov_designed), dtype=np.dtype(L_.QcJob))
    a["fpos"][:n], a["cig_off"][:n], a["n_cigar"][:n] = c.bulk_fpos, np.arange(n), 1
    a["flags"][:n] = np.where(c.bulk_q40, flags | L_.QC_COV_Q40, flags)
    at, words = n, []
    for k, (fpos, ops, q40) in enumerate(c.cov_designed):
        a[n + k] = (fpos, 0, 0, 0, at, len(ops), flags | (L_.QC_COV_Q40 if q40 else 0))
        words += [m << 4 | "MIDSH".index(op) for m, op in ops]
        at += len(ops)
    pool.append(np.array(words, np.uint32))
    return a, np.concatenate(pool)


def cov_events(c, n_jobs=None, again=()):
    """(start, end, q40) of every run of M columns of the first n_jobs jobs (all of them by default), then of the jobs `again` (list form)"""
    nb = len(c.bulk_fpos)
    k = nb if n_jobs is None else min(nb, n_jobs)
    s, e, q = [c.bulk_fpos[:k]], [c.bulk_fpos[:k] + c.bulk_len[:k]], [c.bulk_q40[:k]]
    ds, de, dq = [], [], []
    for fpos, ops, q40 in c.cov_designed[:None if n_jobs is None else max(0, n_jobs - nb)] + list(again):
        y = fpos
        for m, op in ops:
            if op == "M":
                ds.append(y), de.append(y + m), dq.append(q40)
            if op in "MD":
                y += m
    return (np.concatenate(s + [np.array(ds, np.int64)]), np.concatenate(e + [np.array(de, np.int64)]), np.concatenate(q + [np.array(dq, bool)]))


def cov_depth(c, n_jobs=None, again=()):
    """-> int32[L, 2]: the depth of every position, all records and q40 records"""
    s, e, q = cov_events(c, n_jobs, again)
    diff = np.zeros((c.L + 1, 2), np.int32)
    np.add.at(diff[:, 0], s, 1)
    np.add.at(diff[:, 0], e, -1)
    np.add.at(diff[:, 1], s[q], 1)
    np.add.at(diff[:, 1], e[q], -1)
    return np.cumsum(diff, axis=0, dtype=np.int32)[:c.L]


def paint(L, intervals):
    m = np.zeros(L, bool)
    for b, e in intervals:
        m[b:e] = True
    return m


def cpg_sites(c):
    """bool[L]: a C followed by a G of the same contig, neither under an N"""
    g = c.g
    cpg = np.zeros(c.L, bool)
    cpg[:-1] = (g[:-1] == 1) & (g[1:] == 2)
    cpg[c.ctg_off[1:-1] - 1] = False
    return cpg


def cov_tables(c, dep, top=None, bot=None, counted=None, nb=None):
    """the four or twelve tables in the order of _lib.CovTables.  counted: bool[L], the positions (and the CpGs by their C) a pass counts, all
    by default; nb: the bins the pass was given, the largest `all` depth + 1 by default -- what is deeper is dropped, as is a negative depth"""
    L = c.L
    nb = int(dep[:, 0].max()) + 1 if nb is None else nb
    cpg = cpg_sites(c)[:-1]
    cdep = np.minimum(dep[:-1], dep[1:])
    regions = [np.ones(L, bool)] + ([] if top is None else [paint(L, top), paint(L, bot)])
    if counted is None:
        counted = np.ones(L, bool)
    out = []
    for m in regions:
        m2 = m.copy()
        m2[:-1] |= m[1:]
        for cls in range(2):
            for d in (dep[m & counted, cls], cdep[(cpg & m2[:-1] & counted[:-1]), cls]):
                d = d[(d >= 0) & (d < nb)]
                out.append(np.bincount(d, minlength=nb).astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------ conversion records
def _record(r, g, fpos, ops, p_other=0.03, **kw):
    """tests/test_gpu_meth.py's _make, a run of columns at a time"""
    from test_gpu_meth import Job
    seq, y = [], fpos
    for n, op in ops:
        if op == "M":
            b = g[y:y + n].copy()
            other = (b == 4) | (r.random(n) < p_other)
            b[other] = r.integers(0, 4, int(other.sum()))
            half = r.random(n) < 0.5
            b[(b == 1) & half & ~other] = 3
            b[(b == 2) & half & ~other] = 0
            seq.append(b)
            y += n
        elif op == "D":
            y += n
        else:
            seq.append(r.integers(0, 4, n).astype(np.uint8))
    return Job(fpos, ops, np.concatenate(seq), **kw)


def _meth(c, r):
    n_cu, T, L, g = c.n_cu, c.T, c.L, c.g
    total = n_meth(n_cu)
    M60 = [(60, "M")]
    fixed = [_record(r, g, L - 57, [(57, "M"), (3, "S")], p_other=0.0, tag=0)]   # the last tile's cytosines, up to the genome's last base
    where = []                                                                  # the first base of a record's window of at most 80 columns
    for t in c.special[:-1]:
        # forward-strand records over four of the tile's triplets, reverse-strand records over the other four: a CN site at a C and at a G
        fixed += [_record(r, g, t * T + TRIPLET_AT - 5 + 74 * i, M60, p_other=0.0, tag=i >> 1) for i in range(4)]
        where += [int(x) for x in r.integers(t * T, (t + 1) * T - 80, 40)]      # anywhere in the tile
    for at in c.boundaries:
        where += [at - 30, at - 30, at - 12, at - 5, at + 1, at - 55]
    where += [0, 0]
    assert len(where) + len(fixed) < total
    where += [int(x) for x in r.integers(0, L - 80, total - len(fixed) - len(where))]
    jobs = []
    for k in range(len(where)):
        at = where[k]
        n1, n2 = int(r.integers(15, 31)), int(r.integers(25, 31))               # 40 to 60 columns
        mid = [(int(r.integers(1, 4)), "ID"[k >> 1 & 1])] if k % 7 else []
        ops = [(int(r.integers(0, 6)), "SH"[k & 1]), (n1, "M")] + mid + [(n2, "M"), (int(r.integers(0, 6)), "HS"[k & 1])]
        ops = [(n, op) for n, op in ops if n]
        span = sum(n for n, op in ops if op in "MD")
        fpos = min(at, L - span)
        rlen = sum(n for n, op in ops if op in "MISH")
        read2 = k % 3 == 0
        ov = (fpos + int(r.integers(0, span)), fpos + int(r.integers(0, span + 40))) if read2 else (0, 0)
        jobs.append(_record(r, g, fpos, ops, rev=bool(k & 4), read2=read2, tag=(0, 1, 3, 2)[k % 4] if k % 5 else 3,
                            lowq=[int(x) for x in r.integers(0, rlen, int(r.integers(0, 6)))], ov=ov))
    jobs += fixed
    c.meth_jobs = [jobs[i] for i in r.permutation(len(jobs))]                   # the designed places all over the batch, not at its head


def meth_counters(c, jobs):
    """the rule of include/bsx.h (bsx_meth_job_t) over every column at once -> (positions with a counter that is not zero, sorted;
    int64[n, 4] their ret, conv, opp_ref, opp_alt)"""
    g = c.g
    jid, qs, fs, seqs, lows, off = [], [], [], [], [], [0]
    for i, J in enumerate(jobs):
        x, y = 0, J.fpos
        for n, op in J.ops:
            if op == "M":
                qs.append(np.arange(x, x + n)), fs.append(np.arange(y, y + n)), jid.append(np.full(n, i))
                x += n
                y += n
            elif op == "D":
                y += n
            else:
                x += n
        low = np.zeros(len(J.seq), bool)
        low[np.array(sorted(J.lowq), np.int64)] = True
        seqs.append(J.seq), lows.append(low), off.append(off[-1] + len(J.seq))
    jid, q, f, off = np.concatenate(jid), np.concatenate(qs), np.concatenate(fs), np.array(off, np.int64)
    seq, low = np.concatenate(seqs)[off[jid] + q], np.concatenate(lows)[off[jid] + q]
    rlen = np.diff(off)[jid]
    tag = np.array([J.tag for J in jobs])
    gb = g[f]
    n_c2t = np.bincount(jid[~low & (gb == 1) & (seq == 3)], minlength=len(jobs))
    n_g2a = np.bincount(jid[~low & (gb == 2) & (seq == 0)], minlength=len(jobs))
    strand = np.where(tag <= 1, tag, np.where(n_c2t >= n_g2a, 0, 1))[jid]
    read2 = np.array([J.read2 for J in jobs])[jid]
    ov0, ov1 = np.array([J.ov[0] for J in jobs])[jid], np.array([J.ov[1] for J in jobs])[jid]
    keep = ~low & (q + 1 > 3) & (rlen >= q + 1 + 3) & ((gb == 1) | (gb == 2)) & ~(read2 & (ov0 <= f) & (f < ov1))
    own = gb == np.where(strand == 1, 2, 1)
    ref, alt = seq == gb, seq == np.where(gb == 1, 3, 0)
    col = np.where(ref, np.where(own, 0, 2), np.where(own, 1, 3))
    sel = keep & (ref | alt)
    pos, inv = np.unique(f[sel], return_inverse=True)
    val = np.zeros((len(pos), 4), np.int64)
    np.add.at(val, (inv.reshape(-1), col[sel]), 1)
    return pos, val


def dense(pos, val, lo, hi):
    """the counters of [lo, hi) as int64[hi - lo, 4]"""
    out = np.zeros((hi - lo, 4), np.int64)
    a, b = np.searchsorted(pos, [lo, hi])
    out[pos[a:b] - lo] = val[a:b]
    return out


def meth_sites(c, pos, val):
    """the reported sites among pos -> (their positions, contexts, thousandths), uncallable sites: meth_model's context, callable_site, milli"""
    refs = [(int(o), np.array(list("ACGTN"), "S1")[s].tobytes().decode()) for o, (_, s) in zip(c.ctg_off, c.contigs)]
    which = np.searchsorted(c.ctg_off, pos, side="right") - 1
    at, ctx, mil, unc = [], [], [], 0
    for p, w, v in zip(pos.tolist(), which.tolist(), val.tolist()):
        o, s = refs[w]
        if s[p - o] not in "CG" or v[0] + v[1] == 0:
            continue
        if not M.callable_site(*v):
            unc += 1
            continue
        at.append(p), ctx.append(M.context(s, p - o)), mil.append(M.milli(v[0], v[0] + v[1]))
    return np.array(at, np.int64), np.array(ctx, np.int64), np.array(mil, np.int64), unc


def meth_tables(sites, counted=None):
    """(K[5], S[5]) of the sites; counted: bool per site, all by default"""
    at, ctx, mil, _ = sites
    if counted is not None:
        ctx, mil = ctx[counted], mil[counted]
    return np.bincount(ctx, minlength=5).astype(np.int64), np.bincount(ctx, weights=mil, minlength=5).astype(np.int64)


# ------------------------------------------------------------------------------------------ all of it
def build(n_cu, T, conversion=True):
    c = Cases()
    c.n_cu, c.T = n_cu, T
    r = np.random.default_rng(1000 + n_cu)
    _genome(c, r)
    _cov(c, r)
    if conversion:
        _meth(c, r)
    return c


# ------------------------------------------------------------------------------------------ what a pass that forgot its later trips would give
def fault_scan_restart(c, dep):
    """(a) k_cov_scan without `run`: the carries of the tiles from 1024 on lack the sum of the first 1024"""
    at = SCAN_STEP * c.T
    out = dep.copy()
    out[at:] -= dep[at - 1]
    return out


def first_trip(c, grid):
    """(b) bool[L]: the positions of the tiles t < grid"""
    m = np.zeros(c.L, bool)
    m[:grid * c.T] = True
    return m


def fault_sums_first_trip(c, dep):
    """(b) k_cov_sums without its later trips: tsum = 0 from tile 8 n_cu on, so the carry of every later tile is that of tile 8 n_cu"""
    T, t0 = c.T, 8 * c.n_cu
    out = dep.copy()
    for t in range(t0 + 1, c.n_tiles):
        out[t * T:(t + 1) * T] -= dep[t * T - 1] - dep[t0 * T - 1]
    return out


def fault_max_first_trip(c, dep):
    """(b) k_cov_walk<false> without its later trips: the bins end at the largest depth of the tiles below 8 n_cu"""
    return int(dep[:8 * c.n_cu * c.T, 0].max()) + 1


# ------------------------------------------------------------------------------------------ what the cases reach, from their own arrays
def changed(a, b):
    """the tables of a that b does not equal"""
    assert len(a) == len(b)
    return [i for i, (x, y) in enumerate(zip(a, b)) if x.shape != y.shape or (x != y).any()]


def assert_reach(c, dep, sites):
    """the table of DESIGN.md section 5, asserted: every loop of the table passes makes a later trip, and the later trips hold what they must"""
    n_cu, T, L = c.n_cu, c.T, c.L
    assert c.n_tiles == -(-L // T) and c.n_tiles > 8 * n_cu and L % T == 33 and len(c.contigs) >= 3
    assert len(c.top) > 8 * n_cu and len(c.bot) > 8 * n_cu
    assert len(c.bulk_fpos) + len(c.cov_designed) > cov_sweep(n_cu) and len(c.meth_jobs) > meth_sweep(n_cu)
    assert (c.bulk_fpos // T >= 8 * n_cu).any() and (c.bulk_fpos // T < 4 * n_cu).any()
    for iv in (c.top, c.bot):
        n_words = len(set(b >> 5 for b, e in iv) & set((e - 1) >> 5 for b, e in iv if e > b))
        assert n_words >= n_cu // 2 and any(e - b > 3 * T for b, e in iv) and any(b >= c.last_tile for b, e in iv)
    # the piles: deeper than the LDS histograms, in a second-trip tile of the grid of 4 n_cu and, the deepest of all, of the grid of 8 n_cu
    assert 4 * n_cu <= c.pile_a // T < 8 * n_cu <= c.pile_b // T and dep[c.pile_a:c.pile_a + 100, 0].min() > LDS_BINS_MAX
    assert dep[:8 * n_cu * T, 0].max() < dep[c.pile_b:c.pile_b + 100, 0].max() == dep[:, 0].max()
    cpg = cpg_sites(c)
    assert cpg[c.cpg_at].all() and not cpg[np.array(c.junctions) - 1].any() and cpg[0] and cpg[L - 2]
    assert (c.g[np.array(c.n_runs)] == 4).all() and (c.g[np.array(c.n_runs) - 1] == 4).all()
    assert dep[T:L - 7].min() >= 1 and (dep[np.array(c.boundaries)] > 1).all()   # the long run, and events at every boundary
    at, ctx = sites[0], sites[1]
    for t in c.special:                                                          # reported sites of every context in tiles b and b + 8 n_cu
        have = set(ctx[(at >= t * T) & (at < (t + 1) * T)].tolist())
        assert have == {0, 1, 2, 3, 4}, (t, have)
    for p in c.boundaries:                                                       # ... and sites on either side of every planted boundary
        assert ((at >= p - 20) & (at < p)).any() and ((at >= p) & (at < p + 40)).any(), p
    assert (at == c.last_tile + 8).any() and (at >= L - 3).any()                 # the last tile's CN site; a site in the genome's last bases
