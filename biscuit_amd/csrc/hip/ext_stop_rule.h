// ext_stop_rule.h -- when the rows an extension still has to run can no longer change its result.  Plain C++ without device headers: the
// kernels' forms of the rule (ext_stop.hpp) and the scalar model of the loop (tests/host_ext_stop.cpp) state the same thing over their own
// layouts of the row, with the terms below.
//
// ksw_extend2 (lib/aln/ksw.c:412-471) runs until the row maximum m is 0, the z-drop test fires or i == tlen.  An extension that has reached the
// end of its query at score G goes on long after that: E decays from G by e_del a row, m stays positive for about (G - o_del) / e_del rows, the
// z-drop expression stays at max - G + o_del, and none of those rows changes score, qle, tle, gtle, gscore or max_off.
//
// THE RULE.  Let eh[] be the reference's array after row i: eh[end] written, beg and end updated for the next row (ksw.c:466-469).  With
//     PHI = max over a in [beg, qlen] of max( eh[a].h > 0 ? eh[a].h + (qlen - a) mx     : 0,
//                                             eh[a].e > 0 ? eh[a].e + (qlen - 1 - a) mx : 0 )        mx: the largest matrix entry, >= 0
// the extension stops after row i, exactly as if i + 1 == tlen, when PHI < gscore.
//
// WHY IT IS EXACT.  Call h + (qlen - a) mx the potential of an H at entry a (the H of column a - 1, which column a reads as its diagonal) and
// e + (qlen - 1 - a) mx the potential of an E at entry a (of column a): what the value could still grow to on the way to the last column,
// gaining mx a column.  Every H a later row computes is at most PHI, and PHI never grows from row to row.  By induction over the columns j of
// the next row, every value it writes has a potential of at most PHI:
//     M = eh[j].h + s <= eh[j].h + mx is written one entry to the right: one column nearer the end, one mx of potential spent.
//     e' = max(M - oe_del, e - e_del) <= max(M, e) stays at entry j; the potential of an E at j is that of an H at j + 1.
//     F comes from an H further left in the same row, which has more columns to go, hence at least the potential.
//     h = max(M, e, F), written at entry j + 1, is bounded by the three above.
//     The first-column value h0 - o_del - e_del (i + 2) is injected only while beg == 0 and is smaller than the eh[0].h it replaces.
// A zero entry stays zero (M = h ? h + s : 0; the gap terms are clamped at 0), so zeros carry no potential.  Stale entries right of `end`
// lie inside [beg, qlen] and are counted: a later band may reach them (the band only widens by one a row on the right).  Entries left of
// `beg` are never read again: beg never decreases.
// Hence, once PHI < gscore:
//     gscore <= max always, so no later row has m > max: score, qle, tle and max_off are final.
//     no later h1 reaches gscore, so gscore and gtle are final.  The update at ksw.c:451 happens on h1 >= gscore, ties included, which is why
//     the test is strict.
//     gscore == -1 (the end of the query not reached yet): the rule never fires, PHI >= 0.
// The cell that holds the row maximum m is inside PHI, so m < gscore is a necessary condition that costs nothing: while an extension climbs
// the diagonal the gate is shut.
//
// ONE STOPPING ROW PER JOB.  The row the rule fires on depends on the job alone, not on the kernel that runs it: every form evaluates PHI over
// exactly eh[beg .. qlen] on every row with m < gscore (tests/test_gpu_x4_unread.py compares the rows of a job between kernels).
//
// PHI fits 32 bits wherever the rows do: h <= h0 + qlen mx and (qlen - a) mx <= qlen mx, and the kernels bound h0 + qlen mx below 2^21.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXT_STOP_HD __host__ __device__
#else
#define EXT_STOP_HD
#endif

// the potential of entry a of eh[]: q1mx = (qlen - 1 - a) mx
EXT_STOP_HD inline int ext_stop_term(int h, int e, int q1mx, int mx)
{
	const int ph = h > 0 ? h + q1mx + mx : 0, pe = e > 0 ? e + q1mx : 0;
	return ph > pe ? ph : pe;
}
// free necessary condition, then the rule itself
EXT_STOP_HD inline bool ext_stop_gate(int m, int gscore) { return m < gscore; }
EXT_STOP_HD inline bool ext_stop_fires(int phi, int gscore) { return phi < gscore; }

// the rule over the reference's own array (h and e interleaved as in eh_t): entries beg .. qlen
EXT_STOP_HD inline int ext_stop_phi(const int *eh_h, const int *eh_e, int beg, int qlen, int mx)
{
	int phi = 0;
	for (int a = beg; a <= qlen; ++a) { const int t = ext_stop_term(eh_h[a], eh_e[a], (qlen - 1 - a) * mx, mx); phi = phi > t ? phi : t; }
	return phi;
}
