/* c2r_rule.h -- the rules of mem_chain2region (lib/aln/memchain.c), stated once.  Plain C99 that is also C++17, no device headers: the host's
 * state machine (extend.c, chain.c), the region kernels (rg_ext_seed.hpp for stage E of rg_task and for rg_c2r), the extensions made ahead
 * (k_x4prep, k_ext4, k_extl) and tests/c2r_rule_host_main.c all call these.  Scalar functions over values: every caller keeps its own layout of
 * seeds, regions and jobs, and supplies cal_max_gap (memchain.c:576-582) from wherever it keeps it (a table in LDS, bsx_cal_max_gap).
 *
 *   c2r_seed_span      a seed's reach on the reference, mem_chain_reference_span              memchain.c:585-598
 *   c2r_clamp_window   [0, 2 l_pac], the strand boundary (memchain.c:599-604), the contig as bns_fetch_seq clamps it (memchain.c:889)
 *   c2r_in_box, c2r_end_dist, c2r_gap_len, c2r_near_diagonal
 *                      is the seed inside a region made so far                                memchain.c:761-790
 *   c2r_disagrees      does a later long seed lead to another alignment                       memchain.c:794-819
 *   c2r_side_trivial   a side that needs no extension, and what it takes then                 memchain.c:623-626, 688-691
 *   c2r_side_job       the ksw_extend2 call of a side                                         memchain.c:628-638, 654, 693-695, 713
 *   c2r_band_again     once more with twice the band                                          memchain.c:641-659, 700-718
 *   c2r_side_settle    local end or to the end of the read, and the coordinates that follow   memchain.c:661-670, 720-729
 *   c2r_bss            mem_getbss: the strand-boundary rejection compares it at rb and re     memchain.c:265, 842-849
 *   c2r_covers         a seed counted in seedcov                                              memchain.c:857-865
 * side: 0 = left of the seed (towards the read's start), 1 = right.  `.1 * l_query` and `s_len * .95` are double comparisons. */
#ifndef BSX_C2R_RULE_H
#define BSX_C2R_RULE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define C2R_FN static inline __host__ __device__ __attribute__((always_inline))
#else
#define C2R_FN static inline
#endif

C2R_FN void c2r_seed_span(int64_t rbeg, int qbeg, int len, int l_query, int gap_left, int gap_right, int64_t *b, int64_t *e)
{
	*b = rbeg - (qbeg + gap_left); *e = rbeg + len + ((l_query - qbeg - len) + gap_right);
}

/* [ctg_beg, ctg_end): the chain's contig in forward coordinates, mirrored here for a chain on the reverse strand */
C2R_FN void c2r_clamp_window(int64_t *rmax0, int64_t *rmax1, int64_t l_pac, int64_t chain_pos, int64_t ctg_beg, int64_t ctg_end)
{
	*rmax0 = *rmax0 > 0 ? *rmax0 : 0; *rmax1 = *rmax1 < l_pac << 1 ? *rmax1 : l_pac << 1;
	if (*rmax0 < l_pac && l_pac < *rmax1) { if (chain_pos < l_pac) *rmax1 = l_pac; else *rmax0 = l_pac; }
	if (chain_pos >= l_pac) { const int64_t tmp = ctg_beg; ctg_beg = (l_pac << 1) - ctg_end; ctg_end = (l_pac << 1) - tmp; }
	*rmax0 = *rmax0 > ctg_beg ? *rmax0 : ctg_beg; *rmax1 = *rmax1 < ctg_end ? *rmax1 : ctg_end;
}

/* containment, first half: inside the region on both axes, and not much longer than the seed the region grew from */
C2R_FN int c2r_in_box(int64_t s_rbeg, int s_qbeg, int s_len, int l_query, int64_t rg_rb, int64_t rg_re, int rg_qb, int rg_qe, int rg_seedlen0)
{
	if (s_rbeg < rg_rb || s_rbeg + s_len > rg_re || s_qbeg < rg_qb || s_qbeg + s_len > rg_qe) return 0;
	return !(s_len - rg_seedlen0 > .1 * l_query);
}
/* second half, once from each end of the region (end 0: its start): the distances, the length cal_max_gap is asked for, and the test
 * itself; the seed is contained when it is near the diagonal from either end */
C2R_FN void c2r_end_dist(int end, int64_t s_rbeg, int s_qbeg, int s_len, int64_t rg_rb, int64_t rg_re, int rg_qb, int rg_qe, int *qd, int64_t *rd)
{
	if (end == 0) { *qd = s_qbeg - rg_qb; *rd = s_rbeg - rg_rb; }
	else { *qd = rg_qe - (s_qbeg + s_len); *rd = rg_re - (s_rbeg + s_len); }
}
C2R_FN int c2r_gap_len(int qd, int64_t rd) { return (int)(qd < rd ? qd : rd); }
C2R_FN int c2r_near_diagonal(int qd, int64_t rd, int max_gap, int rg_w)
{
	const int w = max_gap < rg_w ? max_gap : rg_w;
	return qd - rd < w && rd - qd < w;
}

/* s: the contained seed; t: a seed after it in the best-first order */
C2R_FN int c2r_disagrees(int64_t s_rbeg, int s_qbeg, int s_len, int64_t t_rbeg, int t_qbeg, int t_len)
{
	if (t_len < s_len * .95) return 0;
	return (s_qbeg <= t_qbeg && s_qbeg + s_len - t_qbeg >= s_len >> 2 && t_qbeg - s_qbeg != t_rbeg - s_rbeg) ||
	       (t_qbeg <= s_qbeg && t_qbeg + t_len - s_qbeg >= s_len >> 2 && s_qbeg - t_qbeg != s_rbeg - t_rbeg);
}

/* 1 and the side's values when the seed reaches that end of the read; else 0 and nothing is touched.  a: the match score */
C2R_FN int c2r_side_trivial(int side, int64_t s_rbeg, int s_qbeg, int s_len, int l_query, int a,
                            int *qb, int64_t *rb, int *qe, int64_t *re, int *score, int *truesc)
{
	if (side == 0) {
		if (s_qbeg != 0) return 0;
		*score = *truesc = s_len * a; *qb = 0; *rb = s_rbeg;
	} else {
		if (s_qbeg + s_len != l_query) return 0;
		*qe = l_query; *re = s_rbeg + s_len;
	}
	return 1;
}

/* the fields of bsx_ext_job_t that a side decides (band width and strand are the caller's); sc0: the score the left side ended with */
typedef struct { int64_t tpos; uint32_t qoff; int qdir, qlen, tdir, tlen, h0, end_bonus; } c2r_job_t;
C2R_FN c2r_job_t c2r_side_job(int side, uint32_t qoff, int64_t s_rbeg, int s_qbeg, int s_len, int l_query, int64_t rmax0, int64_t rmax1,
                              int a, int sc0, int pen_clip5, int pen_clip3)
{
	c2r_job_t j;
	if (side == 0) {
		j.qoff = qoff + (uint32_t)s_qbeg - 1; j.qdir = -1; j.qlen = s_qbeg; j.tpos = s_rbeg - 1; j.tdir = -1; j.tlen = (int)(s_rbeg - rmax0);
		j.h0 = s_len * a; j.end_bonus = pen_clip5;
	} else {
		const int qe = s_qbeg + s_len;
		j.qoff = qoff + (uint32_t)qe; j.qdir = 1; j.qlen = l_query - qe; j.tpos = s_rbeg + s_len; j.tdir = 1; j.tlen = (int)(rmax1 - (s_rbeg + s_len));
		j.h0 = sc0; j.end_bonus = pen_clip3;
	}
	return j;
}

/* after a try with band aw: prev is the region's score before it */
C2R_FN int c2r_band_again(int score, int prev, int max_off, int aw) { return !(score == prev || max_off < (aw >> 1) + (aw >> 2)); }

/* the side's last try returned (score, qle, tle, gtle, gscore); clip: the side's end_bonus */
C2R_FN void c2r_side_settle(int side, int score, int qle, int tle, int gtle, int gscore, int clip, int sc0,
                            int64_t s_rbeg, int s_qbeg, int s_len, int l_query, int *qb, int64_t *rb, int *qe, int64_t *re, int *truesc)
{
	const int local = gscore <= 0 || gscore <= score - clip;
	if (side == 0) {
		if (local) { *qb = s_qbeg - qle; *rb = s_rbeg - tle; *truesc = score; }
		else { *qb = 0; *rb = s_rbeg - gtle; *truesc = gscore; }
	} else {
		if (local) { *qe = s_qbeg + s_len + qle; *re = s_rbeg + s_len + tle; *truesc += score - sc0; }
		else { *qe = l_query; *re = s_rbeg + s_len + gtle; *truesc += gscore - sc0; }
	}
}

C2R_FN int c2r_bss(int parent, int64_t l_pac, int64_t pos) { return ((pos > l_pac) == parent) ? 1 : 0; }

C2R_FN int c2r_covers(int rg_qb, int rg_qe, int64_t rg_rb, int64_t rg_re, int64_t t_rbeg, int t_qbeg, int t_len)
{
	return t_qbeg >= rg_qb && t_qbeg + t_len <= rg_qe && t_rbeg >= rg_rb && t_rbeg + t_len <= rg_re;
}
#endif
