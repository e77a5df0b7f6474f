// rg_ext_seed.hpp -- what stage E of rg_task (rg_task.hpp) and rg_c2r (k_c2r.hip) do with one seed of mem_chain2region1's loop (memchain.c:755-869),
// a wavefront per strand search: the two scans that decide whether the seed is extended, its extension, and the region's way into the list.
// The rules themselves are c2r_rule.h's; here is how a wavefront evaluates them.  The two callers keep their own loops over their own stores:
// a list's seed i reaches the helpers through a callable, seed(i, rbeg, qbeg, len).
#pragma once
#include "c2r_rule.h"
#include "ext_dp.hpp"
#include "ext_pk.hpp"
#include "rgx.hpp"
#include "rg_common.hpp"

// The first of regs[0, nr) that contains the seed (memchain.c:761-790), nr when none does: a lane per region made so far, 64 at a time -- the
// reference's loop stops at the first region that passes
__device__ __forceinline__ int rg_first_container(const bsx_region_t *regs, int nr, long long s_rbeg, int s_qbeg, int s_len, int l_query,
                                                  const int *gap, const RegParams &P, int lane)
{
	int u = nr;
	for (int base = 0; base < nr && u == nr; base += 64) {
		bool hit = false;
		if (base + lane < nr) {
			const bsx_region_t rg = regs[base + lane];   // (the record read whole: field by field through a reference, some instantiations spill more than they did written out)
			if (c2r_in_box(s_rbeg, s_qbeg, s_len, l_query, rg.rb, rg.re, rg.qb, rg.qe, rg.seedlen0)) {
				int qd; int64_t rd;
				c2r_end_dist(0, s_rbeg, s_qbeg, s_len, rg.rb, rg.re, rg.qb, rg.qe, &qd, &rd);
				hit = c2r_near_diagonal(qd, rd, rg_gap(gap, P, c2r_gap_len(qd, rd)), rg.w);
				c2r_end_dist(1, s_rbeg, s_qbeg, s_len, rg.rb, rg.re, rg.qb, rg.qe, &qd, &rd);
				hit = hit || c2r_near_diagonal(qd, rd, rg_gap(gap, P, c2r_gap_len(qd, rd)), rg.w);
			}
		}
		const unsigned long long hm = __ballot(hit);
		if (hm) u = base + (int)__builtin_ctzll(hm);
	}
	return u;
}

// Is there a seed after position k of the best-first order srt[0, nl) that may lead to a different alignment (memchain.c:803-814)?  A lane per seed
template <typename SeedAt>
__device__ __forceinline__ bool rg_later_disagrees(const unsigned long long *srt, int k, int nl, long long s_rbeg, int s_qbeg, int s_len, int lane, SeedAt seed)
{
	bool any = false;
	for (int base = k + 1; base < nl && !any; base += 64) {
		const int i = base + lane;
		bool alt = false;
		if (i < nl && srt[i] != 0) {
			long long t_rbeg; int t_qbeg, t_len;
			seed((int)(uint32_t)srt[i], t_rbeg, t_qbeg, t_len);
			alt = c2r_disagrees(s_rbeg, s_qbeg, s_len, t_rbeg, t_qbeg, t_len);
		}
		any = __ballot(alt) != 0;
	}
	return any;
}

// A region before its seed is extended (memchain.c:827-831)
__device__ __forceinline__ void rg_region_open(bsx_region_t &R, int &aw0, int &aw1, int w, int rid) { memset(&R, 0, sizeof(R)); aw0 = aw1 = w; R.score = R.truesc = -1; R.rid = rid; }

// The extension of one seed into an opened region (memchain.c:839-840): left then right, each with up to MAX_BAND_TRY band widths.  W: the wave's
// scratch (q, win, pf; Hrow, Erow, qrow when ROWS and QCAP > 256); win_ok > 0: the chain's window [rmax0, rmax1) is in W.win.  Returns 0, or 2 for an
// extension none of the forms here holds (-w above 127 with reads beyond 256 bases: left to the caller's batch kernels).
// PK: rows of 64 columns and more in packed 16-bit (reads of up to 256 bases only); XS: the family the stopping rule is counted for, or -1
template <bool PK, int QCAP, bool ROWS, int XS, typename WS>
__device__ __forceinline__ int rg_ext_seed(bsx_region_t &R, int &aw0, int &aw1, WS &W, const DevIndex &ix, const DevScoring &sc, const RegParams &P,
                                           const uint8_t *reads, uint32_t qoff, int l_query, int parent, long long s_rbeg, int s_qbeg, int s_len,
                                           long long rmax0, long long rmax1, int win_ok, int lane, long long &pf_t, unsigned int &pf_ext, unsigned int &pf_rows)
{
	for (int side = 0; side < 2; ++side) {
		if (c2r_side_trivial(side, s_rbeg, s_qbeg, s_len, l_query, P.a, &R.qb, &R.rb, &R.qe, &R.re, &R.score, &R.truesc)) continue;
		const int sc0 = R.score;
		const c2r_job_t j = c2r_side_job(side, qoff, s_rbeg, s_qbeg, s_len, l_query, rmax0, rmax1, P.a, sc0, P.pen_clip5, P.pen_clip3);
		int aw = P.w;
		bsx_ext_res_t res; res.score = -1; res.qle = res.tle = res.gtle = 0; res.gscore = -1; res.max_off = 0;
		bsx_ext_job_t J;
		J.parent = (uint8_t)parent; J.pad = 0; J.end_bonus = j.end_bonus;
		J.qoff = j.qoff; J.qdir = (int8_t)j.qdir; J.qlen = j.qlen; J.tpos = j.tpos; J.tdir = (int8_t)j.tdir; J.tlen = j.tlen; J.h0 = j.h0;
		for (int i = 0; i < 2; ++i) {
			const int prev = R.score;
			aw = P.w << i;
			J.w = aw;
			RG_PF_STAGE(W, 6, pf_t);
			// rows in registers, 64 entries per lane slot: as few slots as the query needs (a row's cost grows with them).  Most extensions of a
			// 150 bp read are shorter than a wavefront is wide: one register entry per lane then, and none of the per-chunk band tests and carries
			// of the wider form
			const uint8_t *win = win_ok > 0 ? W.win : nullptr;
			if (J.qlen < 64) res = ext_dp_reg<1, XS>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);
			else if constexpr (PK && QCAP <= 256) { // two columns per lane: one packed slot up to 127 query bases, two up to 255
				if (J.qlen < 128) res = ext_dp_pk<1, XS>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);
				else res = ext_dp_pk<2, XS>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);
			}
			else if (J.qlen < 128) res = ext_dp_reg<2, XS>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);
			else if (QCAP <= 256 || J.qlen < 256) res = ext_dp_reg<RG_NC, XS>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);   // (QCAP <= 256: qlen <= l_query - 1 <= 255 fits the 256 register entries)
			else if constexpr (QCAP > 256) {
				if (P.ext_win && 2 * J.w + 1 <= 256 && (long long)J.h0 + (long long)J.qlen * (parent ? sc.mx_ct : sc.mx_ga) < (1 << 21))
					res = ext_dp_win<5>(ix, sc, reads, J, lane, win, rmax0, W.q, qoff);   // rows in five register slots that follow the band (round 6)
				else if (ROWS && 2 * J.w + 1 <= 512) { WAVE_SYNC(); res = ext_dp<8>(ix, sc, reads, J, W.Hrow, W.Erow, W.qrow, lane); }   // rows in LDS, the band (<= 8 x 64 columns) in registers
				else return 2;
			}
			res.score = uni(res.score); res.qle = uni(res.qle); res.tle = uni(res.tle); res.gtle = uni(res.gtle);
			res.gscore = uni(res.gscore); res.max_off = uni(res.max_off);
			R.score = res.score;
			RG_PF_STAGE(W, 7, pf_t);
			++pf_ext; pf_rows += (unsigned int)(res.tle > res.gtle ? res.tle : res.gtle);
			if (P.prof && J.qlen >= 64) RG_PF_ADD(W, 15, (unsigned long long)(res.tle > res.gtle ? res.tle : res.gtle) << (J.qlen >= 128 ? 32 : 0));   // rows by query class: [64, 128) | 128 and more
			if (!c2r_band_again(R.score, prev, res.max_off, aw)) break;
		}
		if (side == 0) aw0 = aw; else aw1 = aw;
		c2r_side_settle(side, R.score, res.qle, res.tle, res.gtle, res.gscore, j.end_bonus, sc0, s_rbeg, s_qbeg, s_len, l_query, &R.qb, &R.rb, &R.qe, &R.re, &R.truesc);
	}
	return 0;
}

// The finished region into regs[n_regs] (memchain.c:842-868): dropped when it crosses the strand boundary; seedcov over the list's nl seeds, a lane
// each.  Returns 0, or 6 when the list is full (cap regions).
template <typename SeedAt>
__device__ __forceinline__ int rg_push_region(bsx_region_t &R, int aw0, int aw1, int s_len, float frac_rep, int parent, long long l_pac, int nl, SeedAt seed,
                                              bsx_region_t *regs, int &n_regs, int cap, int lane)
{
	R.bss = (uint8_t)c2r_bss(parent, l_pac, R.rb); R.parent = (uint8_t)parent;
	if (c2r_bss(parent, l_pac, R.re) != R.bss) return 0;   // crosses the strand boundary (memchain.c:846-849)
	int cov = 0;
	for (int i = lane; i < nl; i += 64) {
		long long t_rbeg; int t_qbeg, t_len;
		seed(i, t_rbeg, t_qbeg, t_len);
		if (c2r_covers(R.qb, R.qe, R.rb, R.re, t_rbeg, t_qbeg, t_len)) cov += t_len;
	}
	R.seedcov = uni(wave_sum_i32(cov));
	R.w = aw0 > aw1 ? aw0 : aw1; R.seedlen0 = s_len; R.frac_rep = frac_rep;
	if (uni(n_regs) == cap) return 6;
	WAVE_SYNC();
	if (lane == 0) { regs[n_regs] = R; ++n_regs; }
	WAVE_SYNC();
	return 0;
}
