// host_ext_stop.cpp -- CPU: the extension loop of the kernels (ksw_extend2's recurrence over the eh[] array, as ext_dp.hpp states it) as a scalar
// model with the stopping rule of biscuit_amd/csrc/hip/ext_stop_rule.h -- the rule is the kernels' own header -- and the rule's proof executed:
// with the rule not obeyed, PHI is evaluated after EVERY row and checked against the row before and against every H the later rows compute.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ext_stop_rule.h"

// out[6]: score, qle, tle, gtle, gscore, max_off.
// info[0] the row after which the rule fires (-1: never; evaluated on the rows whose gate is open and that are not the last anyway, as the kernels do)
// info[1] rows run   info[2] rows on which PHI grew   info[3] rows with an H above the PHI of an earlier row   info[4] evaluations behind the gate
// info[5] the row on which the end of the query was first reached (-1: never)
// info[6] later rows that reached it with h1 == gscore > 0: the update at ksw.c:451 takes ties, so each of them moved gtle
// info[7] the last such row (-1: none)
// obey: 1 = stop where the rule fires; 0 = run every row and check the proof
extern "C" int host_ext_stop(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                             int w, int end_bonus, int zdrop, int h0, int obey, int *out, int *info)
{
	if (qlen < 0 || tlen < 0 || e_del < 1 || e_ins < 1) return -1;
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	std::vector<int> H(qlen + 2, 0), E(qlen + 2, 0);
	for (int j = 0; j <= qlen; ++j) { const int v = j == 0 ? h0 : h0 - oe_ins - (j - 1) * e_ins; H[j] = v > 0 ? v : 0; }
	int mx = 0;
	for (int k = 0; k < 25; ++k) mx = mx > mat[k] ? mx : mat[k];
	{
		int max_ins = (int)((double)(qlen * mx + end_bonus - o_ins) / e_ins + 1.); max_ins = max_ins > 1 ? max_ins : 1; w = w < max_ins ? w : max_ins;
		int max_del = (int)((double)(qlen * mx + end_bonus - o_del) / e_del + 1.); max_del = max_del > 1 ? max_del : 1; w = w < max_del ? w : max_del;
	}
	int max = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0, beg = 0, end = qlen;
	int fire_row = -1, rows = 0, grew = 0, above = 0, evals = 0, reach = -1, ties = 0, last_tie = -1;
	long long phi_prev = -1;   // the smallest PHI so far (-1: no row yet)
	for (int i = 0; i < tlen; ++i) {
		++rows;
		const int8_t *s = mat + 5 * (target[i] < 4 ? target[i] : 4);
		if (beg < i - w) beg = i - w;
		if (end > i + w + 1) end = i + w + 1;
		if (end > qlen) end = qlen;
		int h1 = 0;
		if (beg == 0) { h1 = h0 - (o_del + e_del * (i + 1)); if (h1 < 0) h1 = 0; }
		int f = 0, m = 0, mj = -1;
		for (int j = beg; j < end; ++j) {
			int M = H[j], e = E[j];
			H[j] = h1;
			M = M ? M + s[query[j] < 4 ? query[j] : 4] : 0;
			int h = M > e ? M : e; h = h > f ? h : f;
			h1 = h;
			if (phi_prev >= 0 && h > phi_prev) ++above;
			if (m <= h) { m = h; mj = j; }
			int t = M - oe_del; t = t > 0 ? t : 0;
			e -= e_del; e = e > t ? e : t; E[j] = e;
			t = M - oe_ins; t = t > 0 ? t : 0;
			f -= e_ins; f = f > t ? f : t;
		}
		const int jfin = beg < end ? end : beg;
		H[end] = h1; E[end] = 0;
		if (jfin == qlen) { if (reach >= 0 && h1 == gscore && gscore > 0) { ++ties; last_tie = i; } if (reach < 0) reach = i; max_ie = gscore > h1 ? max_ie : i; gscore = gscore > h1 ? gscore : h1; }
		if (m == 0) break;
		if (m > max) {
			max = m; max_i = i; max_j = mj;
			int off = mj - i; off = off < 0 ? -off : off;
			max_off = max_off > off ? max_off : off;
		} else if (zdrop > 0) {
			if (i - max_i > mj - max_j) { if (max - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop) break; }
			else { if (max - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) break; }
		}
		int j;
		for (j = beg; j < end && H[j] == 0 && E[j] == 0; ++j) {}
		beg = j;
		for (j = end; j >= beg && H[j] == 0 && E[j] == 0; --j) {}
		end = j + 2 < qlen ? j + 2 : qlen;
		// the rule
		const int phi = ext_stop_phi(H.data(), E.data(), beg, qlen, mx);
		if (phi_prev >= 0 && phi > phi_prev) ++grew;
		if (phi_prev < 0 || phi < phi_prev) phi_prev = phi;
		if (fire_row < 0 && ext_stop_gate(m, gscore) && i + 1 < tlen) {
			++evals;
			if (ext_stop_fires(phi, gscore)) { fire_row = i; if (obey) break; }
		}
	}
	out[0] = max; out[1] = max_j + 1; out[2] = max_i + 1; out[3] = max_ie + 1; out[4] = gscore; out[5] = max_off;
	info[0] = fire_row; info[1] = rows; info[2] = grew; info[3] = above; info[4] = evals; info[5] = reach; info[6] = ties; info[7] = last_tie;
	return 0;
}
