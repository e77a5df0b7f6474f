// host_ext_pk.cpp -- a scalar restatement of the packed 16-bit extension row (biscuit_amd/csrc/hip/ext_pk.hpp: ext_dp_pk) for the CPU tests:
// 64 lanes x two int16_t halves per packed slot, the same masks (0 / -1 per half from a - beg and a - end), the same scan identity (0), the
// same carries between halves and slots, the same shift of H, the same ballots for the band of the next row -- and the same guard, included
// from the kernels' header.  Every value the row forms goes through chk(), which records whether it left [-32768, 32767]: a job the guard
// admits must never trip it.  tests/test_ext_pk_host.py drives host_ext_pk() against the oracle; with -DHOST_EXT_PK_MAIN the file is a
// stand-alone program that does the same over jobs of its own (the form that runs under the sanitizers).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ext_pk_bound.h"

namespace {
struct Range { long long lo, hi; int bad; };
inline int16_t chk(Range &R, long long v)
{
	if (v < R.lo) R.lo = v;
	if (v > R.hi) R.hi = v;
	if (v < -32768 || v > 32767) R.bad = 1;
	return (int16_t)v;
}
inline int16_t neg_mask(int16_t v) { return (int16_t)(v >> 15); }                                   // -1 where negative
inline int16_t zero_mask(int16_t v) { return (int16_t)(((uint16_t)v < 1 ? (uint16_t)v : 1) - 1); }   // -1 where zero: min_u16(v, 1) - 1
inline int16_t sel(int16_t m, int16_t a, int16_t b) { return (int16_t)((a & m) | (b & ~m)); }
inline int16_t max16(int16_t a, int16_t b) { return a > b ? a : b; }

template <int NP>
int ext_pk_row_model(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                     int w, int end_bonus, int zdrop, int h0, int out[6], Range &R)
{
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	const int16_t k_oe_ins = chk(R, oe_ins), k_oe_del = chk(R, oe_del), k_e_del = chk(R, e_del), k_e_ins = chk(R, e_ins);
	static int16_t Hp[NP][2][64], Ep[NP][2][64], sq[NP][2][64][5];
	for (int p = 0; p < NP; ++p) for (int u = 0; u < 2; ++u) for (int l = 0; l < 64; ++l) {
		const int a = (p << 7) + (u << 6) + l;
		const int q = a < qlen ? (query[a] < 4 ? query[a] : 4) : 4;
		for (int t = 0; t < 5; ++t) sq[p][u][l][t] = mat[t * 5 + q];
		const int v = a == 0 ? h0 : h0 - oe_ins - (a - 1) * e_ins;   // 32-bit, then clamped, as the kernel sets the first row
		Hp[p][u][l] = chk(R, (a <= qlen && v > 0) ? v : 0);
		Ep[p][u][l] = 0;
	}
	int mx = 0;
	for (int k = 0; k < 25; ++k) mx = mx > mat[k] ? mx : mat[k];
	{
		int max_ins = (int)((double)(qlen * mx + end_bonus - o_ins) / e_ins + 1.);
		max_ins = max_ins > 1 ? max_ins : 1;
		w = w < max_ins ? w : max_ins;
		int max_del = (int)((double)(qlen * mx + end_bonus - o_del) / e_del + 1.);
		max_del = max_del > 1 ? max_del : 1;
		w = w < max_del ? w : max_del;
	}
	int max = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
	int beg = 0, end = qlen;
	for (int i = 0; i < tlen; ++i) {
		const int t = target[i] < 4 ? target[i] : 4;
		if (beg < i - w) beg = i - w;
		if (end > i + w + 1) end = i + w + 1;
		if (end > qlen) end = qlen;
		int h1_init = 0;
		if (beg == 0) { h1_init = h0 - (o_del + e_del * (i + 1)); if (h1_init < 0) h1_init = 0; }
		int m = 0, mj = -1, h1_last = h1_init;
		uint64_t nzl[NP], nzh[NP];
		for (int p = 0; p < NP; ++p) nzl[p] = nzh[p] = 0;
		if (beg < end) {
			const int p0 = NP == 1 ? 0 : beg >> 7, p1 = NP == 1 ? 0 : end >> 7;
			const int16_t k_beg = chk(R, beg), k_end = chk(R, end), k_h1 = chk(R, h1_init);
			int carry = 0, edge = 0, key = -1, vlast = 0;
			for (int p = 0; p < NP; ++p) {
				if (!(NP == 1 || (p >= p0 && p <= p1))) continue;
				int16_t act[2][64], isbeg[2][64], isend[2][64], M[2][64], g[2][64], incl[2][64], excl[2][64], h[2][64];
				for (int u = 0; u < 2; ++u) for (int l = 0; l < 64; ++l) {
					const int16_t a = (int16_t)((p << 7) + (u << 6) + l);
					const int16_t db = chk(R, a - k_beg), de = chk(R, a - k_end);
					act[u][l] = neg_mask((int16_t)(de & ~db));
					isbeg[u][l] = zero_mask(db); isend[u][l] = zero_mask(de);
					const int16_t hr = Hp[p][u][l];
					const int16_t s = sq[p][u][l][t];
					M[u][l] = (int16_t)(chk(R, hr + s) & act[u][l] & ~zero_mask(hr));
					const int16_t tins = max16(chk(R, M[u][l] - k_oe_ins), 0);
					g[u][l] = (int16_t)(chk(R, tins + chk(R, a * k_e_ins)) & act[u][l]);
				}
				for (int u = 0; u < 2; ++u) { // the wave's inclusive max-scan of each half, identity 0; then the shift by one lane
					int16_t run = 0;
					for (int l = 0; l < 64; ++l) { run = max16(run, g[u][l]); incl[u][l] = run; }
					for (int l = 0; l < 64; ++l) excl[u][l] = l ? incl[u][l - 1] : 0;
				}
				{
					const int tl = (uint16_t)incl[0][63], th = (uint16_t)incl[1][63];
					const int cl = carry > tl ? carry : tl;
					for (int l = 0; l < 64; ++l) { excl[0][l] = max16(excl[0][l], chk(R, carry)); excl[1][l] = max16(excl[1][l], chk(R, cl)); }
					carry = cl > th ? cl : th;
				}
				int16_t en[2][64], hn[2][64];
				for (int u = 0; u < 2; ++u) for (int l = 0; l < 64; ++l) {
					const int16_t a = (int16_t)((p << 7) + (u << 6) + l);
					const int16_t er = Ep[p][u][l];
					int16_t f = max16(chk(R, excl[u][l] - chk(R, chk(R, a - 1) * k_e_ins)), 0);
					f = (int16_t)(f & ~isbeg[u][l]);
					h[u][l] = (int16_t)(max16(max16(M[u][l], er), f) & act[u][l]);
					const int16_t e = max16(chk(R, er - k_e_del), max16(chk(R, M[u][l] - k_oe_del), 0));
					en[u][l] = sel(act[u][l], e, (int16_t)(er & ~isend[u][l]));
				}
				for (int u = 0; u < 2; ++u) for (int l = 0; l < 64; ++l) {
					const int16_t up = l ? h[u][l - 1] : (u ? h[0][63] : (int16_t)edge);
					hn[u][l] = sel(isbeg[u][l], k_h1, sel((int16_t)((act[u][l] | isend[u][l]) & ~isbeg[u][l]), up, Hp[p][u][l]));
				}
				edge = (uint16_t)h[1][63];
				for (int u = 0; u < 2; ++u) for (int l = 0; l < 64; ++l) {
					const int a = (p << 7) + (u << 6) + l;
					const int k = (int)((uint32_t)(uint16_t)h[u][l] << 9) | a;
					key = key > k ? key : k;
					if (end == qlen && a == end - 1) vlast = (uint16_t)h[u][l];
					Ep[p][u][l] = en[u][l]; Hp[p][u][l] = hn[u][l];
					const int16_t nz = (int16_t)((hn[u][l] | en[u][l]) & (act[u][l] | isend[u][l]));
					if (nz) (u ? nzh[p] : nzl[p]) |= 1ull << l;
				}
			}
			m = key >> 9; mj = key & 511;
			if (end == qlen) h1_last = vlast;
		}
		const int jfin = beg < end ? end : beg;
		if (jfin == qlen) { max_ie = gscore > h1_last ? max_ie : i; gscore = gscore > h1_last ? gscore : h1_last; }
		if (m == 0) break;
		if (m > max) {
			max = m; max_i = i; max_j = mj;
			int off = mj - i; off = off < 0 ? -off : off;
			max_off = max_off > off ? max_off : off;
		} else if (zdrop > 0) {
			if (i - max_i > mj - max_j) { if (max - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop) break; }
			else { if (max - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) break; }
		}
		{
			int nb = end, last = -2;
			for (int p = NP - 1; p >= 0; --p) {
				if (nzh[p]) nb = (p << 7) + 64 + __builtin_ctzll(nzh[p]);
				if (nzl[p]) nb = (p << 7) + __builtin_ctzll(nzl[p]);
			}
			for (int p = 0; p < NP; ++p) {
				if (nzl[p]) last = (p << 7) + 63 - __builtin_clzll(nzl[p]);
				if (nzh[p]) last = (p << 7) + 127 - __builtin_clzll(nzh[p]);
			}
			if (last == -2) last = nb - 1;
			beg = nb;
			end = last + 2 < qlen ? last + 2 : qlen;
		}
	}
	out[0] = max; out[1] = max_j + 1; out[2] = max_i + 1; out[3] = max_ie + 1; out[4] = gscore; out[5] = max_off;
	return 0;
}
}   // namespace

// One ksw_extend2 call through the packed row's restatement.  Returns 0, or -2 when the guard does not admit the job (nothing computed).
// range[0..2] = smallest and largest value formed, and 1 if any left 16 bits
extern "C" int host_ext_pk(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                           int w, int end_bonus, int zdrop, int h0, int out[6], long long range[3])
{
	int mx = 0, mn = 0;
	for (int k = 0; k < 25; ++k) { mx = mx > mat[k] ? mx : mat[k]; mn = mn < mat[k] ? mn : mat[k]; }
	if (!ext_pk_exact(mx, mn, o_del, e_del, o_ins, e_ins, (long long)h0 + (long long)qlen * mx, qlen)) return -2;
	Range R = {0, 0, 0};
	if (qlen < 128) ext_pk_row_model<1>(qlen, query, tlen, target, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, out, R);
	else ext_pk_row_model<2>(qlen, query, tlen, target, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, out, R);
	if (range) { range[0] = R.lo; range[1] = R.hi; range[2] = R.bad; }
	return 0;
}
extern "C" int host_ext_pk_guard(int mx, int mn, int o_del, int e_del, int o_ins, int e_ins, long long hmax, int qmax)
{ return ext_pk_exact(mx, mn, o_del, e_del, o_ins, e_ins, hmax, qmax) ? 1 : 0; }

#ifdef HOST_EXT_PK_MAIN
// stand-alone: random jobs against the oracle's ksw_extend2 restatement (oracle/port.c), jobs right below the guard's threshold among them
extern "C" void oracle_extend1(int qlen, const uint8_t *q, int tlen, const uint8_t *t, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                               int w, int end_bonus, int zdrop, int h0, int out[6]);
static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (uint32_t)((g_s >> 20) % n); }
int main(void)
{
	static const int QL[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 126, 127, 128, 129, 191, 254, 255};
	int n_bad = 0, n_run = 0, n_edge = 0;
	for (int it = 0; it < 4000; ++it) {
		const int qlen = it % 3 ? QL[rnd(17)] : 1 + (int)rnd(255);
		int a = 1 + (int)rnd(3), b = 1 + (int)rnd(5), od = (int)rnd(8), ed = 1 + (int)rnd(3), oi = (int)rnd(8), ei = 1 + (int)rnd(3);
		const bool edge = it % 4 == 0;
		if (edge) { a = 20 + (int)rnd(100); b = 1 + (int)rnd(128); ei = 1 + (int)rnd(20); }
		int8_t mat[25];
		for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : i == j ? a : -b);
		if (rnd(2)) mat[1 * 5 + 3] = (int8_t)a;   // a conversion-tolerant entry, as the strand matrices have
		int h0 = 1 + (int)rnd(60) * a;
		if (edge) { // the largest h0 the guard admits for this query
			const long long big = 255LL * ei > a ? 255LL * ei : a;
			const long long top = 32767 - big - (long long)qlen * a;
			if (top < 1) continue;
			h0 = (int)top;
			if (ext_pk_exact(a, -b < -1 ? -b : -1, od, ed, oi, ei, (long long)h0 + 1 + (long long)qlen * a, qlen)) { printf("guard admits a job above its threshold\n"); return 1; }
			++n_edge;
		}
		const int tlen = qlen + (int)rnd(qlen / 2 + 2);
		uint8_t *q = (uint8_t*)malloc(qlen), *t = (uint8_t*)malloc(tlen);
		for (int i = 0; i < tlen; ++i) t[i] = (uint8_t)rnd(4);
		for (int i = 0, j = 0; i < qlen; ++i) { // the target with substitutions, an insertion or deletion now and then, an N sometimes
			const uint32_t r = rnd(100);
			if (r < 3 && j + 1 < tlen) ++j;
			q[i] = r < 8 ? (uint8_t)rnd(4) : r == 99 ? 4 : t[j < tlen ? j : tlen - 1];
			if (r >= 5 || r < 3) ++j;
		}
		const int w = rnd(2) ? 100 : 3 + (int)rnd(40), zdrop = rnd(4) ? 100 : (int)rnd(30), eb = (int)rnd(10);
		int got[6], want[6]; long long range[3];
		const int rc = host_ext_pk(qlen, q, tlen, t, mat, od, ed, oi, ei, w, eb, zdrop, h0, got, range);
		if (rc == 0) {
			oracle_extend1(qlen, q, tlen, t, mat, od, ed, oi, ei, w, eb, zdrop, h0, want);
			++n_run;
			if (memcmp(got, want, sizeof(got)) != 0 || range[2]) {
				if (++n_bad < 5) printf("job %d qlen %d tlen %d h0 %d a %d b %d gaps %d %d %d %d w %d: got %d %d %d %d %d %d want %d %d %d %d %d %d range %lld..%lld\n", it, qlen, tlen, h0, a, b,
				                        od, ed, oi, ei, w, got[0], got[1], got[2], got[3], got[4], got[5], want[0], want[1], want[2], want[3], want[4], want[5], range[0], range[1]);
			}
		} else if (edge) { printf("guard refuses a job at its threshold\n"); return 1; }
		free(q); free(t);
	}
	printf("%d jobs run (%d at the guard's threshold), %d differ or leave 16 bits\n", n_run, n_edge, n_bad);
	return n_bad || n_run < 3000 || n_edge < 300 ? 1 : 0;
}
#endif
