// host_ssw16.cpp -- a lane-by-lane scalar restatement of the packed 16-bit seed-filter alignment (biscuit_amd/csrc/hip/k_seedsw.hip: k_swl16)
// for the CPU tests: sixteen consecutive jobs to a wavefront, a job in 8 lanes, two jobs in the halves of a lane's registers -- here a
// uint16_t each, with the kernel's three operations (an add that wraps, a subtraction that clamps at 0 as unsigned, a SIGNED maximum) --, one
// stripe count and one row count for the sixteen, the query profile as biased bytes, the padding columns, the rows past a job's target, and
// the closed form of the lazy-F loop: a prefix maximum over the lanes' last F values plus k slen e_ins, taken in the kernel's three shifted
// steps, minus (k - 1) slen e_ins, swept over the stripes whenever any lane of the wavefront has something to carry.  It shares only the
// guard (ssw16_bound.h) with the kernel.  Every 16-bit value goes through chk(), which records whether it left [0, 32767]: a job the guard
// admits must never trip it.  tests/test_ssw16_host.py drives host_ssw16() over the recorded vectors; with -DHOST_SSW16_MAIN the file is a
// stand-alone program that runs jobs of its own against a plain Smith-Waterman (the form that runs under the sanitizers).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssw16_bound.h"

namespace {
struct Range { long long lo, hi; int bad; };
inline uint16_t chk(Range &R, long long v)
{
	if (v < R.lo) R.lo = v;
	if (v > R.hi) R.hi = v;
	if (v < 0 || v > 32767) R.bad = 1;
	return (uint16_t)v;
}
inline uint16_t add16(Range &R, uint16_t a, uint16_t b) { chk(R, (long long)a + b); return (uint16_t)(a + b); }        // v_pk_add_u16: wraps
inline uint16_t subs16(uint16_t a, uint16_t b) { return a > b ? (uint16_t)(a - b) : (uint16_t)0; }                        // v_pk_sub_u16 clamp
inline uint16_t smax16(Range &R, uint16_t a, uint16_t b) { chk(R, a); chk(R, b); return (int16_t)a > (int16_t)b ? a : b; }   // v_pk_max_i16

enum { NL = SSW16_LANES, SL = SSW16_STRIPES };
struct Job { const uint8_t *q, *t; int qlen, tlen, use_ct; };
struct Half {            // one job: a half of every register of its 8 lanes
	uint16_t H[NL][SL], E[NL][SL], hlast[NL], gmax[NL], f[NL], mx[NL], v[NL];
	uint8_t prof[NL][SL][4];   // the biased byte of the lane's column of every stripe against target bases 0..3
};

// one wavefront: jobs[0..15] (qlen = tlen = 0: an empty or absent job)
void wave16(const Job *jobs, const int8_t *ctmat, const int8_t *gamat, int o_del, int e_del, int o_ins, int e_ins, int *scores, Range &R)
{
	static Half W[16];
	int bias = 0;
	for (int i = 0; i < 25; ++i) { bias = (int)ctmat[i] < -bias ? -(int)ctmat[i] : bias; bias = (int)gamat[i] < -bias ? -(int)gamat[i] : bias; }
	int slen = 0, rows = 0;
	for (int s = 0; s < 16; ++s) { const int sl = (jobs[s].qlen + 7) >> 3; slen = sl > slen ? sl : slen; rows = jobs[s].tlen > rows ? jobs[s].tlen : rows; }
	if (slen == 0 || slen > SL) { for (int s = 0; s < 16; ++s) scores[s] = 0; return; }
	const bool uni = o_del == o_ins && e_del == e_ins;
	const uint16_t biasv = chk(R, bias), oe_delv = chk(R, o_del + e_del), oe_insv = chk(R, o_ins + e_ins), e_delv = chk(R, e_del), e_insv = chk(R, e_ins);
	for (int s = 0; s < 16; ++s) {
		Half &A = W[s]; const Job &J = jobs[s];
		const int8_t *mat = J.use_ct ? ctmat : gamat;
		for (int k = 0; k < NL; ++k) {
			for (int j = 0; j < SL; ++j) {
				const int c = j + k * slen;   // word k of stripe j is query column j + k * slen
				int q = (j < slen && c < J.qlen) ? J.q[c] : 5;
				if (q > 4) q = 5;
				for (int tb = 0; tb < 4; ++tb) {
					const long long b = q > 4 ? bias : (long long)mat[tb * 5 + q] + bias;
					if (b < 0 || b > 255) R.bad = 1;
					A.prof[k][j][tb] = (uint8_t)b;
				}
				A.H[k][j] = A.E[k][j] = 0;
			}
			A.hlast[k] = A.gmax[k] = 0;
		}
	}
	uint16_t col0ev[NL], col1ev[NL];
	for (int k = 0; k < NL; ++k) { col0ev[k] = chk(R, (long long)k * slen * e_ins); col1ev[k] = chk(R, k ? (long long)(k - 1) * slen * e_ins : 0); }
	for (int i = 0; i < rows; ++i) {
		bool any = false;
		for (int s = 0; s < 16; ++s) {
			Half &A = W[s]; const Job &J = jobs[s];
			const int tb = i < J.tlen ? (J.t[i] & 3) : 0;   // past the target the packed bases are zero bits
			uint16_t hin[NL];
			for (int k = 0; k < NL; ++k) hin[k] = k ? A.hlast[k - 1] : 0;   // the shift by one lane; nothing enters lane 0
			for (int k = 0; k < NL; ++k) {
				uint16_t h = hin[k], f = 0, mx = 0;
				for (int j = 0; j < slen; ++j) {
					h = subs16(add16(R, h, A.prof[k][j][tb]), biasv);
					const uint16_t e = A.E[k][j];
					h = smax16(R, h, e);
					h = smax16(R, h, f);
					mx = smax16(R, mx, h);
					const uint16_t hold = A.H[k][j];
					A.H[k][j] = h;
					const uint16_t t = subs16(h, oe_delv);
					A.E[k][j] = smax16(R, subs16(e, e_delv), t);
					const uint16_t t2 = uni ? t : subs16(h, oe_insv);
					f = smax16(R, subs16(f, e_insv), t2);
					h = hold;
				}
				A.hlast[k] = A.H[k][slen - 1];
				A.f[k] = f; A.mx[k] = mx;
			}
			// the closed form of the lazy-F loop: the prefix maximum in three shifted steps, then the lane below's value
			uint16_t gl[NL], nx[NL];
			for (int k = 0; k < NL; ++k) gl[k] = add16(R, A.f[k], col0ev[k]);
			for (int d = 1; d <= 4; d <<= 1) {
				for (int k = 0; k < NL; ++k) nx[k] = smax16(R, gl[k], k >= d ? gl[k - d] : 0);
				memcpy(gl, nx, sizeof(gl));
			}
			for (int k = 0; k < NL; ++k) { A.v[k] = subs16(k >= 1 ? gl[k - 1] : 0, col1ev[k]); any = any || A.v[k] != 0; }
		}
		for (int s = 0; s < 16; ++s) {
			Half &A = W[s]; const Job &J = jobs[s];
			if (any) for (int k = 0; k < NL; ++k) {   // one ballot for the wavefront: every lane sweeps, most of them with 0
				uint16_t v = A.v[k];
				for (int j = 0; j < slen; ++j) { A.H[k][j] = smax16(R, A.H[k][j], v); v = subs16(v, e_insv); }
				A.hlast[k] = A.H[k][slen - 1];
			}
			for (int k = 0; k < NL; ++k) A.gmax[k] = smax16(R, A.gmax[k], i < J.tlen ? A.mx[k] : 0);
		}
	}
	for (int s = 0; s < 16; ++s) {
		uint16_t g = 0;
		for (int k = 0; k < NL; ++k) g = smax16(R, g, W[s].gmax[k]);
		scores[s] = g;
	}
}
}   // namespace

// n jobs in the order given, sixteen consecutive ones to a wavefront; qlen[i] = 0: an empty job.  Returns 0, or -2 when the guard does not
// admit the scoring options (nothing computed), -1 for a job beyond 199 x 199.  range[0..2] = smallest and largest 16-bit value formed, and 1
// if any left [0, 32767] (or a biased profile entry left a byte)
extern "C" int host_ssw16(int n, const int32_t *qlen, const int32_t *tlen, const int64_t *qoff, const int64_t *toff, const uint8_t *use_ct,
                          const uint8_t *qbuf, const uint8_t *tbuf, const int8_t *ctmat, const int8_t *gamat, int o_del, int e_del, int o_ins, int e_ins,
                          int32_t *scores, long long range[3])
{
	if (!ssw16_exact_mats(ctmat, gamat, o_del, e_del, o_ins, e_ins)) return -2;
	for (int i = 0; i < n; ++i) if (qlen[i] < 0 || qlen[i] > SSW16_QMAX || tlen[i] < 0 || tlen[i] > SSW16_QMAX) return -1;
	Range R = {0, 0, 0};
	for (int base = 0; base < n; base += 16) {
		Job J[16]; int sc[16];
		for (int s = 0; s < 16; ++s) {
			const int i = base + s;
			J[s].q = J[s].t = nullptr; J[s].qlen = J[s].tlen = J[s].use_ct = 0;
			if (i < n && qlen[i] > 0) { J[s].q = qbuf + qoff[i]; J[s].t = tbuf + toff[i]; J[s].qlen = qlen[i]; J[s].tlen = tlen[i]; J[s].use_ct = use_ct[i]; }
		}
		wave16(J, ctmat, gamat, o_del, e_del, o_ins, e_ins, sc, R);
		for (int s = 0; s < 16 && base + s < n; ++s) scores[base + s] = sc[s];
	}
	if (range) { range[0] = R.lo; range[1] = R.hi; range[2] = R.bad; }
	return 0;
}
extern "C" int host_ssw16_guard(int mx, int mn, int o_del, int e_del, int o_ins, int e_ins) { return ssw16_exact(mx, mn, o_del, e_del, o_ins, e_ins) ? 1 : 0; }

#ifdef HOST_SSW16_MAIN
// stand-alone: random jobs, empty ones among them, under ordinary scoring options and under the largest the guard admits, against a plain
// Smith-Waterman in long long
static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (uint32_t)((g_s >> 20) % n); }
static long long plain_sw(int qlen, const uint8_t *q, int tlen, const uint8_t *t, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins)
{
	long long H[SSW16_QMAX + 1], E[SSW16_QMAX + 1], best = 0;
	for (int j = 0; j <= qlen; ++j) { H[j] = 0; E[j] = -(1ll << 40); }
	for (int i = 0; i < tlen; ++i) {
		long long diag = 0, F = -(1ll << 40), hl = 0;   // hl: H of this row, column j - 1
		for (int j = 1; j <= qlen; ++j) {
			long long h = diag + mat[t[i] * 5 + q[j - 1]];
			h = h > E[j] ? h : E[j]; h = h > 0 ? h : 0;
			F = (j > 1 ? (F - e_ins > hl - o_ins - e_ins ? F - e_ins : hl - o_ins - e_ins) : F);
			h = h > F ? h : F;
			diag = H[j]; H[j] = h; hl = h;
			E[j] = E[j] - e_del > h - o_del - e_del ? E[j] - e_del : h - o_del - e_del;
			best = best > h ? best : h;
		}
	}
	return best;
}
int main(void)
{
	static const int OPT[][6] = { {1, 2, 6, 1, 6, 1}, {2, 9, 2, 1, 3, 1}, {1, 20, 1, 1, 1, 1}, {4, 20, 7, 1, 5, 2}, {127, 4, 6, 1, 6, 1},
	                              {127, 128, 1028, 30, 1028, 30}, {100, 100, 73, 10, 11, 72}, {127, 128, 3594, 1, 3594, 1} };
	enum { N = 16 * 12 + 5 };
	int n_bad = 0, n_run = 0;
	for (int it = 0; it < 160; ++it) {
		const int *o = OPT[it % 8];
		int8_t ct[25], ga[25];
		for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) {
			const bool n_ = i == 4 || j == 4;
			ct[i * 5 + j] = (int8_t)(n_ ? -1 : (i == j || (i == 1 && j == 3)) ? o[0] : -o[1]);
			ga[i * 5 + j] = (int8_t)(n_ ? -1 : (i == j || (i == 2 && j == 0)) ? o[0] : -o[1]);
		}
		if (host_ssw16_guard(o[0], -o[1], o[2], o[3], o[4], o[5]) != 1) { printf("the guard refuses option set %d\n", it % 8); return 1; }
		int32_t qlen[N], tlen[N], got[N]; int64_t qoff[N], toff[N]; uint8_t use_ct[N];
		uint8_t *qb = (uint8_t*)malloc((size_t)N * SSW16_QMAX), *tb = (uint8_t*)malloc((size_t)N * SSW16_QMAX);
		int64_t qa = 0, ta = 0;
		for (int i = 0; i < N; ++i) {
			const uint32_t kind = rnd(10);
			qlen[i] = kind == 0 ? 0 : kind < 3 ? 1 + (int)rnd(8) : kind < 5 ? 199 : 1 + (int)rnd(199);
			tlen[i] = qlen[i] == 0 ? 0 : kind < 3 ? 1 + (int)rnd(3) : kind < 5 ? 199 : 1 + (int)rnd(199);
			qoff[i] = qa; toff[i] = ta; use_ct[i] = (uint8_t)rnd(2);
			for (int j = 0; j < tlen[i]; ++j) tb[ta + j] = (uint8_t)rnd(4);
			const int gap_at = qlen[i] > 60 ? 20 + (int)rnd(20) : -1, gap = (int)rnd(60);   // a run the target lacks
			for (int j = 0, s = 0; j < qlen[i]; ++j) {
				if (j >= gap_at && gap_at >= 0 && j < gap_at + gap) { qb[qa + j] = (uint8_t)rnd(4); continue; }
				const uint32_t r = rnd(100);
				qb[qa + j] = r < 3 ? (uint8_t)rnd(4) : r == 99 ? 4 : tb[ta + (s < tlen[i] ? s : tlen[i] - 1)];
				++s;
			}
			qa += qlen[i]; ta += tlen[i];
		}
		long long range[3];
		if (host_ssw16(N, qlen, tlen, qoff, toff, use_ct, qb, tb, ct, ga, o[2], o[3], o[4], o[5], got, range) != 0) { printf("option set %d: not run\n", it % 8); return 1; }
		for (int i = 0; i < N; ++i) {
			const long long want = qlen[i] ? plain_sw(qlen[i], qb + qoff[i], tlen[i], tb + toff[i], use_ct[i] ? ct : ga, o[2], o[3], o[4], o[5]) : 0;
			++n_run;
			if (want != got[i] && ++n_bad < 5) printf("option set %d job %d (%d x %d): got %d want %lld\n", it % 8, i, qlen[i], tlen[i], got[i], want);
		}
		if (range[2]) { ++n_bad; printf("option set %d: a value left 15 bits (%lld..%lld)\n", it % 8, range[0], range[1]); }
		free(qb); free(tb);
	}
	printf("%d jobs run, %d differ or leave 15 bits\n", n_run, n_bad);
	return n_bad ? 1 : 0;
}
#endif
