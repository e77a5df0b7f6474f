// ext_pk.hpp -- the rows of ext_dp_reg (ext_dp.hpp) with TWO columns per lane: lane l of packed slot p owns entry 128 p + l of the reference's
// eh[] array in the low 16 bits of each register and entry 128 p + 64 + l in the high 16 bits, so one instruction stream serves 128 columns.
// H and E are one register per packed slot; the element-wise steps (M, tins, h, e, the gap terms) are packed 16-bit instructions; the max-plus
// prefix scan for F runs its six DPP steps once for both halves, after which the low half's total is carried into the high half and the slot's
// total into the next slot; the shift of H by one column is one wave_prev of the packed word (lane 0's high half takes the low half's lane 63,
// lane 0's low half the previous slot's high lane 63).  The band tests are masks of 0 / 0xffff per half, made once per slot and row from
// a - beg and a - end and applied with bit-field inserts.  Only the row maximum is unpacked (the last column must win ties: h << 9 | column).
// Nothing here relies on 16-bit wraparound: ext_pk_bound.h states when every intermediate fits, and the caller must have checked it.
// Needs qlen + 1 <= 128 * NP entries.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "ext_pk_bound.h"
#include "ext_stop.hpp"

typedef short pk2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pk2 pk_of(uint32_t w) { return __builtin_bit_cast(pk2, w); }
__device__ __forceinline__ uint32_t pk_word(pk2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ pk2 pk_splat(int v) { return pk_of((uint32_t)(v & 0xffff) * 0x10001u); }
__device__ __forceinline__ pk2 pk_pair(int lo, int hi) { return pk_of((uint32_t)(lo & 0xffff) | (uint32_t)hi << 16); }
__device__ __forceinline__ pk2 pk_max(pk2 a, pk2 b) { return __builtin_elementwise_max(a, b); }
// The masks are written as instructions: left to itself the compiler reads the two steps of a mask as a comparison and makes it per half
// (two compares, two selects and a byte permute for what two packed instructions do).
// 0xffff in a half whose value is negative
__device__ __forceinline__ pk2 pk_neg_mask(pk2 v) { uint32_t w; asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(w) : "v"(pk_word(v))); return pk_of(w); }
// 1 in a half whose value is not zero (any 16-bit pattern), else 0
__device__ __forceinline__ pk2 pk_nonzero_01(pk2 v) { uint32_t w; asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(w) : "v"(pk_word(v))); return pk_of(w); }
// 0xffff in a half whose value is zero / is not zero
__device__ __forceinline__ pk2 pk_zero_mask(pk2 v) { return pk_nonzero_01(v) - (pk2){1, 1}; }
__device__ __forceinline__ pk2 pk_nonzero_mask(pk2 v) { return (pk2){0, 0} - pk_nonzero_01(v); }
// per half: mask ? a : b
__device__ __forceinline__ pk2 pk_sel(pk2 mask, pk2 a, pk2 b) { return (a & mask) | (b & ~mask); }

// inclusive max-scan across the wave of both halves at once, for operands >= 0: lanes without a source take 0
__device__ __forceinline__ pk2 wave_scan_max_incl_pk(pk2 v)
{
	// a lane without a source reads 0 (bound_ctrl); a row a broadcast step leaves out keeps the step before's operand, which is already part
	// of its maximum: no step needs a register set to the identity first
	int t = 0;
#define PK_SCAN_STEP(ctrl, rows) do { t = __builtin_amdgcn_update_dpp(t, (int)pk_word(v), ctrl, rows, 0xf, true); v = pk_max(v, pk_of((uint32_t)t)); } while (0)
	PK_SCAN_STEP(DPP_ROW_SHR(1), 0xf); PK_SCAN_STEP(DPP_ROW_SHR(2), 0xf); PK_SCAN_STEP(DPP_ROW_SHR(4), 0xf); PK_SCAN_STEP(DPP_ROW_SHR(8), 0xf);
	PK_SCAN_STEP(DPP_ROW_BCAST15, 0xa); PK_SCAN_STEP(DPP_ROW_BCAST31, 0xc);
#undef PK_SCAN_STEP
	return v;
}

template <int NP, int XS_FAM = -1>
__device__ __forceinline__ bsx_ext_res_t ext_dp_pk(const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t &J, int lane,
                                                   const uint8_t *win = nullptr, long long win_beg = 0, const uint8_t *qlds = nullptr, uint32_t qlds_off = 0)
{   // win, qlds, XS_FAM: as ext_dp_reg
	const int qlen = J.qlen, tlen = J.tlen, h0 = J.h0;
	const int8_t *mat = J.parent ? sc.ctmat : sc.gamat;
	const int o_del = sc.o_del, e_del = sc.e_del, o_ins = sc.o_ins, e_ins = sc.e_ins;
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins, zdrop = sc.zdrop;
	const pk2 k_oe_ins = pk_splat(oe_ins), k_oe_del = pk_splat(oe_del), k_e_del = pk_splat(e_del), k_e_ins = pk_splat(e_ins), k_zero = pk_splat(0);
	pk2 Hp[NP], Ep[NP], sq4[NP];
	uint32_t sql[NP], sqh[NP];   // scores of the lane's two query bases of slot p against target bases 0..3, a byte each; sq4: against base 4, packed
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		int hv[2], s4[2]; uint32_t sq[2];
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int a = (p << 7) + (u << 6) + lane;
			const int q = a < qlen ? (qlds ? (int)qlds[(int)(J.qoff - qlds_off) + a * J.qdir] : (int)reads[(long long)J.qoff + (long long)a * J.qdir]) : 4;
			sq[u] = (uint32_t)(uint8_t)mat[q] | (uint32_t)(uint8_t)mat[5 + q] << 8 | (uint32_t)(uint8_t)mat[10 + q] << 16 | (uint32_t)(uint8_t)mat[15 + q] << 24;   // q <= 4
			s4[u] = mat[20 + q];
			const int v = a == 0 ? h0 : h0 - oe_ins - (a - 1) * e_ins;   // first row (ksw.c:395-397)
			hv[u] = (a <= qlen && v > 0) ? v : 0;
		}
		sql[p] = sq[0]; sqh[p] = sq[1]; sq4[p] = pk_pair(s4[0], s4[1]);
		Hp[p] = pk_pair(hv[0], hv[1]);
		Ep[p] = k_zero;
	}
	const int mx = J.parent ? sc.mx_ct : sc.mx_ga;
	int w = J.w;
	{ // band clamp (ksw.c:399-407)
		int max_ins = (int)((double)(qlen * mx + J.end_bonus - o_ins) / e_ins + 1.);
		max_ins = max_ins > 1 ? max_ins : 1;
		w = w < max_ins ? w : max_ins;
		int max_del = (int)((double)(qlen * mx + J.end_bonus - o_del) / e_del + 1.);
		max_del = max_del > 1 ? max_del : 1;
		w = w < max_del ? w : max_del;
	}
	int max = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
	int beg = 0, end = qlen;
	int tb_reg = 4;
	[[maybe_unused]] bool xs_fired = false;
	for (int i = 0; i < tlen; ++i) {
		if constexpr (XS_FAM >= 0) if (xs_fired) ext_stop_dead_row(sc, XS_FAM, lane);
		if ((i & 63) == 0) {
			const long long tp = J.tpos + (long long)(i + lane) * J.tdir;
			tb_reg = (i + lane < tlen) ? (win ? (int)win[tp - win_beg] : dev_ref_base(ix.pac, ix.l_pac, tp)) : 4;
		}
		const int t = wave_bcast(tb_reg, i & 63);
		if (beg < i - w) beg = i - w;
		if (end > i + w + 1) end = i + w + 1;
		if (end > qlen) end = qlen;
		int h1_init = 0;
		if (beg == 0) { h1_init = h0 - (o_del + e_del * (i + 1)); if (h1_init < 0) h1_init = 0; }
		int m = 0, mj = -1, h1_last = h1_init;
		unsigned long long nzl[NP], nzh[NP];   // the non-zero cells of entries beg..end after this row, a ballot per half
#pragma unroll
		for (int p = 0; p < NP; ++p) nzl[p] = nzh[p] = 0;
		if (beg < end) {
			// the slots of entries beg .. end (entry `end` gets its E cleared and its H set); one slot: every test on p folds away
			const int p0 = NP == 1 ? 0 : beg >> 7, p1 = NP == 1 ? 0 : end >> 7;
			const pk2 k_beg = pk_splat(beg), k_end = pk_splat(end), k_h1 = pk_splat(h1_init);
			const int tsh = (t & 3) << 3;
			int carry = 0, edge = 0, lkey = -1, vlast = 0;
#pragma unroll
			for (int p = 0; p < NP; ++p) {
				if (NP == 1 || (p >= p0 && p <= p1)) {
					const pk2 a = pk_pair((p << 7) + lane, (p << 7) + 64 + lane);
					// masks: column in the band, a == beg, a == end, H not zero
					const pk2 db = a - k_beg, de = a - k_end;
					const pk2 act = pk_neg_mask(de & ~db);
					const pk2 isbeg = pk_zero_mask(db), isend = pk_zero_mask(de);
					const pk2 hr = Hp[p], er = Ep[p];
					const pk2 s = t < 4 ? pk_pair((int)(int8_t)(sql[p] >> tsh), (int)(int8_t)(sqh[p] >> tsh)) : sq4[p];
					const pk2 M = (hr + s) & act & pk_nonzero_mask(hr);            // hr ? hr + s : 0, in the band
					const pk2 tins = pk_max(M - k_oe_ins, k_zero);
					const pk2 g = (tins + a * k_e_ins) & act;                      // the scan's identity is 0
					const pk2 incl = wave_scan_max_incl_pk(g);
					pk2 excl = pk_of((uint32_t)__builtin_amdgcn_update_dpp(0, (int)pk_word(incl), DPP_WAVE_SHR1, 0xf, 0xf, true));   // lane 0: 0
					{ // the prefix over all earlier columns: the slots before into both halves, this slot's low half into its high half
						const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)pk_word(incl), 63);
						const int tl = (int)(tot & 0xffffu), th = (int)(tot >> 16);
						const int cl = carry > tl ? carry : tl;
						excl = pk_max(excl, pk_pair(carry, cl));
						carry = cl > th ? cl : th;
					}
					pk2 f = pk_max(excl - (a - (pk2){1, 1}) * k_e_ins, k_zero);
					f = f & ~isbeg;
					const pk2 h = pk_max(pk_max(M, er), f) & act;
					const pk2 e = pk_max(er - k_e_del, pk_max(M - k_oe_del, k_zero));
					const pk2 en = pk_sel(act, e, er & ~isend);
					Ep[p] = en;
					// H: entry a takes h(i, a-1) for a-1 in the band, entry beg takes the first-column value
					const uint32_t hw = pk_word(h);
					const uint32_t h63 = (uint32_t)__builtin_amdgcn_readlane((int)hw, 63);
					const pk2 up = pk_of((uint32_t)wave_prev((int)hw, (int)((uint32_t)edge | h63 << 16)));
					edge = (int)(h63 >> 16);
					const pk2 hn = pk_sel(isbeg, k_h1, pk_sel((act | isend) & ~isbeg, up, hr));
					Hp[p] = hn;
					// row maximum and the last column that attains it: (h << 9 | column); a lane outside the band has h = 0 and cannot win a row whose
					// maximum is positive (a row whose maximum is 0 ends the extension, and its column is not read)
					{
						const int kl = (int)((hw & 0xffffu) << 9) | ((p << 7) + lane), kh = (int)((hw >> 16) << 9) | ((p << 7) + 64 + lane);
						lkey = lkey > kl ? lkey : kl; lkey = lkey > kh ? lkey : kh;
					}
					if (end == qlen && ((end - 1) >> 7) == p) vlast = (int)(((end - 1) & 64) ? hw >> 16 : hw & 0xffffu);
					// the non-zero cells as the next row finds them (ksw.c:466-469), among entries beg .. end
					const uint32_t nz = pk_word((hn | en) & (act | isend));
					nzl[p] = __ballot((nz & 0xffffu) != 0);
					nzh[p] = __ballot(nz > 0xffffu);
				}
			}
			{
				const int key = wave_max_i32(lkey);
				m = key >> 9; mj = key & 511;
			}
			if (end == qlen) h1_last = wave_bcast(vlast, (end - 1) & 63);   // h(i, end-1), only read for the to-the-end score
		}
		// (an empty row writes only eh[end] (ksw.c:449), which nothing reads: its maximum is 0 and the extension ends below)
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
		// shrink the band to the non-zero cells (ksw.c:466-469): the first one among beg..end-1 (else end; a first one AT end gives end as
		// well), the last one from there to end (else the one before the first), both out of the same ballots
		{
			int nb = end, last = -2;
#pragma unroll
			for (int p = NP - 1; p >= 0; --p) {
				if (nzh[p]) nb = (p << 7) + 64 + __builtin_ctzll(nzh[p]);
				if (nzl[p]) nb = (p << 7) + __builtin_ctzll(nzl[p]);
			}
#pragma unroll
			for (int p = 0; p < NP; ++p) {
				if (nzl[p]) last = (p << 7) + 63 - __builtin_clzll(nzl[p]);
				if (nzh[p]) last = (p << 7) + 127 - __builtin_clzll(nzh[p]);
			}
			if (last == -2) last = nb - 1;
			beg = nb;
			end = last + 2 < qlen ? last + 2 : qlen;
		}
		// no later row can change a result field (ext_stop_rule.h): as if i + 1 == tlen.  PHI in 32 bits from the packed halves
		if (ext_stop_gate(m, gscore) && i + 1 < tlen && (XS_FAM >= 0 ? !xs_fired && ext_stop_armed(sc) : sc.ext_stop != 0)) {
			const int phi = ext_stop_phi_pk<NP>(Hp, Ep, beg, qlen, J.parent ? sc.mx_ct : sc.mx_ga, lane);
			if constexpr (XS_FAM >= 0) { if (ext_stop_decide(sc, XS_FAM, phi, gscore, tlen - 1 - i, lane, xs_fired)) break; }
			else if (ext_stop_fires(phi, gscore)) break;
		}
	}
	bsx_ext_res_t r;
	r.score = max; r.qle = max_j + 1; r.tle = max_i + 1; r.gtle = max_ie + 1; r.gscore = gscore; r.max_off = max_off;
	return r;
}
