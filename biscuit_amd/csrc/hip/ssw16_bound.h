// ssw16_bound.h -- when the packed 16-bit seed-filter alignment (k_swl16, k_seedsw.hip) is exact.  Plain C++ without device headers: the host
// decides with it once per launch whether the chunk's seeds go through k_swl16 or through the 32-bit alignment of k_seedsw_apply, and the CPU
// restatement of the kernel (tests/host_ssw16.cpp) range-checks every 16-bit value against it.
//
// k_swl16 keeps two jobs of ksw_i16 (lib/aln/ksw.c:232-334) in the halves of a 32-bit register.  Its adds wrap (v_pk_add_u16), its subtractions
// clamp at 0 as unsigned values (v_pk_sub_u16 clamp) and its maxima are SIGNED (v_pk_max_i16), so a half is what ksw_i16's word is only while
// every value that enters a maximum lies in [0, 32767], no add wraps, and every subtrahend is its own value as an unsigned half.  With
//     mx   = the largest matrix entry of either strand's matrix (at least 0),   mn = the smallest (at most 0),   bias = -mn
//     hmax = the largest H of a job: a window holds at most 199 query columns (RG_SHORT_LEN - 1), H(i,j) <= (min(i,j) + 1) mx <= 199 mx;  E, F <= H
//     e = max(e_del, e_ins),   oe = max(o_del + e_del, o_ins + e_ins)
// the kernel forms
//     h + (s + bias)      the row's score read from the biased byte profile and added to H of the previous row, then `- bias` clamped at 0:
//                         <= 198 mx + mx + bias = hmax + bias; the byte s + bias itself lies in [0, mx + bias] and has to fit 8 bits
//     h - oe_del, h - oe_ins, e - e_del, f - e_ins, v - e_ins     clamped at 0, never above hmax
//     f + k slen e_ins    (col0ev) the operand of the prefix maximum that carries F across the job's 8 lanes, k <= 7 and slen <= 25 stripes:
//                         f <= hmax - oe_ins, so <= hmax + 7 * 25 e_ins; a lane whose f is 0 contributes k slen e_ins, which the subtraction
//                         of (k - 1) slen e_ins (col1ev) on the lanes above it brings back to 0 or below
//     the splatted constants bias, oe_del, oe_ins, e_del, e_ins, k slen e_ins, (k - 1) slen e_ins: each at most max(oe, 7 * 25 e, 128)
// The largest of these is bounded by  199 mx + 7 * 25 e + bias;  the rule keeps the margin of 2 oe it has always had on top of that:
//     199 mx + 7 * 25 e + 2 oe + bias <= 32767,   mx + bias <= 255,   oe <= 32767,   0 <= o_*, e_*
// (negative penalties would be splatted as values above 32767: nothing sensible asks for them, and the 32-bit path takes them as they are).
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSW16_HD __host__ __device__
#else
#define SSW16_HD
#endif

#define SSW16_QMAX 199     // columns and rows of a job: RG_SHORT_LEN - 1
#define SSW16_LANES 8      // the words of ksw_i16's SSE register: lanes of a job
#define SSW16_STRIPES 25   // ceil(SSW16_QMAX / SSW16_LANES)

SSW16_HD inline bool ssw16_exact(int mx, int mn, int o_del, int e_del, int o_ins, int e_ins)
{
	if (o_del < 0 || e_del < 0 || o_ins < 0 || e_ins < 0) return false;
	if (mx < 0) mx = 0;
	const int bias = mn < 0 ? -mn : 0;
	const long long oe = (long long)o_del + e_del > (long long)o_ins + e_ins ? (long long)o_del + e_del : (long long)o_ins + e_ins;
	const long long e = e_del > e_ins ? e_del : e_ins;
	if ((long long)SSW16_QMAX * mx + (long long)(SSW16_LANES - 1) * SSW16_STRIPES * e + 2 * oe + bias >= 32768 || mx + bias > 255 || oe >= 32768) return false;
	return true;
}
// over the two strand matrices of a launch
SSW16_HD inline bool ssw16_exact_mats(const signed char *ctmat, const signed char *gamat, int o_del, int e_del, int o_ins, int e_ins)
{
	int mx = 0, mn = 0;
	for (int i = 0; i < 25; ++i) {
		mx = ctmat[i] > mx ? ctmat[i] : mx; mx = gamat[i] > mx ? gamat[i] : mx;
		mn = ctmat[i] < mn ? ctmat[i] : mn; mn = gamat[i] < mn ? gamat[i] : mn;
	}
	return ssw16_exact(mx, mn, o_del, e_del, o_ins, e_ins);
}
