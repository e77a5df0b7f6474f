// ext_pk_bound.h -- when the packed 16-bit extension row (ext_dp_pk, ext_pk.hpp) is exact.  Plain C++ without device headers: the host picks
// the kernel form with it once per launch, the kernels around the row re-check it per job, and the CPU restatement of the row
// (tests/host_ext_pk.cpp) range-checks every intermediate against it.
//
// The row keeps two columns of ksw_extend2 (lib/aln/ksw.c:380-479) in the signed 16-bit halves of a register and never relies on wraparound,
// so every value it forms, on lanes inside the band and outside it, has to lie in [-32768, 32767].  With
//     hmax = the largest H of the job: H(i,j) <= h0 + (j+1) mx <= h0 + qlen mx      (mx: the largest matrix entry; E, F <= H)
//     mn   = the most negative matrix entry,   qmax = the longest query of the launch
// the LARGEST values are
//     hr + s            <= hmax + mx         formed on every lane before the band mask is applied (hr <= hmax anywhere in eh[])
//     tins + a e_ins    <= hmax + 255 e_ins  the scan operand: every lane computes it before the mask, and the row's columns are a <= 255
// and the SMALLEST are
//     M - oe_ins, M - oe_del   >= mn - max(oe_ins, oe_del)     (M = hr + s >= 1 + mn where hr != 0, else M = 0)
//     er - e_del               >= -e_del
//     excl - (a-1) e_ins       >= -254 e_ins                   the scan's identity is 0: every operand is >= 0 and F is clamped at 0 anyway
// The constants splatted into both halves (e_ins, e_del, oe_ins, oe_del) must be representable, and the row's columns (a <= 255) are.
// Hence the inequality:
//     0 <= o_*, 1 <= e_*,  hmax + max(mx, 255 e_ins) <= 32767  and  max(oe_ins, oe_del) - mn <= 32767,  qmax <= 255
// (the second and third smallest follow from these: e_del <= oe_del and 254 e_ins < 32767).
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXT_PK_HD __host__ __device__
#else
#define EXT_PK_HD
#endif

#define EXT_PK_QMAX 255   // queries the packed row holds: qlen + 1 <= 128 * 2 entries

EXT_PK_HD inline bool ext_pk_exact(int mx, int mn, int o_del, int e_del, int o_ins, int e_ins, long long hmax, int qmax)
{
	if (qmax < 0 || qmax > EXT_PK_QMAX || hmax < 0) return false;
	if (o_del < 0 || o_ins < 0 || e_del < 1 || e_ins < 1) return false;
	if (o_del > 32767 || o_ins > 32767 || e_del > 32767 || e_ins > 32767) return false;
	if (mx < 0 || mx > 127 || mn < -128) return false;   // (an int8 matrix; mx >= 0 as in the band clamp of ksw.c:400-401)
	if (mn > 0) mn = 0;
	const long long big = (long long)EXT_PK_QMAX * e_ins > mx ? (long long)EXT_PK_QMAX * e_ins : mx;
	if (hmax + big > 32767) return false;
	const int oe = o_ins + e_ins > o_del + e_del ? o_ins + e_ins : o_del + e_del;
	if (oe - mn > 32767) return false;
	return true;
}
// per launch of the region kernels: reads of at most 255 bases, h0 + qlen mx <= l_query max(a, mx) (h0 is a seed's s_len a or the
// score of the left side; the query is what the seed leaves of the read), so the bound depends on the scoring options alone
EXT_PK_HD inline bool ext_pk_exact_reads(int a, int mx, int mn, int o_del, int e_del, int o_ins, int e_ins, int max_read)
{
	const int top = a > mx ? a : mx;
	return max_read <= EXT_PK_QMAX + 1 && a >= 0 && ext_pk_exact(mx, mn, o_del, e_del, o_ins, e_ins, (long long)max_read * top, max_read < EXT_PK_QMAX ? max_read : EXT_PK_QMAX);
}
