// k_msite.hip -- the per-cytosine methylation list (`biscuit pileup` -> `biscuit vcf2bed -t TYPE -k K`, optionally -> `biscuit mergecg`) from the
// counters k_meth.hip keeps: the state is only read, filtered and compacted here, so that only the sites cross to the host.  include/bsx.h
// (bsx_meth_site_t) has the rule.  Tiles as in k_meth_walk: BSX_COV_TILE positions, 256 lanes with 16 consecutive positions each.
//
//   k_msite_count  cnt[i] = the records that belong to tile t_lo + i (and to [f_lo, f_hi)).  A lane counts its own, a wave adds them up, the four
//                  waves meet in LDS.
//   k_msite_emit   the same walk twice per tile that has records (base[i + 1] > base[i], the host's exclusive sums of cnt): once to count -- a
//                  lane's rank in its wave from five ballots, one per bit of its count, the waves' totals exchanged in LDS -- and once to write
//                  the records at base[i] + rank.  No atomics, nothing depends on the order of the launch; a record is two 16-byte vector stores.
//
// A lane reads the 24 bases p0 - 4 .. p0 + 19 into one 64-bit register (the dword of pac with the byte on either side): the five-base context of
// every position p0 - 1 .. p0 + 16 lies in it -- with `merge` the lane also needs the site before its first position (is the G at p0 joined to a
// C?) and the one behind its last (does a G join the C at p0 + 15?), which may lie in the neighbouring tile; the state is padded by a tile of
// zeroes and position -1 is guarded.  Whether the tile, with four positions on either side, touches a contig start or an N hole is found once
// per wave per tile; almost never, and only then a lane searches, once for each of its 24 positions (two 24-bit masks).
// LDS per workgroup: 32 bytes (two sets of four wave totals, used in turn so that a tile needs one barrier).  No scratch.  Built without
// fast-math like k_meth.hip, although nothing here is floating point: the beta and the merged count are made by the host from ret and n.
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "refn.hpp"
#include "kernels.h"

#define MSITE_V 16
#define MSITE_THREADS 256
static_assert(BSX_COV_TILE == MSITE_V * MSITE_THREADS, "a tile is one step of a workgroup");
static_assert(sizeof(bsx_meth_site_t) == 32, "a record is two 16-byte stores");
static_assert(MSITE_V < 32, "a lane's count has five bits");

struct MSite { uint32_t ret, n; int cls; bool kept, isg; };
// a lane's view of its tile: its first position, the bases p0 - 4 .. p0 + 19, and for the same 24 positions (bit j + 4: position p0 + j) which
// have no base -- an N hole, or outside the genome -- and which are the first base of a contig
struct MTile { long long p0; unsigned long long W; uint32_t nobase, start; };

__device__ __forceinline__ int msite_base(unsigned long long W, int j) { return (int)(W >> (46 - 2 * (j + 4))) & 3; }   // the base at p0 + j, -4 <= j <= 19
__device__ __forceinline__ bool msite_ctg_start(const DevIndex &ix, int c0, long long f)   // c0: the first contig offset that can matter
{
	for (int c = c0; c <= ix.n_seqs && ix.ctg_off[c] <= f; ++c) if (ix.ctg_off[c] == f) return true;
	return false;
}

// the site at p0 + j, -1 <= j <= 16
__device__ __forceinline__ MSite msite_eval(const DevIndex &ix, const ulonglong2 *st, const MTile &T, int j, const bsx_meth_site_opt_t &opt)
{
	MSite s;
	const long long f = T.p0 + j;
	const int b = msite_base(T.W, j);
	const uint32_t nb5 = T.nobase >> (j + 2) & 31u, st4 = T.start >> (j + 3) & 15u;   // no base at f - 2 .. f + 2 (bit 2: f itself), a start at f - 1 .. f + 2
	ulonglong2 v = make_ulonglong2(0, 0);
	if (f >= 0 && f < ix.l_pac && (b == 1 || b == 2) && !(nb5 & 4u)) v = st[f];
	const uint32_t ret = (uint32_t)v.x, conv = (uint32_t)(v.x >> 32), oref = (uint32_t)v.y, oalt = (uint32_t)(v.y >> 32), nn = ret + conv;
	const bool site = nn != 0 && (oalt == 0 || 20ull * oalt < (unsigned long long)ret + oref);   // pileup.c:472-484
	const bool full = !nb5 && !st4;   // all of f - 2 .. f + 2 are bases of the site's contig (ctg_off[0] = 0 is a start, l_pac is no base)
	// bisc_utils.c:61-71 on the cytosine's own strand
	const int n1 = b == 1 ? msite_base(T.W, j + 1) : 3 - msite_base(T.W, j - 1), n2 = b == 1 ? msite_base(T.W, j + 2) : 3 - msite_base(T.W, j - 2);
	const int cls = !full ? BSX_METH_CLS_CN : n1 == 2 ? BSX_METH_CLS_CG : n2 == 2 ? BSX_METH_CLS_CHG : BSX_METH_CLS_CHH;
	const bool want = opt.type == BSX_METH_TYPE_C || (opt.type == BSX_METH_TYPE_CG ? cls == BSX_METH_CLS_CG : cls == BSX_METH_CLS_CHG || cls == BSX_METH_CLS_CHH);
	s.ret = ret; s.n = nn; s.cls = cls; s.isg = b == 2;
	s.kept = site && want && nn >= opt.min_cov;
	return s;
}

// the tile's bases and searches for this lane; false: the lane has no position of the genome
__device__ __forceinline__ bool msite_tile(const DevIndex &ix, long long t, int lane, MTile &T)
{
	const long long tb = t * BSX_COV_TILE, te = tb + BSX_COV_TILE < ix.l_pac ? tb + BSX_COV_TILE : ix.l_pac;
	T.p0 = tb + (long long)threadIdx.x * MSITE_V;
	// does the tile, with four positions on either side, touch a contig start or an N hole?  (one search by every wave; almost never)
	const int c0 = wave_count_le(ix.ctg_off, ix.n_seqs + 1, tb - 5, lane);
	const bool ends = c0 <= ix.n_seqs && ix.ctg_off[c0] <= te + 4;
	const int h0 = wave_count_le(ix.hole_end, ix.n_holes, tb - 5, lane);
	const bool holes = h0 < ix.n_holes && ix.hole_off[h0] <= te + 4;
	T.W = 0; T.nobase = T.start = 0;
	if (T.p0 >= ix.l_pac) return false;
	// (the dword and the byte behind it may lie up to four bytes past pac's l_pac / 4 + 1: the device's copy is padded, kernels.h)
	const uint32_t pw = *reinterpret_cast<const uint32_t*>(ix.pac + (T.p0 >> 2));
	const uint32_t before = T.p0 > 0 ? ix.pac[(T.p0 >> 2) - 1] : 0u, behind = ix.pac[(T.p0 >> 2) + 4];
	T.W = (unsigned long long)before << 40 | (unsigned long long)__builtin_bswap32(pw) << 8 | behind;   // the base at p0 + j in bits 47 - 2 (j + 4), 46 - 2 (j + 4)
	if (ends || holes) { // (the same in every lane; a tile without either lies inside the genome with its margins)
#pragma unroll 1
		for (int k = 0; k < 24; ++k) {
			const long long g = T.p0 - 4 + k;
			const bool outside = g < 0 || g >= ix.l_pac;
			if (outside || ctx_in_hole(ix, h0, g)) T.nobase |= 1u << k;
			if (!outside && msite_ctg_start(ix, c0, g)) T.start |= 1u << k;
		}
	}
	return true;
}

// the records that belong to this lane's 16 positions in ascending order: counted, and with `emit` written to out[rank ..] below out[lim]
__device__ __forceinline__ int msite_walk(const DevIndex &ix, const ulonglong2 *st, const MTile &T, const bsx_meth_site_opt_t &opt, long long f_lo, long long f_hi,
                                          bool emit, bsx_meth_site_t *out, uint32_t rank, uint32_t lim)
{
	int c = 0;
	bool pc = false;          // the position before is a kept C (merge only), its counters:
	uint32_t pret = 0, pn = 0;
	const int j0 = opt.merge ? -1 : 0, j1 = opt.merge ? MSITE_V : MSITE_V - 1;
#pragma unroll 1
	for (int j = j0; j <= j1; ++j) {
		const MSite s = msite_eval(ix, st, T, j, opt);
		long long q = -1;     // the position the record belongs to; its two halves
		uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
		if (opt.merge) {
			const bool g = s.kept && s.isg;
			if (pc) { // mergecg.c:206-215: the G behind a C goes into the C's line
				if (j >= 1) { q = T.p0 + j - 1; a.z = pret; a.w = pn; b.x = g ? s.ret : 0u; b.y = g ? s.n : 0u; b.z = BSX_METH_CLS_CG | BSX_METH_SITE_C | (g ? BSX_METH_SITE_G : 0u); }
			} else if (g && j >= 0 && j < MSITE_V) { q = T.p0 + j; b.x = s.ret; b.y = s.n; b.z = (uint32_t)s.cls | BSX_METH_SITE_G; }
			pc = s.kept && !s.isg; pret = s.ret; pn = s.n;
		} else if (s.kept) {
			q = T.p0 + j;
			if (s.isg) { b.x = s.ret; b.y = s.n; } else { a.z = s.ret; a.w = s.n; }
			b.z = (uint32_t)s.cls | (s.isg ? BSX_METH_SITE_G : BSX_METH_SITE_C);
		}
		if (q < f_lo || q >= f_hi) continue;
		if (emit) {
			if (rank + (uint32_t)c < lim) {
				a.x = (uint32_t)q; a.y = (uint32_t)((unsigned long long)q >> 32);
				uint4 *o = reinterpret_cast<uint4*>(out + rank + c);
				o[0] = a; o[1] = b;
			}
		}
		++c;
	}
	return c;
}

__global__ void __launch_bounds__(MSITE_THREADS)
k_msite_count(DevIndex ix, const ulonglong2 *st, bsx_meth_site_opt_t opt, long long f_lo, long long f_hi, long long t_lo, long long nt, uint32_t *cnt)
{
	__shared__ int wsum[2][4];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	int turn = 0;
	for (long long i = blockIdx.x; i < nt; i += gridDim.x, turn ^= 1) {
		MTile T;
		int c = 0;
		if (msite_tile(ix, t_lo + i, lane, T)) c = msite_walk(ix, st, T, opt, f_lo, f_hi, false, nullptr, 0, 0);
		c = wave_sum_i32(c);
		if (lane == 0) wsum[turn][wave] = c;
		__syncthreads();
		if (threadIdx.x == 0) cnt[i] = (uint32_t)(wsum[turn][0] + wsum[turn][1] + wsum[turn][2] + wsum[turn][3]);
	}
}

__global__ void __launch_bounds__(MSITE_THREADS)
k_msite_emit(DevIndex ix, const ulonglong2 *st, bsx_meth_site_opt_t opt, long long f_lo, long long f_hi, long long t_lo, long long nt, const uint32_t *base,
             bsx_meth_site_t *out)
{
	__shared__ int wsum[2][4];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	int turn = 0;
	for (long long i = blockIdx.x; i < nt; i += gridDim.x) {
		const uint32_t b0 = base[i], lim = base[i + 1];
		if (lim <= b0) continue;   // (the same in every lane of the workgroup)
		MTile T;
		const bool have = msite_tile(ix, t_lo + i, lane, T);
		int c = 0, before = 0;   // this lane's records; those of the lanes below it in the workgroup
#pragma unroll 1
		for (int pass = 0; pass < 2; ++pass) { // count, find the lane's place, write
			const int got = have && (pass == 0 || c) ? msite_walk(ix, st, T, opt, f_lo, f_hi, pass == 1, out, b0 + (uint32_t)before, lim) : 0;
			if (pass == 1) break;
			c = got;
			int total = 0;
#pragma unroll
			for (int bit = 0; bit < 5; ++bit) {
				const unsigned long long m = __ballot((c >> bit) & 1);
				before += __popcll(m & ((1ull << lane) - 1)) << bit;
				total += __popcll(m) << bit;
			}
			if (lane == 0) wsum[turn][wave] = total;
			__syncthreads();
			for (int w = 0; w < wave; ++w) before += wsum[turn][w];
			turn ^= 1;
		}
	}
}

static unsigned msite_grid(long long nt, int n_cu) { const long long cap = (long long)n_cu * 8; return (unsigned)(nt < cap ? nt : cap); }

void launch_msite_count(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, const bsx_meth_site_opt_t &opt, long long f_lo, long long f_hi,
                        long long t_lo, long long nt, uint32_t *cnt)
{
	if (nt <= 0) return;
	hipLaunchKernelGGL(k_msite_count, dim3(msite_grid(nt, n_cu)), dim3(MSITE_THREADS), 0, st, ix, (const ulonglong2*)state, opt, f_lo, f_hi, t_lo, nt, cnt);
}

void launch_msite_emit(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, const bsx_meth_site_opt_t &opt, long long f_lo, long long f_hi,
                       long long t_lo, long long nt, const uint32_t *base, bsx_meth_site_t *out)
{
	if (nt <= 0) return;
	hipLaunchKernelGGL(k_msite_emit, dim3(msite_grid(nt, n_cu)), dim3(MSITE_THREADS), 0, st, ix, (const ulonglong2*)state, opt, f_lo, f_hi, t_lo, nt, base, out);
}
