// k_cov.hip -- the BISCUITqc coverage tables (scripts/QC.sh:136-421: `bedtools genomecov -bga -split`, the CpG intersect with `groupby -o min`, the
// twelve awk histograms) from a depth state that stays on the device: a difference array over forward concatenated coordinates, l_pac + 1 entries
// of two signed 32-bit classes (x: every record, y: records with MAPQ >= 40), padded with zero entries up to a whole tile past the last one so
// that no load below needs a bound.
//
//   k_cov_add    a lane per job (bsx_qc_job_t with BSX_QC_COV): +1 at the first column of every run of M columns, -1 one past its last
//   k_cov_paint  the intervals of a top / bottom GC mask into l_pac bits
//   the tables   four launches that only read the state, none of whose workgroups waits for another:
//                k_cov_sums (a tile's differences summed), k_cov_scan (one workgroup: the tile sums into carries), k_cov_walk<false> (every tile
//                scanned from its carry, the largest `all` depth), k_cov_walk<true> (scanned again, every position and every CpG counted)
//
// A tile is BSX_COV_TILE positions: 256 lanes with 16 consecutive positions each (eight 16-byte loads, the reference bases one dword of pac, the
// mask bits half a word), one more entry / base / bit beyond the lane's last position, so that a CpG is counted by the lane -- and the tile --
// that holds its C.  Histograms of a workgroup are 32-bit counters in LDS for depths below lds_bins; deeper positions go to the 64-bit bins in
// HBM directly.  A workgroup keeps its histograms over all the tiles it takes and adds its non-zero cells to the bins at the end, one atomic per
// cell, and before a cell could wrap.  Integer sums only: the result does not depend on the order.
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "refn.hpp"
#include "kernels.h"

#define COV_V 16
#define COV_THREADS 256
static_assert(BSX_COV_TILE == COV_V * COV_THREADS, "a tile is one step of a workgroup");
static_assert(sizeof(bsx_qc_job_t) == 32, "bsx_qc_job_t");

size_t cov_n_tiles(long long l_pac) { return (size_t)((l_pac + BSX_COV_TILE - 1) / BSX_COV_TILE); }
size_t cov_diff_entries(long long l_pac) { return (cov_n_tiles(l_pac) + 1) * BSX_COV_TILE; }
size_t cov_mask_words(long long l_pac) { return cov_diff_entries(l_pac) / 32 + 2; }

// ------------------------------------------------------------------------------------------ events
__device__ __forceinline__ void cov_emit(int *diff, long long l_pac, long long s, long long e, bool q40)
{
	s = s < 0 ? 0 : s; e = e > l_pac ? l_pac : e;   // (the host has checked the job; never outside the array all the same)
	if (s >= e) return;
	atomicAdd(&diff[2 * s], 1); atomicAdd(&diff[2 * e], -1);
	if (q40) { atomicAdd(&diff[2 * s + 1], 1); atomicAdd(&diff[2 * e + 1], -1); }
}

__global__ void __launch_bounds__(COV_THREADS)
k_cov_add(int *diff, long long l_pac, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool, long long pool_len)
{
	for (long long i = (long long)blockIdx.x * COV_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * COV_THREADS) {
		const bsx_qc_job_t J = jobs[i];
		if (!(J.flags & BSX_QC_COV) || (long long)J.cig_off + J.n_cigar > pool_len) continue;
		const bool q40 = J.flags & BSX_QC_COV_Q40;
		const uint32_t *cig = pool + J.cig_off;
		long long y = J.fpos, rs = 0, re = 0;   // the run of M columns being gathered: I, S and H do not end it, D does
		for (uint32_t k = 0; k < J.n_cigar; ++k) {
			const uint32_t c = cig[k];
			const int op = (int)(c & 0xf);
			const long long len = (long long)(c >> 4);
			if (op == 0) {
				if (re == y && rs < re) re = y + len;
				else { cov_emit(diff, l_pac, rs, re, q40); rs = y; re = y + len; }
				y += len;
			} else if (op == 2) y += len;
		}
		cov_emit(diff, l_pac, rs, re, q40);
	}
}

void launch_cov_add(hipStream_t st, int n_cu, void *diff, long long l_pac, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool, long long pool_len)
{
	if (n <= 0) return;
	const long long want = (n + COV_THREADS - 1) / COV_THREADS, cap = (long long)n_cu * 8;
	hipLaunchKernelGGL(k_cov_add, dim3((unsigned)(want < cap ? want : cap)), dim3(COV_THREADS), 0, st, (int*)diff, l_pac, jobs, n, pool, pool_len);
}

// ------------------------------------------------------------------------------------------ masks
// bit (p & 31) of word p >> 5 stands for position p.  A workgroup per interval, a lane per word: words inside are stored whole (other intervals
// can only set bits of them), the first and the last word are shared with the neighbours' bits
__global__ void __launch_bounds__(COV_THREADS)
k_cov_paint(uint32_t *mask, long long l_pac, const long long *beg_end, long long n)
{
	for (long long i = blockIdx.x; i < n; i += gridDim.x) {
		long long b = beg_end[2 * i], e = beg_end[2 * i + 1];
		b = b < 0 ? 0 : b; e = e > l_pac ? l_pac : e;
		if (b >= e) continue;
		const long long wb = b >> 5, we = (e - 1) >> 5;
		for (long long w = wb + threadIdx.x; w <= we; w += COV_THREADS) {
			uint32_t m = ~0u;
			if (w == wb) m &= ~0u << (b & 31);
			if (w == we) m &= ~0u >> (31 - ((e - 1) & 31));
			if (w == wb || w == we) atomicOr(&mask[w], m);
			else mask[w] = ~0u;
		}
	}
}

void launch_cov_paint(hipStream_t st, int n_cu, uint32_t *mask, long long l_pac, const long long *beg_end, long long n)
{
	if (n <= 0) return;
	const long long cap = (long long)n_cu * 8;
	hipLaunchKernelGGL(k_cov_paint, dim3((unsigned)(n < cap ? n : cap)), dim3(COV_THREADS), 0, st, mask, l_pac, beg_end, n);
}

// ------------------------------------------------------------------------------------------ the final passes
// the lane's 16 entries of the tile at p0 (a multiple of 16)
__device__ __forceinline__ void cov_load(const int2 *diff, long long p0, int2 (&d)[COV_V])
{
	const int4 *src = reinterpret_cast<const int4*>(diff + p0);
#pragma unroll
	for (int k = 0; k < COV_V / 2; ++k) { const int4 v = src[k]; d[2 * k] = make_int2(v.x, v.y); d[2 * k + 1] = make_int2(v.z, v.w); }
}
__device__ __forceinline__ int2 cov_sum(const int2 (&d)[COV_V])
{
	int2 s = make_int2(0, 0);
#pragma unroll
	for (int k = 0; k < COV_V; ++k) { s.x += d[k].x; s.y += d[k].y; }
	return s;
}
// exclusive prefix of `mine` over the workgroup's NW waves (ws: NW cells of LDS), `total` = the sum over all of them
template <int NW>
__device__ __forceinline__ int2 cov_block_excl(int2 mine, int2 *ws, int2 &total)
{
	const int lane = wave_lane(), wave = (int)(threadIdx.x >> 6);
	const int ix_ = wave_scan_sum_incl(mine.x), iy_ = wave_scan_sum_incl(mine.y);
	if (lane == 63) ws[wave] = make_int2(ix_, iy_);
	__syncthreads();
	int2 base = make_int2(0, 0);
	total = make_int2(0, 0);
#pragma unroll
	for (int w = 0; w < NW; ++w) { const int2 v = ws[w]; if (w < wave) { base.x += v.x; base.y += v.y; } total.x += v.x; total.y += v.y; }
	__syncthreads();   // ws is written again by the next call
	return make_int2(base.x + ix_ - mine.x, base.y + iy_ - mine.y);
}

__global__ void __launch_bounds__(COV_THREADS)
k_cov_sums(const int2 *diff, long long n_tiles, int2 *tsum)
{
	__shared__ int2 ws[4];
	for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		int2 d[COV_V], total;
		cov_load(diff, t * BSX_COV_TILE + (long long)threadIdx.x * COV_V, d);
		(void)cov_block_excl<4>(cov_sum(d), ws, total);
		if (threadIdx.x == 0) tsum[t] = total;
	}
}

// tsum[t] := the sum of the tiles before t: one workgroup, 1024 tiles a step
__global__ void __launch_bounds__(1024)
k_cov_scan(int2 *tsum, long long n_tiles)
{
	__shared__ int2 ws[16];
	int2 run = make_int2(0, 0);
	for (long long b = 0; b < n_tiles; b += 1024) {
		const long long t = b + threadIdx.x;
		const int2 v = t < n_tiles ? tsum[t] : make_int2(0, 0);
		int2 total;
		const int2 ex = cov_block_excl<16>(v, ws, total);
		if (t < n_tiles) tsum[t] = make_int2(run.x + ex.x, run.y + ex.y);
		run.x += total.x; run.y += total.y;
	}
}

__device__ __forceinline__ void cov_count(uint32_t *hist, int lds_bins, unsigned long long *bins, long long nb, int tb, int d)
{
	if (d < 0) return;   // (no valid job makes one)
	if (d < lds_bins) atomicAdd(&hist[tb * lds_bins + d], 1u);
	else if (d < nb) atomicAdd(&bins[(long long)tb * nb + d], 1ull);
}
__device__ __forceinline__ void cov_count_pair(uint32_t *hist, int lds_bins, unsigned long long *bins, long long nb, int region, int kind, int2 d)
{
	cov_count(hist, lds_bins, bins, nb, region * 4 + kind, d.x);
	cov_count(hist, lds_bins, bins, nb, region * 4 + 2 + kind, d.y);
}
// the workgroup's non-zero cells added to the bins and zeroed
__device__ __forceinline__ void cov_flush(uint32_t *hist, int n_cells, int lds_bins, unsigned long long *bins, long long nb)
{
	__syncthreads();
	for (int i = threadIdx.x; i < n_cells; i += COV_THREADS) {
		const uint32_t v = hist[i];
		const int tb = i / lds_bins, d = i - tb * lds_bins;
		if (v && d < nb) atomicAdd(&bins[(long long)tb * nb + d], (unsigned long long)v);
		hist[i] = 0;
	}
	__syncthreads();
}
__device__ __forceinline__ bool cov_ctg_start(const DevIndex &ix, int c0, long long f)   // c0: the first contig offset beyond the tile's start
{
	for (int c = c0; c <= ix.n_seqs && ix.ctg_off[c] <= f; ++c) if (ix.ctg_off[c] == f) return true;
	return false;
}

// COUNT = false: *gmax = the largest `all` depth of any position; COUNT = true: the twelve (four without masks) histograms
template <bool COUNT>
__global__ void __launch_bounds__(COV_THREADS)
k_cov_walk(DevIndex ix, const int2 *diff, const int2 *carry, long long n_tiles, const uint32_t *m_top, const uint32_t *m_bot, int lds_bins,
           int flush_tiles, unsigned long long *bins, long long nb, int *gmax)
{
	__shared__ uint32_t hist[COUNT ? BSX_COV_N_TABLES * COV_LDS_BINS_MAX : 1];
	__shared__ int2 ws[4];
	const int lane = wave_lane();
	const bool gc = m_top != nullptr;
	const int n_cells = (gc ? BSX_COV_N_TABLES : 4) * lds_bins;
	const long long l_pac = ix.l_pac;
	int vmax = 0, since = 0;
	if (COUNT) {
		for (int i = threadIdx.x; i < n_cells; i += COV_THREADS) hist[i] = 0;
		__syncthreads();
	}
	for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const long long tb = t * BSX_COV_TILE, p0 = tb + (long long)threadIdx.x * COV_V;
		int2 d[COV_V], total;
		cov_load(diff, p0, d);
		const int2 halo = diff[p0 + COV_V];
		const int2 ex = cov_block_excl<4>(cov_sum(d), ws, total), cin = carry[t];
		int2 dep = make_int2(cin.x + ex.x, cin.y + ex.y);   // the depth of position p0 - 1
		if (!COUNT) {
#pragma unroll
			for (int k = 0; k < COV_V; ++k) { dep.x += d[k].x; if (p0 + k < l_pac && dep.x > vmax) vmax = dep.x; }
			continue;
		}
		// does the tile, with the one position beyond it, touch a contig start or an N hole?  (one search by every wave; almost never)
		const long long te = tb + BSX_COV_TILE < l_pac ? tb + BSX_COV_TILE : l_pac;
		const int c0 = wave_count_le(ix.ctg_off, ix.n_seqs + 1, tb, lane);
		const bool ends = c0 <= ix.n_seqs && ix.ctg_off[c0] <= te;
		const int h0 = wave_count_le(ix.hole_end, ix.n_holes, tb, lane);
		const bool holes = h0 < ix.n_holes && ix.hole_off[h0] <= te;
		uint32_t pw = 0, pn = 0, bt = 0, bb = 0;   // the lane's 16 bases, the next base, its 17 bits of either mask
		if (p0 < l_pac) { // (the dword and the byte behind it may lie up to four bytes past pac's l_pac / 4 + 1: the device's copy is padded, kernels.h)
			pw = *reinterpret_cast<const uint32_t*>(ix.pac + (p0 >> 2));
			pn = ix.pac[(p0 >> 2) + 4] >> 6;
			if (gc) {
				const int sh = (int)(p0 & 16);
				bt = (uint32_t)((((unsigned long long)m_top[(p0 >> 5) + 1] << 32 | m_top[p0 >> 5]) >> sh) & 0x1ffff);
				bb = (uint32_t)((((unsigned long long)m_bot[(p0 >> 5) + 1] << 32 | m_bot[p0 >> 5]) >> sh) & 0x1ffff);
			}
		}
#pragma unroll
		for (int k = 0; k < COV_V; ++k) {
			dep.x += d[k].x; dep.y += d[k].y;
			const long long f = p0 + k;
			if (f >= l_pac) continue;
			const int2 nx = k + 1 < COV_V ? d[k + 1] : halo;
			const bool top = bt >> k & 1, bot = bb >> k & 1;
			cov_count_pair(hist, lds_bins, bins, nb, 0, 0, dep);
			if (top) cov_count_pair(hist, lds_bins, bins, nb, 1, 0, dep);
			if (bot) cov_count_pair(hist, lds_bins, bins, nb, 2, 0, dep);
			const int b = (int)(pw >> (8 * (k >> 2) + ((~k & 3) << 1))) & 3;
			const int b1 = k + 1 < COV_V ? (int)(pw >> (8 * ((k + 1) >> 2) + ((~(k + 1) & 3) << 1))) & 3 : (int)pn;
			bool cpg = b == 1 && b1 == 2 && f + 1 < l_pac;
			if (cpg && ends) cpg = !cov_ctg_start(ix, c0, f + 1);
			if (cpg && holes) cpg = !ctx_in_hole(ix, h0, f) && !ctx_in_hole(ix, h0, f + 1);
			if (cpg) {
				const int2 m = make_int2(dep.x + (nx.x < 0 ? nx.x : 0), dep.y + (nx.y < 0 ? nx.y : 0));   // min(depth[f], depth[f + 1])
				cov_count_pair(hist, lds_bins, bins, nb, 0, 1, m);
				if (top || (bt >> (k + 1) & 1)) cov_count_pair(hist, lds_bins, bins, nb, 1, 1, m);
				if (bot || (bb >> (k + 1) & 1)) cov_count_pair(hist, lds_bins, bins, nb, 2, 1, m);
			}
		}
		if (++since >= flush_tiles) { cov_flush(hist, n_cells, lds_bins, bins, nb); since = 0; }   // (`since` is the same in every lane)
	}
	if (COUNT) cov_flush(hist, n_cells, lds_bins, bins, nb);
	else {
		vmax = wave_max_i32(vmax);
		if (lane == 0 && vmax > 0) atomicMax(gmax, vmax);
	}
}

static unsigned cov_grid(long long n_tiles, int n_cu) { const long long cap = (long long)n_cu * 4; return (unsigned)(n_tiles < cap ? n_tiles : cap); }

void launch_cov_sums(hipStream_t st, int n_cu, const void *diff, long long n_tiles, void *tsum)
{
	if (n_tiles <= 0) return;
	hipLaunchKernelGGL(k_cov_sums, dim3(cov_grid(n_tiles, n_cu * 2)), dim3(COV_THREADS), 0, st, (const int2*)diff, n_tiles, (int2*)tsum);
	hipLaunchKernelGGL(k_cov_scan, dim3(1), dim3(1024), 0, st, (int2*)tsum, n_tiles);
}
void launch_cov_max(hipStream_t st, int n_cu, const DevIndex &ix, const void *diff, const void *carry, long long n_tiles, int *gmax)
{
	if (n_tiles <= 0) return;
	hipLaunchKernelGGL(k_cov_walk<false>, dim3(cov_grid(n_tiles, n_cu * 2)), dim3(COV_THREADS), 0, st, ix, (const int2*)diff, (const int2*)carry, n_tiles,
	                   (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0, 0, (unsigned long long*)nullptr, 0ll, gmax);
}
void launch_cov_count(hipStream_t st, int n_cu, const DevIndex &ix, const void *diff, const void *carry, long long n_tiles, const uint32_t *m_top,
                      const uint32_t *m_bot, int lds_bins, int flush_tiles, unsigned long long *bins, long long nb)
{
	if (n_tiles <= 0) return;
	hipLaunchKernelGGL(k_cov_walk<true>, dim3(cov_grid(n_tiles, n_cu)), dim3(COV_THREADS), 0, st, ix, (const int2*)diff, (const int2*)carry, n_tiles,
	                   m_top, m_bot, lds_bins, flush_tiles, bins, nb, (int*)nullptr);
}
