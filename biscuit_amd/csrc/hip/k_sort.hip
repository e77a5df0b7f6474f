// k_sort.hip -- coordinate-sorted output while aligning (--sort): a stable least-significant-digit radix sort of 64-bit keys with a 32-bit
// payload, 8 bits a pass, on wave64.  include/bsx.h (BSX_SORT_KEY, bsx_sort_run, bsx_sort_schedule) has the key and what is sorted; this file has
// the passes.
//
// A tile is BSX_SORT_TILE = 2048 keys, one workgroup of four waves; wave w holds keys [512 w, 512 w + 512) of the tile, eight to a lane, lane l's
// k-th key being key 512 w + 64 k + l (loads are whole cache lines).  The rank of a key among the keys of its tile with the same digit is
//   (keys with that digit in the waves before) + (in this wave's rounds before k) + (in round k, in lower lanes)
// and every term is counted, not raced for: the lanes of a round that share a digit are found with eight ballots (one per bit of the digit), the
// lowest of them adds their number to the wave's own row of counts in LDS, and the rows of the four waves are added up in wave order.  So the
// order of equal digits is the order of the input whatever the schedule: the sort is stable and its output does not depend on timing.
//
// A pass over more than one tile is four launches on one stream:
//   k_sort_hist     counts[digit * n_tiles + tile] = keys of the tile with that digit (LDS counts; one LDS atomic per distinct digit of a round --
//                   additions commute, so the counts do not depend on their order)
//   k_sort_scan1/2  exclusive prefix sums over counts[] in that (digit-major) order: blocks of 2048 counts, then the block totals
//   k_sort_scatter  the ranks as above, plus the tile's prefix: where the key goes.  Every position is (prefix of a count) + (rank below that count),
//                   so it is below n by construction; it is compared with n before the store all the same.
// k_sort_bits ORs key ^ key[0] over all keys: a pass whose byte of that word is zero would move nothing and is not run (genomic keys: contig
// rank in the upper word, position and strand below -- five or six of the eight bytes vary).  Up to one tile, k_sort_small does everything in
// one workgroup: keys and payloads in two LDS buffers, the same ranks, the digits' prefix by one scan over 256 lanes, no HBM between the passes.
// Stores are vector stores; nothing here spills or uses scratch (tests/test_isa_k_sort.py reads the resource lines).
#include <hip/hip_runtime.h>
#include "wave.hpp"
#include "kernels.h"

#define SORT_THREADS 256
#define SORT_WAVES 4
#define SORT_ITEMS 8
#define SORT_TILE (SORT_THREADS * SORT_ITEMS)
#define SORT_WAVE_KEYS (WAVE * SORT_ITEMS)
static_assert(SORT_TILE == BSX_SORT_TILE, "BSX_SORT_TILE");
static_assert(SORT_SCAN_BLOCK == SORT_THREADS * 8, "SORT_SCAN_BLOCK");

typedef unsigned long long u64;
typedef unsigned int u32;

// the lanes of the wave that are `valid` and hold the same 8-bit digit as the caller (called by every lane of the wave)
__device__ __forceinline__ u64 sort_peers(u32 d, bool valid)
{
	u64 m = __ballot(valid);
#pragma unroll
	for (int b = 0; b < 8; ++b) {
		const u64 v = __ballot((d >> b) & 1);
		m &= ((d >> b) & 1) ? v : ~v;
	}
	return m;
}

// exclusive prefix sum of v over the 256 threads of the workgroup (called by all of them); *total = the sum.  wsum: SORT_WAVES words of LDS
__device__ __forceinline__ u32 sort_block_scan(u32 v, u32 *wsum, u32 *total)
{
	const int w = (int)(threadIdx.x >> 6);
	const u32 inc = (u32)wave_scan_sum_incl((int)v);
	u32 base = 0, tot = 0;
	if (wave_lane() == WAVE - 1) wsum[w] = inc;
	__syncthreads();
#pragma unroll
	for (int i = 0; i < SORT_WAVES; ++i) { const u32 s = wsum[i]; if (i < w) base += s; tot += s; }
	__syncthreads();   // (wsum is written again by the next call)
	*total = tot;
	return base + inc - v;
}

__global__ void __launch_bounds__(SORT_THREADS) k_sort_bits(const u64 *keys, u32 n, u64 *bits)
{
	__shared__ u64 acc;
	const u64 k0 = keys[0];
	u64 v = 0;
	if (threadIdx.x == 0) acc = 0;
	__syncthreads();
	for (u64 i = (u64)blockIdx.x * SORT_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * SORT_THREADS) v |= keys[i] ^ k0;
	if (v) atomicOr(&acc, v);   // (OR commutes: the word does not depend on the order)
	__syncthreads();
	if (threadIdx.x == 0 && acc) atomicOr(bits, acc);
}

__global__ void __launch_bounds__(SORT_THREADS) k_sort_hist(const u64 *keys, u32 n, int shift, u32 *counts, u32 n_tiles)
{
	__shared__ u32 hist[256];
	const u32 tile = blockIdx.x, base = tile * SORT_TILE + (threadIdx.x >> 6) * SORT_WAVE_KEYS + (u32)wave_lane();
	const u64 lt = (1ull << wave_lane()) - 1;
	hist[threadIdx.x] = 0;
	__syncthreads();
#pragma unroll
	for (int k = 0; k < SORT_ITEMS; ++k) {
		const u32 i = base + k * WAVE;
		const bool valid = i < n;
		const u32 d = valid ? (u32)(keys[i] >> shift) & 255u : 0u;
		const u64 peers = sort_peers(d, valid);
		if (valid && (peers & lt) == 0) atomicAdd(&hist[d], (u32)__popcll(peers));
	}
	__syncthreads();
	counts[(size_t)threadIdx.x * n_tiles + tile] = hist[threadIdx.x];
}

// counts[] in blocks of SORT_SCAN_BLOCK (n_counts is a multiple of 256, so of a thread's 8): each count becomes the sum of those before it in its
// block, btot[block] = the block's sum
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scan1(u32 *counts, u32 n_counts, u32 *btot)
{
	__shared__ u32 wsum[SORT_WAVES];
	const u32 i0 = blockIdx.x * SORT_SCAN_BLOCK + threadIdx.x * 8;
	uint4 a = make_uint4(0, 0, 0, 0), b = a;
	u32 tot, ex, s;
	if (i0 < n_counts) { a = *(const uint4*)(counts + i0); b = *(const uint4*)(counts + i0 + 4); }
	s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
	ex = sort_block_scan(s, wsum, &tot);
	if (i0 < n_counts) {
		uint4 o, p;
		o.x = ex; o.y = o.x + a.x; o.z = o.y + a.y; o.w = o.z + a.z;
		p.x = o.w + a.w; p.y = p.x + b.x; p.z = p.y + b.y; p.w = p.z + b.z;
		*(uint4*)(counts + i0) = o; *(uint4*)(counts + i0 + 4) = p;
	}
	if (threadIdx.x == 0) btot[blockIdx.x] = tot;
}

// one workgroup: btot[] becomes its exclusive prefix sums
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scan2(u32 *btot, u32 n_blocks)
{
	__shared__ u32 wsum[SORT_WAVES];
	u32 carry = 0;
	for (u32 base = 0; base < n_blocks; base += SORT_THREADS) {
		const u32 i = base + threadIdx.x;
		const u32 v = i < n_blocks ? btot[i] : 0;
		u32 tot;
		const u32 ex = sort_block_scan(v, wsum, &tot);
		if (i < n_blocks) btot[i] = carry + ex;
		carry += tot;
	}
}

// pay_in == nullptr: the payload is the key's index (the first pass of bsx_sort_run)
__global__ void __launch_bounds__(SORT_THREADS)
k_sort_scatter(const u64 *keys_in, const u32 *pay_in, u64 *keys_out, u32 *pay_out, u32 n, int shift, const u32 *counts, const u32 *btot, u32 n_tiles)
{
	__shared__ u32 wcnt[SORT_WAVES][256];
	const u32 tile = blockIdx.x, w = threadIdx.x >> 6, base = tile * SORT_TILE + w * SORT_WAVE_KEYS + (u32)wave_lane();
	const u64 lt = (1ull << wave_lane()) - 1;
	u64 key[SORT_ITEMS];
	u32 rank[SORT_ITEMS];
#pragma unroll
	for (int i = 0; i < SORT_WAVES; ++i) wcnt[i][threadIdx.x] = 0;
	__syncthreads();
#pragma unroll
	for (int k = 0; k < SORT_ITEMS; ++k) {
		const u32 i = base + k * WAVE;
		const bool valid = i < n;
		key[k] = valid ? keys_in[i] : 0;
		const u32 d = (u32)(key[k] >> shift) & 255u;
		const u64 peers = sort_peers(d, valid);
		const u32 before = wcnt[w][d];
		rank[k] = before + (u32)__popcll(peers & lt);
		WAVE_SYNC();   // every lane has read the wave's row before its leaders write it
		if (valid && (peers & lt) == 0) wcnt[w][d] = before + (u32)__popcll(peers);
		WAVE_SYNC();
	}
	__syncthreads();
	{ // lane d: where the keys of this tile with digit d begin, wave by wave
		const size_t ci = (size_t)threadIdx.x * n_tiles + tile;
		u32 g = counts[ci] + btot[ci / SORT_SCAN_BLOCK];
#pragma unroll
		for (int i = 0; i < SORT_WAVES; ++i) { const u32 c = wcnt[i][threadIdx.x]; wcnt[i][threadIdx.x] = g; g += c; }
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < SORT_ITEMS; ++k) {
		const u32 i = base + k * WAVE;
		if (i < n) {
			const u32 pos = wcnt[w][(u32)(key[k] >> shift) & 255u] + rank[k];
			if (pos < n) { keys_out[pos] = key[k]; pay_out[pos] = pay_in ? pay_in[i] : i; }
		}
	}
}

// up to one tile, one workgroup, all eight passes (those that move something) in LDS
__global__ void __launch_bounds__(SORT_THREADS) k_sort_small(const u64 *keys_in, const u32 *pay_in, u64 *keys_out, u32 *pay_out, u32 n)
{
	__shared__ u64 lk[2][SORT_TILE];
	__shared__ u32 lp[2][SORT_TILE];
	__shared__ u32 wcnt[SORT_WAVES][256];
	__shared__ u32 wsum[SORT_WAVES];
	__shared__ u64 acc;
	const u32 w = threadIdx.x >> 6, base = w * SORT_WAVE_KEYS + (u32)wave_lane();
	const u64 lt = (1ull << wave_lane()) - 1;
	int cur = 0;
	u64 bits = 0;
	if (n > SORT_TILE) n = SORT_TILE;   // (the launcher never asks for more)
	if (threadIdx.x == 0) acc = 0;
	__syncthreads();
	{
		const u64 k0 = n ? keys_in[0] : 0;
		for (u32 i = threadIdx.x; i < n; i += SORT_THREADS) { const u64 k = keys_in[i]; lk[0][i] = k; lp[0][i] = pay_in ? pay_in[i] : i; bits |= k ^ k0; }
		if (bits) atomicOr(&acc, bits);
	}
	__syncthreads();
	bits = acc;
	for (int shift = 0; shift < 64; shift += 8) {
		if (((bits >> shift) & 255u) == 0) continue;   // (the same for every thread)
		u64 key[SORT_ITEMS];
		u32 rank[SORT_ITEMS], pay[SORT_ITEMS];
#pragma unroll
		for (int i = 0; i < SORT_WAVES; ++i) wcnt[i][threadIdx.x] = 0;
		__syncthreads();
#pragma unroll
		for (int k = 0; k < SORT_ITEMS; ++k) {
			const u32 i = base + k * WAVE;
			const bool valid = i < n;
			key[k] = valid ? lk[cur][i] : 0;
			pay[k] = valid ? lp[cur][i] : 0;
			const u32 d = (u32)(key[k] >> shift) & 255u;
			const u64 peers = sort_peers(d, valid);
			const u32 before = wcnt[w][d];
			rank[k] = before + (u32)__popcll(peers & lt);
			WAVE_SYNC();
			if (valid && (peers & lt) == 0) wcnt[w][d] = before + (u32)__popcll(peers);
			WAVE_SYNC();
		}
		__syncthreads();
		{
			u32 c[SORT_WAVES], s = 0, tot;
#pragma unroll
			for (int i = 0; i < SORT_WAVES; ++i) { c[i] = wcnt[i][threadIdx.x]; s += c[i]; }
			u32 g = sort_block_scan(s, wsum, &tot);
#pragma unroll
			for (int i = 0; i < SORT_WAVES; ++i) { wcnt[i][threadIdx.x] = g; g += c[i]; }
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < SORT_ITEMS; ++k) {
			const u32 i = base + k * WAVE;
			if (i < n) {
				const u32 pos = wcnt[w][(u32)(key[k] >> shift) & 255u] + rank[k];
				if (pos < n) { lk[cur ^ 1][pos] = key[k]; lp[cur ^ 1][pos] = pay[k]; }
			}
		}
		__syncthreads();
		cur ^= 1;
	}
	for (u32 i = threadIdx.x; i < n; i += SORT_THREADS) { keys_out[i] = lk[cur][i]; pay_out[i] = lp[cur][i]; }
}

size_t sort_n_tiles(long long n) { return (size_t)((n + SORT_TILE - 1) / SORT_TILE); }
size_t sort_n_scan_blocks(long long n) { return (sort_n_tiles(n) * 256 + SORT_SCAN_BLOCK - 1) / SORT_SCAN_BLOCK; }

void launch_sort_bits(hipStream_t st, const unsigned long long *keys, long long n, unsigned long long *bits)
{
	if (n <= 0) return;
	size_t grid = ((size_t)n + SORT_THREADS * 16 - 1) / (SORT_THREADS * 16);
	if (grid > 2048) grid = 2048;
	hipLaunchKernelGGL(k_sort_bits, dim3((unsigned)grid), dim3(SORT_THREADS), 0, st, keys, (u32)n, bits);
}
void launch_sort_pass(hipStream_t st, const unsigned long long *keys_in, const unsigned int *pay_in, unsigned long long *keys_out, unsigned int *pay_out,
                      long long n, int shift, unsigned int *counts, unsigned int *btot)
{
	if (n <= 0) return;
	const u32 n_tiles = (u32)sort_n_tiles(n), n_counts = n_tiles * 256, n_blocks = (u32)sort_n_scan_blocks(n);
	hipLaunchKernelGGL(k_sort_hist, dim3(n_tiles), dim3(SORT_THREADS), 0, st, keys_in, (u32)n, shift, counts, n_tiles);
	hipLaunchKernelGGL(k_sort_scan1, dim3(n_blocks), dim3(SORT_THREADS), 0, st, counts, n_counts, btot);
	hipLaunchKernelGGL(k_sort_scan2, dim3(1), dim3(SORT_THREADS), 0, st, btot, n_blocks);
	hipLaunchKernelGGL(k_sort_scatter, dim3(n_tiles), dim3(SORT_THREADS), 0, st, keys_in, pay_in, keys_out, pay_out, (u32)n, shift, counts, btot, n_tiles);
}
void launch_sort_small(hipStream_t st, const unsigned long long *keys_in, const unsigned int *pay_in, unsigned long long *keys_out, unsigned int *pay_out, long long n)
{
	if (n <= 0 || n > SORT_TILE) return;
	hipLaunchKernelGGL(k_sort_small, dim3(1), dim3(SORT_THREADS), 0, st, keys_in, pay_in, keys_out, pay_out, (u32)n);
}
