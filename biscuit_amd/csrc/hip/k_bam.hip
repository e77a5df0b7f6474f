// k_bam.hip -- SAM lines -> BAM records (--bam, stage 1; DESIGN.md section 7, include/bsx.h bsx_bam_encode).  The record rule itself is
// csrc/host/bam_rec.h, compiled here for the device: the host's statement and this one are the same source, so they cannot drift apart.
// k_msite's count / emit shape:
//
//   k_bam_count   cnt[t] = the newlines of tile t (BAM_TILE bytes: 256 lanes x 16 bytes, one 16-byte load each, a 16-bit newline mask per
//                 lane, a wave sum, the four waves meet in LDS)
//   k_bam_scan    exclusive sums of up to 2^31 32-bit counts by ONE workgroup (1024 lanes, a carry from trip to trip): a million counts are a
//                 thousand trips, far below the passes around it, and nothing depends on the order workgroups run in
//   k_bam_starts  the same walk as k_bam_count: a lane's rank in its wave by a wave scan, the waves' totals exchanged in LDS; the newline with
//                 global rank r gives start[r + 1]
//   k_bam_lines   a lane per line, both passes: bam_rec_encode without a buffer gives the record's length and, by a store, its refusal code;
//                 with out = payload + off[line], off the exclusive sums of the sizes, the same function writes the record
//   k_bam_refused the first refused line of every 256 (64-bit LDS atomicMin over line << 4 | code) into bad[]; the host takes the least
//
// A lane per line -- not a quarter-wave or a wave per line: the rule is a serial parse with data-dependent field boundaries (tabs, CIGAR
// numbers, tag types), a record is ~350 bytes, and a chunk has a million lines, four thousand per compute unit, so lanes are never short of
// work; a wave per line would spend most of its lanes waiting on the one that parses.  The price is byte-wide stores that do not coalesce
// within a wave; they meet in L2, the stage is a few per cent of a chunk's kernels (profiles/bam_measurements.md).  RNAME and RNEXT go
// through the sorted name table the host uploads once per writer (binary search, bam_ref_find).  No HBM atomics, vector stores only, no
// scratch: bam_rec.h indexes its field table with constants only.
#include <hip/hip_runtime.h>
#include "wave.hpp"
#include "kernels.h"
#define BAM_FN __device__ __forceinline__
#include "bam_rec.h"

#define BAM_THREADS 256
#define BAM_TILE 4096
#define BAM_SCAN_THREADS 1024
static_assert(BAM_TILE == BAM_THREADS * 16, "a lane takes 16 bytes of its tile");

// the newline mask of the 16 bytes at p0 (bit j: text[p0 + j] == '\n'), bytes at or beyond len masked off
__device__ __forceinline__ uint32_t bam_nl_mask(const char *text, long long len, long long p0)
{
	uint32_t m = 0;
	if (p0 >= len) return 0;
	if (p0 + 16 <= len) {
		const uint4 v = *reinterpret_cast<const uint4*>(text + p0);   // (the text starts on a 16-byte boundary: the shim's buffer)
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int k = 0; k < 4; ++k)
#pragma unroll
			for (int b = 0; b < 4; ++b) if (((w[k] >> (8 * b)) & 255u) == '\n') m |= 1u << (4 * k + b);
	} else for (int j = 0; p0 + j < len; ++j) if (text[p0 + j] == '\n') m |= 1u << j;
	return m;
}

__global__ void __launch_bounds__(BAM_THREADS)
k_bam_count(const char *text, long long len, long long n_tiles, uint32_t *cnt)
{
	__shared__ int wsum[2][4];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	int turn = 0;
	for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x, turn ^= 1) {
		int c = __popc(bam_nl_mask(text, len, t * BAM_TILE + (long long)threadIdx.x * 16));
		c = wave_sum_i32(c);
		if (lane == 0) wsum[turn][wave] = c;
		__syncthreads();
		if (threadIdx.x == 0) cnt[t] = (uint32_t)(wsum[turn][0] + wsum[turn][1] + wsum[turn][2] + wsum[turn][3]);
	}
}

// out[i] = in[0] + .. + in[i - 1] for i <= n (out has n + 1 entries; in and out may be the same array)
__global__ void __launch_bounds__(BAM_SCAN_THREADS)
k_bam_scan(const uint32_t *in, uint32_t *out, long long n)
{
	__shared__ uint32_t wtot[BAM_SCAN_THREADS / 64];
	__shared__ uint32_t carry_s;
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for (long long base = 0; base < n; base += BAM_SCAN_THREADS) {
		const long long i = base + threadIdx.x;
		const uint32_t v = i < n ? in[i] : 0u;
		const uint32_t incl = (uint32_t)wave_scan_sum_incl((int)v);
		if (lane == 63) wtot[wave] = incl;
		__syncthreads();
		uint32_t before = carry;
		for (int w = 0; w < wave; ++w) before += wtot[w];
		if (i < n) out[i] = before + incl - v;
		if (threadIdx.x == BAM_SCAN_THREADS - 1) carry_s = before + incl;
		__syncthreads();
		carry = carry_s;
	}
	if (threadIdx.x == 0) out[n] = carry;
}

__global__ void __launch_bounds__(BAM_THREADS)
k_bam_starts(const char *text, long long len, long long n_tiles, const uint32_t *base, uint32_t *start)
{
	__shared__ int wsum[2][4];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	int turn = 0;
	if (blockIdx.x == 0 && threadIdx.x == 0) start[0] = 0;
	for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x, turn ^= 1) {
		const long long p0 = t * BAM_TILE + (long long)threadIdx.x * 16;
		uint32_t m = bam_nl_mask(text, len, p0);
		const int c = __popc(m), incl = wave_scan_sum_incl(c);
		if (lane == 63) wsum[turn][wave] = incl;
		__syncthreads();
		uint32_t r = base[t] + (uint32_t)(incl - c);
		for (int w = 0; w < wave; ++w) r += (uint32_t)wsum[turn][w];
		while (m) { const int j = __ffs(m) - 1; m &= m - 1; start[++r] = (uint32_t)(p0 + j + 1); }
	}
}

struct BamTab { const char *names; const uint32_t *off; const int32_t *id; int32_t n; };

// one kernel for both passes -- out == nullptr: size[i] = the record's length (0 for a refused line), errs[i] = 0 or the refusal code; else the
// record at out + off[i].  Both reach memory by stores inside the parse, not as results: a result live at every early exit of the parse costs
// a mask per exit, more scalar registers than there are.
__global__ void __launch_bounds__(BAM_THREADS)
k_bam_lines(const char *text, const uint32_t *start, long long n_lines, BamTab tab, uint32_t *size, int *errs, const uint32_t *off, uint8_t *out)
{
	bam_reftab_t T;
	T.names = tab.names; T.off = tab.off; T.id = tab.id; T.n = tab.n;
	const long long i = (long long)blockIdx.x * BAM_THREADS + threadIdx.x;   // (no loop over lines: see bam_lines_grid)
	if (i >= n_lines) return;
	const uint32_t a = start[i], l = start[i + 1] - a - 1;   // (without the newline)
	(void)bam_rec_encode(text + a, l, &T, out ? out + off[i] : nullptr, errs + i, out ? nullptr : size + i);
}

// bad[w] = the least (line << 4 | code) among the refused lines of workgroup w's BAM_THREADS lines, all ones for none
__global__ void __launch_bounds__(BAM_THREADS)
k_bam_refused(const int *errs, long long n_lines, unsigned long long *bad)
{
	__shared__ unsigned long long first_bad;
	if (threadIdx.x == 0) first_bad = ~0ull;
	__syncthreads();
	const long long i = (long long)blockIdx.x * BAM_THREADS + threadIdx.x;
	if (i < n_lines) {
		const int e = errs[i];
		if (e) atomicMin(&first_bad, (unsigned long long)i << 4 | (unsigned long long)(e & 15));   // (LDS)
	}
	__syncthreads();
	if (threadIdx.x == 0) bad[blockIdx.x] = first_bad;
}

static unsigned bam_grid(long long n, int n_cu, int per) { const long long want = (n + per - 1) / per, cap = (long long)n_cu * 8; return (unsigned)(want < 1 ? 1 : want < cap ? want : cap); }

long long bam_n_tiles(long long len) { return (len + BAM_TILE - 1) / BAM_TILE; }
// a lane takes ONE line: a loop around the parse makes the compiler keep its constants live across it, beyond the scalar registers
int bam_lines_grid(long long n_lines) { const long long g = (n_lines + BAM_THREADS - 1) / BAM_THREADS; return (int)(g < 1 ? 1 : g); }

void launch_bam_count(hipStream_t st, int n_cu, const char *text, long long len, uint32_t *cnt)
{
	const long long nt = bam_n_tiles(len);
	if (nt <= 0) return;
	hipLaunchKernelGGL(k_bam_count, dim3(bam_grid(nt, n_cu, 1)), dim3(BAM_THREADS), 0, st, text, len, nt, cnt);
}
void launch_bam_scan(hipStream_t st, const uint32_t *in, uint32_t *out, long long n)
{
	hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(BAM_SCAN_THREADS), 0, st, in, out, n);
}
void launch_bam_starts(hipStream_t st, int n_cu, const char *text, long long len, const uint32_t *base, uint32_t *start)
{
	const long long nt = bam_n_tiles(len);
	if (nt <= 0) return;
	hipLaunchKernelGGL(k_bam_starts, dim3(bam_grid(nt, n_cu, 1)), dim3(BAM_THREADS), 0, st, text, len, nt, base, start);
}
void launch_bam_size(hipStream_t st, const char *text, const uint32_t *start, long long n_lines, const char *names, const uint32_t *noff,
                     const int32_t *nid, int n_names, uint32_t *size, int *errs, unsigned long long *bad)
{
	const BamTab tab = {names, noff, nid, n_names};
	hipLaunchKernelGGL(k_bam_lines, dim3(bam_lines_grid(n_lines)), dim3(BAM_THREADS), 0, st, text, start, n_lines, tab, size, errs, (const uint32_t*)nullptr,
	                   (uint8_t*)nullptr);
	hipLaunchKernelGGL(k_bam_refused, dim3(bam_lines_grid(n_lines)), dim3(BAM_THREADS), 0, st, (const int*)errs, n_lines, bad);
}
void launch_bam_emit(hipStream_t st, const char *text, const uint32_t *start, long long n_lines, const char *names, const uint32_t *noff,
                     const int32_t *nid, int n_names, int *errs, const uint32_t *off, uint8_t *out)
{
	const BamTab tab = {names, noff, nid, n_names};
	if (n_lines <= 0) return;
	hipLaunchKernelGGL(k_bam_lines, dim3(bam_lines_grid(n_lines)), dim3(BAM_THREADS), 0, st, text, start, n_lines, tab, (uint32_t*)nullptr, errs, off, out);
}
