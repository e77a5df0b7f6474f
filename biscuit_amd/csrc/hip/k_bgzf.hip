// k_bgzf.hip -- the uncompressed BAM stream -> BGZF blocks (--bam, stage 2; DESIGN.md section 7, include/bsx.h bsx_bgzf_deflate): a whole
// deflate coder -- LZ77 matches, dynamic Huffman codes, CRC32, the gzip member around them -- per 0xff00-byte block, one workgroup of 256 lanes
// per block, the block and its match table in LDS (138 848 bytes of the 163 840, declared statically: one workgroup per compute unit).
//
//   1  the block into LDS (16-byte loads), the table zeroed
//   2  match candidates in ordered phases of 256 positions: every lane looks up the head of its position's 3-byte hash -- the table then
//      holds exactly the positions before the phase -- and notes the candidate (16 bits, in an HBM workspace); after a barrier the phase's
//      positions enter the table with LDS atomicMax, so a head is the LARGEST earlier position with that hash whichever lane wrote last.  A
//      candidate further back than 32768 is dropped.  Positions of the same phase (distance below 256) are not candidates of each other;
//      the distance-1 run, where quality strings live, is checked directly in step 3
//   3  greedy parse: lane i owns the 255 bytes that END at n - (255 - i) * 255 (the leading lanes of a short block own nothing) and parses
//      them against the whole block behind: the longer of the run and the candidate, at least 3, at most 258 and not beyond the segment's end
//      (segments stay disjoint, so nothing depends on a neighbour's parse), and only when its estimated bits -- 7 for the length code, 5 for the
//      distance code, their extra bits -- are fewer than those of the literals it replaces (step 1b: log2(n / count) per byte value from the
//      block's own counts, at least one bit; without this a block of few byte values would pay 20 bits for matches its 2-bit literals beat).  Tokens go to the lane's row of an HBM workspace, symbol counts
//      to LDS histograms (integer adds: order-free)
//   4  code lengths by wave 0, nodes in registers (nine per lane): n - 1 times the two lightest nodes by wave min over weight << 10 | index
//      (ties by index: deterministic), depths by walking the parent links; deeper than 15: every weight halved (rounded up) and again
//   5  canonical codes, bit-reversed (lane 0).  The code-length header sends all 286 + 30 lengths literally through a flat 4-bit code for
//      the lengths 0 .. 15 (no repeat codes): 1338 header bits, 0.26 % of a full block
//   6  every lane adds up its tokens' bits; an exclusive sum over the lanes gives each its bit offset
//   7  packing into LDS (the table's room) with atomicOr on 32-bit words: order-free.  If the coded stream would not beat it, the block is
//      one stored deflate block instead (n + 5 bytes)
//   8  CRC32: a lane over its segment (byte table in LDS), combined pairwise up a tree with the zero-byte shift operators of crc32_combine
//      (GF(2) 32 x 32 matrices for 255 << level bytes, made by the host once); an empty segment has CRC 0, which the operators keep
//   9  the member -- 18 header bytes, the stream, CRC32, ISIZE -- into the block's 64 KiB slot; k_bgzf_compact then moves every member to its
//      final offset (exclusive sums of the sizes, k_bam_scan), so that one contiguous copy crosses to the host
//
// No HBM atomics; nothing depends on the order workgroups or lanes run in; vector stores only; no scratch.
#include <hip/hip_runtime.h>
#include "wave.hpp"
#include "kernels.h"

#define BGZF_THREADS 256
#define BGZF_SEG 255
#define BGZF_MAX 0xff00
#define BGZF_HASH_BITS 14
#define BGZF_NLIT 286
#define BGZF_NDIST 30
#define BGZF_DBASE 288                 // where the distance symbols start in freq / clen / code
#define BGZF_HDR_BITS (3 + 5 + 5 + 4 + 19 * 3 + (BGZF_NLIT + BGZF_NDIST) * 4)
#define BGZF_NOCAND 0xffffu
#define BGZF_LAUNCH_MAX 1024             // blocks of one launch: the workspaces are per workgroup (384 KiB each)
static_assert(BGZF_THREADS * BGZF_SEG == BGZF_MAX, "the lanes' segments tile a full block");
static_assert(BGZF_HDR_BITS == 1338, "header bits");

struct BgzfLds {
	uint8_t data[BGZF_MAX + 16];                 // the block, zero behind its end
	uint32_t table[1 << BGZF_HASH_BITS];         // hash heads (position + 1); later the packed stream
	uint32_t freq[320];
	uint16_t par[640];
	uint8_t clen[320];
	uint16_t code[320];
	uint32_t crc_tab[256];
	uint32_t lbits[BGZF_THREADS], lcnt[BGZF_THREADS], lcrc[BGZF_THREADS];
	uint32_t blc[16], nxt[16];
	uint32_t wtot[4];
	uint8_t lcost[256];                          // what a literal of each byte value is taken to cost, in half bits
};
static_assert(sizeof(BgzfLds) <= 160 * 1024, "LDS of one compute unit");
static_assert(sizeof(uint32_t) * (1 << BGZF_HASH_BITS) >= BGZF_MAX + 5 + 8, "the packed stream fits the table's room");

__device__ __forceinline__ uint32_t bgzf_hash(const uint8_t *p)
{
	const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
	return (v * 0x9E3779B1u) >> (32 - BGZF_HASH_BITS);
}
// length 3..258 -> symbol, extra bits
__device__ __forceinline__ void bgzf_len_sym(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
	const uint32_t x = len - 3;
	if (x < 8) { sym = 257 + x; eb = 0; ev = 0; }
	else if (x == 255) { sym = 285; eb = 0; ev = 0; }
	else { const uint32_t e = 31 - __clz(x) - 2; sym = 261 + 4 * e + ((x >> e) & 3); eb = e; ev = x & ((1u << e) - 1); }
}
// distance - 1 (0..32767) -> symbol, extra bits
__device__ __forceinline__ void bgzf_dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
	if (d < 4) { sym = d; eb = 0; ev = 0; }
	else { const uint32_t e = 31 - __clz(d) - 1; sym = 2 * e + 2 + ((d >> e) & 1); eb = e; ev = d & ((1u << e) - 1); }
}
// 2 log2(v) rounded down to an integer, v >= 1 below 2^16
__device__ __forceinline__ int bgzf_log2x2(uint32_t v) { const int m = 31 - __clz(v); return 2 * m + (v * v >= (2u << (2 * m)) ? 1 : 0); }
__device__ __forceinline__ void bgzf_put(uint32_t *buf, uint32_t pos, uint32_t value, uint32_t nbits)
{
	if (!nbits) return;
	const unsigned long long v = (unsigned long long)value << (pos & 31);
	atomicOr(&buf[pos >> 5], (uint32_t)v);
	if (v >> 32) atomicOr(&buf[(pos >> 5) + 1], (uint32_t)(v >> 32));
}

// code lengths of NS symbols with weights f[0 .. NS) into clen[0 .. NS), at most 15 bits; the whole of wave 0, every lane active
template<int NS> __device__ __forceinline__ void bgzf_lengths(int lane, const uint32_t *f, uint16_t *par, uint8_t *clen)
{
	constexpr int NSLOT = (2 * NS + 63) / 64, LSLOT = (NS + 63) / 64;
	constexpr uint32_t INF = 0xffffffffu;
	uint32_t lw[LSLOT];
	int used = 0, only = -1;
#pragma unroll
	for (int k = 0; k < LSLOT; ++k) { const int i = k * 64 + lane; lw[k] = i < NS ? f[i] : 0u; if (lw[k]) { ++used; only = i; } }
	used = wave_sum_i32(used);
	only = wave_max_i32(only);
#pragma unroll
	for (int k = 0; k < LSLOT; ++k) { const int i = k * 64 + lane; if (i < NS) clen[i] = 0; }
	if (used == 0) return;
	if (used == 1) { if (lane == 0) clen[only] = 1; return; }   // (one code of one bit: an incomplete code inflate accepts)
	for (;;) {
		uint32_t w[NSLOT];
#pragma unroll
		for (int k = 0; k < NSLOT; ++k) w[k] = k < LSLOT && lw[k < LSLOT ? k : 0] ? lw[k < LSLOT ? k : 0] : INF;
		for (int m = 0; m < used - 1; ++m) {
			int key[2];
#pragma unroll
			for (int r = 0; r < 2; ++r) {
				int best = 0x7fffffff;
#pragma unroll
				for (int k = 0; k < NSLOT; ++k) { const int c = w[k] == INF ? 0x7fffffff : (int)(w[k] << 10 | (uint32_t)(k * 64 + lane)); best = c < best ? c : best; }
				key[r] = wave_min_i32(best);
				const int idx = key[r] & 1023;
#pragma unroll
				for (int k = 0; k < NSLOT; ++k) if (k * 64 + lane == idx) w[k] = INF;
			}
			const int nu = NS + m;
#pragma unroll
			for (int k = 0; k < NSLOT; ++k) if (k * 64 + lane == nu) w[k] = (uint32_t)(key[0] >> 10) + (uint32_t)(key[1] >> 10);
			if (lane == 0) { par[key[0] & 1023] = (uint16_t)nu; par[key[1] & 1023] = (uint16_t)nu; }
		}
		WAVE_SYNC();
		const int root = NS + used - 2;
		int maxd = 0;
#pragma unroll
		for (int k = 0; k < LSLOT; ++k) {
			const int i = k * 64 + lane;
			int d = 0;
			if (i < NS && lw[k]) { int v = i; while (v != root) { v = par[v]; ++d; } clen[i] = (uint8_t)(d > 255 ? 255 : d); }
			maxd = d > maxd ? d : maxd;
		}
		maxd = wave_max_i32(maxd);
		WAVE_SYNC();
		if (maxd <= 15) return;
#pragma unroll
		for (int k = 0; k < LSLOT; ++k) if (lw[k]) lw[k] = (lw[k] + 1) >> 1;   // flatter, and again
	}
}

// canonical codes of clen[0 .. ns) into code[], bit-reversed for the LSB-first stream; one lane
__device__ __forceinline__ void bgzf_codes(int ns, const uint8_t *clen, uint16_t *code, uint32_t *blc, uint32_t *nxt)
{
	for (int b = 0; b < 16; ++b) blc[b] = 0;
	for (int i = 0; i < ns; ++i) ++blc[clen[i]];
	uint32_t c = 0;
	blc[0] = 0;
	for (int b = 1; b < 16; ++b) { c = (c + blc[b - 1]) << 1; nxt[b] = c; }
	for (int i = 0; i < ns; ++i) {
		const uint32_t l = clen[i];
		code[i] = l ? (uint16_t)(__brev(nxt[l]++) >> (32 - l)) : (uint16_t)0;
	}
}

__global__ void __launch_bounds__(BGZF_THREADS)
k_bgzf_deflate(const uint8_t *payload, long long len, long long b0, const uint32_t *crc_ops, uint32_t *ws_tok, uint16_t *ws_cand, uint8_t *slots, uint32_t *sizes)
{
	__shared__ __align__(16) BgzfLds S;
	const int tid = threadIdx.x, lane = wave_lane(), wave = tid >> 6;
	uint32_t *tok = ws_tok + ((size_t)blockIdx.x * BGZF_THREADS + tid) * 256;
	uint16_t *cand = ws_cand + (size_t)blockIdx.x * 65536;
	{ // (one block per workgroup and no loop over blocks: the compiler would keep every address of the body live around it, beyond the scalar registers)
		const long long b = b0 + blockIdx.x;
		const uint8_t *src = payload + b * BGZF_MAX;
		const int n = (int)(len - b * BGZF_MAX < BGZF_MAX ? len - b * BGZF_MAX : BGZF_MAX);
		uint8_t *slot = slots + (size_t)b * 65536;
		// 1
		for (int i = tid * 16; i < n + 16; i += BGZF_THREADS * 16) {
			if (i + 16 <= n) *reinterpret_cast<uint4*>(S.data + i) = *reinterpret_cast<const uint4*>(src + i);
			else for (int j = 0; j < 16; ++j) S.data[i + j] = i + j < n ? src[i + j] : (uint8_t)0;
		}
		for (int i = tid; i < (1 << BGZF_HASH_BITS); i += BGZF_THREADS) S.table[i] = 0;
		for (int i = tid; i < 320; i += BGZF_THREADS) { S.freq[i] = 0; S.clen[i] = 0; S.code[i] = 0; }
		{ uint32_t c = (uint32_t)tid; for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1; S.crc_tab[tid] = c; }
		__syncthreads();
		// 1b: what a literal costs, from the block's byte counts (log2(n / count), at least one bit); the counts are then cleared for step 3
		for (int i = tid; i < n; i += BGZF_THREADS) atomicAdd(&S.freq[S.data[i]], 1u);
		__syncthreads();
		{
			const uint32_t f = S.freq[tid];
			const int c = f ? bgzf_log2x2((uint32_t)n) - bgzf_log2x2(f) : 30;
			S.lcost[tid] = (uint8_t)(c < 2 ? 2 : c > 30 ? 30 : c);
			S.freq[tid] = 0;
		}
		__syncthreads();
		// 2
		for (int base = 0; base < n; base += BGZF_THREADS) {
			const int p = base + tid;
			const bool valid = p + 3 <= n;
			uint32_t h = 0;
			if (valid) {
				h = bgzf_hash(S.data + p);
				const uint32_t c = S.table[h];
				cand[p] = (uint16_t)(c && (uint32_t)p - (c - 1) <= 32768u ? c - 1 : BGZF_NOCAND);
			} else if (p < n) cand[p] = (uint16_t)BGZF_NOCAND;
			__syncthreads();
			if (valid) atomicMax(&S.table[h], (uint32_t)p + 1);
			__syncthreads();
		}
		// 3  (cand[] was written by the lane of each position and is read here by the lane that owns the segment: the exchange goes through
		//     global memory and rests on __syncthreads() -- the last one of step 2 -- ordering global accesses too at workgroup scope)
		const int seg_e = n - (BGZF_THREADS - 1 - tid) * BGZF_SEG > 0 ? n - (BGZF_THREADS - 1 - tid) * BGZF_SEG : 0;
		const int seg_s = seg_e - BGZF_SEG > 0 ? seg_e - BGZF_SEG : 0;
		uint32_t n_tok = 0;
		for (int p = seg_s; p < seg_e; ) {
			const int maxl = seg_e - p < 258 ? seg_e - p : 258;
			int best = 0, dist = 0;
			if (maxl >= 3) {
				if (p >= 1 && S.data[p] == S.data[p - 1]) { int l = 1; while (l < maxl && S.data[p + l] == S.data[p + l - 1]) ++l; best = l; dist = 1; }
				const uint32_t c = cand[p];
				if (c != BGZF_NOCAND && best < maxl) { int l = 0; while (l < maxl && S.data[c + l] == S.data[p + l]) ++l; if (l > best) { best = l; dist = p - (int)c; } }
			}
			uint32_t ls = 0, ds = 0, eb, ev;
			if (best >= 3) { // worth it?  A length code is taken as 7 bits, a distance code as 5, plus their extra bits, against the literals' costs
				uint32_t lit2 = 0, ebl;
				for (int j = 0; j < best; ++j) lit2 += S.lcost[S.data[p + j]];
				bgzf_len_sym((uint32_t)best, ls, ebl, ev);
				bgzf_dist_sym((uint32_t)dist - 1, ds, eb, ev);
				if (2 * (12 + ebl + eb) >= lit2) best = 0;
			}
			if (best >= 3) {
				atomicAdd(&S.freq[ls], 1u); atomicAdd(&S.freq[BGZF_DBASE + ds], 1u);
				tok[n_tok++] = 0x80000000u | (uint32_t)(best - 3) << 16 | (uint32_t)(dist - 1);
				p += best;
			} else { const uint32_t v = S.data[p]; atomicAdd(&S.freq[v], 1u); tok[n_tok++] = v; ++p; }
		}
		S.lcnt[tid] = n_tok;
		if (tid == 0) S.freq[256] = 1;   // end of block
		__syncthreads();
		// 4, 5
		if (wave == 0) {
			bgzf_lengths<BGZF_NLIT>(lane, S.freq, S.par, S.clen);
			bgzf_lengths<BGZF_NDIST>(lane, S.freq + BGZF_DBASE, S.par, S.clen + BGZF_DBASE);
			WAVE_SYNC();
			if (lane == 0) { bgzf_codes(BGZF_NLIT, S.clen, S.code, S.blc, S.nxt); bgzf_codes(BGZF_NDIST, S.clen + BGZF_DBASE, S.code + BGZF_DBASE, S.blc, S.nxt); }
		}
		__syncthreads();
		// 6
		uint32_t bits = 0;
		for (uint32_t k = 0; k < n_tok; ++k) {
			const uint32_t t = tok[k];
			if (t & 0x80000000u) {
				uint32_t s, eb, ev;
				bgzf_len_sym(((t >> 16) & 255u) + 3, s, eb, ev); bits += S.clen[s] + eb;
				bgzf_dist_sym(t & 0x7fffu, s, eb, ev); bits += S.clen[BGZF_DBASE + s] + eb;
			} else bits += S.clen[t];
		}
		const uint32_t incl = (uint32_t)wave_scan_sum_incl((int)bits);
		if (lane == 63) S.wtot[wave] = incl;
		for (int i = tid; i < (1 << BGZF_HASH_BITS); i += BGZF_THREADS) S.table[i] = 0;   // the stream's room
		__syncthreads();
		uint32_t pos = BGZF_HDR_BITS + incl - bits;
		for (int w = 0; w < wave; ++w) pos += S.wtot[w];
		const uint32_t body_bits = S.wtot[0] + S.wtot[1] + S.wtot[2] + S.wtot[3];
		const uint32_t total_bits = BGZF_HDR_BITS + body_bits + S.clen[256];
		const uint32_t n_coded = (total_bits + 7) >> 3;
		const bool stored = n_coded >= (uint32_t)n + 5;
		const uint32_t n_raw = stored ? (uint32_t)n + 5 : n_coded;
		// 7
		if (!stored) {
			if (tid == 0) {
				static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
				bgzf_put(S.table, 0, 1u | 2u << 1, 3);                           // BFINAL, BTYPE 2
				bgzf_put(S.table, 3, BGZF_NLIT - 257, 5); bgzf_put(S.table, 8, BGZF_NDIST - 1, 5); bgzf_put(S.table, 13, 19 - 4, 4);
				for (int k = 0; k < 19; ++k) bgzf_put(S.table, 17 + 3 * k, order[k] < 16 ? 4u : 0u, 3);
				bgzf_put(S.table, BGZF_HDR_BITS + body_bits, S.code[256], S.clen[256]);
			}
			for (int i = tid; i < BGZF_NLIT + BGZF_NDIST; i += BGZF_THREADS) { // a length l is the 4-bit code l, most significant bit first
				const uint32_t l = S.clen[i < BGZF_NLIT ? i : BGZF_DBASE + i - BGZF_NLIT];
				bgzf_put(S.table, 17 + 57 + 4 * i, __brev(l) >> 28, 4);
			}
			for (uint32_t k = 0; k < n_tok; ++k) {
				const uint32_t t = tok[k];
				if (t & 0x80000000u) {
					uint32_t s, eb, ev;
					bgzf_len_sym(((t >> 16) & 255u) + 3, s, eb, ev);
					bgzf_put(S.table, pos, S.code[s], S.clen[s]); pos += S.clen[s];
					bgzf_put(S.table, pos, ev, eb); pos += eb;
					bgzf_dist_sym(t & 0x7fffu, s, eb, ev);
					bgzf_put(S.table, pos, S.code[BGZF_DBASE + s], S.clen[BGZF_DBASE + s]); pos += S.clen[BGZF_DBASE + s];
					bgzf_put(S.table, pos, ev, eb); pos += eb;
				} else { bgzf_put(S.table, pos, S.code[t], S.clen[t]); pos += S.clen[t]; }
			}
		}
		// 8
		{
			uint32_t c = 0xffffffffu;
			for (int p = seg_s; p < seg_e; ++p) c = S.crc_tab[(c ^ S.data[p]) & 255u] ^ (c >> 8);
			S.lcrc[tid] = c ^ 0xffffffffu;
		}
		__syncthreads();
		for (int lev = 0; lev < 8; ++lev) {
			const int stride = 1 << lev;
			if ((tid & (2 * stride - 1)) == 0) {
				const uint32_t *M = crc_ops + lev * 32;
				uint32_t v = S.lcrc[tid], r = 0;
				for (int k = 0; v; ++k, v >>= 1) if (v & 1) r ^= M[k];
				S.lcrc[tid] = r ^ S.lcrc[tid + stride];
			}
			__syncthreads();
		}
		// 9
		const uint32_t total = 18 + n_raw + 8;
		if (tid < 18) {
			static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
			slot[tid] = tid < 16 ? head[tid] : (uint8_t)((total - 1) >> (8 * (tid - 16)));
		}
		if (stored) {
			if (tid < 5) slot[18 + tid] = tid == 0 ? (uint8_t)1 : tid == 1 ? (uint8_t)n : tid == 2 ? (uint8_t)(n >> 8) : tid == 3 ? (uint8_t)~n : (uint8_t)(~n >> 8);
			for (int i = tid; i < n; i += BGZF_THREADS) slot[23 + i] = S.data[i];
		} else {
			const uint8_t *z = reinterpret_cast<const uint8_t*>(S.table);
			for (uint32_t i = tid; i < n_raw; i += BGZF_THREADS) slot[18 + i] = z[i];
		}
		if (tid < 8) { const uint32_t v = tid < 4 ? S.lcrc[0] : (uint32_t)n; slot[18 + n_raw + tid] = (uint8_t)(v >> (8 * (tid & 3))); }
		if (tid == 0) sizes[b] = total;
	}
}

// every member from its slot to its final offset
__global__ void __launch_bounds__(BGZF_THREADS)
k_bgzf_compact(const uint8_t *slots, const uint32_t *off, long long n_blocks, uint8_t *out)
{
	for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
		const uint8_t *s = slots + (size_t)b * 65536;
		uint8_t *o = out + off[b];
		const uint32_t n = off[b + 1] - off[b];
		for (uint32_t i = threadIdx.x; i < n; i += BGZF_THREADS) o[i] = s[i];
	}
}

size_t bgzf_lds_bytes(void) { return sizeof(BgzfLds); }
int bgzf_grid(long long n_blocks) { return (int)(n_blocks < BGZF_LAUNCH_MAX ? (n_blocks < 1 ? 1 : n_blocks) : BGZF_LAUNCH_MAX); }   // blocks, and workgroups, of one launch
size_t bgzf_tok_bytes(int grid) { return (size_t)grid * BGZF_THREADS * 256 * 4; }
size_t bgzf_cand_bytes(int grid) { return (size_t)grid * 65536 * 2; }

// the operators of step 8: ops[lev * 32 + k] = column k of the matrix that appends 255 << lev zero bytes to a CRC32 (crc32_combine's)
static uint32_t gf2_times(const uint32_t *m, uint32_t v) { uint32_t r = 0; for (int k = 0; v; ++k, v >>= 1) if (v & 1) r ^= m[k]; return r; }
static void gf2_mul(uint32_t *c, const uint32_t *a, const uint32_t *b) { uint32_t t[32]; for (int k = 0; k < 32; ++k) t[k] = gf2_times(a, b[k]); for (int k = 0; k < 32; ++k) c[k] = t[k]; }
void bgzf_crc_ops(uint32_t *ops)
{
	uint32_t bit[32], byte[32], acc[32];
	bit[0] = 0xedb88320u;
	for (int k = 1; k < 32; ++k) bit[k] = 1u << (k - 1);
	for (int k = 0; k < 32; ++k) byte[k] = bit[k];
	for (int s = 0; s < 3; ++s) gf2_mul(byte, byte, byte);     // 2, 4, 8 zero bits
	for (int k = 0; k < 32; ++k) acc[k] = 1u << k;
	{ uint32_t p[32]; for (int k = 0; k < 32; ++k) p[k] = byte[k]; for (int e = BGZF_SEG; e; e >>= 1) { if (e & 1) gf2_mul(acc, p, acc); gf2_mul(p, p, p); } }   // 255 bytes
	for (int lev = 0; lev < 8; ++lev) { for (int k = 0; k < 32; ++k) ops[lev * 32 + k] = acc[k]; gf2_mul(acc, acc, acc); }
}

void launch_bgzf_deflate(hipStream_t st, const uint8_t *payload, long long len, long long b0, int n_launch, const uint32_t *crc_ops, uint32_t *ws_tok,
                        uint16_t *ws_cand, uint8_t *slots, uint32_t *sizes)
{
	hipLaunchKernelGGL(k_bgzf_deflate, dim3(n_launch), dim3(BGZF_THREADS), 0, st, payload, len, b0, crc_ops, ws_tok, ws_cand, slots, sizes);
}
void launch_bgzf_compact(hipStream_t st, int n_cu, const uint8_t *slots, const uint32_t *off, long long n_blocks, uint8_t *out)
{
	const long long cap = (long long)n_cu * 4;
	hipLaunchKernelGGL(k_bgzf_compact, dim3((unsigned)(n_blocks < cap ? n_blocks : cap)), dim3(BGZF_THREADS), 0, st, slots, off, n_blocks, out);
}
