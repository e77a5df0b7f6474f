// k_meth.hip -- BISCUITqc's base-averaged conversion table (scripts/QC.sh:423-450: `biscuit pileup` -> `biscuit vcf2bed -e -t c` -> awk) from four
// counters per forward reference position that stay on the device: ret, conv, opp_ref, opp_alt, 32 bits each, as two 64-bit words per position
// (ret | conv << 32, opp_ref | opp_alt << 32), padded with zero entries up to a whole tile past l_pac so that no load of the table pass needs a
// bound.  include/bsx.h (bsx_meth_job_t) has the rule.
//
//   k_meth_add   one wavefront per job, four to a workgroup, a persistent grid.  The wave stages METH_TILE forward reference bases in LDS (4 = an
//                N hole) and walks the CIGAR's M runs that fall into the tile, a lane per column: the read base from the resident read buffer,
//                the quality bit from the job's mask, one 64-bit atomic add per surviving column.  A read of any length goes tile by tile.  A
//                job whose strand tag is neither f nor r takes a counting pass first (ref C / read T against ref G / read A over the columns
//                whose quality bit is set, counted with ballots).
//   k_meth_walk  the table pass, which only reads the state: a tile is BSX_COV_TILE positions, 256 lanes with 16 consecutive positions each, the
//                bases one dword of pac plus the neighbour on either side.  A C or G outside N holes with ret + conv > 0 that is callable is a
//                site: its context from the neighbour (CN where that is a hole or another contig), its beta in thousandths from integer
//                division, a tie decided in IEEE double as printf decides it.  A lane keeps the ten sums (sites and thousandths per context)
//                in registers, a wave adds them to the 64-bit cells every flush_tiles tiles: no 32-bit sum can wrap before.
// Integer sums only: the result does not depend on the order.  Vector stores and atomics only.
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "refn.hpp"
#include "kernels.h"

#define METH_TILE 1024
#define METH_V 16
#define METH_THREADS 256
static_assert(BSX_COV_TILE == METH_V * METH_THREADS, "a tile is one step of a workgroup");
static_assert(sizeof(bsx_meth_job_t) == 56, "bsx_meth_job_t");
// a lane's sum of thousandths grows by at most 16 x 1000 a tile; 64 lanes are summed in a signed 32-bit register
static_assert((long long)METH_FLUSH_TILES_MAX * METH_V * 1000 * 64 < (1ll << 31), "the sums of a wave between two flushes fit 32 bits");

size_t meth_n_tiles(long long l_pac) { return (size_t)((l_pac + BSX_COV_TILE - 1) / BSX_COV_TILE); }
size_t meth_state_entries(long long l_pac) { return (meth_n_tiles(l_pac) + 1) * BSX_COV_TILE; }

// ------------------------------------------------------------------------------------------ columns
__global__ void __launch_bounds__(256)
k_meth_add(DevIndex ix, const uint8_t *reads, long long reads_len, const bsx_meth_job_t *jobs, long long n, const uint32_t *pool, long long pool_len,
           unsigned long long *st)
{
	__shared__ uint8_t stage[4][METH_TILE];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	uint8_t *fx = stage[wave];   // fx[k]: the forward base at reference column t0 + k of the tile that starts at column t0
	for (long long jj = (long long)blockIdx.x * 4 + wave; jj < n; jj += (long long)gridDim.x * 4) {
		const bsx_meth_job_t J = jobs[jj];
		if ((long long)J.cig_off + J.n_cigar > pool_len || (long long)J.qm_off + (J.rlen + 31) / 32 > pool_len) continue;   // (the host has checked the job)
		const uint32_t *cig = pool + J.cig_off, *qm = pool + J.qm_off;
		const int nc = (int)J.n_cigar, rlen = (int)J.rlen;
		const bool rev = J.flags & BSX_QC_REVERSE, read2 = J.flags & BSX_QC_READ2;
		const int tag = (int)BSX_QC_TAG(J.flags);
		int rl;   // reference columns the record spans
		{
			int part = 0;
			for (int k = lane; k < nc; k += 64) { const uint32_t c = cig[k]; const int op = (int)(c & 0xf); part += op == 0 || op == 2 ? (int)(c >> 4) : 0; }
			rl = wave_sum_i32(part);
		}
		const int64_t f0 = J.fpos;
		const int h0 = wave_count_le(ix.hole_end, ix.n_holes, f0, lane);   // does the window touch an N hole?  (one search by the wave; almost never)
		const bool holes = h0 < ix.n_holes && ix.hole_off[h0] < f0 + rl;
		// get_bsstrand (bisc_utils.c:208-238): YD:f 0, YD:r 1, anything else inferred from the record itself at base quality 20
		const int npass = tag != 0 && tag != 1 ? 2 : 1;
		int strand = tag == 1 ? 1 : 0, nC2T = 0, nG2A = 0;
		for (int pass = 0; pass < npass; ++pass) {
			const bool infer = npass == 2 && pass == 0;
			int k = 0, x = 0, y = 0;   // CIGAR word, position in the whole read as the record has it, reference column: the same in every lane
			for (int t0 = 0; t0 < rl; t0 += METH_TILE) {
				const int t1 = t0 + METH_TILE < rl ? t0 + METH_TILE : rl;
				WAVE_SYNC();   // the tile before has been read
				for (int i = lane; i < t1 - t0; i += 64) {
					const int64_t f = f0 + t0 + i;
					int b = 4;
					if (f >= 0 && f < ix.l_pac) b = dev_ref_base(ix.pac, ix.l_pac, f);
					if (b < 4 && holes && ctx_in_hole(ix, h0, f)) b = 4;
					fx[i] = (uint8_t)b;
				}
				WAVE_SYNC();
				while (k < nc) {
					const uint32_t cg = (uint32_t)__builtin_amdgcn_readfirstlane((int)cig[k]);
					const int op = (int)(cg & 0xf), len = (int)(cg >> 4);
					if (op == 0) {
						if (y >= t1) break;
						const int lo = y > t0 ? y : t0, hi = y + len < t1 ? y + len : t1;
						for (int c0 = lo; c0 < hi; c0 += 64) {
							const int c = c0 + lane;
							const int qp = x + (c - y);
							bool ok = c < hi && qp < rlen;
							if (ok) ok = qm[qp >> 5] >> (qp & 31) & 1;   // pileup.c:380, bisc_utils.c:180
							int r = 4, q = 4;
							if (ok) {
								r = fx[c - t0];
								const long long at = (long long)J.roff + (rev ? rlen - 1 - qp : qp) - J.rskip;
								if (at >= 0 && at < reads_len) q = reads[at];
								if (rev) q = q < 4 ? 3 - q : 4;
							}
							if (infer) {
								nC2T += __popcll(__ballot(r == 1 && q == 3));
								nG2A += __popcll(__ballot(r == 2 && q == 0));
							} else if ((r == 1 || r == 2) && qp + 1 > 3 && rlen >= qp + 1 + 3) {   // pileup.c:383
								const int64_t f = f0 + c;
								const bool own = r == (strand ? 2 : 1), ref = q == r, alt = q == (r == 1 ? 3 : 0);
								if ((ref || alt) && !(read2 && f >= J.ov_beg && f < J.ov_end) && f >= 0 && f < ix.l_pac)   // pileup.c:773-778
									atomicAdd(&st[2 * f + (own ? 0 : 1)], alt ? 1ull << 32 : 1ull);
							}
						}
						if (y + len > t1) break;   // the run goes on in the next tile
						x += len; y += len; ++k;
					} else if (op == 2) { y += len; ++k; }
					else { x += len; ++k; }   // I, S, H: read bases without a column
				}
			}
			if (infer) strand = nC2T >= nG2A ? 0 : 1;   // infer_bsstrand, bisc_utils.c:204
		}
	}
}

void launch_meth_add(hipStream_t st, const DevIndex &ix, const uint8_t *reads, long long reads_len, const bsx_meth_job_t *jobs, long long n,
                     const uint32_t *pool, long long pool_len, void *state, int n_cu)
{
	if (n <= 0) return;
	const long long want = (n + 3) / 4, cap = (long long)n_cu * 8;
	hipLaunchKernelGGL(k_meth_add, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, ix, reads, reads_len, jobs, n, pool, pool_len,
	                   (unsigned long long*)state);
}

// ------------------------------------------------------------------------------------------ the table pass
// the integer printf("%1.3f", (double)r / (double)n) shows, times 1000 (0 <= r <= n, n > 0): bsx_meth_milli of meth.c
__device__ __forceinline__ uint32_t meth_milli(uint32_t r, uint32_t n)
{
	uint32_t m0;
	unsigned long long rem;
	if (r < 4000000u) { const uint32_t num = 1000u * r; m0 = num / n; rem = num - m0 * n; }
	else { const unsigned long long num = 1000ull * r; m0 = (uint32_t)(num / n); rem = num - (unsigned long long)m0 * n; }
	if (2 * rem < n) return m0;
	if (2 * rem > n) return m0 + 1;
	const double d = (double)r / (double)n, e = fma(d, (double)n, -(double)r);   // IEEE division and fma: this file is built without fast-math
	return e > 0 ? m0 + 1 : e < 0 ? m0 : (m0 & 1) ? m0 + 1 : m0;
}
__device__ __forceinline__ bool meth_ctg_start(const DevIndex &ix, int c0, long long f)   // c0: the first contig offset at or beyond the tile's start
{
	for (int c = c0; c <= ix.n_seqs && ix.ctg_off[c] <= f; ++c) if (ix.ctg_off[c] == f) return true;
	return false;
}
__device__ __forceinline__ int meth_base(uint32_t pw, int k) { return (int)(pw >> (8 * (k >> 2) + ((~k & 3) << 1))) & 3; }

__global__ void __launch_bounds__(METH_THREADS)
k_meth_walk(DevIndex ix, const ulonglong2 *st, long long n_tiles, int flush_tiles, unsigned long long *out)
{
	const int lane = wave_lane();
	const long long l_pac = ix.l_pac;
	uint32_t K[BSX_METH_N_CTX], S[BSX_METH_N_CTX];
	int since = 0;
#pragma unroll
	for (int x = 0; x < BSX_METH_N_CTX; ++x) K[x] = S[x] = 0;
	for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const long long tb = t * BSX_COV_TILE, p0 = tb + (long long)threadIdx.x * METH_V;
		// does the tile, with the one position on either side, touch a contig start or an N hole?  (one search by every wave; almost never)
		const long long te = tb + BSX_COV_TILE < l_pac ? tb + BSX_COV_TILE : l_pac;
		const int c0 = wave_count_le(ix.ctg_off, ix.n_seqs + 1, tb - 1, lane);
		const bool ends = c0 <= ix.n_seqs && ix.ctg_off[c0] <= te;
		const int h0 = wave_count_le(ix.hole_end, ix.n_holes, tb - 1, lane);
		const bool holes = h0 < ix.n_holes && ix.hole_off[h0] <= te;
		if (p0 < l_pac) { // (the dword and the byte behind it may lie up to four bytes past pac's l_pac / 4 + 1: the device's copy is padded, kernels.h)
			const uint32_t pw = *reinterpret_cast<const uint32_t*>(ix.pac + (p0 >> 2));
			const int pn = ix.pac[(p0 >> 2) + 4] >> 6, pp = p0 > 0 ? ix.pac[(p0 >> 2) - 1] & 3 : 0;   // the bases at p0 + 16 and at p0 - 1
#pragma unroll
			for (int k = 0; k < METH_V; ++k) {
				const long long f = p0 + k;
				const int b = meth_base(pw, k);
				if (f >= l_pac || (b != 1 && b != 2)) continue;
				const ulonglong2 v = st[f];
				const uint32_t ret = (uint32_t)v.x, conv = (uint32_t)(v.x >> 32), oref = (uint32_t)v.y, oalt = (uint32_t)(v.y >> 32), nn = ret + conv;
				if (!nn || (holes && ctx_in_hole(ix, h0, f))) continue;
				if (oalt && !(20ull * oalt < (unsigned long long)ret + oref)) continue;   // pileup.c:472-484
				int ctx = 4;   // the next base on the cytosine's own strand; CN: an N hole, or no base of this contig
				if (b == 1) {
					const int nb = k + 1 < METH_V ? meth_base(pw, k + 1) : pn;
					if (f + 1 < l_pac && !(ends && meth_ctg_start(ix, c0, f + 1)) && !(holes && ctx_in_hole(ix, h0, f + 1))) ctx = nb;
				} else {
					const int nb = k > 0 ? meth_base(pw, k - 1) : pp;
					if (f > 0 && !(ends && meth_ctg_start(ix, c0, f)) && !(holes && ctx_in_hole(ix, h0, f - 1))) ctx = 3 - nb;
				}
				const uint32_t m = meth_milli(ret, nn);
#pragma unroll
				for (int x = 0; x < BSX_METH_N_CTX; ++x) { K[x] += ctx == x ? 1u : 0u; S[x] += ctx == x ? m : 0u; }
			}
		}
		if (++since >= flush_tiles || t + gridDim.x >= n_tiles) {   // (`since` and t are the same in every lane)
#pragma unroll
			for (int x = 0; x < BSX_METH_N_CTX; ++x) {
				const int k = wave_sum_i32((int)K[x]), s = wave_sum_i32((int)S[x]);
				if (lane == 0 && k) { atomicAdd(&out[x], (unsigned long long)k); atomicAdd(&out[BSX_METH_N_CTX + x], (unsigned long long)s); }
				K[x] = S[x] = 0;
			}
			since = 0;
		}
	}
}

void launch_meth_tables(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, long long n_tiles, int flush_tiles, unsigned long long *out)
{
	if (n_tiles <= 0) return;
	const long long cap = (long long)n_cu * 8;
	hipLaunchKernelGGL(k_meth_walk, dim3((unsigned)(n_tiles < cap ? n_tiles : cap)), dim3(METH_THREADS), 0, st, ix, (const ulonglong2*)state, n_tiles,
	                   flush_tiles, out);
}
