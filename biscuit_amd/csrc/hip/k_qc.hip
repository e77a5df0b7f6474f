// k_qc.hip -- the column counts of `biscuit qc` (src/qc.c:112-179) over records as they are written: bsstrand_func (src/bsstrand.c:60-168),
// cinread_func for the targets CG and CH (src/cinread.c:50-187) and the totals of bsconv_func (src/bsconv.c:63-109); bsx_qc_job_t in
// include/bsx.h has what a job carries.  No DP here: a job is a walk of the record's final CIGAR over the read (resident since the chunk's
// upload) and the forward reference.
//
// One wavefront per job, four to a workgroup, a persistent grid.  The wave stages QC_TILE forward reference bases plus one neighbour on each
// side in LDS (4 = no base there: an N hole or beyond the contig, found as in k_global's counts by context) and walks the CIGAR's M runs
// that fall into the tile, a lane per column; a read of any length goes tile by tile, nothing in HBM.  C>T and G>A columns are counted with
// ballots.  The marks need the record's strand first: YD:f / YD:r records are marked in the same pass, a YD:u record takes a second pass
// once its own nC2T / nG2A are known.  All histograms of the workgroup -- the read-position table, the eight conversion totals, the
// confusion cells -- are 32-bit counters in LDS; at the end of the block its non-zero cells are added to the device's 64-bit table, one
// atomic per cell per block.  Integer sums: the result does not depend on the order.
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "refn.hpp"
#include "kernels.h"

#define QC_TILE 1024
#define QC_POS (2 * 2 * BSX_QC_READ_LEN * 2)   // cells of the read-position table; then conv[8], confusion[16]: bsx_qc_counts_t's order
#define QC_CELLS (QC_POS + 8 + 16)
static_assert(sizeof(bsx_qc_counts_t) == (size_t)QC_CELLS * 8, "the LDS counters mirror bsx_qc_counts_t");
static_assert(sizeof(bsx_qc_job_t) == 32, "bsx_qc_job_t");

__global__ void __launch_bounds__(256)
k_qc(DevIndex ix, const uint8_t *reads, long long reads_len, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool, unsigned long long *table)
{
	__shared__ uint32_t cnt[QC_CELLS];
	__shared__ uint8_t stage[4][QC_TILE + 8];
	const int lane = wave_lane(), wave = threadIdx.x >> 6;
	uint8_t *fx = stage[wave];   // fx[k]: the forward base at reference column t0 - 1 + k of the tile that starts at column t0
	uint32_t *pos = cnt, *cv = cnt + QC_POS, *cf = cnt + QC_POS + 8;
	for (int i = threadIdx.x; i < QC_CELLS; i += blockDim.x) cnt[i] = 0;
	__syncthreads();
	for (long long jj = (long long)blockIdx.x * 4 + wave; jj < n; jj += (long long)gridDim.x * 4) {
		const bsx_qc_job_t J = jobs[jj];
		const uint32_t *cig = pool + J.cig_off;
		const int nc = (int)J.n_cigar, rlen = (int)J.rlen;
		const bool rev = J.flags & BSX_QC_REVERSE;
		const int read2 = J.flags & BSX_QC_READ2 ? 1 : 0, tag = (int)BSX_QC_TAG(J.flags);
		const bool cin = J.flags & BSX_QC_CINREAD, bsc = J.flags & BSX_QC_BSCONV, marks = cin || bsc;
		int rl;   // reference columns the record spans
		{
			int part = 0;
			for (int k = lane; k < nc; k += 64) { const uint32_t c = cig[k]; const int op = (int)(c & 0xf); part += op == 0 || op == 2 ? (int)(c >> 4) : 0; }
			rl = wave_sum_i32(part);
		}
		// does the window with its two neighbours touch a contig end or an N hole?  (one search by the wave; almost never)
		const int64_t f0 = J.fpos, wlo = f0 - 1, whi = f0 + rl;
		int ci = wave_count_le(ix.ctg_off, ix.n_seqs + 1, f0, lane) - 1;
		ci = ci < 0 ? 0 : ci > ix.n_seqs - 1 ? ix.n_seqs - 1 : ci;
		const int64_t cb = ix.ctg_off[ci], ce = ix.ctg_off[ci + 1];
		const int h0 = wave_count_le(ix.hole_end, ix.n_holes, wlo, lane);
		const bool holes = h0 < ix.n_holes && ix.hole_off[h0] <= whi;
		const bool special = holes || wlo < cb || whi >= ce;
		// get_bsstrand (bisc_utils.c:208-238): YD:f 0, YD:r 1, anything else inferred from the record itself
		const int npass = marks && tag != 0 && tag != 1 ? 2 : 1;
		int strand = tag == 1 ? 1 : 0, nC2T = 0, nG2A = 0;
		for (int pass = 0; pass < npass; ++pass) {
			const bool count = pass == 0, mark = marks && pass == npass - 1;
			int k = 0, x = 0, y = 0;   // CIGAR word, position in the whole read as the record has it, reference column: the same in every lane
			for (int t0 = 0; t0 < rl; t0 += QC_TILE) {
				const int t1 = t0 + QC_TILE < rl ? t0 + QC_TILE : rl;
				WAVE_SYNC();   // the tile before has been read
				for (int i = lane; i < t1 - t0 + 2; i += 64) {
					const int64_t f = f0 + t0 - 1 + i;
					int b = 4;
					if (f >= 0 && f < ix.l_pac) b = dev_ref_base(ix.pac, ix.l_pac, f);
					if (b < 4 && special && (f < cb || f >= ce || (holes && ctx_in_hole(ix, h0, f)))) b = 4;
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
							const bool act = c < hi;
							const int qp = x + (c - y);
							int r = 4, q = 4;
							if (act) {
								r = fx[c - t0 + 1];
								const long long at = (long long)J.roff + (rev ? rlen - 1 - qp : qp) - J.rskip;
								if (at >= 0 && at < reads_len) q = reads[at];
								if (rev) q = q < 4 ? 3 - q : 4;
							}
							if (count) {
								nC2T += __popcll(__ballot(r == 1 && q == 3));
								nG2A += __popcll(__ballot(r == 2 && q == 0));
							}
							if (mark && r == (strand ? 2 : 1)) {
								// the next base on the cytosine's own strand (fivenuc[3], bisc_utils.c:33-52): 4 where the reference has none
								const int nf = strand ? fx[c - t0] : fx[c - t0 + 2], nb = strand ? (nf < 4 ? 3 - nf : 4) : nf;
								const bool ret = q == r, conv = strand ? q == 0 : q == 3;
								if (ret || conv) {
									if (bsc && nb < 4) atomicAdd(&cv[nb * 2 + (conv ? 1 : 0)], 1u);
									const int idx = rev ? rlen - qp : qp;
									if (cin && idx >= 0 && idx < BSX_QC_READ_LEN)
										atomicAdd(&pos[(((nb == 2 ? 0 : 1) * 2 + read2) * BSX_QC_READ_LEN + idx) * 2 + (conv ? 0 : 1)], 1u);
								}
							}
						}
						if (y + len > t1) break;   // the run goes on in the next tile
						x += len; y += len; ++k;
					} else if (op == 2) { y += len; ++k; }
					else { x += len; ++k; }   // I, S, H: read bases without a column
				}
			}
			if (count) {
				if (J.flags & BSX_QC_STRAND) { // bsstrand.c:115-132: min / max is an integer division, so "conflict" is a tie
					const int inferred = nC2T == 0 && nG2A == 0 ? 3 : nC2T > nG2A ? 0 : nC2T < nG2A ? 1 : 2;
					if (lane == 0) atomicAdd(&cf[tag * 4 + inferred], 1u);
				}
				if (tag != 0 && tag != 1) strand = nC2T >= nG2A ? 0 : 1;   // infer_bsstrand, bisc_utils.c:204
			}
		}
	}
	__syncthreads();
	for (int i = threadIdx.x; i < QC_CELLS; i += blockDim.x) {
		const uint32_t v = cnt[i];
		if (v) atomicAdd(&table[i], (unsigned long long)v);
	}
}

void launch_qc(hipStream_t st, const DevIndex &ix, const uint8_t *reads, long long reads_len, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool,
               unsigned long long *table, int n_cu)
{
	if (n <= 0) return;
	const long long want = (n + 3) / 4, cap = (long long)n_cu * 4;
	hipLaunchKernelGGL(k_qc, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, ix, reads, reads_len, jobs, n, pool, table);
}
