// k_c2r.hip -- chains -> regions for the strand searches the LDS tiers exported (mem_chain2region + mem_chain2region1, memchain.c:742-904):
// the seed loop of stage E of rg_task over the exported lists (what the two do with one seed is rg_ext_seed.hpp).  One wavefront per strand search; nothing but the regions made
// so far, the read, the current chain's seeds and its reference window live in LDS (5.5 KB per wave), so the launch runs at the
// occupancy the registers allow.
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "kernels.h"
#include "ext_dp.hpp"
#include "ext_pk.hpp"
#include "rgx.hpp"
#include "rg_common.hpp"
#include "rg_ext_seed.hpp"

#define RG_XSEEDS 128    // seeds of one list (main or seeds_extra) of a chain held in LDS; longer lists: the next tier takes the strand search
#define RG_XREGS 64      // regions of one strand search (a lane each in the containment test); a read inside a high-copy repeat has dozens
#define RG_XCBLK 16      // chain records staged at a time
template <int QC, int WC, int XSD, int XRG = RG_XREGS, bool ROWS_ = true>
struct RgC2rT {
	static const int QCAP = QC, WINCAP = WC, XSEEDS = XSD, XREGS = XRG, GAPCAP = QC > RG_QCAP ? RG_QCAP : QC;   // (cal_max_gap tabulated up to GAPCAP; LDS is what bounds the long-read launch)
	static const bool HBM = false, ROWS = ROWS_;   // ROWS: LDS for an extension's rows (ext_dp: bands of more than 255 columns of a long read); without them such a strand search is handed on
	unsigned long long pf[RG_NPF];
	bsx_region_t regs[XRG];
	RgXChain xc[RG_XCBLK];   // chains [xc_lo, xc_lo + RG_XCBLK) of the exported record
	RgXExt xe[RG_XCBLK];     // and, when the record has them, the extensions made ahead of this launch (k_ext4.hip)
	RgXSeed sd[XSD];         // a window [sd_lo, sd_hi) over the record's seeds: the current chain's lists lie inside it
	unsigned long long srt[XSD];
	uint8_t q[QC];
	uint8_t win[WC];
	int n_regs;
	// long reads: the extension's rows in LDS (ext_dp: registers for the band only, so that the launch keeps several waves per SIMD;
	// rows in registers would need a slot per 64 query bases, 16 of them for a kilobase)
	int32_t Hrow[(ROWS_ && QC > RG_QCAP) ? QC + 2 : 1], Erow[(ROWS_ && QC > RG_QCAP) ? QC + 2 : 1];
	uint8_t qrow[(ROWS_ && QC > RG_QCAP) ? QC : 4];
};
typedef RgC2rT<RG_QCAP, RG_WIN, RG_XSEEDS> RgC2r;
// (round 6: no LDS rows -- 9 KB of the wave's 22 -- since the extensions of a long read keep their rows in a register window, ext_dp_win; the few
// whose band outgrows it, a second band width of 401 columns, go on to k_c2r<RgC2rHL> with the strand search: twelve waves per CU instead of six)
typedef RgC2rT<RG_QCAP_LONG, 1536, 256, RG_XREGS, false> RgC2rL;
// The same workspace with its three large tables -- the regions made so far, the window over the record's seeds, the sort keys -- in a slab of
// HBM per wave (round 6): for the strand searches of reads inside repeat families that outgrow RgC2rB (up to 1024 regions, 1024 seeds a list: what
// the first HBM tier holds).  Until round 6 those went through that tier's monolithic form, whose extensions run inline, a wavefront each -- 58 % of
// the tier's cycles, a quarter of all wave cycles of a chunk; through this launch their chains' extensions come from k_extl / k_ext4 (several
// jobs to a wavefront, made ahead) and only the seed loop's bookkeeping pays HBM round trips.
template <int QC, int WC, int XSD, int XRG>
struct RgC2rHT {
	static const int QCAP = QC, WINCAP = WC, XSEEDS = XSD, XREGS = XRG, GAPCAP = QC > RG_QCAP ? RG_QCAP : QC;
	static const bool HBM = true, ROWS = true;
	unsigned long long pf[RG_NPF];
	bsx_region_t *regs;      // XRG entries in the wave's slab of HBM: written once per region, read a lane per region by the containment test
	RgXChain xc[RG_XCBLK];
	RgXExt xe[RG_XCBLK];
	RgXSeed sd[XSD];         // (the seed window and its sort keys stay in LDS: the rank by counting reads every key once per seed)
	unsigned long long srt[XSD];
	uint8_t q[QC];
	uint8_t win[WC];
	int n_regs;
	int32_t Hrow[QC > RG_QCAP ? QC + 2 : 1], Erow[QC > RG_QCAP ? QC + 2 : 1];   // (long reads: the extension's rows in LDS, as in RgC2rT)
	uint8_t qrow[QC > RG_QCAP ? QC : 4];
	static constexpr size_t slab_bytes() { return (size_t)XRG * sizeof(bsx_region_t); }
};
typedef RgC2rHT<RG_QCAP, RG_WIN, 1024, 1024> RgC2rH;   // 27 KB of LDS: five workgroups of one wave per CU
// (8192 regions: in a sequence whose every tier exports this launch is the last maker of regions, and the last HBM tier exports up to RgHuge::CCAP
// chains -- with 1024, a strand search of 1025 regions under the seed filter, or of a kilobase read, was left to the caller; only the slab grows)
typedef RgC2rHT<RG_QCAP_LONG, 1536, 1024, 8192> RgC2rHL;   // reads up to a kilobase: what k_c2r<RgC2rL> declines (64 regions, 256 seeds a list) -- chained on the host until round 6
static_assert(RgC2rHL::XREGS == RgHuge::CCAP, "the last chains -> regions launch of an exporting sequence holds a region for every chain the last tier can export");
typedef RgC2rT<RG_QCAP, RG_WIN, 256, 256> RgC2rB;   // reads inside repeat families: up to 256 regions of a strand search, 256 seeds of a chain (22 KB: seven waves per CU); for what k_c2r<RgC2r> declines   // reads up to a kilobase: a chain's window is the read plus its two gaps, a true chain has a few hundred seeds

// TALLY ($BSX_PHASES with extensions made ahead, RgXPoolArg::rows set): an extension of launch_x4 that the loop does not read, its seed being contained in a
// region made before, is counted by the kernel that ran the job (CTR_X4W + 4 * k): jobs, their rows, and of both those inside the strand
// search's first region.  An instantiation of its own: the others are the code they were.
template <bool PK = false, bool TALLY = false, typename WT>   // PK: as in rg_task (tables for reads of up to 256 bases only)
__device__ int rg_c2r(WT &W, const DevIndex &ix, const DevScoring &sc, const RegParams &P, const uint8_t *reads, int l_query, int parent, uint32_t qoff,
                      const RgXHdr *H, int lane, unsigned long long *counters, const int *gap, const long long *ctg, const RgXPool &X)
{
	const long long l_pac = ix.l_pac;
	long long pf_t = P.prof ? (long long)__builtin_readcyclecounter() : 0;
	unsigned int pf_ext = 0, pf_rows = 0, pf_seen = 0, pf_skip = 0, pf_cached = 0, pf_inl = 0;
	// The exported record (header, chains in processing order, their seeds in the same order) is staged through LDS a block of
	// chains and a window of seeds at a time: two round trips to HBM per strand search (header + read, then chains + seeds) where
	// reading each chain's record and lists where they lie was three per chain, twelve chains per strand search.
	for (int i = lane; i < l_query; i += 64) W.q[i] = reads[qoff + i];
	const int nk = uni(H->n_chains), n_sd = uni(H->n_seeds);
	// routing, before anything is started: a strand search with more chains than this launch holds regions, or with a list longer than its seed
	// window, goes on to the launch with larger tables (it would be declined half-way otherwise, its work done twice)
	if (nk > 4 * WT::XREGS) return 6;
	{
		const RgXChain *XCh = (const RgXChain*)(H + 1);
		int mx = 0;
		for (int c = lane; c < nk; c += 64) { const int a = XCh[c].n_main, b = XCh[c].n_extra; mx = mx > a ? mx : a; mx = mx > b ? mx : b; }
		if (uni(wave_max_i32(mx)) > WT::XSEEDS) return 2;
	}
	const float frac_rep = H->frac_rep;
	const unsigned long long *XCw = (const unsigned long long*)(H + 1);                           // RgXChain = 3 words, RgXSeed = 2
	const unsigned long long *XSw = XCw + (size_t)nk * (sizeof(RgXChain) / 8);
	const int has_ext = uni(H->has_ext);
	const unsigned long long *XEw = XSw + (size_t)n_sd * (sizeof(RgXSeed) / 8);
	if (lane == 0) W.n_regs = 0;
	int xc_lo = 0, sd_lo = 0, sd_hi = 0;
#define C2R_STAGE_CHAINS(from) do { const int n_ = (nk - (from) < RG_XCBLK ? nk - (from) : RG_XCBLK) * (int)(sizeof(RgXChain) / 8); \
		for (int i_ = lane; i_ < n_; i_ += 64) ((unsigned long long*)W.xc)[i_] = XCw[(size_t)(from) * (sizeof(RgXChain) / 8) + i_]; \
		if (has_ext == 1) for (int i_ = lane; i_ < n_ * 2; i_ += 64) ((unsigned long long*)W.xe)[i_] = XEw[(size_t)(from) * (sizeof(RgXExt) / 8) + i_]; xc_lo = (from); } while (0)
#define C2R_STAGE_SEEDS(from) do { const int m_ = n_sd - (from) < WT::XSEEDS ? n_sd - (from) : WT::XSEEDS; \
		for (int i_ = lane; i_ < m_ * 2; i_ += 64) ((unsigned long long*)W.sd)[i_] = XSw[(size_t)(from) * 2 + i_]; sd_lo = (from); sd_hi = (from) + m_; } while (0)
	C2R_STAGE_CHAINS(0);
	C2R_STAGE_SEEDS(0);
	WAVE_SYNC();
	for (int ci = 0; ci < nk; ++ci) {
		if (ci >= xc_lo + RG_XCBLK) { WAVE_SYNC(); C2R_STAGE_CHAINS(ci); WAVE_SYNC(); }
		const RgXChain &XCc = W.xc[ci - xc_lo];
		const long long ch_pos = uni64(XCc.pos);
		const int rid = uni(XCc.rid), seed_off = uni(XCc.seed_off), n_main = uni((int)XCc.n_main), n_extra = uni((int)XCc.n_extra);
		if (n_main == 0) continue;   // every seed of the chain failed the seed-SW filter (memchain.c:880)
		if (n_main > WT::XSEEDS || n_extra > WT::XSEEDS) return 2;
		if (seed_off + n_main > sd_hi) { WAVE_SYNC(); C2R_STAGE_SEEDS(seed_off); WAVE_SYNC(); }
		// mem_chain_reference_span (memchain.c:585-605) over the main list + bns_fetch_seq's contig clamp
		int64_t rmax0 = l_pac << 1, rmax1 = 0;
		for (int o = lane; o < n_main; o += 64) {
			const RgXSeed sd = W.sd[seed_off - sd_lo + o];
			int64_t b, e;
			c2r_seed_span(sd.rbeg, sd.qbeg, sd.len, l_query, rg_gap(gap, P, sd.qbeg), rg_gap(gap, P, l_query - sd.qbeg - sd.len), &b, &e);
			rmax0 = rmax0 < b ? rmax0 : b; rmax1 = rmax1 > e ? rmax1 : e;
		}
		if (n_main == 1) { // most chains are one seed: lane 0 holds the span
			rmax0 = uni64(rmax0); rmax1 = uni64(rmax1);
		} else { rmax0 = uni64(-wave_max_i64(-rmax0)); rmax1 = uni64(wave_max_i64(rmax1)); }
		c2r_clamp_window(&rmax0, &rmax1, l_pac, ch_pos, uni64(ctg[rid]), uni64(ctg[rid + 1]));
		const int n0 = uni(W.n_regs);
		int win_ok = 0;
		for (int pass = 0; pass < 2; ++pass) {
			if (pass == 1 && !(uni(W.n_regs) == n0 && n_extra > 0)) break;
			const int nl = pass ? n_extra : n_main;
			const int l0 = seed_off + (pass ? n_main : 0);
			if (l0 + nl > sd_hi) { WAVE_SYNC(); C2R_STAGE_SEEDS(l0); WAVE_SYNC(); }
			const RgXSeed *Lsd = W.sd + (l0 - sd_lo);   // this list, in place in the window
			for (int i = lane; i < nl; i += 64) { // keys score<<32|i are unique: rank by counting (ks_introsort_64, memchain.c:752)
				const unsigned long long key = (unsigned long long)(unsigned)XS_SCORE(Lsd[i]) << 32 | (unsigned)i;
				int r = 0;
				for (int k = 0; k < nl; ++k) r += ((unsigned long long)(unsigned)XS_SCORE(Lsd[k]) << 32 | (unsigned)k) < key;
				W.srt[r] = key;
			}
			WAVE_SYNC();
			for (int k = nl - 1; k >= 0; --k) {
				const int si = uni((int)(uint32_t)W.srt[k]);
				const RgXSeed sd = Lsd[si];
				if (uni(XS_BAD(sd))) continue;   // asymmetric_flt_seed (memchain.c:138-149), tested by the tier that exported the seed
				const long long s_rbeg = uni64(sd.rbeg); const int s_qbeg = uni((int)sd.qbeg), s_len = uni((int)sd.len);
				++pf_seen;
				// contained in a region of this strand search, and no later seed of the list disagrees? (memchain.c:761-819)
				const auto seed_at = [&](int i, long long &t_rbeg, int &t_qbeg, int &t_len) { const RgXSeed td = Lsd[i]; t_rbeg = td.rbeg; t_qbeg = td.qbeg; t_len = td.len; };
				const int nr = uni(W.n_regs);
				const int u = rg_first_container(W.regs, nr, s_rbeg, s_qbeg, s_len, l_query, gap, P, lane);
				if (u < nr && !rg_later_disagrees(W.srt, k, nl, s_rbeg, s_qbeg, s_len, lane, seed_at)) {
					// the chain's extension was made ahead and is never read: this is the seed k_x4prep chose (the first one the loop reaches in the main list)
					if constexpr (TALLY) if (has_ext == 1 && pass == 0 && uni(W.xe[ci - xc_lo].status) == 1 && uni(W.xe[ci - xc_lo].si) == si) {
						const unsigned long long at = (unsigned long long)((const unsigned char*)(XEw + (size_t)ci * (sizeof(RgXExt) / 8)) - X.base);
						const unsigned int rw = (unsigned int)uni((int)((const unsigned int*)(X.base + rgx_rows_offset(X.cap)))[RGX_ROWS_AT(at)]);
						const unsigned long long rows = rw & ~RGX_ROWS_L;
						const unsigned long long v = lane == X4W_JOBS ? 1ull : lane == X4W_ROWS ? rows : u != 0 ? 0ull : lane == X4W_JOBS_R0 ? 1ull : rows;
						if (lane < 4 && v) atomicAdd(&counters[CTR_X4W + ((rw & RGX_ROWS_L) ? 4 : 0) + lane], v);
					}
					++pf_skip; WAVE_SYNC(); if (lane == 0) W.srt[k] = 0; WAVE_SYNC(); continue;
				}
				// extension (memchain.c:613-730): left then right, each with up to MAX_BAND_TRY band widths -- taken from the record when this
				// is the seed k_ext4 extended ahead of the loop (the first one the loop reaches in a chain's main list)
				RgXExt xe = W.xe[ci - xc_lo];
				if (has_ext == 2 && pass == 0) { // a slot per seed, where the extension kernels left it: one 48-byte read, six lanes
					const unsigned long long *xp = XEw + (size_t)(l0 + si) * (sizeof(RgXExt) / 8);
					const unsigned long long v = lane < (int)(sizeof(RgXExt) / 8) ? xp[lane] : 0ull;
					unsigned long long w6[sizeof(RgXExt) / 8];
#pragma unroll
					for (int q = 0; q < (int)(sizeof(RgXExt) / 8); ++q) w6[q] = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), q) << 32 | (unsigned)__builtin_amdgcn_readlane((int)v, q);
					memcpy(&xe, w6, sizeof(xe));
				}
				const bool cached = has_ext && pass == 0 && uni(xe.status) == 1 && uni(xe.si) == si;
				if (cached) ++pf_cached; else ++pf_inl;
				if (!cached && win_ok == 0) { // the chain's reference window (bns_fetch_seq, memchain.c:889) into LDS, once, when a seed of it is first extended
					const int span = (int)(rmax1 - rmax0);
					if (span > 0 && span <= WT::WINCAP) {
						dev_fetch_window(W.win, ix.pac, l_pac, rmax0, span, lane);
						win_ok = 1;
						WAVE_SYNC();
					} else win_ok = -1;
				}
				bsx_region_t R; int aw0, aw1;
				rg_region_open(R, aw0, aw1, P.w, rid);
				if (cached) {
					R.rb = uni64(xe.rb); R.re = uni64(xe.re); R.qb = uni(xe.qb); R.qe = uni(xe.qe); R.score = uni(xe.score); R.truesc = uni(xe.truesc);
					aw0 = uni(xe.aw0); aw1 = uni(xe.aw1);
				} else {
					constexpr int XC = TALLY ? XS_FAM_C2R : -1;   // ($BSX_PHASES: the stopping rule counted, ext_stop.hpp)
					const int st = rg_ext_seed<PK, WT::QCAP, WT::ROWS, XC>(R, aw0, aw1, W, ix, sc, P, reads, qoff, l_query, parent, s_rbeg, s_qbeg, s_len, rmax0, rmax1, win_ok, lane, pf_t, pf_ext, pf_rows);
					if (st) return st;
				}
				if (rg_push_region(R, aw0, aw1, s_len, frac_rep, parent, l_pac, nl, seed_at, W.regs, W.n_regs, WT::XREGS, lane)) return 6;
			}
		}
	}
	RG_PF_STAGE(W, 6, pf_t);
	if (P.prof) { RG_PF_ADD(W, 8, pf_ext); RG_PF_ADD(W, 9, pf_rows); RG_PF_ADD(W, 11, pf_seen); RG_PF_ADD(W, 12, pf_skip); RG_PF_ADD(W, 13, pf_cached); RG_PF_ADD(W, 14, pf_inl); }
	return 0;
#undef C2R_STAGE_CHAINS
#undef C2R_STAGE_SEEDS
}

#ifndef C2R_WPB
#define C2R_WPB 1    // waves per workgroup (a workgroup's slots come back when its last wave ends)
#endif
template <typename WT, int OCC, bool PK = false, bool TALLY = false>
__global__ void __launch_bounds__(64 * C2R_WPB, OCC)
k_c2r(DevIndex ix, DevScoring sc, RegParams P, const uint8_t *reads, const bsx_seed_task_t *tasks, RgXPool X,
      bsx_region_t *out, unsigned long long out_cap, unsigned long long *out_cursor, long long *reg_off, int *reg_n,
      unsigned int *cursor, int *next_list, unsigned int *next_count, unsigned long long *counters, int quota, unsigned char *slab)
{
	__shared__ WT lds[C2R_WPB];
	__shared__ int gap_tab[WT::GAPCAP + 1];
	__shared__ long long ctg_lds[RG_CTG_LDS + 1];
	P.gap_cap = WT::GAPCAP;
	for (int q = threadIdx.x; q <= WT::GAPCAP; q += blockDim.x) gap_tab[q] = rg_cal_max_gap(P, q);
	if (ix.n_seqs <= RG_CTG_LDS) for (int q = threadIdx.x; q <= ix.n_seqs; q += blockDim.x) ctg_lds[q] = ix.ctg_off[q];
	const long long *ctg_tab = ix.n_seqs <= RG_CTG_LDS ? (const long long*)ctg_lds : (const long long*)ix.ctg_off;
	__syncthreads();
	const int lane = wave_lane();
	WT &W = lds[threadIdx.x >> 6];
	RG_PF_ZERO(W);
	if constexpr (WT::HBM) { // the large tables: this wave's slab
		unsigned char *sl = slab + ((size_t)blockIdx.x * C2R_WPB + (threadIdx.x >> 6)) * WT::slab_bytes();
		if (lane == 0) W.regs = (bsx_region_t*)sl;
		WAVE_SYNC();
	}
	const int n = (int)*X.xcount;
	// a wave takes `quota` strand searches and leaves (the launch covers the worst case): workgroups with a bounded life let the
	// back half's short high-priority batches (k_sw, k_global) of an older chunk get compute units while this one runs
	for (int taken = 0; taken < quota; ++taken) {
		int i = 0;
		if (lane == 0) i = (int)atomicAdd(cursor, 1u);
		i = uni(__shfl(i, 0));
		if (i >= n) break;
		const int t = uni(X.xlist[i]);
		const int l_query = uni(tasks[t].len), parent = uni(tasks[t].parent);
		const uint32_t qoff = (uint32_t)uni((int)tasks[t].qoff);
		const RgXHdr *H = (const RgXHdr*)(X.base + uni64(X.xoff[t]));
		int status = rg_c2r<PK, TALLY>(W, ix, sc, P, reads, l_query, parent, qoff, H, lane, counters, gap_tab, ctg_tab, X);
		WAVE_SYNC();
		if constexpr (WT::HBM) { // publish: hundreds of regions, all lanes copy
			const int nr = status ? 0 : uni(W.n_regs);
			unsigned long long base = 0;
			if (nr > 0) {
				if (lane == 0) base = atomicAdd(out_cursor, (unsigned long long)nr);
				base = (unsigned long long)uni64((long long)base);
				if (base + nr <= out_cap) { const bsx_region_t *src = W.regs; for (int k = lane; k < nr; k += 64) out[base + k] = src[k]; }
				else status = 7;
			}
			if (lane == 0) {
				reg_off[t] = (long long)base;
				reg_n[t] = status ? -status : nr;
				if (next_list && (status == 2 || status == 6)) next_list[atomicAdd(next_count, 1u)] = t;
			}
		} else
		if (lane == 0) { // publish (as rg_publish)
			const int nr = status ? 0 : W.n_regs;
			unsigned long long base = 0;
			if (nr > 0) {
				base = atomicAdd(out_cursor, (unsigned long long)nr);
				if (base + nr <= out_cap) for (int k = 0; k < nr; ++k) out[base + k] = W.regs[k];
				else status = 7;
			}
			reg_off[t] = (long long)base;
			reg_n[t] = status ? -status : nr;
			if (next_list && (status == 2 || status == 6)) { next_list[atomicAdd(next_count, 1u)] = t; if (P.prof) atomicAdd(counters + CTR_HANDON + status, 1ull); }
		}
		WAVE_SYNC();
	}
	RG_PF_FLUSH(W);
}

size_t c2r_hbm_slab_bytes(bool long_form) { return (long_form ? RgC2rHL::slab_bytes() : RgC2rH::slab_bytes()) * C2R_WPB; }   // per workgroup of launch_c2r(.., RG_C2R_H) / (.., RG_C2R_HL)
void launch_c2r(hipStream_t st, int grid, const RgLaunch &G, const RgXPoolArg &XA, unsigned int *cursor, int *next_list, unsigned int *next_count,
                int quota, RgC2rForm form, void *slab)
{
	RgXPool X = rgx_pool(&XA);
	// the forms with their tables in LDS: `grid` counts groups of four waves; in HBM: workgroups, with c2r_hbm_slab_bytes(form == RG_C2R_HL) of `slab` each
#define RG_C2R_(TAB, OCC, GRID, SLAB, ...) hipLaunchKernelGGL((k_c2r<TAB, OCC, ##__VA_ARGS__>), dim3(GRID), dim3(64 * C2R_WPB), 0, st, RG_COMMON_, X, RG_OUT_, cursor, next_list, next_count, G.counters, quota, (unsigned char*)(SLAB))
	// (G.ext_pk: the instantiations whose extension rows are packed 16-bit; the forms for long reads have none)
	// XA.rows ($BSX_PHASES): the counting instantiations of the two launches every ordinary chunk makes over records with extensions made ahead
	if (XA.rows && form == RG_C2R_B) { if (G.ext_pk) RG_C2R_(RgC2rB, 2, grid * (4 / C2R_WPB), nullptr, true, true); else RG_C2R_(RgC2rB, 2, grid * (4 / C2R_WPB), nullptr, false, true); }
	else if (XA.rows && form == RG_C2R) { if (G.ext_pk) RG_C2R_(RgC2r, 4, grid * (4 / C2R_WPB), nullptr, true, true); else RG_C2R_(RgC2r, 4, grid * (4 / C2R_WPB), nullptr, false, true); }
	else if (G.ext_pk && form == RG_C2R_H) RG_C2R_(RgC2rH, 2, grid, slab, true);
	else if (G.ext_pk && form == RG_C2R_B) RG_C2R_(RgC2rB, 2, grid * (4 / C2R_WPB), nullptr, true);
	else if (G.ext_pk && form == RG_C2R) RG_C2R_(RgC2r, 4, grid * (4 / C2R_WPB), nullptr, true);
	else
	switch (form) {
	case RG_C2R_HL: RG_C2R_(RgC2rHL, 1, grid, slab); break;
	case RG_C2R_H:  RG_C2R_(RgC2rH, 2, grid, slab); break;
	case RG_C2R_B:  RG_C2R_(RgC2rB, 2, grid * (4 / C2R_WPB), nullptr); break;
	case RG_C2R_L:  RG_C2R_(RgC2rL, 3, grid * (4 / C2R_WPB), nullptr); break;
	case RG_C2R:    RG_C2R_(RgC2r, 4, grid * (4 / C2R_WPB), nullptr); break;
	}
#undef RG_C2R_
}
