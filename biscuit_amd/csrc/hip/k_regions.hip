// k_regions.hip -- the chaining tiers: the kernels that run rg_task (rg_task.hpp), one wavefront per strand search, over tables
// of growing size (LDS, larger LDS, a slab of HBM per wave), and their launchers.  Everything lives in the wave's tables;
// nothing goes back to the host between seeding and regions.
//
// A tier only takes what its tables hold and says so per task (status != 0, the list in front of rg_task: the next tier takes the
// strand search, and after the last one the host runs its own C1/C2/C4 for it through the batch kernels).
// What runs beside the tiers: k_occ.hip (K3 for the whole chunk ahead of them), k_seedsw.hip (the seed filter over the exported
// chains) and k_c2r.hip (chains -> regions for what the tiers export).
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "kernels.h"
#include "tune.h"
#include "rg_common.hpp"
#include "rg_task.hpp"

// Debug builds of the LDS tiers (tools/dbg/lds_variants.sh; never the product's): RG_DBG 1 = guard words around every LDS object of the
// workgroup, checked when it ends (tests/test_gpu_lds_guards.py); 2 = the wave's tables filled with 0xff before every strand search (an
// answer that changes with the fill reads LDS it did not write)
#ifndef RG_DBG
#define RG_DBG 0
#endif
#if RG_DBG == 2
#define RG_DBG_FILL(S, D) do { WAVE_SYNC(); for (int i_ = lane; i_ < (int)(sizeof(S) / 4); i_ += 64) ((int*)&(S))[i_] = -1; \
		for (int i_ = (int)(sizeof((D).pf) / 4) + lane; i_ < (int)(sizeof(D) / 4); i_ += 64) ((int*)&(D))[i_] = -1; WAVE_SYNC(); } while (0)
#else
#define RG_DBG_FILL(S, D) do { } while (0)
#endif
#if RG_DBG == 1
#define RG_GUARD_WORD(q) ((int)0xC0DE0000 + (q))
#define RG_DBG_GUARDS(name) do { __syncthreads(); for (int q_ = threadIdx.x; q_ < 64; q_ += blockDim.x) { const int w_ = RG_GUARD_WORD(q_); \
		if (DL.c0[q_] != w_ || DL.c1[q_] != w_ || DL.c2[q_] != w_ || DL.c3[q_] != w_) \
			printf("LDS GUARD %s block %d word %d: %08x %08x %08x %08x\n", name, (int)blockIdx.x, q_, DL.c0[q_], DL.c1[q_], DL.c2[q_], DL.c3[q_]); } } while (0)
#else
#define RG_DBG_GUARDS(name) do { } while (0)
#endif
// strand search t as the three tier kernels hand it to rg_task, every value wave-uniform; po: where its positions looked up ahead begin
// (k_occ), or -1.  (The contig-table prologue stays written out in each kernel: as a helper it changed their code.)
struct RgFetch { int l_query, parent, n_iv; uint32_t qoff; long long po; };
__device__ __forceinline__ RgFetch rg_fetch(const bsx_seed_task_t *tasks, const int *task_n, const long long *pos_off, const unsigned long long *pos, int t)
{
	RgFetch F;
	F.l_query = uni(tasks[t].len); F.parent = uni(tasks[t].parent); F.n_iv = uni(task_n[t]);
	F.qoff = (uint32_t)uni((int)tasks[t].qoff);
	F.po = pos ? uni64(pos_off[t]) : -1;
	return F;
}

// first tier: tables in LDS.  Tasks declined for table size (or for tied chain starts) go on retry_list for the second tier.
#ifndef RG_WPB
#define RG_WPB 1     // waves per workgroup of the LDS tiers, as C2R_WPB
#endif
template <int OCC, typename DPT>
__global__ void __launch_bounds__(64 * RG_WPB, OCC)
k_regions(DevIndex ix, DevScoring sc, RegParams P, const uint8_t *reads, const bsx_seed_task_t *tasks, int n_tasks,
          const DevIntv *seeds_dense, const long long *task_off, const int *task_n,
          bsx_region_t *out, unsigned long long out_cap, unsigned long long *out_cursor, long long *reg_off, int *reg_n,
          unsigned int *task_cursor, int *retry_list, unsigned int *retry_count, int quota, unsigned long long *counters,
          const long long *pos_off, const unsigned long long *pos, const unsigned char *cls, RgXPool X)
{
#if RG_DBG == 1
	struct DbgLds { int c0[64]; RgSmall lds[RG_WPB]; int c1[64]; DPT dp[RG_WPB]; int c2[64]; long long ctg_lds[RG_CTG_LDS + 1]; int c3[64]; };
	__shared__ DbgLds DL;
	RgSmall *lds = DL.lds; DPT *dp = DL.dp; long long *ctg_lds = DL.ctg_lds;
	for (int q = threadIdx.x; q < 64; q += blockDim.x) { DL.c0[q] = DL.c1[q] = DL.c2[q] = DL.c3[q] = RG_GUARD_WORD(q); }
#else
	__shared__ RgSmall lds[RG_WPB];
	__shared__ DPT dp[RG_WPB];
	__shared__ long long ctg_lds[RG_CTG_LDS + 1];
#endif
	const int *gap_tab = nullptr;   // (cal_max_gap is read by the chain-to-region loop, which this tier leaves to k_c2r: its table was a kilobyte of LDS per workgroup)
	P.gap_cap = -1;
	if (ix.n_seqs <= RG_CTG_LDS) for (int q = threadIdx.x; q <= ix.n_seqs; q += blockDim.x) ctg_lds[q] = ix.ctg_off[q];
	const long long *ctg_tab = ix.n_seqs <= RG_CTG_LDS ? (const long long*)ctg_lds : (const long long*)ix.ctg_off;
	__syncthreads();
	const int lane = wave_lane();
	RgSmall &S = lds[threadIdx.x >> 6];
	DPT &D = dp[threadIdx.x >> 6];
	RG_PF_ZERO(D);
	// each wave takes `quota` tasks and leaves (bounded workgroup life, see k_seed); the launch covers all tasks
	for (int taken = 0; taken < quota; ++taken) {
		int t = 0;
		if (lane == 0) t = (int)atomicAdd(task_cursor, 1u);
		t = uni(__shfl(t, 0));
		if (t >= n_tasks) break;
		const int cl = cls ? uni((int)cls[t]) : 0;
		if (cl != 0) { // larger than this tier's tables: straight to the next one (3: the last HBM tier has it already, launch_occ's early list)
			if (lane == 0 && cl != 3) retry_list[atomicAdd(retry_count, 1u)] = t;
			--taken;   // costs nothing: the quota counts strand searches done here
			continue;
		}
		const auto [l_query, parent, n_iv, qoff, po] = rg_fetch(tasks, task_n, pos_off, pos, t);
		RG_DBG_FILL(S, D);
		int status = rg_task<RgSmall, true, DPT>(S, D, ix, sc, P, reads, l_query, parent, qoff, seeds_dense + uni64(task_off[t]), n_iv, po >= 0 ? pos + po : nullptr, lane, counters, gap_tab, ctg_tab, &X, t);
		if (status == 11) continue;   // exported: k_c2r makes and publishes its regions
		status = rg_publish(S, t, status, out, out_cap, out_cursor, reg_off, reg_n, lane);
		if ((status == 8 || status == 2 || status == 3 || status == 4 || status == 6 || status == 10) && lane == 0) retry_list[atomicAdd(retry_count, 1u)] = t;   // (10: the HBM tiers walk an over-represented interval further)
	}
	RG_PF_FLUSH(D);
	RG_DBG_GUARDS("k_regions");
}

// second and third tier: the same code over per-wave tables in HBM, for the strand searches of repeat-rich reads.
// `list` names the tasks (null: 0..*count-1); what this tier declines for table size goes on next_list.
template <typename Store, bool XSPLIT, typename DPT, bool PK = false>
__global__ void __launch_bounds__(256, 3)
k_regions_slab(DevIndex ix, DevScoring sc, RegParams P, const uint8_t *reads, const bsx_seed_task_t *tasks,
               const DevIntv *seeds_dense, const long long *task_off, const int *task_n,
               bsx_region_t *out, unsigned long long out_cap, unsigned long long *out_cursor, long long *reg_off, int *reg_n,
               const int *list, const unsigned int *count, unsigned int *cursor, Store *slabs, int *next_list, unsigned int *next_count,
               unsigned long long *counters, const long long *pos_off, const unsigned long long *pos, RgXPool X)
{
	__shared__ DPT dp[4];
	__shared__ int gap_tab[DPT::QCAP + 1];
	__shared__ long long ctg_lds[RG_CTG_LDS + 1];
	P.gap_cap = DPT::QCAP;
	for (int q = threadIdx.x; q <= DPT::QCAP; q += blockDim.x) gap_tab[q] = rg_cal_max_gap(P, q);
	if (ix.n_seqs <= RG_CTG_LDS) for (int q = threadIdx.x; q <= ix.n_seqs; q += blockDim.x) ctg_lds[q] = ix.ctg_off[q];
	const long long *ctg_tab = ix.n_seqs <= RG_CTG_LDS ? (const long long*)ctg_lds : (const long long*)ix.ctg_off;
	__syncthreads();
	const int lane = wave_lane();
	Store &S = slabs[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)];
	DPT &D = dp[threadIdx.x >> 6];
	RG_PF_ZERO(D);
	unsigned long long wave_cyc = 0;
	const int n = (int)*count;
	for (;;) {
		int i = 0;
		if (lane == 0) i = (int)atomicAdd(cursor, 1u);
		i = uni(__shfl(i, 0));
		if (i >= n) break;
		const int t = list ? uni(list[i]) : i;
		const auto [l_query, parent, n_iv, qoff, po] = rg_fetch(tasks, task_n, pos_off, pos, t);
		const long long tk0 = P.prof ? (long long)__builtin_readcyclecounter() : 0;
		// status 10: an over-represented interval has to be walked past its first max_occ occurrences; again with eight times as many of it, ...
		int bi[4], bl[4], nb = 0, status;
		for (;;) {
			status = rg_task<Store, XSPLIT, DPT, PK>(S, D, ix, sc, P, reads, l_query, parent, qoff, seeds_dense + uni64(task_off[t]), n_iv, po >= 0 ? pos + po : nullptr, lane, counters, gap_tab, ctg_tab, &X, t, nb, bi, bl);
			if (status != 10 || !Store::NODES || !P.walk_on) break;
			WAVE_SYNC();
			const int iv = uni(S.boost_iv);
			int j = 0;
			while (j < nb && bi[j] != iv) ++j;
			if (j == nb) { if (nb == 4) break; bi[nb] = iv; bl[nb] = 8; ++nb; }
			else if (bl[j] >= (1 << 20)) break;
			else bl[j] <<= 3;
			WAVE_SYNC();
		}
		if (P.prof && lane == 0) { // $BSX_PHASES: the longest strand search of the launch, their sum and number, the busiest wave
			const unsigned long long dt = (unsigned long long)((long long)__builtin_readcyclecounter() - tk0);
			unsigned long long *c = counters + (Store::SCAP > 1024 ? CTR_TIER3_TIME : CTR_TIER2_TIME);
			atomicMax(c, dt); atomicAdd(c + 1, dt); atomicAdd(c + 2, 1ull); wave_cyc += dt;
			if (Store::SCAP > 1024) { // the last tier: its strand searches by duration (powers of two of 2^16 cycles), and what the longest one looked like
				const unsigned long long b = dt >> 16;
				atomicAdd(counters + CTR_T3_HIST + (b ? 64 - __builtin_clzll(b) : 0), 1ull);
				const unsigned long long nk_ = (unsigned long long)(S.n_chains < 0 ? 0 : S.n_chains > 16383 ? 16383 : S.n_chains), nr_ = (unsigned long long)(S.n_regs < 0 ? 0 : S.n_regs > 16383 ? 16383 : S.n_regs);
				atomicMax(counters + CTR_T3_LONGEST, (dt >> 14) << 38 | (unsigned long long)(n_iv > 4095 ? 4095 : n_iv) << 26 | (nk_ & 8191) << 13 | (nr_ & 8191));
			}
		}
		if (status == 11) continue;   // exported (XSPLIT: chunks with long reads, whose chains go through k_seedsw and k_c2r)
		status = rg_publish(S, t, status, out, out_cap, out_cursor, reg_off, reg_n, lane);
		if (next_list && (status == 8 || status == 2 || status == 3 || status == 4 || status == 6) && lane == 0) next_list[atomicAdd(next_count, 1u)] = t;
	}
	RG_PF_FLUSH(D);
	if (P.prof && lane == 0 && wave_cyc) atomicMax(counters + (Store::SCAP > 1024 ? CTR_TIER3_TIME : CTR_TIER2_TIME) + 3, wave_cyc);
}

// Between the first tier and the HBM tiers: the same tables four times larger, still in LDS (two waves per workgroup, three
// workgroups per CU).  On a larger genome a repeat family has more copies, and a quarter of the strand searches outgrow the
// first tier's 96 seeds; in HBM slabs every table access is a memory round trip.  Same list protocol as k_regions_slab.
#define MID_WPB 2    // 14 KB of tables per wave: five workgroups of two waves fit a CU, only nine of one
template <typename Store, typename DPT, int WPB, int OCC>
__global__ void __launch_bounds__(64 * WPB, OCC)
k_regions_mid(DevIndex ix, DevScoring sc, RegParams P, const uint8_t *reads, const bsx_seed_task_t *tasks,
              const DevIntv *seeds_dense, const long long *task_off, const int *task_n,
              bsx_region_t *out, unsigned long long out_cap, unsigned long long *out_cursor, long long *reg_off, int *reg_n,
              const int *list, const unsigned int *count, unsigned int *cursor, int *next_list, unsigned int *next_count,
              unsigned long long *counters, const long long *pos_off, const unsigned long long *pos, RgXPool X, int quota)
{
#if RG_DBG == 1
	struct DbgLds { int c0[64]; Store lds[WPB]; int c1[64]; DPT dp[WPB]; int c2[64]; long long ctg_lds[RG_CTG_LDS + 1]; int c3[64]; };
	__shared__ DbgLds DL;
	Store *lds = DL.lds; DPT *dp = DL.dp; long long *ctg_lds = DL.ctg_lds;
	for (int q = threadIdx.x; q < 64; q += blockDim.x) { DL.c0[q] = DL.c1[q] = DL.c2[q] = DL.c3[q] = RG_GUARD_WORD(q); }
#else
	__shared__ Store lds[WPB];
	__shared__ DPT dp[WPB];
	__shared__ long long ctg_lds[RG_CTG_LDS + 1];
#endif
	const int *gap_tab = nullptr;   // (as in k_regions: this tier stops before the loop that reads cal_max_gap)
	P.gap_cap = -1;
	if (ix.n_seqs <= RG_CTG_LDS) for (int q = threadIdx.x; q <= ix.n_seqs; q += blockDim.x) ctg_lds[q] = ix.ctg_off[q];
	const long long *ctg_tab = ix.n_seqs <= RG_CTG_LDS ? (const long long*)ctg_lds : (const long long*)ix.ctg_off;
	__syncthreads();
	const int lane = wave_lane();
	Store &S = lds[threadIdx.x >> 6];
	DPT &D = dp[threadIdx.x >> 6];
	RG_PF_ZERO(D);
	const int n = (int)*count;
	for (int taken = 0; taken < quota; ++taken) {   // bounded workgroup life, as in k_c2r
		int i = 0;
		if (lane == 0) i = (int)atomicAdd(cursor, 1u);
		i = uni(__shfl(i, 0));
		if (i >= n) break;
		const int t = uni(list[i]);
		const auto [l_query, parent, n_iv, qoff, po] = rg_fetch(tasks, task_n, pos_off, pos, t);
		RG_DBG_FILL(S, D);
		int status = rg_task<Store, true, DPT>(S, D, ix, sc, P, reads, l_query, parent, qoff, seeds_dense + uni64(task_off[t]), n_iv, po >= 0 ? pos + po : nullptr, lane, counters, gap_tab, ctg_tab, &X, t);
		if (status == 11) continue;
		status = rg_publish(S, t, status, out, out_cap, out_cursor, reg_off, reg_n, lane);
		if ((status == 8 || status == 2 || status == 3 || status == 4 || status == 6 || status == 10) && lane == 0) {
			next_list[atomicAdd(next_count, 1u)] = t;
			if (P.prof) atomicAdd(counters + CTR_HANDON + status, 1ull);   // ($BSX_PHASES=2: why this tier hands a strand search on)
		}
	}
	RG_PF_FLUSH(D);
	RG_DBG_GUARDS("k_regions_mid");
}

size_t regions_slab_bytes(int tier) { return tier == 2 ? sizeof(RgBig) : sizeof(RgHuge); }
int regions_long_max_query(void) { return RG_QCAP_LONG; }

void launch_regions(hipStream_t st, int grid, const RgLaunch &G, unsigned int *task_cursor, int *retry_list, unsigned int *retry_count, int quota,
                    const unsigned char *cls, const RgXPoolArg &XA, bool long_reads)
{
	RgXPool X = rgx_pool(&XA);
	const int occ = (int)bsx_tune_long("regions_occ", 5);   // waves per SIMD the register allocation targets (the tables in LDS allow five workgroups per CU)
#define RG_T1_(OCC, DP) hipLaunchKernelGGL((k_regions<OCC, DP>), dim3(grid * (4 / RG_WPB)), dim3(64 * RG_WPB), 0, st, RG_COMMON_, G.n_tasks, RG_LISTS_, \
	                                   RG_OUT_, task_cursor, retry_list, retry_count, quota, RG_POS_, cls, X)
	if (long_reads) RG_T1_(3, RgDpLiteL);
	else if (occ >= 5) RG_T1_(5, RgDpLite);
	else if (occ >= 4) RG_T1_(4, RgDpLite);
	else RG_T1_(3, RgDpLite);
#undef RG_T1_
}

void launch_regions_mid(hipStream_t st, int grid, const RgLaunch &G, const int *list, const unsigned int *count, unsigned int *cursor,
                        int *next_list, unsigned int *next_count, const RgXPoolArg &XA, int quota, RgMidForm form)
{
	RgXPool X = rgx_pool(&XA);
	// `grid` counts pairs of waves
#define RG_MID_(TAB, DP, WPB, OCC) hipLaunchKernelGGL((k_regions_mid<TAB, DP, WPB, OCC>), dim3(grid * (2 / WPB)), dim3(64 * WPB), 0, st, RG_COMMON_, RG_LISTS_, \
	                                              RG_OUT_, list, count, cursor, next_list, next_count, RG_POS_, X, quota)
	switch (form) {
	case RG_MID_LONGB_L: RG_MID_(RgLongB, RgDpLiteL, 1, 1); break;
	case RG_MID2:        RG_MID_(RgMid2, RgDpLite, 1, 2); break;
	case RG_MID_LONGB:   RG_MID_(RgLongB, RgDpLite, 1, 1); break;
	case RG_MID_LONGS:   RG_MID_(RgLongS, RgDpLiteL, 1, 1); break;
	case RG_MID:         RG_MID_(RgMid, RgDpLite, MID_WPB, 2); break;
	}
#undef RG_MID_
}
void launch_regions_slab(hipStream_t st, int tier, int grid, const RgLaunch &G, const int *list, const unsigned int *count, unsigned int *cursor,
                         void *slabs, int *next_list, unsigned int *next_count, const RgXPoolArg *XA)
{
	RgXPool X = rgx_pool(XA);
	// XA given: the tier stops after the chain filter and exports (chunks with long reads or an active seed-SW filter)
#define RG_SLAB_(TAB, EXPORTS, DP, ...) hipLaunchKernelGGL((k_regions_slab<TAB, EXPORTS, DP, ##__VA_ARGS__>), dim3(grid), dim3(256), 0, st, RG_COMMON_, RG_LISTS_, \
	                                              RG_OUT_, list, count, cursor, (TAB*)slabs, next_list, next_count, RG_POS_, X)
	if (tier == 2 && XA) RG_SLAB_(RgBig, true, RgDpLiteL);
	else if (tier == 2 && G.ext_pk) RG_SLAB_(RgBig, false, RgDp, true);
	else if (tier == 2) RG_SLAB_(RgBig, false, RgDp);
	else if (XA) RG_SLAB_(RgHuge, true, RgDpLiteL);
	else if (G.ext_pk) RG_SLAB_(RgHuge, false, RgDp, true);
	else RG_SLAB_(RgHuge, false, RgDp);
#undef RG_SLAB_
}
