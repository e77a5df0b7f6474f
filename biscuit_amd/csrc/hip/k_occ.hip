// k_occ.hip -- K3 for the whole chunk ahead of the region kernels: the LF walks are pure pointer chasing, and run an order of
// magnitude faster with one walk per lane and thousands of waves in flight than inside the wave-per-task kernels.
// k_occ_expand lists the SA ranks of every occurrence each strand search will visit (lane per strand search),
// k_occ turns each rank into its reference position in place (lane per occurrence, bwt_sa, bwt.c:87-97).
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "kernels.h"
#include "rg_common.hpp"

#define OCC_MAX_PER_TASK 8192   // nothing on the device visits more
static_assert(OCC_MAX_PER_TASK == RgHuge::SCAP, "k_occ_expand looks up ahead what the last tier's seed table can hold");
__global__ void __launch_bounds__(256)
k_occ_expand(const bsx_seed_task_t *tasks, int n_tasks, const DevIntv *seeds_dense, const long long *task_off, const int *task_n, int max_occ,
             unsigned long long *desc, unsigned long long desc_cap, unsigned long long *cursor, long long *pos_off, unsigned char *cls,
             int *early_list, unsigned int *early_count)
{
	const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (t >= n_tasks) return;
	const int n_iv = task_n[t];
	long long off = -1;
	unsigned char tier = 0;
	if (n_iv > 0) {
		const DevIntv *src = seeds_dense + task_off[t];
		unsigned long long tot = 0; int over = 0;
		for (int i = 0; i < n_iv; ++i) { const unsigned long long x2 = src[i].x2; tot += x2 > (unsigned long long)max_occ ? (unsigned long long)max_occ : x2; }   // the first max_occ of an over-represented interval
		// which tier's tables hold this strand search: decided here, where the sizes are known, so that the first tier does not start
		// what it would have to give up (chains and regions can still outgrow a tier: that is found out along the way)
		tier = (n_iv <= RgSmall::ICAP && tot <= (unsigned long long)RgSmall::SCAP) ? 0 : (n_iv <= RgMid::ICAP && tot <= (unsigned long long)RgMid::SCAP) ? 1 : 2;
		// what only the last HBM tier's tables hold (rg_task's own tests, statuses 8 and 2, of every tier before it) is listed for it here: that
		// launch -- a couple of thousand strand searches, as long as its longest -- then runs beside the other tiers instead of behind them
		if (early_list && (n_iv > RgBig::ICAP || tot > (unsigned long long)RgBig::SCAP)) { tier = 3; early_list[atomicAdd(early_count, 1u)] = t; }
		if (!over && tot > 0 && tot <= OCC_MAX_PER_TASK) {
			const unsigned long long base = atomicAdd(cursor, tot);
			if (base + tot <= desc_cap) {
				const unsigned long long par = (unsigned long long)(tasks[t].parent & 1) << 63;
				unsigned long long j = base;
				for (int i = 0; i < n_iv; ++i) {
					const unsigned long long x0 = src[i].x0, x2 = src[i].x2 > (unsigned long long)max_occ ? (unsigned long long)max_occ : src[i].x2;
					for (unsigned long long k = 0; k < x2; ++k) desc[j++] = (x0 + k) | par;
				}
				off = (long long)base;
			} else {
				// no room: the strand search is chained with inline LF walks instead (pos_off = -1).  k_occ still visits every slot up to
				// min(cursor, cap): what this task reserved of them is given rank 0, where a walk ends at once, instead of whatever an earlier
				// chunk left there
				for (unsigned long long j = base; j < desc_cap && j < base + tot; ++j) desc[j] = 0;
			}
		}
	}
	pos_off[t] = off;
	if (cls) cls[t] = tier;
}

__global__ void __launch_bounds__(256)
k_occ(DevIndex ix, unsigned long long *desc, unsigned long long desc_cap, const unsigned long long *cursor, unsigned long long *counters, const unsigned long long *start)
{
	unsigned long long n = *cursor;
	if (n > desc_cap) n = desc_cap;
	uint32_t lf = 0, calls = 0;
	// start: where this launch's ranks begin (what lies before was turned into positions by an earlier launch over the same pool)
	for (unsigned long long j = (start ? *start : 0ull) + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) {
		const unsigned long long v = desc[j];
		desc[j] = (unsigned long long)rg_sa(ix, (int)(v >> 63), v & 0x7fffffffffffffffull, lf);
		++calls;
	}
	for (int off = 32; off > 0; off >>= 1) { lf += __shfl_down(lf, off); calls += __shfl_down(calls, off); }
	if ((threadIdx.x & 63) == 0) { atomicAdd(&counters[CTR_LF_STEPS], (unsigned long long)lf); atomicAdd(&counters[CTR_LF_CALLS], (unsigned long long)calls); }
}

void launch_occ(hipStream_t st, int n_cu, const RgLaunch &G, int max_occ, unsigned long long desc_cap, unsigned long long *cursor, unsigned char *cls,
                unsigned long long *start, int *early_list, unsigned int *early_count)
{
	if (start) (void)hipMemcpyAsync(start, cursor, 8, hipMemcpyDeviceToDevice, st);   // a later launch over the same pool: only the ranks it adds
	hipLaunchKernelGGL(k_occ_expand, dim3((G.n_tasks + 255) / 256), dim3(256), 0, st, G.tasks, G.n_tasks, G.seeds_dense, G.task_off, G.task_n, max_occ, G.pos, desc_cap, cursor, G.pos_off, cls, early_list, early_count);
	hipLaunchKernelGGL(k_occ, dim3(n_cu * 32), dim3(256), 0, st, *G.ix, G.pos, desc_cap, cursor, G.counters, (const unsigned long long*)start);
}

// The index files sample the suffix array every 32nd rank (bwtindex.c:328,340), which makes bwt_sa a walk of 31 LF steps
// on average.  HBM has room for a much denser sample: at upload time every `intv`-th rank's position is computed once from
// the sparse samples (the value of SA[k] does not depend on the sampling), and all later lookups walk ~intv - 1 steps.
__global__ void __launch_bounds__(256)
k_sa_dense(DevIndex ix, int parent, unsigned int intv, unsigned long long n, unsigned long long *out)
{
	uint32_t lf = 0;
	for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x)
		out[j] = (unsigned long long)rg_sa(ix, parent, j * intv, lf);
}
void launch_sa_dense(hipStream_t st, int n_cu, const DevIndex &ix, int parent, unsigned int intv, unsigned long long n, unsigned long long *out)
{
	hipLaunchKernelGGL(k_sa_dense, dim3(n_cu * 32), dim3(256), 0, st, ix, parent, intv, n, out);
}

// The last HBM tier lasts as long as its longest strand search: a couple of thousand of them on a thousand waves, 40 ms each on average and 190 ms
// the longest -- when that one is taken off the cursor late, the launch is its 190 ms behind everything before it.  So the list is put in order of
// decreasing size first (the occurrences the strand search will visit, what k_occ_expand counted): longest first, the short ones fill in behind.
// One workgroup; ranks by counting (n is a few thousand).  Lists longer than the table are left as they are: they are bound by throughput anyway.
#define ORDER_CAP 6144
__global__ void __launch_bounds__(256)
k_order_list(int *list, const unsigned int *count, const DevIntv *seeds_dense, const long long *task_off, const int *task_n, int max_occ)
{
	__shared__ unsigned int cost[ORDER_CAP];
	__shared__ int task[ORDER_CAP];
	const int n = (int)*count;
	if (n < 2 || n > ORDER_CAP) return;
	for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
		const int t = list[i], n_iv = task_n[t];
		const DevIntv *src = seeds_dense + task_off[t];
		unsigned long long tot = 0;
		for (int k = 0; k < n_iv; ++k) { const unsigned long long x2 = src[k].x2; tot += x2 > (unsigned long long)max_occ ? (unsigned long long)max_occ : x2; }
		cost[i] = tot > 0xffffffffull ? 0xffffffffu : (unsigned int)tot; task[i] = t;
	}
	__syncthreads();
	for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
		const unsigned int c = cost[i];
		int r = 0;
		for (int j = 0; j < n; ++j) { const unsigned int cj = cost[j]; r += (cj > c || (cj == c && j < i)) ? 1 : 0; }
		list[r] = task[i];
	}
}
void launch_order_list(hipStream_t st, int *list, const unsigned int *count, const DevIntv *seeds_dense, const long long *task_off, const int *task_n, int max_occ)
{
	// (four waves: a workgroup of sixteen waited 13 ms on average for a CU with room for all of them in the pipelined trace; the ranks of 2 400 take 40 us either way)
	hipLaunchKernelGGL(k_order_list, dim3(1), dim3(256), 0, st, list, count, seeds_dense, task_off, task_n, max_occ);
}
