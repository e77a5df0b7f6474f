// meth_bench.hip -- what the table pass behind --qc-meth costs at genome size (k_meth.hip's k_meth_walk): a 3.1 Gbp genome of 25 contigs with a
// few hundred N holes, random bases, and counters filled as a 30x library leaves them (every C and G a site, one in 64 with reads of the other
// strand that disagree); the launch alone between two events, five times.  The 50 GB of counters are only read.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ibiscuit_amd/csrc/host -Ibiscuit_amd/csrc/hip -o tools/ubench/meth_bench tools/ubench/meth_bench.hip \
//         && tools/ubench/meth_bench [genome Mbp, default 3100]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../../biscuit_amd/csrc/hip/k_meth.hip"   // the launchers (the library keeps them to itself)

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__device__ __forceinline__ uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; return x ^ (x >> 33); }
__global__ void fill(uint8_t *pac, long long pac_bytes, ulonglong2 *st, long long l_pac)
{
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < l_pac; i += (long long)gridDim.x * blockDim.x) {
		const uint64_t h = mix((uint64_t)i);
		const uint32_t n = 1 + (uint32_t)(h >> 8) % 30, ret = (uint32_t)(h >> 16) % (n + 1);
		st[i] = make_ulonglong2((unsigned long long)ret | (unsigned long long)(n - ret) << 32, (h >> 40) % 64 ? 15ull : 15ull | 1ull << 32);
		if (i < pac_bytes) pac[i] = (uint8_t)mix((uint64_t)i + 0x1234567);
	}
}

int main(int argc, char **argv)
{
	const long long l_pac = (argc > 1 ? atoll(argv[1]) : 3100) * 1000000ll, pac_bytes = l_pac / 4 + 16;
	const int n_seqs = 25, n_holes = 400;
	hipDeviceProp_t prop;
	CHK(hipGetDeviceProperties(&prop, 0));
	std::vector<int64_t> ctg(n_seqs + 1), hoff(n_holes), hend(n_holes);
	for (int i = 0; i <= n_seqs; ++i) ctg[i] = l_pac / n_seqs * i;
	ctg[n_seqs] = l_pac;
	for (int i = 0; i < n_holes; ++i) { hoff[i] = l_pac / n_holes * i + 1000; hend[i] = hoff[i] + 50000; }
	uint8_t *pac; ulonglong2 *st; int64_t *d_ctg, *d_hoff, *d_hend; unsigned long long *cells;
	CHK(hipMalloc(&pac, pac_bytes));
	CHK(hipMalloc(&st, meth_state_entries(l_pac) * 16));
	CHK(hipMemset(st, 0, meth_state_entries(l_pac) * 16));
	CHK(hipMalloc(&d_ctg, ctg.size() * 8)); CHK(hipMalloc(&d_hoff, n_holes * 8)); CHK(hipMalloc(&d_hend, n_holes * 8)); CHK(hipMalloc(&cells, 80));
	CHK(hipMemcpy(d_ctg, ctg.data(), ctg.size() * 8, hipMemcpyHostToDevice));
	CHK(hipMemcpy(d_hoff, hoff.data(), n_holes * 8, hipMemcpyHostToDevice));
	CHK(hipMemcpy(d_hend, hend.data(), n_holes * 8, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(fill, dim3(prop.multiProcessorCount * 8), dim3(256), 0, 0, pac, pac_bytes, st, l_pac);
	CHK(hipDeviceSynchronize());
	DevIndex ix;
	memset(&ix, 0, sizeof(ix));
	ix.pac = pac; ix.l_pac = l_pac; ix.ctg_off = d_ctg; ix.n_seqs = n_seqs; ix.hole_off = d_hoff; ix.hole_end = d_hend; ix.n_holes = n_holes;
	hipEvent_t e0, e1;
	CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
	std::vector<float> ms(5);
	unsigned long long out[10];
	for (int r = 0; r < 5; ++r) {
		CHK(hipMemset(cells, 0, 80));
		CHK(hipEventRecord(e0, 0));
		launch_meth_tables(0, prop.multiProcessorCount, ix, st, (long long)meth_n_tiles(l_pac), METH_FLUSH_TILES_MAX, cells);
		CHK(hipEventRecord(e1, 0));
		CHK(hipEventSynchronize(e1));
		CHK(hipEventElapsedTime(&ms[r], e0, e1));
	}
	CHK(hipMemcpy(out, cells, 80, hipMemcpyDeviceToHost));
	std::sort(ms.begin(), ms.end());
	printf("{\"what\": \"meth_tables\", \"genome_bp\": %lld, \"state_bytes\": %zu, \"ms_min\": %.3f, \"ms_median\": %.3f, \"ms_max\": %.3f, \"state_GB_per_s\": %.1f, "
	       "\"sites\": [%llu, %llu, %llu, %llu, %llu], \"milli\": [%llu, %llu, %llu, %llu, %llu]}\n", l_pac, meth_state_entries(l_pac) * 16, ms[0], ms[2], ms[4],
	       (double)l_pac * 16 / 1e6 / ms[2], out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8], out[9]);
	return 0;
}
