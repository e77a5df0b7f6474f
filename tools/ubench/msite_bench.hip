// msite_bench.hip -- what the site extraction behind --meth-bed costs at genome size (k_msite.hip): the genome and the counters of
// tools/ubench/meth_bench.hip (3.1 Gbp, 25 contigs, 400 N holes, random bases, every C and G a site).  Per mode: the count pass over the whole
// genome between two events, three times; the tiles' counts brought to the host and summed; then the genome window by window through a buffer
// of 64 Mi records as bsx_meth_sites does it -- the emit pass between two events, the records copied to pageable host memory -- and the first
// window's records formatted by bsx_meth_bed_line (csrc/host/meth.c), into memory and into /dev/null.  The 50 GB of counters are only read.
//   gcc -O3 -DNDEBUG -std=gnu11 -Iinclude -Ibiscuit_amd/csrc/host -c biscuit_amd/csrc/host/meth.c -o /tmp/msite_bench_meth.o && \
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ibiscuit_amd/csrc/host -Ibiscuit_amd/csrc/hip -c tools/ubench/msite_bench.hip -o /tmp/msite_bench.o && \
//   hipcc --offload-arch=gfx950 -o tools/ubench/msite_bench /tmp/msite_bench.o /tmp/msite_bench_meth.o -lm -lpthread && tools/ubench/msite_bench [genome Mbp, default 3100]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <chrono>
#include "../../biscuit_amd/csrc/hip/k_msite.hip"   // the launchers (the library keeps them to itself)

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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
	const long long nt = (l_pac + BSX_COV_TILE - 1) / BSX_COV_TILE, cap = 64ll << 20;
	const size_t st_entries = (size_t)(nt + 1) * BSX_COV_TILE;
	const int n_seqs = 25, n_holes = 400;
	hipDeviceProp_t prop;
	CHK(hipGetDeviceProperties(&prop, 0));
	std::vector<int64_t> ctg(n_seqs + 1), hoff(n_holes), hend(n_holes);
	for (int i = 0; i <= n_seqs; ++i) ctg[i] = l_pac / n_seqs * i;
	ctg[n_seqs] = l_pac;
	for (int i = 0; i < n_holes; ++i) { hoff[i] = l_pac / n_holes * i + 1000; hend[i] = hoff[i] + 50000; }
	uint8_t *pac; ulonglong2 *st; int64_t *d_ctg, *d_hoff, *d_hend; uint32_t *cnt; bsx_meth_site_t *recs;
	CHK(hipMalloc(&pac, pac_bytes));
	CHK(hipMalloc(&st, st_entries * 16));
	CHK(hipMemset(st, 0, st_entries * 16));
	CHK(hipMalloc(&d_ctg, ctg.size() * 8)); CHK(hipMalloc(&d_hoff, n_holes * 8)); CHK(hipMalloc(&d_hend, n_holes * 8));
	CHK(hipMalloc(&cnt, ((size_t)nt + 1) * 4)); CHK(hipMalloc(&recs, (size_t)cap * sizeof(bsx_meth_site_t)));
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
	std::vector<uint32_t> h((size_t)nt + 1), base;
	bsx_meth_site_t *host = (bsx_meth_site_t*)malloc((size_t)cap * sizeof(bsx_meth_site_t));
	char *text = (char*)malloc(200 * 4096);
	FILE *null = fopen("/dev/null", "w");
	if (!host || !text || !null) { printf("no memory\n"); return 1; }
	static const struct { const char *name; bsx_meth_site_opt_t opt; } MODES[] = {
		{"cg", {BSX_METH_TYPE_CG, 0, 1, 0}}, {"cg merged", {BSX_METH_TYPE_CG, 1, 1, 0}}, {"cg, at least 24", {BSX_METH_TYPE_CG, 0, 24, 0}}, {"c", {BSX_METH_TYPE_C, 0, 1, 0}}};
	for (const auto &M : MODES) {
		std::vector<float> ms(3);
		for (int r = 0; r < 3; ++r) {
			CHK(hipEventRecord(e0, 0));
			launch_msite_count(0, prop.multiProcessorCount, ix, st, M.opt, 0, l_pac, 0, nt, cnt);
			CHK(hipEventRecord(e1, 0));
			CHK(hipEventSynchronize(e1));
			CHK(hipEventElapsedTime(&ms[r], e0, e1));
		}
		std::sort(ms.begin(), ms.end());
		double t = now_ms();
		CHK(hipMemcpy(h.data(), cnt, (size_t)nt * 4, hipMemcpyDeviceToHost));
		const double counts_ms = now_ms() - t;
		double emit_ms = 0, copy_ms = 0, sums_ms = 0, fmt_mem_ms = 0, fmt_file_ms = 0;
		unsigned long long lines = 0, fmt_lines = 0, fmt_bytes = 0;
		int windows = 0;
		for (long long t0 = 0; t0 < nt; ) { // the window that fits the buffer, as bsx_meth_sites (shim_tables.hip) cuts it
			t = now_ms();
			long long w = 0;
			uint64_t total = 0;
			base.clear();
			for (; t0 + w < nt && total + h[(size_t)(t0 + w)] <= (uint64_t)cap; ++w) { base.push_back((uint32_t)total); total += h[(size_t)(t0 + w)]; }
			base.push_back((uint32_t)total);
			sums_ms += now_ms() - t;
			if (w == 0) { printf("a tile beyond the buffer\n"); return 1; }
			CHK(hipMemcpy(cnt, base.data(), base.size() * 4, hipMemcpyHostToDevice));
			float ems;
			CHK(hipEventRecord(e0, 0));
			launch_msite_emit(0, prop.multiProcessorCount, ix, st, M.opt, 0, l_pac, t0, w, cnt, recs);
			CHK(hipEventRecord(e1, 0));
			CHK(hipEventSynchronize(e1));
			CHK(hipEventElapsedTime(&ems, e0, e1));
			emit_ms += ems;
			t = now_ms();
			if (total) CHK(hipMemcpy(host, recs, (size_t)total * sizeof(bsx_meth_site_t), hipMemcpyDeviceToHost));
			copy_ms += now_ms() - t;
			if (windows == 0) { // host formatting: the first window's records, 4096 lines at a time
				for (int pass = 0; pass < 2; ++pass) {
					t = now_ms();
					size_t used = 0;
					for (uint64_t k = 0; k < total; ++k) {
						if (k && host[k].fpos <= host[k - 1].fpos) { printf("records out of order at %llu\n", (unsigned long long)k); return 1; }
						used += bsx_meth_bed_line(text + used, "chr1", 0, &M.opt, &host[k]);
						if (((k + 1) & 4095) == 0 || k + 1 == total) { if (pass) fwrite(text, 1, used, null); else fmt_bytes += used; used = 0; }
					}
					(pass ? fmt_file_ms : fmt_mem_ms) = now_ms() - t;
				}
				fmt_lines = total;
			}
			lines += total; t0 += w; ++windows;
		}
		printf("{\"what\": \"meth_sites\", \"mode\": \"%s\", \"genome_bp\": %lld, \"tiles\": %lld, \"count_ms_min\": %.3f, \"count_ms_median\": %.3f, \"count_ms_max\": %.3f, "
		       "\"counts_bytes\": %lld, \"counts_copy_ms\": %.3f, \"sums_ms\": %.3f, \"lines\": %llu, \"windows\": %d, \"emit_ms_total\": %.3f, \"record_bytes\": %llu, "
		       "\"records_copy_ms\": %.1f, \"records_GB_per_s\": %.2f, \"format_lines\": %llu, \"format_ms_per_million_lines\": %.2f, \"format_and_fwrite_ms_per_million_lines\": %.2f, "
		       "\"bytes_per_line\": %.1f}\n", M.name, l_pac, nt, ms[0], ms[1], ms[2], nt * 4, counts_ms, sums_ms, lines, windows, emit_ms, lines * 32ull, copy_ms,
		       copy_ms > 0 ? (double)lines * 32 / 1e6 / copy_ms : 0.0, fmt_lines, fmt_lines ? fmt_mem_ms * 1e6 / (double)fmt_lines : 0.0,
		       fmt_lines ? fmt_file_ms * 1e6 / (double)fmt_lines : 0.0, fmt_lines ? (double)fmt_bytes / (double)fmt_lines : 0.0);
		fflush(stdout);
	}
	return 0;
}
