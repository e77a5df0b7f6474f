// sort_bench.hip -- what the sort behind --sort costs (k_sort.hip), beside rocprim::radix_sort_pairs on the same arrays in the same process:
//   bsx_sort_run on one chunk's records (1.1 M and 2.2 M genomic keys; without and with unmapped records, whose rank is all ones): the call
//   through the C ABI (upload, passes, the run kept, the permutation back) and the launches alone between two events;
//   bsx_sort_schedule over 50 such runs (110 M keys): the call, and rocprim on the concatenation with the run ids as values.
// Every result is compared with rocprim's (both sorts are stable: the outputs must be equal).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Iinclude -Ibiscuit_amd/csrc/host -Ibiscuit_amd/csrc/hip -o tools/ubench/sort_bench tools/ubench/sort_bench.hip \
//         -Lbiscuit_amd -lbiscuit_amd -Wl,-rpath,'$ORIGIN/../../biscuit_amd' && tools/ubench/sort_bench
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <vector>
#include <algorithm>
#include "../../biscuit_amd/csrc/hip/k_sort.hip"   // the launchers, for the launches alone (the library keeps them to itself)

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

// records of reads placed uniformly over a 3.1 Gbp genome of 25 contigs (ranks by position), both strands; `star` in 1000 unmapped
static void genomic(std::vector<uint64_t> &k, size_t n, int star)
{
	static const uint32_t len_mbp[25] = {248, 242, 198, 190, 181, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51, 156, 57, 16};
	k.resize(n);
	for (size_t i = 0; i < n; ++i) {
		if ((int)(rnd() % 1000) < star) { k[i] = BSX_SORT_KEY(0xffffffffu, 0, 0); continue; }
		uint64_t p = rnd() % 3100000000ull, r = 0;
		while (r < 24 && p >= (uint64_t)len_mbp[r] * 1000000) { p -= (uint64_t)len_mbp[r] * 1000000; ++r; }
		k[i] = BSX_SORT_KEY(r, p + 1, rnd() & 1);
	}
}
static int passes_of(const std::vector<uint64_t> &k)
{
	uint64_t bits = 0; int n = 0;
	for (uint64_t x : k) bits |= x ^ k[0];
	for (int s = 0; s < 64; s += 8) n += ((bits >> s) & 255) != 0;
	return n;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(void)
{
	bsx_device_t *dev = 0;
	if (bsx_device_open(0, &dev) != BSX_OK) { printf("no device\n"); return 1; }
	hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
	hipStream_t st; CHK(hipStreamCreate(&st));
	const size_t N[2] = {1100000, 2200000};
	for (int star = 0; star <= 30; star += 30) for (int t = 0; t < 2; ++t) {
		const size_t n = N[t];
		std::vector<uint64_t> keys; genomic(keys, n, star);
		std::vector<uint32_t> perm(n), ref(n);
		std::vector<double> t_call, t_kern, t_rp;
		uint64_t *dk[2], *rk[2]; uint32_t *dp[2], *rv[2], *counts, *btot; unsigned long long *bits_d; void *tmp = 0; size_t tb = 0;
		for (int i = 0; i < 2; ++i) { CHK(hipMalloc((void**)&dk[i], n * 8)); CHK(hipMalloc((void**)&dp[i], n * 4)); CHK(hipMalloc((void**)&rk[i], n * 8)); CHK(hipMalloc((void**)&rv[i], n * 4)); }
		CHK(hipMalloc((void**)&counts, sort_n_tiles((long long)n) * 256 * 4)); CHK(hipMalloc((void**)&btot, sort_n_scan_blocks((long long)n) * 4)); CHK(hipMalloc((void**)&bits_d, 8));
		for (int rep = 0; rep < 6; ++rep) { // the call through the ABI (the first one makes the buffers: not counted)
			bsx_sort_reset(dev);
			const double t0 = now();
			if (bsx_sort_run(dev, (int64_t)n, keys.data(), perm.data()) != BSX_OK) { printf("bsx_sort_run failed\n"); return 1; }
			if (rep) t_call.push_back((now() - t0) * 1e3);
		}
		int n_passes = 0;
		for (int rep = 0; rep < 6; ++rep) { // the launches alone, the skipped passes decided as the library decides them
			CHK(hipMemcpy(dk[0], keys.data(), n * 8, hipMemcpyHostToDevice));
			unsigned long long bits = 0; int cur = 0; n_passes = 0;
			CHK(hipEventRecord(e0, st));
			CHK(hipMemsetAsync(bits_d, 0, 8, st));
			launch_sort_bits(st, (const unsigned long long*)dk[0], (long long)n, bits_d);
			CHK(hipMemcpyAsync(&bits, bits_d, 8, hipMemcpyDeviceToHost, st)); CHK(hipStreamSynchronize(st));
			for (int s = 0; s < 64; s += 8) if ((bits >> s) & 255) {
				launch_sort_pass(st, (const unsigned long long*)dk[cur], n_passes ? dp[cur] : nullptr, (unsigned long long*)dk[cur ^ 1], dp[cur ^ 1], (long long)n, s, counts, btot);
				cur ^= 1; ++n_passes;
			}
			CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1));
			float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
			if (rep) t_kern.push_back(ms);
		}
		std::vector<uint32_t> iota(n); for (size_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
		CHK(hipMemcpy(rk[0], keys.data(), n * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(rv[0], iota.data(), n * 4, hipMemcpyHostToDevice));
		CHK(rocprim::radix_sort_pairs(nullptr, tb, rk[0], rk[1], rv[0], rv[1], n, 0u, 64u, st)); CHK(hipMalloc(&tmp, tb));
		for (int rep = 0; rep < 6; ++rep) {
			CHK(hipEventRecord(e0, st));
			CHK(rocprim::radix_sort_pairs(tmp, tb, rk[0], rk[1], rv[0], rv[1], n, 0u, 64u, st));
			CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1));
			float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
			if (rep) t_rp.push_back(ms);
		}
		CHK(hipMemcpy(ref.data(), rv[1], n * 4, hipMemcpyDeviceToHost));
		printf("{\"what\": \"sort_run\", \"n\": %zu, \"unmapped_per_1000\": %d, \"passes_run\": %d, \"passes_skipped\": %d, \"call_ms\": %.3f, \"kernels_ms\": %.3f, \"rocprim_ms\": %.3f, \"equal_to_rocprim\": %s}\n",
		       n, star, n_passes, 8 - n_passes, median(t_call), median(t_kern), median(t_rp), perm == ref ? "true" : "false");
		if (n_passes != passes_of(keys)) printf("passes: %d on the device, %d by the host's count\n", n_passes, passes_of(keys));
		for (int i = 0; i < 2; ++i) { CHK(hipFree(dk[i])); CHK(hipFree(dp[i])); CHK(hipFree(rk[i])); CHK(hipFree(rv[i])); }
		CHK(hipFree(counts)); CHK(hipFree(btot)); CHK(hipFree(bits_d)); CHK(hipFree(tmp));
	}
	{ // the schedule over 50 runs of 2.2 M
		const int R = 50; const size_t n = N[1], tot = n * R;
		std::vector<uint64_t> cat(tot), keys; std::vector<uint32_t> perm(n), rid(tot), ref(tot);
		bsx_sort_reset(dev);
		for (int r = 0; r < R; ++r) {
			genomic(keys, n, 30);
			if (bsx_sort_run(dev, (int64_t)n, keys.data(), perm.data()) != BSX_OK) { printf("bsx_sort_run failed\n"); return 1; }
			for (size_t i = 0; i < n; ++i) { cat[(size_t)r * n + i] = keys[perm[i]]; rid[(size_t)r * n + i] = (uint32_t)r; }
		}
		std::vector<double> t_call, t_rp;
		bool equal = true;
		uint64_t *rk[2]; uint32_t *rv[2]; void *tmp = 0; size_t tb = 0;
		for (int i = 0; i < 2; ++i) { CHK(hipMalloc((void**)&rk[i], tot * 8)); CHK(hipMalloc((void**)&rv[i], tot * 4)); }
		CHK(hipMemcpy(rk[0], cat.data(), tot * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(rv[0], rid.data(), tot * 4, hipMemcpyHostToDevice));
		CHK(rocprim::radix_sort_pairs(nullptr, tb, rk[0], rk[1], rv[0], rv[1], tot, 0u, 64u, st)); CHK(hipMalloc(&tmp, tb));
		for (int rep = 0; rep < 4; ++rep) {
			CHK(hipEventRecord(e0, st));
			CHK(rocprim::radix_sort_pairs(tmp, tb, rk[0], rk[1], rv[0], rv[1], tot, 0u, 64u, st));
			CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1));
			float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
			if (rep) t_rp.push_back(ms);
		}
		CHK(hipMemcpy(ref.data(), rv[1], tot * 4, hipMemcpyDeviceToHost));
		for (int rep = 0; rep < 4; ++rep) {
			int64_t nt = 0; uint32_t *run_of = 0;
			const double t0 = now();
			if (bsx_sort_schedule(dev, &nt, &run_of) != BSX_OK) { printf("bsx_sort_schedule failed\n"); return 1; }
			if (rep) t_call.push_back((now() - t0) * 1e3);
			equal = equal && (size_t)nt == tot && memcmp(run_of, ref.data(), tot * 4) == 0;
			free(run_of);
		}
		printf("{\"what\": \"sort_schedule\", \"runs\": %d, \"n\": %zu, \"passes_run\": %d, \"call_ms\": %.3f, \"rocprim_ms\": %.3f, \"equal_to_rocprim\": %s}\n",
		       R, tot, passes_of(cat), median(t_call), median(t_rp), equal ? "true" : "false");
	}
	bsx_device_close(dev);
	return 0;
}
