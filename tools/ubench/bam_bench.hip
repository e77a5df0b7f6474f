// bam_bench.hip -- what the two stages behind --bam cost on a chunk-sized text (k_bam.hip, k_bgzf.hip): N records (default 1 066 666, a
// chunk of 2 x 150 bp) of synthetic SAM as the aligner writes it -- 25 contigs, 150M or a small indel, random bases, binned qualities in
// runs, the aligner's tags -- uploaded once; then every kernel between two events, medians of five: the newline counts, the one-workgroup
// scan, the line starts, the size pass with the refusal reduction, the scan of the sizes, the emit pass; the deflate launches (1024 blocks
// each) and the compaction over the payload that came out.  Prints the times, the bytes per record in and out, and zlib level 1's size over
// the first 64 blocks for comparison (host, one thread, timed).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ibiscuit_amd/csrc/host -Ibiscuit_amd/csrc/hip tools/ubench/bam_bench.hip -o tools/ubench/bam_bench -lz && tools/ubench/bam_bench [records]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <string>
#include <algorithm>
#include <chrono>
#include <zlib.h>
#include "bsx.h"
#include "../../biscuit_amd/csrc/hip/k_bam.hip"    // the launchers (the library keeps them to itself)
#include "../../biscuit_amd/csrc/hip/k_bgzf.hip"

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static uint64_t g_s = 88172645463325252ull;
static inline uint32_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (uint32_t)(g_s >> 11); }

template<class F> static int timed(const char *what, hipEvent_t a, hipEvent_t b, F f)
{
	std::vector<float> ms;
	for (int r = 0; r < 5; ++r) {
		CHK(hipEventRecord(a, 0)); f(); CHK(hipGetLastError()); CHK(hipEventRecord(b, 0)); CHK(hipEventSynchronize(b));
		float t = 0; CHK(hipEventElapsedTime(&t, a, b)); ms.push_back(t);
	}
	std::sort(ms.begin(), ms.end());
	printf("%-28s %9.3f ms (min %.3f, max %.3f)\n", what, ms[2], ms[0], ms[4]);
	return 0;
}

int main(int argc, char **argv)
{
	const long long n_rec = argc > 1 ? atoll(argv[1]) : 1066666;
	hipDeviceProp_t prop;
	CHK(hipGetDeviceProperties(&prop, 0));
	const int n_cu = prop.multiProcessorCount;
	// the name table: chr1 .. chr25, sorted bytewise
	std::vector<std::string> names;
	for (int i = 1; i <= 25; ++i) names.push_back("chr" + std::to_string(i));
	std::vector<int> order(25);
	for (int i = 0; i < 25; ++i) order[i] = i;
	std::sort(order.begin(), order.end(), [&](int x, int y) { return names[x] < names[y]; });
	std::string blob; std::vector<uint32_t> noff; std::vector<int32_t> nid;
	for (int k : order) { noff.push_back((uint32_t)blob.size()); blob += names[k]; nid.push_back(k); }
	noff.push_back((uint32_t)blob.size());
	// the text
	std::string text;
	text.reserve((size_t)n_rec * 520);
	char line[1024], seq[151], qual[151];
	static const char QB[4] = {'F', ':', ',', '#'};
	for (long long i = 0; i < n_rec; ++i) {
		const int rev = (int)(rnd() & 1), second = (int)(i & 1), contig = 1 + (int)(rnd() % 25);
		const long pos = 1 + (long)(rnd() % 120000000u);
		for (int k = 0; k < 150; ) { const char q = QB[(rnd() % 16) < 12 ? 0 : 1 + rnd() % 3]; int run = 1 + (int)(rnd() % 24); while (run-- && k < 150) qual[k++] = q; }
		for (int k = 0; k < 150; ++k) seq[k] = "ACGT"[rnd() & 3];
		seq[150] = qual[150] = 0;
		const int indel = (int)(rnd() % 10) == 0, a = 20 + (int)(rnd() % 100);
		char cig[32];
		if (indel) snprintf(cig, sizeof(cig), "%dM1I%dM", a, 149 - a); else snprintf(cig, sizeof(cig), "150M");
		const int nm = (int)(rnd() % 6), zc = (int)(rnd() % 40), zr = (int)(rnd() % 6), as = 150 - 5 * nm, tl = 200 + (int)(rnd() % 200);
		const int n = snprintf(line, sizeof(line), "read%09lld\t%d\tchr%d\t%ld\t%d\t%s\t=\t%ld\t%d\t%s\t%s\tNM:i:%d\tMD:Z:%d%c%d\tZC:i:%d\tZR:i:%d\tAS:i:%d\tXS:i:%d\tXL:i:150\tMC:Z:150M\tMQ:i:60\tYD:A:%c\n",
		                       i / 2, (second ? 128 : 64) | 1 | 2 | (rev ? 16 : 32), contig, pos, 60, cig, pos + (rev ? -tl : tl), rev ? -tl : tl, seq, qual, nm, a, "ACGT"[rnd() & 3],
		                       149 - a, zc, zr, as, (int)(rnd() % 60), rev ? 'r' : 'f');
		text.append(line, (size_t)n);
	}
	const long long len = (long long)text.size(), nt = bam_n_tiles(len);
	printf("device %s, %d CUs; %lld records, %lld bytes of SAM text (%.1f per record)\n", prop.name, n_cu, n_rec, len, (double)len / n_rec);
	char *d_text, *d_names; uint32_t *d_noff, *cnt, *start, *size; int32_t *d_nid; int *errs; unsigned long long *bad;
	const int lgrid = bam_lines_grid(n_rec);
	CHK(hipMalloc(&d_text, len + 16)); CHK(hipMalloc(&d_names, blob.size() + 16)); CHK(hipMalloc(&d_noff, noff.size() * 4)); CHK(hipMalloc(&d_nid, nid.size() * 4));
	CHK(hipMalloc(&cnt, (nt + 1) * 4)); CHK(hipMalloc(&start, (n_rec + 1) * 4)); CHK(hipMalloc(&size, (n_rec + 1) * 4)); CHK(hipMalloc(&errs, (n_rec + 1) * 4)); CHK(hipMalloc(&bad, (size_t)lgrid * 8));
	double t0 = now_ms();
	CHK(hipMemcpy(d_text, text.data(), len, hipMemcpyHostToDevice));
	printf("%-28s %9.3f ms (pageable host memory)\n", "text to the device", now_ms() - t0);
	CHK(hipMemcpy(d_names, blob.data(), blob.size(), hipMemcpyHostToDevice)); CHK(hipMemcpy(d_noff, noff.data(), noff.size() * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(d_nid, nid.data(), nid.size() * 4, hipMemcpyHostToDevice));
	hipEvent_t ea, eb;
	CHK(hipEventCreate(&ea)); CHK(hipEventCreate(&eb));
	if (timed("k_bam_count", ea, eb, [&] { launch_bam_count(0, n_cu, d_text, len, cnt); })) return 1;
	if (timed("k_bam_scan (tiles)", ea, eb, [&] { launch_bam_count(0, n_cu, d_text, len, cnt); launch_bam_scan(0, cnt, cnt, nt); })) return 1;   // (with the count pass: the scan is in place)
	uint32_t n_lines = 0;
	CHK(hipMemcpy(&n_lines, cnt + nt, 4, hipMemcpyDeviceToHost));
	if ((long long)n_lines != n_rec) { printf("%u lines counted\n", n_lines); return 1; }
	if (timed("k_bam_starts", ea, eb, [&] { launch_bam_starts(0, n_cu, d_text, len, cnt, start); })) return 1;
	if (timed("k_bam_lines (size) + refused", ea, eb, [&] { launch_bam_size(0, d_text, start, n_rec, d_names, d_noff, d_nid, 25, size, errs, bad); })) return 1;
	std::vector<unsigned long long> hb((size_t)lgrid);
	CHK(hipMemcpy(hb.data(), bad, (size_t)lgrid * 8, hipMemcpyDeviceToHost));
	for (unsigned long long v : hb) if (v != ~0ull) { printf("line %llu refused (%llu)\n", v >> 4, v & 15); return 1; }
	uint32_t *off; CHK(hipMalloc(&off, (n_rec + 1) * 4));
	if (timed("k_bam_scan (sizes)", ea, eb, [&] { launch_bam_scan(0, size, off, n_rec); })) return 1;
	uint32_t total = 0;
	CHK(hipMemcpy(&total, off + n_rec, 4, hipMemcpyDeviceToHost));
	uint8_t *pay; CHK(hipMalloc(&pay, (size_t)total + 16));
	if (timed("k_bam_lines (emit)", ea, eb, [&] { launch_bam_emit(0, d_text, start, n_rec, d_names, d_noff, d_nid, 25, errs, off, pay); })) return 1;
	printf("payload %u bytes (%.1f per record)\n", total, (double)total / n_rec);
	// stage 2
	const long long nb = ((long long)total + BSX_BGZF_BLOCK - 1) / BSX_BGZF_BLOCK;
	const int grid = bgzf_grid(nb);
	uint32_t *tok, *sizes, *ops; uint16_t *cand; uint8_t *slots, *out;
	CHK(hipMalloc(&tok, bgzf_tok_bytes(grid))); CHK(hipMalloc(&cand, bgzf_cand_bytes(grid))); CHK(hipMalloc(&slots, (size_t)nb * 65536)); CHK(hipMalloc(&sizes, (nb + 1) * 4)); CHK(hipMalloc(&ops, 1024));
	{ uint32_t h[256]; bgzf_crc_ops(h); CHK(hipMemcpy(ops, h, 1024, hipMemcpyHostToDevice)); }
	if (timed("k_bgzf_deflate", ea, eb, [&] { for (long long b0 = 0; b0 < nb; b0 += grid) launch_bgzf_deflate(0, pay, total, b0, (int)std::min<long long>(grid, nb - b0), ops, tok, cand, slots, sizes); })) return 1;
	if (timed("k_bam_scan (blocks)", ea, eb, [&] { launch_bam_scan(0, sizes, sizes, nb); })) return 1;
	for (long long b0 = 0; b0 < nb; b0 += grid) launch_bgzf_deflate(0, pay, total, b0, (int)std::min<long long>(grid, nb - b0), ops, tok, cand, slots, sizes);   // (the timed scans ran in place five times)
	launch_bam_scan(0, sizes, sizes, nb);
	uint32_t ctotal = 0;
	CHK(hipMemcpy(&ctotal, sizes + nb, 4, hipMemcpyDeviceToHost));
	CHK(hipMalloc(&out, ctotal));
	if (timed("k_bgzf_compact", ea, eb, [&] { launch_bgzf_compact(0, n_cu, slots, sizes, nb, out); })) return 1;
	printf("%lld blocks, %u compressed bytes (%.1f per record, %.1f %% of the payload, %.1f %% of the text)\n", nb, ctotal, (double)ctotal / n_rec, 100.0 * ctotal / total, 100.0 * ctotal / len);
	// zlib level 1 over the first blocks, for size and host time
	{
		const long long k = std::min<long long>(nb, 64);
		std::vector<uint8_t> hp((size_t)k * BSX_BGZF_BLOCK), hc((size_t)ctotal), z(70000);
		std::vector<uint32_t> hs((size_t)nb + 1);
		const size_t hn = (size_t)std::min<long long>((long long)hp.size(), total);
		CHK(hipMemcpy(hp.data(), pay, hn, hipMemcpyDeviceToHost)); CHK(hipMemcpy(hs.data(), sizes, (nb + 1) * 4, hipMemcpyDeviceToHost)); CHK(hipMemcpy(hc.data(), out, ctotal, hipMemcpyDeviceToHost));
		size_t zb = 0; long long blocks = 0;
		t0 = now_ms();
		for (size_t at = 0; at < hn; at += BSX_BGZF_BLOCK, ++blocks) {
			z_stream s; memset(&s, 0, sizeof(s));
			deflateInit2(&s, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
			s.next_in = hp.data() + at; s.avail_in = (uInt)std::min<size_t>(BSX_BGZF_BLOCK, hn - at); s.next_out = z.data(); s.avail_out = (uInt)z.size();
			deflate(&s, Z_FINISH); zb += s.total_out + 26; deflateEnd(&s);
		}
		const double zms = now_ms() - t0;
		printf("first %lld blocks: device %u bytes, zlib level 1 %zu bytes (ratio %.4f); zlib %.2f ms a block on one host core, %.0f core-ms for all %lld blocks\n", blocks, hs[blocks], zb,
		       (double)hs[blocks] / zb, zms / blocks, zms / blocks * nb, nb);
		// the device's first member must inflate to the payload's first block
		z_stream s; memset(&s, 0, sizeof(s)); inflateInit2(&s, 31);
		std::vector<uint8_t> back(70000);
		s.next_in = hc.data(); s.avail_in = hs[1]; s.next_out = back.data(); s.avail_out = (uInt)back.size();
		const int zr = inflate(&s, Z_FINISH);
		printf("first member inflates: %s\n", zr == Z_STREAM_END && s.total_out == std::min<size_t>(BSX_BGZF_BLOCK, hn) && memcmp(back.data(), hp.data(), s.total_out) == 0 ? "yes" : "NO");
		inflateEnd(&s);
	}
	return 0;
}
