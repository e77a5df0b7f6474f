/* Stand-alone program over csrc/host/bam.c and bam_rec.h (tests/test_bam_host.py builds it with AddressSanitizer and
 * UndefinedBehaviorSanitizer): the host statement of --bam's record rule on the hand-worked lines of tests/test_bam_model.py (the same expected
 * bytes), every refusal, the name table's search, the header part, and the writer -- pieces of 1 byte to 1 MB over the same text must give the
 * same file, every member must inflate (zlib, gzip framing) to 0xff00 bytes but the header's and the last, a refused line stops everything
 * behind it, a failing sink is BSX_E_IO from then on.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "bam.h"
#include "tune.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

int bsx_hip_backend(bsx_device_t *dev, bsx_backend_t *out) { (void)dev; (void)out; return BSX_E_NODEVICE; }   /* (no device in this program) */

static const char HDR[] = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:300000000\n@SQ\tSN:chr2\tLN:5000\n@SQ\tSN:chr1\tLN:7\n@PG\tID:x\n";
static const char R1[] = "r1\t99\tchr1\t100\t60\t5M\t=\t200\t105\tACGTN\tIIIII\tNM:i:0";
static const char B1[] = "3300000000000000630000" "00033c49120100630005000000" "00000000c700000069000000" "72310050000000" "1248f02828282828" "4e4d4300";
static const char R2[] = "r2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*";
static const char B2[] = "23000000ffffffffffffffff0300481200000400" "00000000ffffffffffffffff00000000723200";
static const char R3[] = "r3\t147\tchr2\t1\t0\t2S3M\tchr1\t5\t-7\tACGTA\t*\tXA:A:x\tPA:f:0.500\tZZ:Z:hi\tXN:i:-129";
static const char B3[] = "490000000100000000000000030049120200930005000000" "0000000004000000f9ffffff723300" "2400000030000000124810ffffffffff"
                         "58414178" "5041660000003f" "5a5a5a686900" "584e737fff";

typedef struct { uint8_t *a; size_t n, m; int fail_after, calls, headers; } buf_t;
static int sink(void *ud, const void *data, size_t len, int is_header)
{
	buf_t *b = (buf_t*)ud;
	if (b->fail_after >= 0 && b->calls++ >= b->fail_after) return 1;
	if (is_header) { CHECK(b->n == 0); ++b->headers; }
	if (b->n + len > b->m) { b->m = (b->n + len) * 2; b->a = (uint8_t*)realloc(b->a, b->m); }
	memcpy(b->a + b->n, data, len); b->n += len;
	return 0;
}

static size_t unhex(const char *h, uint8_t *o)
{
	size_t n = 0;
	unsigned v;
	for (; h[0] && h[1]; h += 2) { sscanf(h, "%2x", &v); o[n++] = (uint8_t)v; }
	return n;
}

/* encode `text` (whole lines) with the host statement; returns the payload (malloc'd) */
static uint8_t *encode(const bsx_bam_refs_t *refs, const char *text, size_t *n, int64_t *n_rec, int64_t *bad, int *why)
{
	uint8_t *out = 0;
	size_t cap = 0;
	CHECK(bsx_bam_encode(0, refs, text, strlen(text), &out, &cap, n, n_rec, bad, why) == BSX_OK);
	return out;
}

static void expect_record(const bsx_bam_refs_t *refs, const char *line, const char *hex)
{
	uint8_t want[512], *got;
	char text[600];
	size_t nw = unhex(hex, want), n;
	int64_t n_rec, bad;
	int why;
	snprintf(text, sizeof(text), "%s\n", line);
	got = encode(refs, text, &n, &n_rec, &bad, &why);
	CHECK(bad == -1 && n_rec == 1 && n == nw && memcmp(got, want, n) == 0);
	free(got);
}

static void expect_refused(const bsx_bam_refs_t *refs, const char *line, int code)
{
	char *text = (char*)malloc(strlen(line) + 400);
	uint8_t w1[512], w2[512], *got;
	size_t n1 = unhex(B1, w1), n2 = unhex(B2, w2), n;
	int64_t n_rec, bad;
	int why;
	sprintf(text, "%s\n%s\n%s\n%s\n", R1, R2, line, R3);
	got = encode(refs, text, &n, &n_rec, &bad, &why);
	if (!(bad == 2 && why == code)) fprintf(stderr, "line %.60s: bad %ld why %d, expected %d\n", line, (long)bad, why, code);
	CHECK(bad == 2 && why == code && n_rec == 2 && n == n1 + n2 && memcmp(got, w1, n1) == 0 && memcmp(got + n1, w2, n2) == 0);
	CHECK(bsx_bam_strerror(code)[0] != 'u');
	free(got); free(text);
}

/* the members of a BGZF file, inflated: payload (malloc'd), sizes of the members' payloads */
static uint8_t *inflate_all(const uint8_t *d, size_t n, size_t *n_pay, size_t *sizes, int *n_sizes)
{
	uint8_t *pay = (uint8_t*)malloc(n * 40 + 65536);
	size_t at = 0, w = 0;
	*n_sizes = 0;
	while (at < n) {
		z_stream z;
		size_t bsize;
		CHECK(at + 28 <= n && d[at] == 0x1f && d[at + 1] == 0x8b && d[at + 2] == 8 && d[at + 3] == 4 && d[at + 12] == 'B' && d[at + 13] == 'C');
		bsize = (size_t)d[at + 16] + ((size_t)d[at + 17] << 8) + 1;
		CHECK(at + bsize <= n);
		memset(&z, 0, sizeof(z));
		CHECK(inflateInit2(&z, 31) == Z_OK);
		z.next_in = (Bytef*)(d + at); z.avail_in = (uInt)bsize; z.next_out = pay + w; z.avail_out = 65536;
		CHECK(inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_in == 0);   /* one whole gzip member: zlib has checked CRC32 and ISIZE */
		inflateEnd(&z);
		sizes[(*n_sizes)++] = z.total_out;
		w += z.total_out; at += bsize;
	}
	*n_pay = w;
	return pay;
}

static char *make_text(int n_lines, size_t *len)
{
	char *t = (char*)malloc((size_t)n_lines * 200 + 1);
	size_t at = 0;
	int i;
	for (i = 0; i < n_lines; ++i)
		at += (size_t)sprintf(t + at, "read%07d\t%d\tchr%d\t%d\t%d\t20M1I9M\t=\t%d\t%d\tACGTACGTACGTACGTACGTACGTACGTAC\tFFFFFFFFFFFFFFF,,,,:::::FFFFF#\tNM:i:%d\tPA:f:0.%03d\tYD:A:f\tMD:Z:%dA%d\n",
		                      i, i % 3 ? 99 : 147, 1 + i % 2, 1000 + i * 7, i % 61, 1100 + i * 7, i % 2 ? -130 : 130, i % 300 - 3, i % 1000, i % 29, 28 - i % 29);
	*len = at;
	return t;
}

static void run_writer(const char *text, size_t len, const char *piece, size_t call, buf_t *out)
{
	bsx_bam_writer_t *w = 0;
	size_t at = 0;
	CHECK(bsx_tune_set("bam_piece_bytes", piece) == BSX_OK);
	memset(out, 0, sizeof(*out)); out->fail_after = -1;
	CHECK(bsx_bam_writer_open(0, HDR, sink, out, &w) == BSX_OK);
	while (at < len) { /* calls of about `call` bytes, whole lines */
		size_t e = at + call < len ? at + call : len;
		while (e < len && text[e - 1] != '\n') ++e;
		CHECK(bsx_bam_writer_add(w, text + at, e - at) == BSX_OK);
		at = e;
	}
	CHECK(bsx_bam_writer_close(w, 1) == BSX_OK);
	CHECK(out->headers == 1);
}

int main(void)
{
	bsx_bam_refs_t *refs = 0;
	uint8_t *h = 0, *pay, *want;
	size_t nh = 0, len, n_pay, n_want, sizes[4096];
	int n_sizes, i, why;
	int64_t n_rec, bad;
	char *text, name[300];
	static char line[140000];
	buf_t a, b;

	CHECK(bsx_bam_refs_open(HDR, &refs) == BSX_OK && refs->n == 2);
	CHECK(bsx_bam_header(HDR, &h, &nh) == BSX_OK && nh == 12 + strlen(HDR) + 3 * (8 + 5) && memcmp(h, "BAM\1", 4) == 0 && h[8 + strlen(HDR)] == 3);
	expect_record(refs, R1, B1); expect_record(refs, R2, B2); expect_record(refs, R3, B3);
	{
		static const struct { const char *tail; int code; } tags[] = {
			{"foo", BSX_BAM_E_TAG}, {"XX:H:1AE3", BSX_BAM_E_TAG}, {"XX:B:c,1,2", BSX_BAM_E_TAG}, {"XX:A:ab", BSX_BAM_E_TAG}, {"XX:i:", BSX_BAM_E_TAG}, {"XX:i:1x", BSX_BAM_E_TAG},
			{"XX:f:1e5", BSX_BAM_E_TAG}, {"XX:f:1.", BSX_BAM_E_TAG}, {"XX:f:1000000000000000", BSX_BAM_E_TAG}, {"", BSX_BAM_E_TAG}, {"X:i:1", BSX_BAM_E_TAG}, {"X", BSX_BAM_E_TAG},
			{"XX:i:4294967296", BSX_BAM_E_INT}, {"XX:i:-2147483649", BSX_BAM_E_INT}, {"XX:i:99999999999999999999", BSX_BAM_E_INT}};
		for (i = 0; i < (int)(sizeof(tags) / sizeof(tags[0])); ++i) { snprintf(line, sizeof(line), "%s\t%s", R1, tags[i].tail); expect_refused(refs, line, tags[i].code); }
	}
	memset(name, 'n', 255); name[255] = 0;
	snprintf(line, sizeof(line), "%s%s", name, R2 + 2); expect_refused(refs, line, BSX_BAM_E_NAME);
	snprintf(line, sizeof(line), "%s%s", name + 1, R2 + 2);                                      /* 254 bytes pass */
	{ char t[700]; size_t n; snprintf(t, sizeof(t), "%.600s\n", line); pay = encode(refs, t, &n, &n_rec, &bad, &why); CHECK(bad == -1 && n == 4 + 32 + 255 && pay[12] == 255); free(pay); }
	{ size_t at = (size_t)sprintf(line, "r\t0\tchr1\t1\t0\t"); for (i = 0; i < 32768; ++i) at += (size_t)sprintf(line + at, "1M1I"); sprintf(line + at, "\t*\t0\t0\t*\t*"); }
	expect_refused(refs, line, BSX_BAM_E_CIGAR);
	expect_refused(refs, "r1\t99\tchr3\t100\t60\t5M\t=\t200\t105\tACGTN\tIIIII", BSX_BAM_E_REF);
	expect_refused(refs, "r1\t99\tchr1\t100\t60\t5M\tchr\t200\t105\tACGTN\tIIIII", BSX_BAM_E_REF);
	expect_refused(refs, "r1\t99\tchr1\t100\t60\t5M\t=\t200\t105\tACGTN\tIIII", BSX_BAM_E_QUAL);
	expect_refused(refs, "r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*", BSX_BAM_E_LINE);
	expect_refused(refs, "", BSX_BAM_E_LINE);
	expect_refused(refs, "r\tx\tchr1\t1\t0\t*\t*\t0\t0\t*\t*", BSX_BAM_E_LINE);
	expect_refused(refs, "r\t0\tchr1\t1\t0\t3Q\t*\t0\t0\t*\t*", BSX_BAM_E_LINE);
	expect_refused(refs, "r\t0\tchr1\t\t0\t*\t*\t0\t0\t*\t*", BSX_BAM_E_LINE);
	expect_refused(refs, "r\t0\tchr1\t9999999999\t0\t*\t*\t0\t0\t*\t*", BSX_BAM_E_LINE);
	{ uint8_t *o = 0; size_t cap = 0, n = 0; CHECK(bsx_bam_encode(0, refs, "no newline", 10, &o, &cap, &n, &n_rec, &bad, &why) == BSX_E_ARG); CHECK(bsx_bam_encode(0, refs, "", 0, &o, &cap, &n, &n_rec, &bad, &why) == BSX_OK && n == 0 && n_rec == 0 && bad == -1); free(o); }
	bsx_bam_refs_close(refs);

	/* a table of a thousand names with common prefixes, out of name order, some twice: every name finds the first line that has it */
	{
		char *hdr = (char*)malloc(1100 * 40), *q = hdr;
		bsx_bam_refs_t *r2 = 0;
		for (i = 0; i < 1100; ++i) q += sprintf(q, "@SQ\tSN:c%d%s\tLN:%d\n", (i * 37) % 1000, i % 3 ? "" : "_alt", 1000 + i);
		CHECK(bsx_bam_refs_open(hdr, &r2) == BSX_OK);
		for (i = 0; i < 1100; ++i) {
			char t[400];
			size_t n;
			int j, first = -1;
			snprintf(name, sizeof(name), "c%d%s", (i * 37) % 1000, i % 3 ? "" : "_alt");
			for (j = 0; j < 1100 && first < 0; ++j) { char o[64]; snprintf(o, sizeof(o), "c%d%s", (j * 37) % 1000, j % 3 ? "" : "_alt"); if (strcmp(o, name) == 0) first = j; }
			snprintf(t, sizeof(t), "r\t0\t%.299s\t1\t0\t1M\t*\t0\t0\tA\t*\n", name);
			pay = encode(r2, t, &n, &n_rec, &bad, &why);
			CHECK(bad == -1 && (int)(pay[4] | pay[5] << 8) == first);
			free(pay);
		}
		pay = encode(r2, "r\t0\tc\t1\t0\t1M\t*\t0\t0\tA\t*\n", &n_pay, &n_rec, &bad, &why); CHECK(bad == 0 && why == BSX_BAM_E_REF); free(pay);
		pay = encode(r2, "r\t0\tc9999\t1\t0\t1M\t*\t0\t0\tA\t*\n", &n_pay, &n_rec, &bad, &why); CHECK(bad == 0 && why == BSX_BAM_E_REF); free(pay);
		bsx_bam_refs_close(r2); free(hdr);
	}

	/* the writer: the same file whatever the pieces and the calls */
	text = make_text(3000, &len);
	CHECK(bsx_bam_refs_open(HDR, &refs) == BSX_OK);
	want = encode(refs, text, &n_want, &n_rec, &bad, &why);
	CHECK(bad == -1 && n_rec == 3000 && n_want > 4 * BSX_BGZF_BLOCK);
	run_writer(text, len, "1048576", len, &a);
	pay = inflate_all(a.a, a.n, &n_pay, sizes, &n_sizes);
	CHECK(n_pay == nh + n_want && memcmp(pay, h, nh) == 0 && memcmp(pay + nh, want, n_want) == 0);
	CHECK(sizes[0] == nh && sizes[n_sizes - 1] == 0 && (size_t)n_sizes == 2 + (n_want + BSX_BGZF_BLOCK - 1) / BSX_BGZF_BLOCK);
	for (i = 1; i < n_sizes - 2; ++i) CHECK(sizes[i] == BSX_BGZF_BLOCK);
	CHECK(sizes[n_sizes - 2] == n_want % BSX_BGZF_BLOCK);
	CHECK(a.n >= 28 && a.a[a.n - 28] == 0x1f && a.a[a.n - 12] == 0x1b && a.a[a.n - 10] == 3);
	free(pay);
	{
		static const char *pieces[] = {"1", "100", "65280", "70001"};
		static const size_t calls[] = {1, 5000, 100000};
		int p, c;
		for (p = 0; p < 4; ++p) for (c = 0; c < 3; ++c) { run_writer(text, len, pieces[p], calls[c], &b); CHECK(b.n == a.n && memcmp(a.a, b.a, a.n) == 0); free(b.a); }
	}
	/* random bytes are stored: n + 31 bytes a member */
	{
		uint8_t *rnd = (uint8_t*)malloc(70000), *o = 0;
		size_t cap = 0, n = 0;
		uint32_t s = 12345;
		for (i = 0; i < 70000; ++i) { s = s * 1664525u + 1013904223u; rnd[i] = (uint8_t)(s >> 24); }
		CHECK(bsx_bgzf_deflate(0, rnd, 70000, &o, &cap, &n) == BSX_OK && n == 70000 + 2 * 31);
		pay = inflate_all(o, n, &n_pay, sizes, &n_sizes);
		CHECK(n_pay == 70000 && memcmp(pay, rnd, 70000) == 0 && n_sizes == 2 && sizes[0] == BSX_BGZF_BLOCK);
		CHECK(bsx_bgzf_deflate(0, rnd, 0, &o, &cap, &n) == BSX_OK && n == 0);
		free(pay); free(o); free(rnd);
	}
	/* a refused line in the fourth call: the record's index counts from the first record, nothing of its piece or behind it is written */
	{
		bsx_bam_writer_t *w = 0;
		size_t q = len / 4, before;
		int64_t rec;
		while (text[q - 1] != '\n') ++q;
		CHECK(bsx_tune_set("bam_piece_bytes", "1048576") == BSX_OK);
		memset(&b, 0, sizeof(b)); b.fail_after = -1;
		CHECK(bsx_bam_writer_open(0, HDR, sink, &b, &w) == BSX_OK);
		CHECK(bsx_bam_writer_add(w, text, q) == BSX_OK && b.n > 0);
		before = b.n;
		{ static const char badline[] = "x\t0\tchr9\t1\t0\t*\t*\t0\t0\t*\t*\n"; CHECK(bsx_bam_writer_add(w, badline, strlen(badline)) == BSX_E_FORMAT && b.n == before); }
		bsx_bam_writer_refused(w, &rec, &why);
		CHECK(why == BSX_BAM_E_REF && rec > 0 && text[q - 1] == '\n');
		{ int64_t nl = 0; size_t k; for (k = 0; k < q; ++k) nl += text[k] == '\n'; CHECK(rec == nl); }
		CHECK(bsx_bam_writer_add(w, text + q, len - q) == BSX_E_FORMAT && b.n == before);
		CHECK(bsx_bam_writer_close(w, 0) == BSX_OK && b.n == before);
		free(b.a);
		/* refused in the first piece: the sink has seen nothing, not even the header */
		memset(&b, 0, sizeof(b)); b.fail_after = -1;
		CHECK(bsx_bam_writer_open(0, HDR, sink, &b, &w) == BSX_OK);
		CHECK(bsx_bam_writer_add(w, "x\n", 2) == BSX_E_FORMAT && b.n == 0 && b.headers == 0);
		CHECK(bsx_bam_writer_close(w, 0) == BSX_OK && b.n == 0);
		/* a sink that fails at its third call */
		memset(&b, 0, sizeof(b)); b.fail_after = 2;
		CHECK(bsx_bam_writer_open(0, HDR, sink, &b, &w) == BSX_OK);
		CHECK(bsx_bam_writer_add(w, text, q) == BSX_OK);
		CHECK(bsx_bam_writer_add(w, text + q, len - q) == BSX_E_IO && bsx_bam_writer_add(w, text, q) == BSX_E_IO);
		CHECK(bsx_bam_writer_close(w, 1) == BSX_E_IO);
		free(b.a);
		/* no record at all: the header's block and the EOF block */
		memset(&b, 0, sizeof(b)); b.fail_after = -1;
		CHECK(bsx_bam_writer_open(0, HDR, sink, &b, &w) == BSX_OK && bsx_bam_writer_close(w, 1) == BSX_OK && b.headers == 1);
		pay = inflate_all(b.a, b.n, &n_pay, sizes, &n_sizes);
		CHECK(n_sizes == 2 && n_pay == nh && memcmp(pay, h, nh) == 0);
		free(pay); free(b.a);
	}
	bsx_bam_refs_close(refs);
	free(a.a); free(want); free(text); free(h);
	bsx_tune_set("bam_piece_bytes", 0);
	printf("ok\n");
	return 0;
}
