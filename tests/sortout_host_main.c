/* tests/sortout_host_main.c -- a stand-alone program over the host side of --sort (csrc/host/sortout.c: keys from SAM lines, the host's stable
 * merge sort, the temporary file, the merge through per-run buffers, the header), meant to be built with -fsanitize=address,undefined and run
 * directly (tests/test_sortout_host.py does both).  Records with many equal keys, one of them longer than every buffer, go in as five chunks
 * (one of them empty) and come back through buffers of 1, 7 and 4 096 bytes, with the host's sort and with a backend that has the seam; the
 * result is compared with an insertion sort of all lines.  Then a file size limit makes the temporary file's write fail.  Prints "ok" and
 * returns 0, or says what differed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <signal.h>
#include <sys/resource.h>
#include "sortout.h"
#include "tune.h"

static int n_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++n_bad; } } while (0)

static const char HDR[] = "@SQ\tSN:b\tLN:100000\n@SQ\tLN:5\tSN:a\n@CO\tSN:c\n@SQ\tSN:chr_long_name\tLN:7\n@PG\tID:x\n";
static uint64_t rng = 88172645463325252ull;
static uint64_t rnd(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

static void keys_of_lines(void)
{
	bsx_sorter_t *s = 0;
	static const struct { const char *line; uint64_t key; } R[] = {
		{"r\t0\tb\t17\t60\t4M\n", BSX_SORT_KEY(0, 17, 0)}, {"r\t16\ta\t17\t60\n", BSX_SORT_KEY(1, 17, 1)}, {"r\t147\tchr_long_name\t2147483647", BSX_SORT_KEY(2, 2147483647u, 1)},
		{"r\t77\t*\t0\t0\t*\n", BSX_SORT_KEY(0xffffffffu, 0, 0)}, {"r\t133\tb\t40\t0\t*\n", BSX_SORT_KEY(0, 40, 0)}, {"r\t0\tc\t5\t0\n", BSX_SORT_KEY(0xffffffffu, 5, 0)},
		{"r\t0\tchr_long\t5\t0\n", BSX_SORT_KEY(0xffffffffu, 5, 0)}, {"no fields\n", ~0ull}, {"\n", ~0ull}, {"r\t16\tb\n", ~0ull},
	};
	size_t i;
	CHECK(bsx_sorter_open_backend(0, HDR, 0, &s) == BSX_OK && s, "open");
	for (i = 0; i < sizeof(R) / sizeof(R[0]); ++i) {
		const uint64_t k = bsx_sorter_key(s, R[i].line, strlen(R[i].line));
		CHECK(k == R[i].key, "key of line %zu: %llx, expected %llx", i, (unsigned long long)k, (unsigned long long)R[i].key);
	}
	bsx_sorter_close(s);
	CHECK(bsx_sorter_open_backend(0, "", 0, &s) == BSX_OK, "open without @SQ lines");
	CHECK(bsx_sorter_key(s, "r\t0\tb\t3\n", 8) == BSX_SORT_KEY(0xffffffffu, 3, 0), "no table: every name ranks last");
	bsx_sorter_close(s);
	CHECK(bsx_sorter_dir_ok("/nonexistent/dir") == BSX_E_IO && bsx_sorter_open_backend(0, HDR, "/nonexistent/dir", &s) == BSX_E_IO && !s, "a directory that is not there");
}

static void host_perm(void)
{
	static const int N[] = {0, 1, 2, 3, 64, 100, 1000, 4097};
	size_t t;
	for (t = 0; t < sizeof(N) / sizeof(N[0]); ++t) {
		const int n = N[t];
		uint64_t *k = (uint64_t*)malloc((size_t)(n + 1) * 8);
		uint32_t *p = (uint32_t*)malloc((size_t)(n + 1) * 8);
		int i;
		for (i = 0; i < n; ++i) k[i] = rnd() % 17 == 0 ? ~0ull : rnd() % (uint64_t)(n / 3 + 2);
		bsx_sort_host_perm(n, k, p, p + n);
		for (i = 1; i < n; ++i) CHECK(k[p[i - 1]] < k[p[i]] || (k[p[i - 1]] == k[p[i]] && p[i - 1] < p[i]), "n %d: position %d out of stable order", n, i);
		free(k); free(p);
	}
}

/* the records of the run: chunk by chunk */
#define N_CHUNKS 5
typedef struct { char *text; size_t len; } chunk_t;
static chunk_t g_chunk[N_CHUNKS];
static char **g_line; static size_t g_n_lines;

static void make_records(void)
{
	static const int per[N_CHUNKS] = {300, 1, 0, 257, 40};
	static const char *names[] = {"b", "a", "chr_long_name", "*", "b"};
	int c, i, serial = 0;
	size_t m = 0;
	for (c = 0; c < N_CHUNKS; ++c) m += (size_t)per[c];
	g_line = (char**)calloc(m, sizeof(char*));
	for (c = 0; c < N_CHUNKS; ++c) {
		size_t cap = 1 << 20, at = 0;
		g_chunk[c].text = (char*)malloc(cap);
		for (i = 0; i < per[c]; ++i, ++serial) {
			const int body = serial == 123 ? 10000 : (int)(rnd() % 60), rev = (int)(rnd() & 1);
			const char *nm = names[rnd() % 5];
			const int pos = nm[0] == '*' ? 0 : 1 + (int)(rnd() % 40);
			int l, j;
			if (at + (size_t)body + 256 > cap) { cap *= 2; g_chunk[c].text = (char*)realloc(g_chunk[c].text, cap); }
			l = sprintf(g_chunk[c].text + at, "read%d\t%d\t%s\t%d\t60\t*\t*\t0\t0\t", serial, rev ? 16 : 0, nm, pos);
			for (j = 0; j < body; ++j) g_chunk[c].text[at + (size_t)l + (size_t)j] = "ACGT"[rnd() & 3];
			g_chunk[c].text[at + (size_t)l + (size_t)body] = '\n';
			l += body + 1;
			g_line[g_n_lines] = (char*)malloc((size_t)l + 1);
			memcpy(g_line[g_n_lines], g_chunk[c].text + at, (size_t)l);
			g_line[g_n_lines++][l] = 0;
			at += (size_t)l;
		}
		g_chunk[c].len = at;
	}
}

typedef struct { char *a; size_t n, m; int pieces, bad_piece; } sink_t;
static int sink(void *ud, const char *text, size_t len)
{
	sink_t *k = (sink_t*)ud;
	if (len == 0 || text[len - 1] != '\n') k->bad_piece = 1;   /* pieces of whole lines */
	if (k->n + len + 1 > k->m) { k->m = (k->n + len + 1) * 2; k->a = (char*)realloc(k->a, k->m); }
	memcpy(k->a + k->n, text, len);
	k->n += len; k->a[k->n] = 0; ++k->pieces;
	return 0;
}
static int sink_refuses(void *ud, const char *text, size_t len) { (void)ud; (void)text; (void)len; return 1; }

/* a backend that has the seam: the same permutation by the host's sort, the runs kept here */
static struct { uint64_t *keys[16]; int64_t n[16]; int n_runs, resets; } g_fake;
static int fake_sort(void *ctx, int op, int64_t n, const uint64_t *keys, uint32_t *perm, int64_t *n_total, uint32_t **run_of)
{
	int r;
	int64_t i, o = 0, tot = 0;
	(void)ctx;
	if (op == BSX_SORT_OP_RESET) { for (r = 0; r < g_fake.n_runs; ++r) free(g_fake.keys[r]); g_fake.n_runs = 0; ++g_fake.resets; return BSX_OK; }
	if (op == BSX_SORT_OP_RUN) {
		uint32_t *tmp = (uint32_t*)malloc((size_t)n * 4);
		uint64_t *sk = (uint64_t*)malloc((size_t)n * 8);
		bsx_sort_host_perm(n, keys, perm, tmp);
		for (i = 0; i < n; ++i) sk[i] = keys[perm[i]];
		free(tmp);
		g_fake.keys[g_fake.n_runs] = sk; g_fake.n[g_fake.n_runs++] = n;
		return BSX_OK;
	}
	for (r = 0; r < g_fake.n_runs; ++r) tot += g_fake.n[r];
	{
		uint64_t *cat = (uint64_t*)malloc((size_t)tot * 8 + 8);
		uint32_t *perm2 = (uint32_t*)malloc((size_t)tot * 8 + 8), *out = (uint32_t*)malloc((size_t)tot * 4 + 4), *rid = (uint32_t*)malloc((size_t)tot * 4 + 4);
		for (r = 0; r < g_fake.n_runs; ++r) for (i = 0; i < g_fake.n[r]; ++i, ++o) { cat[o] = g_fake.keys[r][i]; rid[o] = (uint32_t)r; }
		bsx_sort_host_perm(tot, cat, perm2, perm2 + tot);
		for (i = 0; i < tot; ++i) out[i] = rid[perm2[i]];
		free(cat); free(perm2); free(rid);
		*n_total = tot; *run_of = out;
	}
	return BSX_OK;
}

static char *expected(bsx_sorter_t *s, size_t *len)
{
	size_t i, j, tot = 0;
	uint64_t *k = (uint64_t*)malloc(g_n_lines * 8);
	size_t *ord = (size_t*)malloc(g_n_lines * sizeof(size_t));
	char *out;
	for (i = 0; i < g_n_lines; ++i) { k[i] = bsx_sorter_key(s, g_line[i], strlen(g_line[i])); tot += strlen(g_line[i]); }
	for (i = 0; i < g_n_lines; ++i) { /* insertion sort: behind every line whose key is not larger */
		for (j = i; j > 0 && k[ord[j - 1]] > k[i]; --j) ord[j] = ord[j - 1];
		ord[j] = i;
	}
	out = (char*)malloc(tot + 1);
	for (i = 0, tot = 0; i < g_n_lines; ++i) { memcpy(out + tot, g_line[ord[i]], strlen(g_line[ord[i]])); tot += strlen(g_line[ord[i]]); }
	out[tot] = 0; *len = tot;
	free(k); free(ord);
	return out;
}

static void through_the_file(void)
{
	static const char *bufs[] = {"1", "7", "4096", 0};   /* (0: the default) */
	int b, with_be, c;
	for (with_be = 0; with_be < 2; ++with_be) for (b = 0; b < 4; ++b) {
		bsx_sorter_t *s = 0;
		bsx_backend_t be;
		sink_t k;
		char *want;
		size_t want_len;
		uint64_t nr, nrec;
		memset(&be, 0, sizeof(be)); memset(&k, 0, sizeof(k));
		be.sort_batch = fake_sort;
		bsx_tune_set("sort_buf_bytes", bufs[b]);
		CHECK(bsx_sorter_open_backend(with_be ? &be : 0, HDR, 0, &s) == BSX_OK, "open");
		for (c = 0; c < N_CHUNKS; ++c) CHECK(bsx_sorter_add(s, g_chunk[c].text, g_chunk[c].len) == BSX_OK, "add chunk %d", c);
		bsx_sorter_counts(s, &nr, &nrec);
		CHECK(nr == N_CHUNKS - 1 && nrec == g_n_lines, "%llu runs, %llu records", (unsigned long long)nr, (unsigned long long)nrec);   /* the empty chunk is no run */
		CHECK(bsx_sorter_finish(s, sink, &k) == BSX_OK, "finish (buffer %s)", bufs[b] ? bufs[b] : "default");
		want = expected(s, &want_len);
		CHECK(k.n == want_len && memcmp(k.a, want, want_len) == 0, "backend %d, buffer %s: the merged text differs", with_be, bufs[b] ? bufs[b] : "default");
		CHECK(!k.bad_piece && k.pieces >= 1, "pieces");
		CHECK(bsx_sorter_finish(s, sink_refuses, 0) == BSX_E_IO, "a sink that refuses");
		bsx_sorter_close(s);
		free(want); free(k.a);
	}
	CHECK(g_fake.resets == 8 && g_fake.n_runs == 0, "the backend's runs are freed at open and at close (%d resets)", g_fake.resets);
	bsx_tune_set("sort_buf_bytes", 0);
	{ /* nothing added: nothing comes out */
		bsx_sorter_t *s = 0;
		sink_t k;
		memset(&k, 0, sizeof(k));
		CHECK(bsx_sorter_open_backend(0, HDR, 0, &s) == BSX_OK && bsx_sorter_add(s, "", 0) == BSX_OK && bsx_sorter_finish(s, sink, &k) == BSX_OK && k.pieces == 0, "an empty run");
		bsx_sorter_close(s);
	}
}

static void headers(void)
{
	static const char *R[][2] = {
		{"@SQ\tSN:a\tLN:1\n@PG\tID:x\n", "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:1\n@PG\tID:x\n"},
		{"@SQ\tSN:a\tLN:1\n@HD\tVN:1.5\tSO:unsorted\tGO:none\n@CO\tx\n", "@HD\tVN:1.5\tSO:coordinate\tGO:none\n@SQ\tSN:a\tLN:1\n@CO\tx\n"},
		{"@HD\tVN:1.6\n@SQ\tSN:a\tLN:1\n", "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:1\n"},
		{"@HD\n", "@HD\tSO:coordinate\n"}, {"", "@HD\tVN:1.6\tSO:coordinate\n"}, {"@HDX\tSO:none\n", "@HD\tVN:1.6\tSO:coordinate\n@HDX\tSO:none\n"},
	};
	size_t i;
	for (i = 0; i < sizeof(R) / sizeof(R[0]); ++i) {
		char *h = bsx_sort_header(R[i][0]);
		CHECK(h && strcmp(h, R[i][1]) == 0, "header %zu: \"%s\"", i, h ? h : "(null)");
		free(h);
	}
}

static void a_write_that_fails(void)
{
	struct rlimit lim = {4096, 4096};
	bsx_sorter_t *s = 0;
	sink_t k;
	memset(&k, 0, sizeof(k));
	signal(SIGXFSZ, SIG_IGN);
	CHECK(bsx_sorter_open_backend(0, HDR, 0, &s) == BSX_OK, "open");
	CHECK(setrlimit(RLIMIT_FSIZE, &lim) == 0, "setrlimit");
	CHECK(bsx_sorter_add(s, g_chunk[0].text, g_chunk[0].len) == BSX_E_IO, "a chunk larger than the file may get");
	CHECK(bsx_sorter_add(s, g_chunk[1].text, g_chunk[1].len) == BSX_E_IO && bsx_sorter_finish(s, sink, &k) == BSX_E_IO && k.pieces == 0, "nothing after a failed write");
	bsx_sorter_close(s);
}

int main(void)
{
	size_t i;
	int c;
	keys_of_lines();
	host_perm();
	headers();
	make_records();
	through_the_file();
	a_write_that_fails();
	for (i = 0; i < g_n_lines; ++i) free(g_line[i]);
	free(g_line);
	for (c = 0; c < N_CHUNKS; ++c) free(g_chunk[c].text);
	if (n_bad) { fprintf(stderr, "%d checks failed\n", n_bad); return 1; }
	printf("ok\n");
	return 0;
}
