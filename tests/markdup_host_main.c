/* tests/markdup_host_main.c -- a stand-alone program over the host side of duplicate marking (csrc/host/markdup.c: key construction, the host
 * table, the tickets), meant to be built with -fsanitize=address,undefined and run directly (tests/test_markdup_host.py does both).
 * It feeds the records of tests/test_markdup_model.py, then a few thousand random keys through a table that starts at 64 slots and grows,
 * in one batch and in several, with whole and with 8-bit claim words, against a quadratic search; then slices handed over out of order by
 * two threads.  Prints "ok" and returns 0, or says what differed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include "markdup.h"
#include "tune.h"

static int n_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++n_bad; } } while (0)

static int parse_cigar(const char *s, uint32_t *out)
{
	int n = 0;
	while (*s && *s != '*') {
		char *e;
		long len = strtol(s, &e, 10);
		const char *op = strchr("MIDSH", *e);
		out[n++] = (uint32_t)len << 4 | (uint32_t)(op - "MIDSH");
		s = e + 1;
	}
	return n;
}
static int64_t u5_of(uint64_t w) { return (int64_t)(w & 0x1ffffffffull) - BSX_MD_U5_BIAS; }
static uint64_t end_of(int rid, int64_t pos1, const char *cigar, int rev, int yd)   /* pos1: POS as the SAM has it */
{
	uint32_t cg[16];
	int n = parse_cigar(cigar, cg);
	return bsx_md_end_key(rid, pos1 - 1, rev, yd, n, cg);
}

static void keys_of_records(void)
{
	static const struct { int64_t pos; const char *cigar; int rev; int64_t u5; } R[] = {
		{100, "50M", 0, 100}, {100, "7S43M", 0, 93}, {100, "7H43M", 0, 93}, {100, "3H4S43M5S", 0, 93}, {3, "7S43M", 0, -4}, {100, "*", 0, 100},
		{100, "50M", 1, 149}, {100, "20M2D10M3I17M", 1, 148}, {100, "20M2D10M3I12M5S", 1, 148}, {100, "6S20M2D10M3I12M2S3H", 1, 148},
		{980, "40M10S", 1, 1029}, {112, "12S38M", 0, 100}, {300, "40M6S4H", 1, 349}, {51, "50M", 1, 100},
	};
	size_t i;
	for (i = 0; i < sizeof(R) / sizeof(R[0]); ++i) {
		const uint64_t w = end_of(2, R[i].pos, R[i].cigar, R[i].rev, 1);
		CHECK(u5_of(w) == R[i].u5, "record %zu: u5 %lld, expected %lld", i, (long long)u5_of(w), (long long)R[i].u5);
		CHECK((w & BSX_MD_PLACED) && !(w & BSX_MD_REVERSE) == !R[i].rev && (w & BSX_MD_YD) && ((w >> 33) & 0xfffffff) == 2, "record %zu: bits", i);
	}
	CHECK(end_of(0, 100, "50M", 0, 0) != end_of(0, 51, "50M", 1, 0), "same coordinate, other strand");
	CHECK(end_of(0, 100, "50M", 0, 0) != end_of(0, 100, "50M", 0, 1), "same coordinate, other YD");
	CHECK(end_of(0, 960, "41M5S", 1, 0) != end_of(1, 960, "41M5S", 1, 0), "overhangs on neighbouring contigs");
	CHECK(end_of(1, 1, "5S45M", 0, 0) != end_of(0, 996, "50M", 0, 0), "a negative u5 against the contig before");
	CHECK(end_of(0, 100, "50M", 0, 0) != 0 && end_of(0, 100, "50M", 0, 0) != BSX_MD_SINGLE, "a placed end is neither absent nor the single-read mark");
}

static uint64_t rng_s = 88172645463325252ull;
static uint64_t rng(void) { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }

static void naive(int64_t n, const bsx_markdup_key_t *k, uint8_t *out)
{
	int64_t i, j;
	for (i = 0; i < n; ++i) {
		out[i] = 0;
		if (k[i].w[0] == ~0ull && k[i].w[1] == ~0ull) continue;
		for (j = 0; j < i && !out[i]; ++j) out[i] = k[j].w[0] == k[i].w[0] && k[j].w[1] == k[i].w[1];
	}
}
static void table_runs(int64_t n, int universe, const char *bits, int step)
{
	bsx_markdup_key_t *k = (bsx_markdup_key_t*)malloc(sizeof(*k) * (size_t)n);
	uint8_t *want = (uint8_t*)malloc((size_t)n), *got = (uint8_t*)malloc((size_t)n);
	bsx_md_table_t T;
	int64_t i, a;
	memset(&T, 0, sizeof(T));
	for (i = 0; i < n; ++i) {
		const uint64_t v = rng() % (uint64_t)universe;
		k[i].w[0] = BSX_MD_END(v % 5, 1000 + (int64_t)(v / 5) - 2000, v & 1, (v >> 1) & 1);
		k[i].w[1] = v % 3 == 0 ? 0 : v % 3 == 1 ? BSX_MD_SINGLE : BSX_MD_END(v % 5, 1300 + (int64_t)(v / 5), 1, 0);
		if (rng() % 16 == 0) k[i].w[0] = k[i].w[1] = ~0ull;
	}
	naive(n, k, want);
	bsx_tune_set("markdup_slots", "64");
	bsx_tune_set("markdup_hash_bits", bits);
	for (a = 0; a < n; a += step) {
		const int rc = bsx_md_table_batch(&T, a + step <= n ? step : n - a, k + a, (uint64_t)a, got + a);
		CHECK(rc == BSX_OK, "batch at %lld: %d", (long long)a, rc);
	}
	CHECK(memcmp(want, got, (size_t)n) == 0, "n %lld universe %d bits %s step %d: flags differ", (long long)n, universe, bits ? bits : "64", step);
	CHECK(T.n_slots >= 2 * T.n_used && (T.n_slots & (T.n_slots - 1)) == 0, "load: %llu of %llu", (unsigned long long)T.n_used, (unsigned long long)T.n_slots);
	if (universe >= 4096) CHECK(T.n_slots >= 64 << 4, "the table did not grow: %llu slots", (unsigned long long)T.n_slots);
	bsx_md_table_free(&T);
	bsx_tune_set("markdup_slots", 0);
	bsx_tune_set("markdup_hash_bits", 0);
	free(k); free(want); free(got);
}

/* two threads take the slices of two chunks alternately, as back_slices does; every slice has the same eight keys, so only the slice that
 * reaches the table first may leave them unmarked, and that must be slice 0 of chunk 0 whichever thread runs first */
typedef struct { bsx_md_state_t q; bsx_backend_t be; bsx_markdup_key_t key[8]; uint8_t dup[4][8]; } turn_t;
typedef struct { turn_t *t; int first; } turn_arg_t;
static void *turn_thread(void *arg)
{
	turn_arg_t *a = (turn_arg_t*)arg;
	int k;
	for (k = a->first; k < 4; k += 2) {   /* ticket k: slice k % 2 of chunk k / 2 */
		const int rc = bsx_md_slice(&a->t->q, &a->t->be, k / 2, k % 2, 2, 8, a->t->key, (uint64_t)k * 8, a->t->dup[k]);
		CHECK(rc == BSX_OK, "slice %d: %d", k, rc);
	}
	return 0;
}
static void tickets(void)
{
	turn_t *T = (turn_t*)calloc(1, sizeof(*T));
	turn_arg_t A[2];
	pthread_t th;
	bsx_markdup_totals_t tot;
	int64_t seq; uint64_t ord;
	int k, i;
	bsx_md_state_set(&T->q, 1);
	for (i = 0; i < 8; ++i) { T->key[i].w[0] = BSX_MD_END(0, 500 + i, 0, 0); T->key[i].w[1] = BSX_MD_SINGLE; }
	bsx_md_chunk_begin(&T->q, 16, &seq, &ord); CHECK(seq == 0 && ord == 0, "first chunk");
	bsx_md_chunk_begin(&T->q, 16, &seq, &ord); CHECK(seq == 1 && ord == 16, "second chunk");
	A[0].t = A[1].t = T; A[0].first = 0; A[1].first = 1;
	pthread_create(&th, 0, turn_thread, &A[1]);   /* the thread with slice 1 starts first */
	turn_thread(&A[0]);
	pthread_join(th, 0);
	for (k = 0; k < 4; ++k) for (i = 0; i < 8; ++i) CHECK(T->dup[k][i] == (k > 0), "slice %d key %d: %d", k, i, T->dup[k][i]);
	tot = T->q.tot;
	CHECK(tot.n_templates == 32 && tot.n_keyed == 32 && tot.n_dup == 24, "totals %llu %llu %llu", (unsigned long long)tot.n_templates, (unsigned long long)tot.n_keyed, (unsigned long long)tot.n_dup);
	bsx_md_fail(&T->q);   /* after a failure nobody waits: a slice out of turn comes back with an error */
	CHECK(bsx_md_slice(&T->q, &T->be, 7, 1, 2, 8, T->key, 0, T->dup[0]) != BSX_OK, "a slice after a failure");
	bsx_md_state_end(&T->q);
	free(T);
}

int main(void)
{
	keys_of_records();
	table_runs(1, 4, 0, 1);
	table_runs(65, 40, 0, 1);
	table_runs(65, 64, "8", 7);       /* different keys with one claim word: the next salt */
	table_runs(5000, 4096, 0, 5000);
	table_runs(5000, 4096, 0, 64);
	table_runs(5000, 4096, 0, 997);
	table_runs(3000, 100, "8", 37);
	tickets();
	if (n_bad) { fprintf(stderr, "%d checks failed\n", n_bad); return 1; }
	printf("ok\n");
	return 0;
}
