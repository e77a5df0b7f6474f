/* Stand-alone program over csrc/host/meth.c (tests/test_meth_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer): the beta in
 * thousandths against printf for every 0 <= r <= n <= 1200, the host statement of the rule on the hand-worked records of
 * tests/test_meth_model.py, the table pass (contexts, holes, contig ends, callability), the state of a backend without the seam, the writer.
 * argv[1]: a directory to write into.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "meth.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

/* c1 = TTATTCGTTATTCATTATTGATTATTCCTTATTCTTTATTCnGTTATTACGC (52 bases, pac holds a C under the N at 41), c2 = GTTATTAC */
static const char C1[] = "TTATTCGTTATTCATTATTGATTATTCCTTATTCTTTATTCCGTTATTACGC", C2[] = "GTTATTAC";
#define L1 52
#define LG 60
static bsx_ann_t g_anns[2];
static bsx_amb_t g_ambs[1];
static bsx_index_t g_idx;

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
static void make_index(void)
{
	int64_t i;
	memset(&g_idx, 0, sizeof(g_idx));
	g_idx.pac = (uint8_t*)calloc(LG / 4 + 1, 1);
	for (i = 0; i < LG; ++i) { const int b = code(i < L1 ? C1[i] : C2[i - L1]); g_idx.pac[i >> 2] |= (uint8_t)(b << ((~i & 3) << 1)); }
	g_anns[0].offset = 0; g_anns[0].len = L1; g_anns[0].name = (char*)"c1";
	g_anns[1].offset = L1; g_anns[1].len = 8; g_anns[1].name = (char*)"c2";
	g_ambs[0].offset = 41; g_ambs[0].len = 1; g_ambs[0].amb = 'N';
	g_idx.ref.l_pac = LG; g_idx.ref.n_seqs = 2; g_idx.ref.anns = g_anns; g_idx.ref.n_holes = 1; g_idx.ref.ambs = g_ambs;
}

static void test_milli(void)
{
	uint32_t r, n, ties = 0;
	for (n = 1; n <= 1200; ++n) for (r = 0; r <= n; ++r) {
		char a[32], b[32];
		const uint32_t m = bsx_meth_milli(r, n);
		snprintf(a, sizeof(a), "%1.3f", (double)r / (double)n);
		snprintf(b, sizeof(b), "%u.%03u", m / 1000, m % 1000);
		CHECK(strcmp(a, b) == 0);
		ties += 2 * (1000 * r % n) == n;
	}
	CHECK(ties == 1560);
	CHECK(bsx_meth_milli(1, 16) == 62 && bsx_meth_milli(3, 16) == 188 && bsx_meth_milli(1, 80) == 13 && bsx_meth_milli(3, 80) == 37 && bsx_meth_milli(7, 80) == 87);
	CHECK(bsx_meth_milli(4000000000u, 4000000001u) == 1000 && bsx_meth_milli(2147483648u, 4294967295u) == 500 && bsx_meth_milli(0, 4294967295u) == 0);
}

#define CG(len, op) ((uint32_t)(len) << 4 | (op))   /* MIDSH */
/* the pool: CIGARs, then masks */
static uint32_t POOL[32];
static uint8_t READS[512];
static size_t n_reads;
static uint32_t put_read(const char *s, int revcomp)
{
	const size_t l = strlen(s), at = n_reads;
	size_t i;
	for (i = 0; i < l; ++i) READS[n_reads++] = (uint8_t)(revcomp ? 3 - code(s[l - 1 - i]) : code(s[i]));
	return (uint32_t)at;
}
static bsx_meth_job_t job(int64_t fpos, uint32_t roff, uint32_t rlen, uint32_t cig_off, uint32_t n_cigar, uint32_t flags, uint32_t qm_off, int64_t ob, int64_t oe)
{
	bsx_meth_job_t j;
	memset(&j, 0, sizeof(j));
	j.fpos = fpos; j.roff = roff; j.rlen = rlen; j.cig_off = cig_off; j.n_cigar = n_cigar; j.flags = flags; j.qm_off = qm_off; j.ov_beg = ob; j.ov_end = oe;
	return j;
}

static void test_rule_tables_and_state(void)
{
	/* the read over all of c1 (A over the N), the same with T at 5 and A at 6 and 19 */
	static const char R0[] = "TTATTCGTTATTCATTATTGATTATTCCTTATTCTTTATTCAGTTATTACGC", R2[] = "TTATTTATTATTCATTATTAATTATTCCTTATTCTTTATTCAGTTATTACGC";
	char r4[64], r5[64];
	bsx_meth_job_t jobs[6], bad[2];
	uint32_t *cnt = (uint32_t*)calloc(LG, 16), *want = (uint32_t*)calloc(LG, 16), *before = (uint32_t*)malloc(LG * 16);
	bsx_meth_tables_t t;
	bsx_meth_state_t st;
	bsx_backend_t be;
	int i;
	enum { CIG_M = 0, CIG_HS = 1, CIG_ID = 4, ALL = 9, LOWQ = 11 };
	for (i = 0; i < L1; ++i) CHECK(R0[i] == (i == 41 ? 'A' : C1[i]) && R2[i] == (i == 5 ? 'T' : i == 6 || i == 19 ? 'A' : R0[i]));
	CHECK(strlen(R0) == L1 && strlen(R2) == L1);
	POOL[0] = CG(52, 0);
	POOL[1] = CG(2, 4); POOL[2] = CG(3, 3); POOL[3] = CG(40, 0);                                           /* 2H3S40M */
	POOL[4] = CG(10, 0); POOL[5] = CG(2, 1); POOL[6] = CG(10, 0); POOL[7] = CG(3, 2); POOL[8] = CG(20, 0);   /* 10M2I10M3D20M */
	POOL[ALL] = ~0u; POOL[ALL + 1] = ~0u;
	POOL[LOWQ] = ~0u & ~(1u << 6) & ~(1u << 19); POOL[LOWQ + 1] = ~0u;                                      /* low quality at 6 and 19 */
	snprintf(r4, sizeof(r4), "AAGGG%.40s", R0 + 5);
	snprintf(r5, sizeof(r5), "%.10sCC%.10s%.20s", R0, R0 + 10, R0 + 23);
	jobs[0] = job(0, put_read(R0, 0), 52, CIG_M, 1, 0, ALL, 0, 0);                                         /* YD:f */
	jobs[1] = job(0, put_read(R0, 1), 52, CIG_M, 1, BSX_QC_REVERSE, ALL, 20, 40);                          /* reverse; the interval is read 2's business */
	jobs[2] = job(0, put_read(R2, 0), 52, CIG_M, 1, 3u << 2, LOWQ, 0, 0);                                  /* YD:u: nC2T 1, nG2A 0 above the floor -> strand 0 */
	jobs[3] = job(0, jobs[0].roff, 52, CIG_M, 1, BSX_QC_READ2, ALL, 20, 40);
	jobs[4] = job(5, put_read(r4, 0), 45, CIG_HS, 3, 0, ALL, 0, 0);
	jobs[5] = job(0, put_read(r5, 0), 42, CIG_ID, 5, 0, ALL, 0, 0);
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 6, jobs, POOL, 13) == BSX_OK);
	{ /* tests/test_meth_model.py has every job's columns; summed: */
		static const int RET[][2] = {{5, 5}, {12, 6}, {26, 5}, {27, 5}, {33, 5}, {40, 5}}, OPP[][2] = {{6, 5}, {19, 5}, {42, 4}};
		for (i = 0; i < 6; ++i) want[4 * RET[i][0]] = (uint32_t)RET[i][1];
		want[4 * 5 + 1] = 1;
		for (i = 0; i < 3; ++i) want[4 * OPP[i][0] + 2] = (uint32_t)OPP[i][1];
	}
	for (i = 0; i < 4 * LG; ++i) if (cnt[i] != want[i]) { fprintf(stderr, "position %d counter %d: %u, not %u\n", i / 4, i % 4, cnt[i], want[i]); exit(1); }
	CHECK(bsx_meth_host_tables(&g_idx, cnt, &t) == BSX_OK);
	{ static const uint64_t K[5] = {1, 1, 1, 2, 1}, S[5] = {1000, 1000, 833, 2000, 1000}; CHECK(memcmp(t.k, K, 40) == 0 && memcmp(t.s, S, 40) == 0); }
	/* YD:u with every quality high: nG2A 2 > nC2T 1 -> strand 1 */
	memcpy(before, cnt, LG * 16);
	jobs[2].qm_off = ALL;
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 1, &jobs[2], POOL, 13) == BSX_OK);
	CHECK(cnt[4 * 5 + 3] == before[4 * 5 + 3] + 1 && cnt[4 * 6 + 1] == 1 && cnt[4 * 19 + 1] == 1 && cnt[4 * 42] == 1 && cnt[4 * 12 + 2] == 1 && cnt[4 * 12] == before[4 * 12]);
	/* a job out of range: BSX_E_ARG, and nothing of the batch is added */
	memcpy(before, cnt, LG * 16);
	bad[0] = jobs[0];
	bad[1] = job(9, jobs[0].roff, 52, CIG_M, 1, 0, ALL, 0, 0);   /* 52M from 9: one beyond the genome */
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	bad[1] = job(-1, jobs[0].roff, 52, CIG_M, 1, 0, ALL, 0, 0);
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	bad[1] = job(0, jobs[0].roff, 52, 12, 2, 0, ALL, 0, 0);      /* CIGAR words beyond the pool */
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	bad[1] = job(0, jobs[0].roff, 52, CIG_M, 1, 0, 12, 0, 0);    /* the second mask word beyond the pool */
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	bad[1] = job(0, jobs[0].roff, 0, CIG_M, 1, 0, ALL, 0, 0);
	CHECK(bsx_meth_host_add(&g_idx, cnt, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	CHECK(memcmp(before, cnt, LG * 16) == 0);
	/* the table pass on counters set by hand: contig ends, the hole, callability on either side of its boundary */
	memset(cnt, 0, LG * 16);
	cnt[4 * 51] = 1;                                   /* c1's last base, a C before c2's G: CN */
	cnt[4 * 52] = 2;                                   /* c2's first base, a G: CN */
	cnt[4 * 59 + 1] = 3;                               /* c2's last base, a C: CN, beta 0 */
	cnt[4 * 41] = 7;                                   /* the N: no site whatever pac holds */
	cnt[4 * 40] = 1; cnt[4 * 42 + 1] = 1;              /* C before and G behind the N: CN */
	cnt[4 * 0] = 9;                                    /* a T: no site */
	cnt[4 * 6 + 1] = 3; cnt[4 * 6 + 2] = 20; cnt[4 * 6 + 3] = 1;   /* G at 6 behind a C (CG): 20 * 1 < 0 + 20 fails */
	cnt[4 * 19] = 1; cnt[4 * 19 + 1] = 2; cnt[4 * 19 + 2] = 20; cnt[4 * 19 + 3] = 1;   /* G at 19 behind a T (CA): 20 < 1 + 20 holds; 1 of 3 */
	cnt[4 * 12 + 2] = 4; cnt[4 * 12 + 3] = 1;          /* ret + conv == 0 */
	cnt[4 * 49] = 1; cnt[4 * 49 + 1] = 15;             /* C at 49 before a G: 1 of 16, an exact tie to even: 62 */
	CHECK(bsx_meth_host_tables(&g_idx, cnt, &t) == BSX_OK);
	{ static const uint64_t K[5] = {1, 0, 1, 0, 5}, S[5] = {333, 0, 62, 0, 3000}; CHECK(memcmp(t.k, K, 40) == 0 && memcmp(t.s, S, 40) == 0); }
	cnt[4 * 6 + 2] = 21;
	CHECK(bsx_meth_host_tables(&g_idx, cnt, &t) == BSX_OK && t.k[2] == 2 && t.s[2] == 62);
	/* the state of a backend without the seam */
	memset(&be, 0, sizeof(be));
	memset(&st, 0, sizeof(st));
	pthread_mutex_init(&st.mu, 0);
	CHECK(bsx_meth_state_tables(&st, &t) == BSX_E_ARG);   /* off */
	bsx_meth_state_set(&st, 1);
	CHECK(bsx_meth_state_tables(&st, &t) == BSX_OK && t.k[0] + t.k[1] + t.k[2] + t.k[3] + t.k[4] == 0);   /* no chunk yet */
	CHECK(bsx_meth_slice(&st, &be, &g_idx, READS, n_reads, 1, jobs, POOL, 13) == BSX_E_INTERNAL);        /* not attached */
	CHECK(bsx_meth_attach(&st, &be, &g_idx) == BSX_OK && bsx_meth_attach(&st, &be, &g_idx) == BSX_OK);
	jobs[2].qm_off = LOWQ;
	CHECK(bsx_meth_slice(&st, &be, &g_idx, READS, n_reads, 2, jobs, POOL, 13) == BSX_OK);
	CHECK(bsx_meth_slice(&st, &be, &g_idx, READS, n_reads, 0, 0, 0, 0) == BSX_OK);
	CHECK(bsx_meth_slice(&st, &be, &g_idx, READS, n_reads, 4, jobs + 2, POOL, 13) == BSX_OK);
	CHECK(bsx_meth_slice(&st, &be, &g_idx, READS, n_reads, 2, bad, POOL, 13) == BSX_E_ARG);
	CHECK(bsx_meth_state_tables(&st, &t) == BSX_OK);
	{ static const uint64_t K[5] = {1, 1, 1, 2, 1}, S[5] = {1000, 1000, 833, 2000, 1000}; CHECK(memcmp(t.k, K, 40) == 0 && memcmp(t.s, S, 40) == 0); }
	bsx_meth_state_set(&st, 1);                           /* set again: from zero, what it held freed */
	CHECK(st.cnt == 0 && !st.attached);
	bsx_meth_state_set(&st, 0);
	free(cnt); free(want); free(before);
}

static void test_writer(const char *dir)
{
	static const bsx_meth_tables_t T = {{19, 20, 0, 3000000, 7}, {19000, 12345, 0, 1234567891, 7000}}, Z = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
	char prefix[4096], fn[4200], buf[512];
	FILE *f;
	size_t n;
	snprintf(prefix, sizeof(prefix), "%s/w", dir);
	snprintf(fn, sizeof(fn), "%s_totalBaseConversionRate.txt", prefix);
	CHECK(bsx_meth_write(prefix, &T) == BSX_OK);
	CHECK((f = fopen(fn, "r")) != 0); n = fread(buf, 1, sizeof(buf) - 1, f); buf[n] = 0; fclose(f);
	CHECK(strcmp(buf, "BISCUITqc Conversion Rate by Base Average Table\nCA\tCC\tCG\tCT\n-1\t0.61725\t-1\t0.411523\n") == 0);
	CHECK(bsx_meth_write(prefix, &Z) == BSX_OK);
	CHECK((f = fopen(fn, "r")) != 0); n = fread(buf, 1, sizeof(buf) - 1, f); buf[n] = 0; fclose(f);
	CHECK(strcmp(buf, "BISCUITqc Conversion Rate by Base Average Table\nCA\tCC\tCG\tCT\n-1\t-1\t-1\t-1\n") == 0);
	snprintf(prefix, sizeof(prefix), "%s/no/such/dir/w", dir);
	CHECK(bsx_meth_write(prefix, &T) == BSX_E_IO && bsx_meth_write(0, &T) == BSX_E_ARG && bsx_meth_write(prefix, 0) == BSX_E_ARG);
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
	make_index();
	test_milli();
	test_rule_tables_and_state();
	test_writer(argv[1]);
	free(g_idx.pac);
	printf("ok\n");
	return 0;
}
