/* Stand-alone program over csrc/host/cov.c (tests/test_cov_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer): the host
 * statement of the depth rule on the hand-worked records of tests/test_cov_model.py, the state of a backend without the seam, the BED reader on
 * good and malformed files, the writer.  argv[1]: a directory to write into.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "cov.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static bsx_ann_t g_anns[2];
static bsx_amb_t g_ambs[2];
static bsx_index_t g_idx;
static const char *DIR;

static void make_index(void)
{
	/* c1 ACGTTCGANNCGTTCGC, c2 GCnGCG; pac holds a G under c2's N (C G over the hole's edge is no CpG) and C G under c1's two */
	static const char *fwd = "ACGTTCGACGCGTTCGC" "GCGGCG";
	const int64_t L = 23;
	int64_t i;
	memset(&g_idx, 0, sizeof(g_idx));
	g_idx.pac = (uint8_t*)calloc((size_t)L / 4 + 1, 1);
	for (i = 0; i < L; ++i) { const int b = fwd[i] == 'A' ? 0 : fwd[i] == 'C' ? 1 : fwd[i] == 'G' ? 2 : 3; g_idx.pac[i >> 2] |= (uint8_t)(b << ((~i & 3) << 1)); }
	g_anns[0].offset = 0; g_anns[0].len = 17; g_anns[0].name = (char*)"c1";
	g_anns[1].offset = 17; g_anns[1].len = 6; g_anns[1].name = (char*)"c2";
	g_ambs[0].offset = 8; g_ambs[0].len = 2; g_ambs[0].amb = 'N';
	g_ambs[1].offset = 19; g_ambs[1].len = 1; g_ambs[1].amb = 'N';
	g_idx.ref.l_pac = L; g_idx.ref.n_seqs = 2; g_idx.ref.anns = g_anns; g_idx.ref.n_holes = 2; g_idx.ref.ambs = g_ambs;
}

#define CG(len, op) ((uint32_t)(len) << 4 | (op))   /* MIDSH */
static const uint32_t POOL[] = {CG(2, 3), CG(4, 0), CG(1, 1), CG(2, 0), CG(2, 2), CG(3, 0), CG(1, 4),   /* 2S4M1I2M2D3M1H */
                                CG(8, 0), CG(1, 0), CG(2, 0), CG(1, 0)};
static bsx_qc_job_t job(int64_t fpos, uint32_t off, uint32_t n, uint32_t flags)
{
	bsx_qc_job_t j;
	memset(&j, 0, sizeof(j));
	j.fpos = fpos; j.cig_off = off; j.n_cigar = n; j.flags = flags;
	return j;
}
static void expect(const bsx_cov_table_t *t, int n, const uint64_t *want, uint64_t nb)
{
	uint64_t d;
	CHECK(t->n_bins == nb);
	for (d = 0; d < nb; ++d) CHECK(t->count[d] == (d < (uint64_t)n ? want[d] : 0));
}
static void expect_hand_tables(const bsx_cov_tables_t *t, int gc)
{
	static const uint64_t W[12][4] = {{9, 8, 5, 1}, {1, 4}, {12, 10, 1}, {3, 2}, {0, 0, 0, 1}, {0, 1}, {0, 0, 1}, {1}, {4, 6, 2, 1}, {0, 3}, {5, 7, 1}, {1, 2}};
	int i;
	CHECK(t->have_gc == gc);
	for (i = 0; i < 12; ++i) {
		if (i < 4 || gc) expect(&t->t[i], 4, W[i], 4);
		else CHECK(t->t[i].n_bins == 0 && t->t[i].count == 0);
	}
}
static const int64_t TOP[] = {5, 6}, BOT[] = {0, 3, 2, 7, 17, 23};

static void test_rule(void)
{
	bsx_qc_job_t jobs[6];
	int32_t *diff = (int32_t*)calloc(24, 8), *before = (int32_t*)malloc(24 * 8);
	uint32_t mt[2] = {0, 0}, mb[2] = {0, 0};
	bsx_cov_tables_t t;
	jobs[0] = job(0, 0, 7, BSX_QC_COV | BSX_QC_COV_Q40);
	jobs[1] = job(4, 7, 1, BSX_QC_COV | BSX_QC_REVERSE);
	jobs[2] = job(5, 8, 1, BSX_QC_COV | BSX_QC_COV_Q40);
	jobs[3] = job(17 + 4, 9, 1, BSX_QC_COV | BSX_QC_COV_Q40);
	jobs[4] = job(17 + 5, 10, 1, BSX_QC_COV);
	jobs[5] = job(0, 7, 1, BSX_QC_STRAND);   /* without BSX_QC_COV: adds nothing */
	CHECK(bsx_cov_host_add(&g_idx, diff, 6, jobs, POOL, 11) == BSX_OK);
	CHECK(bsx_cov_host_tables(&g_idx, diff, 0, 0, &t) == BSX_OK);
	expect_hand_tables(&t, 0);
	bsx_cov_tables_free(&t);
	CHECK(bsx_cov_host_paint(&g_idx, mt, 1, TOP) == BSX_OK && mt[0] == 1u << 5);
	CHECK(bsx_cov_host_paint(&g_idx, mb, 3, BOT) == BSX_OK && mb[0] == (0x7fu | 0x3fu << 17));
	CHECK(bsx_cov_host_tables(&g_idx, diff, mt, mb, &t) == BSX_OK);
	expect_hand_tables(&t, 1);
	bsx_cov_tables_free(&t);
	CHECK(bsx_cov_host_tables(&g_idx, diff, mt, 0, &t) == BSX_E_ARG);
	{ /* a job out of range: BSX_E_ARG, and nothing of the batch is added */
		bsx_qc_job_t bad[2];
		static const int64_t over[] = {0, 24}, rev[] = {5, 4};
		memcpy(before, diff, 24 * 8);
		bad[0] = jobs[0];
		bad[1] = job(17, 7, 1, BSX_QC_COV);   /* 8M from c2's first base: two beyond the genome */
		CHECK(bsx_cov_host_add(&g_idx, diff, 2, bad, POOL, 11) == BSX_E_ARG);
		bad[1] = job(-1, 8, 1, BSX_QC_COV);
		CHECK(bsx_cov_host_add(&g_idx, diff, 2, bad, POOL, 11) == BSX_E_ARG);
		bad[1] = job(0, 10, 2, BSX_QC_COV);   /* CIGAR words beyond the pool */
		CHECK(bsx_cov_host_add(&g_idx, diff, 2, bad, POOL, 11) == BSX_E_ARG);
		CHECK(memcmp(before, diff, 24 * 8) == 0);
		bad[1] = job(17 - 2, 7, 1, BSX_QC_COV);   /* ... ending on the last base is fine */
		CHECK(bsx_cov_host_add(&g_idx, diff, 1, bad + 1, POOL, 11) == BSX_OK && diff[2 * 23] == -1 - 2);
		CHECK(bsx_cov_host_paint(&g_idx, mt, 1, over) == BSX_E_ARG && bsx_cov_host_paint(&g_idx, mt, 1, rev) == BSX_E_ARG);
	}
	free(diff); free(before);
}

static void test_state(void)
{
	bsx_backend_t be;
	bsx_cov_state_t c;
	bsx_cov_tables_t t;
	bsx_qc_job_t jobs[5];
	int round;
	memset(&be, 0, sizeof(be));
	memset(&c, 0, sizeof(c));
	jobs[0] = job(0, 0, 7, BSX_QC_COV | BSX_QC_COV_Q40); jobs[1] = job(4, 7, 1, BSX_QC_COV); jobs[2] = job(5, 8, 1, BSX_QC_COV | BSX_QC_COV_Q40);
	jobs[3] = job(21, 9, 1, BSX_QC_COV | BSX_QC_COV_Q40); jobs[4] = job(22, 10, 1, BSX_QC_COV);
	bsx_cov_state_set(&c, 0);
	CHECK(bsx_cov_state_tables(&c, &t) == BSX_E_ARG && bsx_cov_state_mask(&c, 0, 1, TOP) == BSX_E_ARG);
	for (round = 0; round < 2; ++round) { /* without masks, then with: a state set again starts from nothing */
		bsx_cov_state_set(&c, 1);
		CHECK(bsx_cov_state_tables(&c, &t) == BSX_OK && t.t[0].n_bins == 0);   /* nothing aligned yet: no rows */
		if (round) {
			CHECK(bsx_cov_state_mask(&c, BSX_COV_MASK_TOPGC, 1, TOP) == BSX_OK);
			CHECK(bsx_cov_attach(&c, &be, &g_idx) == BSX_E_ARG);   /* one mask without the other */
			CHECK(bsx_cov_state_mask(&c, BSX_COV_MASK_BOTGC, 3, BOT) == BSX_OK);
		}
		CHECK(bsx_cov_attach(&c, &be, &g_idx) == BSX_OK && bsx_cov_attach(&c, &be, &g_idx) == BSX_OK);
		CHECK(bsx_cov_state_mask(&c, 0, 1, TOP) == BSX_E_ARG);   /* too late */
		CHECK(bsx_cov_slice(&c, &be, &g_idx, 2, jobs, POOL, 11) == BSX_OK && bsx_cov_slice(&c, &be, &g_idx, 0, 0, 0, 0) == BSX_OK);
		CHECK(bsx_cov_slice(&c, &be, &g_idx, 3, jobs + 2, POOL, 11) == BSX_OK);
		CHECK(bsx_cov_state_tables(&c, &t) == BSX_OK);
		expect_hand_tables(&t, round);
		bsx_cov_tables_free(&t);
		CHECK(bsx_cov_state_tables(&c, &t) == BSX_OK);   /* read again: the same */
		expect_hand_tables(&t, round);
		bsx_cov_tables_free(&t);
	}
	{ /* an empty mask is a mask; an interval beyond the genome is refused when the state attaches */
		static const int64_t far[] = {0, 24};
		bsx_cov_state_set(&c, 1);
		CHECK(bsx_cov_state_mask(&c, 0, 0, 0) == BSX_OK && bsx_cov_state_mask(&c, 1, 1, far) == BSX_OK);
		CHECK(bsx_cov_attach(&c, &be, &g_idx) == BSX_E_ARG);
		CHECK(bsx_cov_state_mask(&c, 1, 0, 0) == BSX_OK && bsx_cov_attach(&c, &be, &g_idx) == BSX_OK);
		CHECK(bsx_cov_state_tables(&c, &t) == BSX_OK && t.have_gc == 1 && t.t[0].n_bins == 1 && t.t[0].count[0] == 23 && t.t[1].count[0] == 5 && t.t[4].count[0] == 0);
		bsx_cov_tables_free(&t);
	}
	bsx_cov_state_set(&c, 0);
}

static char *path_of(const char *name)
{
	static char buf[8][4200];
	static int k;
	char *p = buf[k++ & 7];
	snprintf(p, 4200, "%s/%s", DIR, name);
	return p;
}
static const char *put(const char *name, const char *text, int gz)
{
	char *p = path_of(name);
	if (gz) { gzFile f = gzopen(p, "wb"); CHECK(f && gzwrite(f, text, (unsigned)strlen(text)) == (int)strlen(text)); gzclose(f); }
	else { FILE *f = fopen(p, "w"); CHECK(f && fputs(text, f) >= 0); fclose(f); }
	return p;
}
static void test_bed(void)
{
	static const char *good = "# a comment\ntrack name=x\nbrowser position c1\n\nc1\t5\t6\twin\t0.61\nc2 0 6\r\nc1\t3\t3\n  c1\t0\t17\n";
	static const char *bad[] = {"c1\t5\n", "c1\n", "c1\tx\t6\n", "c1\t5\t6x\n", "c1\t7\t6\n", "c1\t0\t18\n", "c3\t0\t1\n", "c1\t-1\t3\n", "c1\t5\t\n", "c1\t1.5\t3\n", "c2\t0\t7",
	                            "track1\t0\t1\n", "browser_chr\t0\t1\n"};   /* contig names, not the two header words: not in this index */
	int64_t n = -1, *iv = 0;
	size_t i;
	int gz;
	for (gz = 0; gz < 2; ++gz) {
		CHECK(bsx_cov_read_bed(put(gz ? "good.bed.gz" : "good.bed", good, gz), &g_idx, &n, &iv) == BSX_OK);
		CHECK(n == 3 && iv[0] == 5 && iv[1] == 6 && iv[2] == 17 && iv[3] == 23 && iv[4] == 0 && iv[5] == 17);
		free(iv);
	}
	{ /* a line longer than the reader's buffer: the columns at its start count, the next line is read whole; no newline at the end of the file */
		char *text = (char*)malloc(20000);
		size_t l = (size_t)sprintf(text, "c1\t1\t2\t");
		memset(text + l, 'x', 15000); l += 15000;
		strcpy(text + l, "\nc2\t1\t3");
		CHECK(bsx_cov_read_bed(put("long.bed", text, 0), &g_idx, &n, &iv) == BSX_OK && n == 2 && iv[0] == 1 && iv[1] == 2 && iv[2] == 18 && iv[3] == 20);
		free(iv); free(text);
	}
	CHECK(bsx_cov_read_bed(put("empty.bed", "", 0), &g_idx, &n, &iv) == BSX_OK && n == 0 && iv);
	free(iv);
	for (i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
		iv = (int64_t*)1; n = 7;
		CHECK(bsx_cov_read_bed(put("bad.bed", bad[i], (int)(i & 1)), &g_idx, &n, &iv) == BSX_E_FORMAT && iv == 0 && n == 0);
	}
	CHECK(bsx_cov_read_bed(path_of("none.bed"), &g_idx, &n, &iv) == BSX_E_IO && iv == 0);
	CHECK(bsx_cov_read_bed(0, &g_idx, &n, &iv) == BSX_E_ARG);
}

static void expect_file(const char *prefix, const char *suffix, const char *want)
{
	char fn[4400], got[4096];
	FILE *f;
	size_t n;
	snprintf(fn, sizeof(fn), "%s%s", prefix, suffix);
	CHECK((f = fopen(fn, "r")) != 0);
	n = fread(got, 1, sizeof(got) - 1, f);
	got[n] = 0;
	fclose(f);
	if (strcmp(got, want) != 0) { fprintf(stderr, "%s:\n got: %s\nwant: %s\n", fn, got, want); exit(1); }
}
static int exists(const char *prefix, const char *suffix) { char fn[4400]; FILE *f; snprintf(fn, sizeof(fn), "%s%s", prefix, suffix); f = fopen(fn, "r"); if (f) fclose(f); return f != 0; }
static void test_writer(void)
{
	bsx_backend_t be;
	bsx_cov_state_t c;
	bsx_cov_tables_t t;
	bsx_qc_job_t jobs[5];
	char *p1 = path_of("w1"), *p2 = path_of("w2"), *p3 = path_of("no/such/dir/w");
	memset(&be, 0, sizeof(be));
	memset(&c, 0, sizeof(c));
	jobs[0] = job(0, 0, 7, BSX_QC_COV | BSX_QC_COV_Q40); jobs[1] = job(4, 7, 1, BSX_QC_COV); jobs[2] = job(5, 8, 1, BSX_QC_COV | BSX_QC_COV_Q40);
	jobs[3] = job(21, 9, 1, BSX_QC_COV | BSX_QC_COV_Q40); jobs[4] = job(22, 10, 1, BSX_QC_COV);
	bsx_cov_state_set(&c, 1);
	CHECK(bsx_cov_state_mask(&c, 0, 1, TOP) == BSX_OK && bsx_cov_state_mask(&c, 1, 3, BOT) == BSX_OK && bsx_cov_attach(&c, &be, &g_idx) == BSX_OK);
	CHECK(bsx_cov_slice(&c, &be, &g_idx, 5, jobs, POOL, 11) == BSX_OK && bsx_cov_state_tables(&c, &t) == BSX_OK);
	CHECK(bsx_cov_write(p1, &t) == BSX_OK);
	expect_file(p1, "_covdist_all_base_table.txt", "BISCUITqc Depth Distribution - All Bases\ndepth\tcount\n0\t9\n1\t8\n2\t5\n3\t1\n");
	expect_file(p1, "_covdist_q40_cpg_topgc_table.txt", "BISCUITqc Depth Distribution - Q40 Top GC CpGs\ndepth\tcount\n0\t1\n");
	expect_file(p1, "_covdist_all_base_botgc_table.txt", "BISCUITqc Depth Distribution - All Bot GC Bases\ndepth\tcount\n0\t4\n1\t6\n2\t2\n3\t1\n");
	expect_file(p1, "_cv_table.txt", "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
	            "all_base\t0.913043\t0.880368\t0.964212\nall_cpg\t0.8\t0.4\t0.5\nq40_base\t0.521739\t0.580072\t1.11181\nq40_cpg\t0.4\t0.489898\t1.22474\n"
	            "all_base_topgc\t3\t0\t0\nall_cpg_topgc\t1\t0\t0\nq40_base_topgc\t2\t0\t0\n"
	            "all_base_botgc\t1\t0.877058\t0.877058\nall_cpg_botgc\t1\t0\t0\nq40_base_botgc\t0.692308\t0.605693\t0.87489\nq40_cpg_botgc\t0.666667\t0.471405\t0.707107\n");
	t.have_gc = 0;   /* the four whole-genome tables only */
	CHECK(bsx_cov_write(p2, &t) == BSX_OK && exists(p2, "_covdist_q40_cpg_table.txt") && exists(p2, "_cv_table.txt") && !exists(p2, "_covdist_all_base_topgc_table.txt"));
	expect_file(p2, "_cv_table.txt", "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
	            "all_base\t0.913043\t0.880368\t0.964212\nall_cpg\t0.8\t0.4\t0.5\nq40_base\t0.521739\t0.580072\t1.11181\nq40_cpg\t0.4\t0.489898\t1.22474\n");
	t.have_gc = 1;
	CHECK(bsx_cov_write(p3, &t) == BSX_E_IO && bsx_cov_write(0, &t) == BSX_E_ARG);
	bsx_cov_tables_free(&t);
	bsx_cov_tables_free(&t);   /* (twice: harmless) */
	bsx_cov_state_set(&c, 0);
}

int main(int argc, char **argv)
{
	CHECK(argc == 2);
	DIR = argv[1];
	make_index();
	test_rule();
	test_state();
	test_bed();
	test_writer();
	free(g_idx.pac);
	printf("ok\n");
	return 0;
}
