/* Stand-alone program over csrc/host/meth.c (tests/test_methbed_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer): the host
 * statement of --meth-bed's rule (bsx_meth_host_sites) and the writer (bsx_meth_bed_write, _line, _order) on counters set by hand.  The contigs
 * c1 .. c6 and their counters are those of tests/test_methbed_model.py, with the same hand-written lines; c7 = T (CG)x5000 puts a CpG across
 * each tile boundary and more sites into a tile than the smallest buffer holds.  argv[1]: a directory to write into.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "meth.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static const char *SEQ[6] = {"TTATACGATCGTATCGAATTATATTAATTA", "TTATATTAATATTATAACGA", "TTATATTAATATTATAATAC", "GATTATATTAATATTATAAT",
                             "TTATACGCTTATATTATAAT" /* N at 7, a C under it */, "TTAAACGATTATATTATAAT" /* N at 3 */};
#define N7 10001
#define O7 130
#define LG (O7 + N7)
static bsx_ann_t g_anns[7];
static bsx_amb_t g_ambs[2];
static bsx_index_t g_idx;
static uint32_t *g_cnt;

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
static void set_base(int64_t i, int b) { g_idx.pac[i >> 2] |= (uint8_t)(b << ((~i & 3) << 1)); }
static void make_index(void)
{
	static char names[7][4];
	int64_t off = 0, i;
	int c;
	memset(&g_idx, 0, sizeof(g_idx));
	g_idx.pac = (uint8_t*)calloc(LG / 4 + 1, 1);
	for (c = 0; c < 6; ++c) {
		const int64_t l = (int64_t)strlen(SEQ[c]);
		for (i = 0; i < l; ++i) set_base(off + i, code(SEQ[c][i]));
		snprintf(names[c], 4, "c%d", c + 1);
		g_anns[c].offset = off; g_anns[c].len = (int32_t)l; g_anns[c].name = names[c];
		off += l;
	}
	CHECK(off == O7);
	for (i = 1; i < N7; ++i) set_base(O7 + i, i & 1 ? 1 : 2);
	set_base(O7, 3);
	snprintf(names[6], 4, "c7");
	g_anns[6].offset = O7; g_anns[6].len = N7; g_anns[6].name = names[6];
	g_ambs[0].offset = 90 + 7; g_ambs[0].len = 1; g_ambs[0].amb = 'N';
	g_ambs[1].offset = 110 + 3; g_ambs[1].len = 1; g_ambs[1].amb = 'N';
	g_idx.ref.l_pac = LG; g_idx.ref.n_seqs = 7; g_idx.ref.anns = g_anns; g_idx.ref.n_holes = 2; g_idx.ref.ambs = g_ambs;
}
static void set_cnt(int64_t f, uint32_t ret, uint32_t conv) { g_cnt[4 * f] = ret; g_cnt[4 * f + 1] = conv; }
static void make_counters(void)
{
	int64_t i;
	g_cnt = (uint32_t*)calloc(LG + 1, 16);
	set_cnt(5, 1, 1); set_cnt(9, 0, 2); set_cnt(10, 1, 0); set_cnt(15, 0, 1);       /* c1: test_lone_c_lone_g_and_a_joined_pair */
	set_cnt(30 + 17, 1, 0); set_cnt(30 + 18, 1, 0);                                 /* c2: the CpG at the contig's end */
	set_cnt(50 + 19, 1, 0); set_cnt(70 + 0, 1, 0);                                  /* c3's last C, c4's first G */
	set_cnt(90 + 5, 1, 0); set_cnt(90 + 6, 1, 0); set_cnt(90 + 7, 5, 0);            /* c5: the N behind the CpG (counters under the N: no site) */
	set_cnt(110 + 5, 1, 0); set_cnt(110 + 6, 1, 0);                                 /* c6: the N two before the C */
	for (i = 1; i < N7; ++i) set_cnt(O7 + i, 1, i & 1 ? 1 : 0);                     /* c7: every C 1 of 2, every G 1 of 1 .. */
	set_cnt(O7 + 4000, 0, 0);                                                       /* .. but the G at 4000: the C at 3999 stays alone */
	set_cnt(O7 + 8061, 0, 0);                                                       /* .. and the C at 8061, the last position of a tile: the G at 8062 stays alone */
	set_cnt(O7 + 5001, 9, 1); g_cnt[4 * (O7 + 5001) + 3] = 1;                       /* .. and an uncallable C (opp_alt 1 of ret + opp_ref 9) beside a callable G */
	CHECK((O7 + 8062) % BSX_COV_TILE == 0 && (O7 + 3966) % BSX_COV_TILE == 0);
}

static int host_sites(void *ud, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n, int64_t *f_next)
{
	++*(int*)ud;
	return bsx_meth_host_sites(&g_idx, g_cnt, opt, f_lo, f_hi, out, cap, n, f_next);
}
static char *file_text(const char *dir, const int32_t *order, const bsx_meth_site_opt_t *opt, int64_t cap, uint64_t *lines, int *calls)
{
	char fn[4200], *buf;
	FILE *f;
	long n;
	snprintf(fn, sizeof(fn), "%s/out.bed", dir);
	CHECK((f = fopen(fn, "w")) != 0);
	*calls = 0;
	CHECK(bsx_meth_bed_write(f, &g_idx, order, opt, host_sites, calls, cap, lines) == BSX_OK);
	CHECK(fclose(f) == 0);
	CHECK((f = fopen(fn, "r")) != 0);
	fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
	buf = (char*)malloc((size_t)n + 1);
	CHECK(fread(buf, 1, (size_t)n, f) == (size_t)n);
	buf[n] = 0;
	fclose(f);
	return buf;
}
static int begins(const char *text, const char *with) { return strncmp(text, with, strlen(with)) == 0; }
static int ends(const char *text, const char *with) { return strlen(text) >= strlen(with) && strcmp(text + strlen(text) - strlen(with), with) == 0; }

static void test_files(const char *dir)
{
	bsx_meth_site_opt_t o = {BSX_METH_TYPE_CG, 0, 1, 0};
	uint64_t lines;
	int calls, small_calls;
	char *t, *t2;
	/* type cg */
	t = file_text(dir, 0, &o, 0, &lines, &calls);
	CHECK(lines == 4 + 1 + 1 + 9994 && calls == 7);
	CHECK(begins(t, "c1\t5\t6\t0.500\t2\nc1\t9\t10\t0.000\t2\nc1\t10\t11\t1.000\t1\nc1\t15\t16\t0.000\t1\n" "c2\t17\t18\t1.000\t1\n" "c6\t6\t7\t1.000\t1\n"
	                "c7\t2\t3\t1.000\t1\n" "c7\t3\t4\t0.500\t2\n"));
	CHECK(strstr(t, "\nc7\t3999\t4000\t0.500\t2\nc7\t4001\t4002\t0.500\t2\n") && strstr(t, "\nc7\t8060\t8061\t1.000\t1\nc7\t8062\t8063\t1.000\t1\n"));
	CHECK(strstr(t, "\nc7\t5000\t5001\t1.000\t1\nc7\t5002\t5003\t1.000\t1\n"));   /* the uncallable C at 5001 */
	CHECK(ends(t, "\nc7\t9997\t9998\t0.500\t2\nc7\t9998\t9999\t1.000\t1\n"));
	t2 = file_text(dir, 0, &o, BSX_COV_TILE, &lines, &small_calls);          /* the smallest buffer: a tile a call */
	CHECK(strcmp(t, t2) == 0 && small_calls == 6 + 3 && lines == 10000);
	free(t); free(t2);
	/* a coverage floor of 2 */
	o.min_cov = 2;
	t = file_text(dir, 0, &o, 0, &lines, &calls);
	CHECK(begins(t, "c1\t5\t6\t0.500\t2\nc1\t9\t10\t0.000\t2\nc7\t3\t4\t0.500\t2\nc7\t5\t6\t0.500\t2\n") && lines == 2 + 4996);
	free(t);
	o.min_cov = 1;
	/* type ch: none of these; type c: every site, CN included */
	o.type = BSX_METH_TYPE_CH;
	t = file_text(dir, 0, &o, 0, &lines, &calls);
	CHECK(lines == 0 && t[0] == 0);
	free(t);
	o.type = BSX_METH_TYPE_C;
	t = file_text(dir, 0, &o, 0, &lines, &calls);
	CHECK(begins(t, "c1\t5\t6\t0.500\t2\nc1\t9\t10\t0.000\t2\nc1\t10\t11\t1.000\t1\nc1\t15\t16\t0.000\t1\n" "c2\t17\t18\t1.000\t1\nc2\t18\t19\t1.000\t1\n" "c3\t19\t20\t1.000\t1\n"
	                "c4\t0\t1\t1.000\t1\n" "c5\t5\t6\t1.000\t1\nc5\t6\t7\t1.000\t1\n" "c6\t5\t6\t1.000\t1\nc6\t6\t7\t1.000\t1\n" "c7\t1\t2\t0.500\t2\nc7\t2\t3\t1.000\t1\n"));
	CHECK(lines == 12 + 9997 && ends(t, "\nc7\t9999\t10000\t0.500\t2\nc7\t10000\t10001\t1.000\t1\n"));
	free(t);
	/* merge */
	o.type = BSX_METH_TYPE_CG; o.merge = 1;
	t = file_text(dir, 0, &o, 0, &lines, &calls);
	CHECK(begins(t, "c1\t5\t7\t0.500\t2\tC:0.500:2,G:.:0\n" "c1\t9\t11\t0.333\t3\tC:0.000:2,G:1.000:1\n" "c1\t14\t16\t0.000\t1\tC:.:0,G:0.000:1\n"
	                "c2\t17\t19\t1.000\t1\tC:1.000:1,G:.:0\n" "c6\t5\t7\t1.000\t1\tC:.:0,G:1.000:1\n"
	                "c7\t1\t3\t1.000\t1\tC:.:0,G:1.000:1\n" "c7\t3\t5\t0.667\t3\tC:0.500:2,G:1.000:1\n"));
	CHECK(strstr(t, "\nc7\t3965\t3967\t0.667\t3\tC:0.500:2,G:1.000:1\n"));                 /* joined across the first tile boundary */
	CHECK(strstr(t, "\nc7\t3999\t4001\t0.500\t2\tC:0.500:2,G:.:0\nc7\t4001\t4003\t0.667\t3\t"));
	CHECK(strstr(t, "\nc7\t5001\t5003\t1.000\t1\tC:.:0,G:1.000:1\n"));
	CHECK(strstr(t, "\nc7\t8059\t8061\t0.667\t3\tC:0.500:2,G:1.000:1\nc7\t8061\t8063\t1.000\t1\tC:.:0,G:1.000:1\nc7\t8063\t8065\t"));
	CHECK(lines == 5 + 4999);
	t2 = file_text(dir, 0, &o, BSX_COV_TILE, &lines, &small_calls);
	CHECK(strcmp(t, t2) == 0 && small_calls == 6 + 2);
	free(t2);
	{ /* the contigs in a header's order: c7 first, c2, c1; the others behind them in the index's order; equal names and unknown ones ignored */
		int32_t *order = bsx_meth_bed_order(&g_idx, "@HD\tVN:1.5\n@SQ\tSN:c7\tLN:10001\n@SQ\tLN:20\tSN:c2\n@SQ\tSN:c1\tLN:30\n@SQ\tSN:c7\tLN:1\n@SQ\tSN:c\tLN:1\n@SQ\tSN:c77\tLN:1\n@PG\tID:x\tSN:c3");
		static const int32_t WANT[7] = {6, 1, 0, 2, 3, 4, 5};
		CHECK(order && memcmp(order, WANT, sizeof(WANT)) == 0);
		t2 = file_text(dir, order, &o, 0, &lines, &calls);
		CHECK(begins(t2, "c7\t1\t3\t1.000\t1\tC:.:0,G:1.000:1\n") && lines == 5 + 4999 && strlen(t2) == strlen(t));
		CHECK(ends(t2, "c2\t17\t19\t1.000\t1\tC:1.000:1,G:.:0\n" "c1\t5\t7\t0.500\t2\tC:0.500:2,G:.:0\n" "c1\t9\t11\t0.333\t3\tC:0.000:2,G:1.000:1\n"
		             "c1\t14\t16\t0.000\t1\tC:.:0,G:0.000:1\n" "c6\t5\t7\t1.000\t1\tC:.:0,G:1.000:1\n"));
		free(t2); free(order);
		order = bsx_meth_bed_order(&g_idx, "");
		{ static const int32_t ID[7] = {0, 1, 2, 3, 4, 5, 6}; CHECK(order && memcmp(order, ID, sizeof(ID)) == 0); }
		free(order);
	}
	free(t);
}

static void test_windows_and_arguments(void)
{
	bsx_meth_site_opt_t o = {BSX_METH_TYPE_C, 0, 1, 0};
	bsx_meth_site_t *r = (bsx_meth_site_t*)malloc(sizeof(*r) * 20000), guard;
	int64_t n = -1, next = -1, f, total = 0;
	/* the whole genome with the smallest buffer: tiles one at a time (the second holds 4093 sites) */
	static const int64_t NEXT[3] = {4096, 8192, LG};
	int k = 0;
	for (f = 0; f < LG; f = next, ++k) {
		CHECK(k < 3 && bsx_meth_host_sites(&g_idx, g_cnt, &o, f, LG, r, BSX_COV_TILE, &n, &next) == BSX_OK && next == NEXT[k]);
		CHECK(n > 0 && r[0].fpos >= f && r[n - 1].fpos < next);
		total += n;
	}
	CHECK(total == 12 + 9997);
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG, r, 20000, &n, &next) == BSX_OK && n == total && next == LG);
	/* a range inside a tile, merge: the C at the first boundary owns the line, the G behind it none */
	o.type = BSX_METH_TYPE_CG; o.merge = 1;
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 4095, 4097, r, BSX_COV_TILE, &n, &next) == BSX_OK && n == 1 && next == 4097);
	CHECK(r[0].fpos == 4095 && r[0].flags == (BSX_METH_CLS_CG | BSX_METH_SITE_C | BSX_METH_SITE_G) && r[0].ret_c == 1 && r[0].n_c == 2 && r[0].ret_g == 1 && r[0].n_g == 1);
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 4096, 4097, r, BSX_COV_TILE, &n, &next) == BSX_OK && n == 0 && next == 4097);
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 8192, 8193, r, BSX_COV_TILE, &n, &next) == BSX_OK && n == 1 && r[0].fpos == 8192 && r[0].flags == (BSX_METH_CLS_CG | BSX_METH_SITE_G));
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 77, 77, r, BSX_COV_TILE, &n, &next) == BSX_OK && n == 0 && next == 77);
	/* refused, and nothing written */
	memset(&guard, 0x5a, sizeof(guard)); r[0] = guard; n = -7; next = -7;
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG, r, BSX_COV_TILE - 1, &n, &next) == BSX_E_ARG);
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, -1, LG, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG && bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG + 1, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG);
	CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 9, 8, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG);
	o.min_cov = 0; CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG); o.min_cov = 1;
	o.type = BSX_METH_TYPE_C; CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG);   /* merge with type c */
	o.merge = 0; o.type = 3; CHECK(bsx_meth_host_sites(&g_idx, g_cnt, &o, 0, LG, r, BSX_COV_TILE, &n, &next) == BSX_E_ARG);
	CHECK(memcmp(&r[0], &guard, sizeof(guard)) == 0 && n == -7 && next == -7);
	free(r);
}

static void test_line_and_state(void)
{
	bsx_meth_site_opt_t o = {BSX_METH_TYPE_CG, 1, 1, 0};
	bsx_meth_site_t r, out[4];
	bsx_meth_state_t st;
	bsx_backend_t be;
	char buf[256];
	int64_t n = -1, next = -1;
	size_t l;
	/* mergecg's count: 501 of 1001 prints 0.500, and 0.5 * 1001 rounds to the even 500; 1 of 1500 prints 0.001, and 0.001 * 1500 = 1.5 rounds to 2 */
	memset(&r, 0, sizeof(r));
	r.fpos = 1000000005; r.ret_c = 501; r.n_c = 1001; r.ret_g = 1; r.n_g = 1500; r.flags = BSX_METH_SITE_C | BSX_METH_SITE_G;
	l = bsx_meth_bed_line(buf, "chr1", 1000000000, &o, &r); buf[l] = 0;
	CHECK(strcmp(buf, "chr1\t5\t7\t0.201\t2501\tC:0.500:1001,G:0.001:1500\n") == 0);   /* 502 of 2501 = 0.2007 */
	r.flags = BSX_METH_SITE_G; r.ret_c = r.n_c = 0; r.fpos = 1000000006;
	l = bsx_meth_bed_line(buf, "chr1", 1000000000, &o, &r); buf[l] = 0;
	CHECK(strcmp(buf, "chr1\t5\t7\t0.001\t1500\tC:.:0,G:0.001:1500\n") == 0);          /* 2 of 1500 */
	o.merge = 0; r.ret_g = 4294967295u; r.n_g = 4294967295u;
	l = bsx_meth_bed_line(buf, "chr1", 1000000000, &o, &r); buf[l] = 0;
	CHECK(strcmp(buf, "chr1\t6\t7\t1.000\t4294967295\n") == 0);
	/* the state of a backend without the seam */
	memset(&be, 0, sizeof(be));
	memset(&st, 0, sizeof(st));
	pthread_mutex_init(&st.mu, 0);
	o.merge = 1;
	CHECK(bsx_meth_state_sites(&st, &o, 0, LG, out, BSX_COV_TILE, &n, &next) == BSX_E_ARG);   /* off */
	bsx_meth_state_set(&st, 1);
	CHECK(bsx_meth_state_sites(&st, &o, 0, LG, out, BSX_COV_TILE, &n, &next) == BSX_OK && n == 0 && next == LG);   /* no chunk yet */
	CHECK(bsx_meth_attach(&st, &be, &g_idx) == BSX_OK);
	CHECK(bsx_meth_state_sites(&st, &o, 0, LG, out, BSX_COV_TILE, &n, &next) == BSX_OK && n == 0 && next == LG);   /* no record yet */
	st.cnt[4 * 9 + 1] = 2; st.cnt[4 * 10] = 1;
	CHECK(bsx_meth_state_sites(&st, &o, 0, LG, out, BSX_COV_TILE, &n, &next) == BSX_OK && n == 1 && next == LG && out[0].fpos == 9 && out[0].n_c == 2 && out[0].ret_g == 1);
	CHECK(bsx_meth_state_sites(&st, &o, 0, LG, out, 4, &n, &next) == BSX_E_ARG);
	bsx_meth_state_set(&st, 0);
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
	make_index();
	make_counters();
	test_files(argv[1]);
	test_windows_and_arguments();
	test_line_and_state();
	free(g_idx.pac); free(g_cnt);
	printf("ok\n");
	return 0;
}
