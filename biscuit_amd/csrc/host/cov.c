/* cov.c -- the BISCUITqc coverage tables while aligning: what scripts/QC.sh:136-421 derives from four `bedtools genomecov -bga -split` passes, two
 * intersects with a CpG list and twelve awk scripts, from a depth state kept while the records are written.  Per slice the jobs qc.c built go
 * to the backend's state (k_cov.hip); a backend without the seam (the CPU checker's) keeps the same state here: a difference array over forward
 * coordinates, scanned once for the largest depth and once for the histograms.  Also the BED reader of --qc-topgc / --qc-botgc and the files. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <zlib.h>
#include "cov.h"

/* ------------------------------------------------------------------ the rule on plain arrays */
int bsx_cov_host_add(const bsx_index_t *idx, int32_t *diff, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *pool, size_t pool_len)
{
	const int64_t L = idx->ref.l_pac;
	int64_t i;
	uint32_t k;
	for (i = 0; i < n; ++i) { /* nothing is added unless every job is valid */
		const bsx_qc_job_t *j = &jobs[i];
		uint64_t span = 0;
		if ((size_t)j->cig_off + j->n_cigar > pool_len || j->fpos < 0 || j->fpos > L) return BSX_E_ARG;
		for (k = 0; k < j->n_cigar; ++k) { const uint32_t c = pool[j->cig_off + k], op = c & 0xf; if (op > 4) return BSX_E_ARG; if (op == 0 || op == 2) span += c >> 4; }
		if ((uint64_t)j->fpos + span > (uint64_t)L) return BSX_E_ARG;
	}
	for (i = 0; i < n; ++i) {
		const bsx_qc_job_t *j = &jobs[i];
		const int q40 = j->flags & BSX_QC_COV_Q40 ? 1 : 0;
		int64_t y = j->fpos;
		if (!(j->flags & BSX_QC_COV)) continue;
		for (k = 0; k < j->n_cigar; ++k) {
			const uint32_t c = pool[j->cig_off + k], op = c & 0xf;
			const int64_t len = (int64_t)(c >> 4);
			if (op == 0 && len > 0) {
				++diff[2 * y]; --diff[2 * (y + len)];
				if (q40) { ++diff[2 * y + 1]; --diff[2 * (y + len) + 1]; }
			}
			if (op == 0 || op == 2) y += len;
		}
	}
	return BSX_OK;
}

int bsx_cov_host_paint(const bsx_index_t *idx, uint32_t *mask, int64_t n, const int64_t *beg_end)
{
	int64_t i, p;
	for (i = 0; i < n; ++i) if (beg_end[2 * i] < 0 || beg_end[2 * i] > beg_end[2 * i + 1] || beg_end[2 * i + 1] > idx->ref.l_pac) return BSX_E_ARG;
	for (i = 0; i < n; ++i) {
		const int64_t b = beg_end[2 * i], e = beg_end[2 * i + 1];
		for (p = b; p < e && (p & 31); ++p) mask[p >> 5] |= 1u << (p & 31);
		for (; p + 32 <= e; p += 32) mask[p >> 5] = ~0u;
		for (; p < e; ++p) mask[p >> 5] |= 1u << (p & 31);
	}
	return BSX_OK;
}

#define MBIT(m, p) ((m)[(p) >> 5] >> ((p) & 31) & 1)
int bsx_cov_host_tables(const bsx_index_t *idx, const int32_t *diff, const uint32_t *m_top, const uint32_t *m_bot, bsx_cov_tables_t *out)
{
	const int64_t L = idx->ref.l_pac;
	const bsx_amb_t *H = idx->ref.ambs;
	const int nh = idx->ref.n_holes, ns = idx->ref.n_seqs, gc = m_top && m_bot;
	int64_t p;
	int32_t a = 0, q = 0, vmax = 0;
	int h0 = 0, h1 = 0, ci = 0, i;
	uint64_t nb;
	memset(out, 0, sizeof(*out));
	if ((m_top != 0) != (m_bot != 0)) return BSX_E_ARG;
	for (p = 0; p < L; ++p) { a += diff[2 * p]; if (a > vmax) vmax = a; }
	nb = (uint64_t)vmax + 1;
	out->have_gc = gc;
	for (i = 0; i < (gc ? BSX_COV_N_TABLES : 4); ++i) {
		if (!(out->t[i].count = (uint64_t*)calloc(nb, 8))) { bsx_cov_tables_free(out); return BSX_E_NOMEM; }
		out->t[i].n_bins = nb;
	}
	for (p = 0, a = 0; p < L; ++p) {
		int top, bot, cpg;
		a += diff[2 * p]; q += diff[2 * p + 1];
		if (a < 0 || q < 0 || q > a) { bsx_cov_tables_free(out); return BSX_E_INTERNAL; }
		top = gc && MBIT(m_top, p); bot = gc && MBIT(m_bot, p);
		++out->t[0].count[a]; ++out->t[2].count[q];
		if (top) { ++out->t[4].count[a]; ++out->t[6].count[q]; }
		if (bot) { ++out->t[8].count[a]; ++out->t[10].count[q]; }
		cpg = p + 1 < L && bsx_pac_get(idx->pac, p) == 1 && bsx_pac_get(idx->pac, p + 1) == 2;
		if (!cpg) continue;
		/* both bases in one contig, neither in an N hole (sorted, disjoint: a cursor each for p and p + 1) */
		while (ci < ns && idx->ref.anns[ci].offset <= p) ++ci;
		if (ci < ns && idx->ref.anns[ci].offset == p + 1) continue;
		while (h0 < nh && H[h0].offset + H[h0].len <= p) ++h0;
		if (h0 < nh && H[h0].offset <= p) continue;
		while (h1 < nh && H[h1].offset + H[h1].len <= p + 1) ++h1;
		if (h1 < nh && H[h1].offset <= p + 1) continue;
		{
			const int32_t na = a + diff[2 * (p + 1)], nq = q + diff[2 * (p + 1) + 1], ma = na < a ? na : a, mq = nq < q ? nq : q;
			const int top1 = top || (gc && MBIT(m_top, p + 1)), bot1 = bot || (gc && MBIT(m_bot, p + 1));
			if (ma < 0 || mq < 0) { bsx_cov_tables_free(out); return BSX_E_INTERNAL; }
			++out->t[1].count[ma]; ++out->t[3].count[mq];
			if (top1) { ++out->t[5].count[ma]; ++out->t[7].count[mq]; }
			if (bot1) { ++out->t[9].count[ma]; ++out->t[11].count[mq]; }
		}
	}
	return BSX_OK;
}

BSX_API void bsx_cov_tables_free(bsx_cov_tables_t *t)
{
	int i;
	if (!t) return;
	for (i = 0; i < BSX_COV_N_TABLES; ++i) { free(t->t[i].count); t->t[i].count = 0; t->t[i].n_bins = 0; }
	t->have_gc = 0;
}

/* ------------------------------------------------------------------ state of a stream / of the process */
static void state_free(bsx_cov_state_t *c)
{
	free(c->iv[0]); free(c->iv[1]); free(c->diff);
	c->iv[0] = c->iv[1] = 0; c->diff = 0;
}
void bsx_cov_state_set(bsx_cov_state_t *c, int on)
{
	state_free(c);
	memset(c, 0, sizeof(*c));
	pthread_mutex_init(&c->mu, 0);
	c->on = on ? 1 : 0;
}

int bsx_cov_state_mask(bsx_cov_state_t *c, int which, int64_t n, const int64_t *beg_end)
{
	if (!c->on || c->attached || which < 0 || which > 1 || n < 0 || (n && !beg_end)) return BSX_E_ARG;
	free(c->iv[which]);
	c->iv[which] = (int64_t*)malloc((size_t)(n ? n : 1) * 16);
	if (!c->iv[which]) return BSX_E_NOMEM;
	if (n) memcpy(c->iv[which], beg_end, (size_t)n * 16);
	c->n_iv[which] = n; c->have_iv[which] = 1;
	return BSX_OK;
}

int bsx_cov_attach(bsx_cov_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx)
{
	int rc = BSX_OK, w;
	pthread_mutex_lock(&c->mu);
	if (!c->attached) {
		if (c->have_iv[0] != c->have_iv[1]) rc = BSX_E_ARG;
		else if (be->cov_batch) {
			rc = be->cov_batch(be->ctx, BSX_COV_OP_RESET, 0, 0, 0, 0, 0, 0);
			for (w = 0; w < 2 && rc == BSX_OK; ++w)
				if (c->have_iv[w]) rc = be->cov_batch(be->ctx, BSX_COV_OP_MASK + w, c->n_iv[w], 0, 0, 0, c->iv[w], 0);
			c->fn = be->cov_batch; c->ctx = be->ctx;
		} else {
			for (w = 0; w < 2 && rc == BSX_OK; ++w)   /* (checked here as the device checks them) */
				if (c->have_iv[w]) { int64_t i; for (i = 0; i < c->n_iv[w]; ++i) if (c->iv[w][2 * i] < 0 || c->iv[w][2 * i] > c->iv[w][2 * i + 1] || c->iv[w][2 * i + 1] > idx->ref.l_pac) rc = BSX_E_ARG; }
			if (rc == BSX_OK && !(c->diff = (int32_t*)calloc((size_t)idx->ref.l_pac + 1, 8))) rc = BSX_E_NOMEM;
			c->idx = idx;
		}
		if (rc == BSX_OK) c->attached = 1;
	}
	pthread_mutex_unlock(&c->mu);
	return rc;
}

int bsx_cov_slice(bsx_cov_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *pool, size_t pool_len)
{
	int rc;
	if (n <= 0) return BSX_OK;
	if (be->cov_batch) return be->cov_batch(be->ctx, BSX_COV_OP_BATCH, n, jobs, pool, pool_len, 0, 0);
	pthread_mutex_lock(&c->mu);
	rc = c->diff ? bsx_cov_host_add(idx, c->diff, n, jobs, pool, pool_len) : BSX_E_INTERNAL;
	pthread_mutex_unlock(&c->mu);
	return rc;
}

int bsx_cov_state_tables(bsx_cov_state_t *c, bsx_cov_tables_t *out)
{
	int rc = BSX_OK, w;
	if (!out) return BSX_E_ARG;
	memset(out, 0, sizeof(*out));
	if (!c->on) return BSX_E_ARG;
	pthread_mutex_lock(&c->mu);
	if (!c->attached) out->have_gc = c->have_iv[0] && c->have_iv[1];   /* no chunk was aligned: tables without rows */
	else if (c->fn) rc = c->fn(c->ctx, BSX_COV_OP_TABLES, 0, 0, 0, 0, 0, out);
	else {
		uint32_t *m[2] = {0, 0};
		for (w = 0; w < 2 && rc == BSX_OK; ++w) if (c->have_iv[w]) {
			if (!(m[w] = (uint32_t*)calloc((size_t)(c->idx->ref.l_pac + 63) / 32, 4))) rc = BSX_E_NOMEM;
			else rc = bsx_cov_host_paint(c->idx, m[w], c->n_iv[w], c->iv[w]);
		}
		if (rc == BSX_OK) rc = bsx_cov_host_tables(c->idx, c->diff, m[0], m[1], out);
		free(m[0]); free(m[1]);
	}
	pthread_mutex_unlock(&c->mu);
	return rc;
}

/* ------------------------------------------------------------------ the BED files of --qc-topgc / --qc-botgc */
static int bed_fail(const char *path, long line, const char *what) { fprintf(stderr, "[E::%s] %s, line %ld: %s\n", "bsx_cov_read_bed", path, line, what); return BSX_E_FORMAT; }
BSX_API int bsx_cov_read_bed(const char *path, const bsx_index_t *idx, int64_t *n_out, int64_t **out)
{
	gzFile f;
	char buf[4096];
	int64_t n = 0, cap = 0, *iv = 0;
	long line = 0;
	int rc = BSX_OK, last = 0, errnum = 0;
	if (!path || !idx || !n_out || !out) return BSX_E_ARG;
	*n_out = 0; *out = 0;
	if (!(f = gzopen(path, "rb"))) { fprintf(stderr, "[E::%s] cannot read %s\n", "bsx_cov_read_bed", path); return BSX_E_IO; }
	while (rc == BSX_OK && gzgets(f, buf, sizeof(buf))) {
		size_t l = strlen(buf);
		char *p = buf, *chrom, *e;
		long long beg, end;
		int ci;
		++line;
		if (l && buf[l - 1] == '\n') buf[--l] = 0;
		else if (l == sizeof(buf) - 1) { /* a long line: the three columns are at its start, the rest is skipped */
			char more[4096];
			while (gzgets(f, more, sizeof(more))) { size_t m = strlen(more); if (m && more[m - 1] == '\n') break; }
		}
		if (l && buf[l - 1] == '\r') buf[--l] = 0;
		while (*p == ' ' || *p == '\t') ++p;
		if (!*p || *p == '#') continue;
		chrom = p;
		while (*p && *p != '\t' && *p != ' ') ++p;
		if ((p - chrom == 5 && strncmp(chrom, "track", 5) == 0) || (p - chrom == 7 && strncmp(chrom, "browser", 7) == 0)) continue;   /* (the whole first word) */
		if (!*p) { rc = bed_fail(path, line, "fewer than three columns"); break; }
		*p++ = 0;
		while (*p == ' ' || *p == '\t') ++p;
		if (*p < '0' || *p > '9') { rc = bed_fail(path, line, "the start is not a number"); break; }
		beg = strtoll(p, &e, 10);
		if (*e != '\t' && *e != ' ') { rc = bed_fail(path, line, *e ? "the start is not a number" : "fewer than three columns"); break; }
		p = e;
		while (*p == ' ' || *p == '\t') ++p;
		if (*p < '0' || *p > '9') { rc = bed_fail(path, line, *p ? "the end is not a number" : "fewer than three columns"); break; }
		end = strtoll(p, &e, 10);
		if (*e && *e != '\t' && *e != ' ') { rc = bed_fail(path, line, "the end is not a number"); break; }
		ci = last;
		if (ci >= idx->ref.n_seqs || strcmp(idx->ref.anns[ci].name, chrom) != 0)
			for (ci = 0; ci < idx->ref.n_seqs; ++ci) if (strcmp(idx->ref.anns[ci].name, chrom) == 0) break;
		if (ci >= idx->ref.n_seqs) { fprintf(stderr, "[E::%s] %s, line %ld: contig %s is not in the index\n", "bsx_cov_read_bed", path, line, chrom); rc = BSX_E_FORMAT; break; }
		last = ci;
		if (beg > end || end > idx->ref.anns[ci].len) { rc = bed_fail(path, line, "the interval is not inside its contig"); break; }
		if (beg == end) continue;
		if (n == cap) {
			int64_t *t = (int64_t*)realloc(iv, (size_t)(cap = cap ? cap * 2 : 1024) * 16);
			if (!t) { rc = BSX_E_NOMEM; break; }
			iv = t;
		}
		iv[2 * n] = idx->ref.anns[ci].offset + beg; iv[2 * n + 1] = idx->ref.anns[ci].offset + end; ++n;
	}
	if (rc == BSX_OK) { (void)gzerror(f, &errnum); if (errnum != Z_OK && errnum != Z_STREAM_END) { fprintf(stderr, "[E::%s] %s: damaged or truncated\n", "bsx_cov_read_bed", path); rc = BSX_E_IO; } }
	gzclose(f);
	if (rc != BSX_OK) { free(iv); return rc; }
	if (!iv) iv = (int64_t*)malloc(16);
	*n_out = n; *out = iv;
	return BSX_OK;
}

/* ------------------------------------------------------------------ the files (scripts/QC.sh:153-415) */
static const char *const COV_NAME[BSX_COV_N_TABLES] = {"all_base", "all_cpg", "q40_base", "q40_cpg", "all_base_topgc", "all_cpg_topgc", "q40_base_topgc", "q40_cpg_topgc",
	"all_base_botgc", "all_cpg_botgc", "q40_base_botgc", "q40_cpg_botgc"};
static const char *const COV_TITLE[BSX_COV_N_TABLES] = {"All Bases", "All CpGs", "Q40 Bases", "Q40 CpGs", "All Top GC Bases", "All Top GC CpGs", "Q40 Top GC Bases", "Q40 Top GC CpGs",
	"All Bot GC Bases", "All Bot GC CpGs", "Q40 Bot GC Bases", "Q40 Bot GC CpGs"};
static FILE *cov_open(const char *prefix, const char *mid, const char *suffix)
{
	size_t l = strlen(prefix) + strlen(mid) + strlen(suffix) + 1;
	char *fn = (char*)malloc(l);
	FILE *f;
	snprintf(fn, l, "%s%s%s", prefix, mid, suffix);
	f = fopen(fn, "w");
	if (!f) fprintf(stderr, "[E::%s] cannot write %s\n", "bsx_cov_write", fn);
	free(fn);
	return f;
}
BSX_API int bsx_cov_write(const char *prefix, const bsx_cov_tables_t *t)
{
	FILE *cv, *f;
	int i, bad = 0;
	if (!prefix || !t) return BSX_E_ARG;
	if (!(cv = cov_open(prefix, "_cv_table", ".txt"))) return BSX_E_IO;
	fprintf(cv, "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n");
	for (i = 0; i < (t->have_gc ? BSX_COV_N_TABLES : 4); ++i) {
		char mid[64];
		unsigned __int128 s_cnt = 0, s_cov = 0;
		uint64_t d;
		/* _covdist_all_base_topgc_table.txt: class, kind, region */
		snprintf(mid, sizeof(mid), "_covdist_%s_table", COV_NAME[i]);
		if (!(f = cov_open(prefix, mid, ".txt"))) { fclose(cv); return BSX_E_IO; }
		fprintf(f, "BISCUITqc Depth Distribution - %s\ndepth\tcount\n", COV_TITLE[i]);
		for (d = 0; d < t->t[i].n_bins; ++d) {
			const uint64_t c = t->t[i].count[d];
			if (!c) continue;
			fprintf(f, "%llu\t%llu\n", (unsigned long long)d, (unsigned long long)c);
			s_cnt += c; s_cov += (unsigned __int128)c * d;
		}
		bad |= fclose(f) != 0;
		if (s_cnt > 0 && s_cov > 0) {
			const double mu = (double)s_cov / (double)s_cnt;
			double var = 0, sigma;
			for (d = 0; d < t->t[i].n_bins; ++d) if (t->t[i].count[d]) var += (double)t->t[i].count[d] * (((double)d - mu) * ((double)d - mu));
			sigma = sqrt(var / (double)s_cnt);
			fprintf(cv, "%s\t%.6g\t%.6g\t%.6g\n", COV_NAME[i], mu, sigma, sigma / mu);
		}
	}
	bad |= fclose(cv) != 0;
	return bad ? BSX_E_IO : BSX_OK;
}
