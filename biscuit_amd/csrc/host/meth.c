/* meth.c -- BISCUITqc's base-averaged conversion table while aligning: what scripts/QC.sh:423-450 derives with `biscuit pileup`, `biscuit vcf2bed
 * -e -t c` and awk from a sorted BAM, from four counters per forward reference position kept while the records are written.  Per slice the jobs
 * qc.c built go to the backend's counters (k_meth.hip); a backend without the seam (the CPU checker's) keeps the same counters here and makes
 * the sums here.  Also the beta in thousandths without printf, and the file.  And --meth-bed: the methylation sites of the same counters -- the
 * host statement of what k_msite.hip lists, the state's hand-over to the backend -- their lines without printf, the contig order of a SAM
 * header, and the BED file window by window. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "meth.h"

/* ------------------------------------------------------------------ the beta in thousandths */
BSX_API uint32_t bsx_meth_milli(uint32_t r, uint32_t n)
{
	const uint64_t num = 1000ull * r;
	const uint32_t m0 = (uint32_t)(num / n);
	const uint64_t rem = num - (uint64_t)m0 * n;
	if (2 * rem < n) return m0;
	if (2 * rem > n) return m0 + 1;
	{ /* a rational tie: printf rounds the double quotient, which lies on one side of the tie or is it (then: to even) */
		const double d = (double)r / (double)n, e = fma(d, (double)n, -(double)r);
		return e > 0 ? m0 + 1 : e < 0 ? m0 : (m0 & 1) ? m0 + 1 : m0;
	}
}

/* ------------------------------------------------------------------ the rule on plain arrays */
static int in_hole(const bsx_index_t *idx, int64_t f)
{
	const bsx_amb_t *h = idx->ref.ambs;
	int lo = 0, hi = idx->ref.n_holes;   /* the last hole that starts at or before f */
	while (lo < hi) { int mid = (lo + hi) >> 1; if (h[mid].offset <= f) lo = mid + 1; else hi = mid; }
	return lo > 0 && f < h[lo - 1].offset + h[lo - 1].len;
}
static int ctg_start(const bsx_index_t *idx, int64_t f)
{
	int lo = 0, hi = idx->ref.n_seqs;
	while (lo < hi) { int mid = (lo + hi) >> 1; if (idx->ref.anns[mid].offset < f) lo = mid + 1; else hi = mid; }
	return lo < idx->ref.n_seqs && idx->ref.anns[lo].offset == f;
}

static int job_valid(const bsx_index_t *idx, const bsx_meth_job_t *j, const uint32_t *pool, size_t pool_len)
{
	uint64_t span = 0, rspan = 0;
	uint32_t k;
	if ((size_t)j->cig_off + j->n_cigar > pool_len || j->rlen < 1 || j->rlen > (1u << 30) || (size_t)j->qm_off + (j->rlen + 31) / 32 > pool_len) return 0;
	if (j->fpos < 0 || j->fpos >= idx->ref.l_pac) return 0;
	for (k = 0; k < j->n_cigar; ++k) { const uint32_t c = pool[j->cig_off + k], op = c & 0xf; if (op > 4) return 0; span += c >> 4; if (op == 0 || op == 2) rspan += c >> 4; }
	return span <= (1u << 30) && (uint64_t)j->fpos + rspan <= (uint64_t)idx->ref.l_pac;
}

int bsx_meth_host_add(const bsx_index_t *idx, uint32_t *cnt, const uint8_t *reads, size_t reads_len, int64_t n, const bsx_meth_job_t *jobs,
                      const uint32_t *pool, size_t pool_len)
{
	int64_t i;
	for (i = 0; i < n; ++i) if (!job_valid(idx, &jobs[i], pool, pool_len)) return BSX_E_ARG;
	for (i = 0; i < n; ++i) {
		const bsx_meth_job_t *j = &jobs[i];
		const uint32_t *cig = pool + j->cig_off, *qm = pool + j->qm_off;
		const int rev = j->flags & BSX_QC_REVERSE ? 1 : 0, read2 = j->flags & BSX_QC_READ2 ? 1 : 0, tag = (int)BSX_QC_TAG(j->flags);
		const int64_t rlen = (int64_t)j->rlen;
		const int npass = tag != 0 && tag != 1 ? 2 : 1;   /* get_bsstrand (bisc_utils.c:208-238): YD:f 0, YD:r 1, anything else inferred first */
		int pass, strand = tag == 1 ? 1 : 0, nC2T = 0, nG2A = 0;
		for (pass = 0; pass < npass; ++pass) {
			const int infer = npass == 2 && pass == 0;
			int64_t x = 0, y = 0, c;
			uint32_t k;
			for (k = 0; k < j->n_cigar; ++k) {
				const int op = (int)(cig[k] & 0xf);
				const int64_t len = (int64_t)(cig[k] >> 4);
				if (op == 0) {
					for (c = 0; c < len; ++c) {
						const int64_t qp = x + c, f = j->fpos + y + c, at = (int64_t)j->roff + (rev ? rlen - 1 - qp : qp) - j->rskip;
						int q, r, own, ref, alt;
						if (qp >= rlen || !(qm[qp >> 5] >> (qp & 31) & 1)) continue;   /* pileup.c:380, bisc_utils.c:180 */
						q = at >= 0 && (size_t)at < reads_len ? reads[at] : 4;
						if (rev) q = q < 4 ? 3 - q : 4;
						r = in_hole(idx, f) ? 4 : bsx_pac_get(idx->pac, f);
						if (infer) { nC2T += r == 1 && q == 3; nG2A += r == 2 && q == 0; continue; }
						if (qp + 1 <= 3 || rlen < qp + 1 + 3) continue;   /* pileup.c:383 */
						if (read2 && f >= j->ov_beg && f < j->ov_end) continue;   /* pileup.c:773-778 */
						if (r != 1 && r != 2) continue;
						own = r == (strand ? 2 : 1); ref = q == r; alt = q == (r == 1 ? 3 : 0);
						if (ref || alt) ++cnt[4 * f + (own ? 0 : 2) + alt];
					}
					x += len; y += len;
				} else if (op == 2) y += len;
				else x += len;
			}
			if (infer) strand = nC2T >= nG2A ? 0 : 1;   /* infer_bsstrand, bisc_utils.c:204 */
		}
	}
	return BSX_OK;
}

int bsx_meth_host_tables(const bsx_index_t *idx, const uint32_t *cnt, bsx_meth_tables_t *out)
{
	const int64_t L = idx->ref.l_pac;
	int64_t p;
	memset(out, 0, sizeof(*out));
	for (p = 0; p < L; ++p) {
		const uint32_t *c = cnt + 4 * p;
		const uint32_t n = c[0] + c[1];
		const int b = bsx_pac_get(idx->pac, p);
		int ctx = 4;
		if (!n || (b != 1 && b != 2) || in_hole(idx, p)) continue;
		if (c[3] != 0 && !(20ull * c[3] < (uint64_t)c[0] + c[2])) continue;   /* pileup.c:472-484 */
		if (b == 1) { if (p + 1 < L && !ctg_start(idx, p + 1) && !in_hole(idx, p + 1)) ctx = bsx_pac_get(idx->pac, p + 1); }
		else if (p > 0 && !ctg_start(idx, p) && !in_hole(idx, p - 1)) ctx = 3 - bsx_pac_get(idx->pac, p - 1);
		++out->k[ctx]; out->s[ctx] += bsx_meth_milli(c[0], n);
	}
	return BSX_OK;
}

/* ------------------------------------------------------------------ state of a stream / of the process */
void bsx_meth_state_set(bsx_meth_state_t *c, int on)
{
	free(c->cnt);
	memset(c, 0, sizeof(*c));
	pthread_mutex_init(&c->mu, 0);
	c->on = on ? 1 : 0;
}

int bsx_meth_attach(bsx_meth_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx)
{
	int rc = BSX_OK;
	pthread_mutex_lock(&c->mu);
	if (!c->attached) {
		if (be->meth_batch) { rc = be->meth_batch(be->ctx, BSX_METH_OP_RESET, 0, 0, 0, 0, 0); c->fn = be->meth_batch; c->sites = be->meth_sites; c->ctx = be->ctx; }
		else if (!(c->cnt = (uint32_t*)calloc((size_t)idx->ref.l_pac + 1, 16))) rc = BSX_E_NOMEM;
		c->idx = idx;
		if (rc == BSX_OK) c->attached = 1;
	}
	pthread_mutex_unlock(&c->mu);
	return rc;
}

int bsx_meth_slice(bsx_meth_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx, const uint8_t *reads, size_t reads_len, int64_t n,
                   const bsx_meth_job_t *jobs, const uint32_t *pool, size_t pool_len)
{
	int rc;
	if (n <= 0) return BSX_OK;
	if (be->meth_batch) return be->meth_batch(be->ctx, BSX_METH_OP_BATCH, n, jobs, pool, pool_len, 0);
	pthread_mutex_lock(&c->mu);
	rc = c->cnt ? bsx_meth_host_add(idx, c->cnt, reads, reads_len, n, jobs, pool, pool_len) : BSX_E_INTERNAL;
	pthread_mutex_unlock(&c->mu);
	return rc;
}

int bsx_meth_state_tables(bsx_meth_state_t *c, bsx_meth_tables_t *out)
{
	int rc = BSX_OK;
	if (!out) return BSX_E_ARG;
	memset(out, 0, sizeof(*out));
	if (!c->on) return BSX_E_ARG;
	pthread_mutex_lock(&c->mu);
	if (!c->attached) ;   /* no chunk was aligned: no site */
	else if (c->fn) rc = c->fn(c->ctx, BSX_METH_OP_TABLES, 0, 0, 0, 0, out);
	else rc = bsx_meth_host_tables(c->idx, c->cnt, out);
	pthread_mutex_unlock(&c->mu);
	return rc;
}

/* ------------------------------------------------------------------ the file (scripts/QC.sh:424-450) */
BSX_API int bsx_meth_write(const char *prefix, const bsx_meth_tables_t *t)
{
	static const char suffix[] = "_totalBaseConversionRate.txt";
	char *fn;
	FILE *f;
	int i;
	if (!prefix || !t) return BSX_E_ARG;
	if (!(fn = (char*)malloc(strlen(prefix) + sizeof(suffix)))) return BSX_E_NOMEM;
	sprintf(fn, "%s%s", prefix, suffix);
	f = fopen(fn, "w");
	if (!f) fprintf(stderr, "[E::%s] cannot write %s\n", "bsx_meth_write", fn);
	free(fn);
	if (!f) return BSX_E_IO;
	fprintf(f, "BISCUITqc Conversion Rate by Base Average Table\nCA\tCC\tCG\tCT\n");
	for (i = 0; i < 4; ++i) { /* (the mean of the betas as printed to three places, from exact integer sums) */
		if (i) fprintf(f, "\t");
		if (t->k[i] < 20) fprintf(f, "-1");
		else fprintf(f, "%.6g", (double)t->s[i] / (1000.0 * (double)t->k[i]));
	}
	fprintf(f, "\n");
	return fclose(f) != 0 ? BSX_E_IO : BSX_OK;
}

/* ------------------------------------------------------------------ the methylation sites of the counters (--meth-bed): the rule on plain arrays */
typedef struct { uint32_t ret, n; int cls, isg, kept; } msite_t;

/* the site at f: pileup's CX (bisc_utils.c:33-72) over f - 2 .. f + 2 on the cytosine's own strand, vcf2bed's -t and -k */
static msite_t host_site(const bsx_index_t *idx, const uint32_t *cnt, const bsx_meth_site_opt_t *opt, int64_t f)
{
	const int64_t L = idx->ref.l_pac;
	msite_t s = {0, 0, BSX_METH_CLS_CN, 0, 0};
	const uint32_t *c;
	int b, d, full, n1, n2;
	if (f < 0 || f >= L) return s;
	b = bsx_pac_get(idx->pac, f);
	c = cnt + 4 * f;
	if ((b != 1 && b != 2) || c[0] + c[1] == 0 || in_hole(idx, f)) return s;
	if (c[3] != 0 && !(20ull * c[3] < (uint64_t)c[0] + c[2])) return s;   /* pileup.c:472-484 */
	full = f >= 2 && f + 2 < L;
	for (d = -2; d <= 2 && full; ++d) if ((d != -2 && ctg_start(idx, f + d)) || (d != 0 && in_hole(idx, f + d))) full = 0;
	if (full) {
		n1 = b == 1 ? bsx_pac_get(idx->pac, f + 1) : 3 - bsx_pac_get(idx->pac, f - 1);
		n2 = b == 1 ? bsx_pac_get(idx->pac, f + 2) : 3 - bsx_pac_get(idx->pac, f - 2);
		s.cls = n1 == 2 ? BSX_METH_CLS_CG : n2 == 2 ? BSX_METH_CLS_CHG : BSX_METH_CLS_CHH;
	}
	s.ret = c[0]; s.n = c[0] + c[1]; s.isg = b == 2;
	s.kept = (opt->type == BSX_METH_TYPE_C || (opt->type == BSX_METH_TYPE_CG ? s.cls == BSX_METH_CLS_CG : s.cls == BSX_METH_CLS_CHG || s.cls == BSX_METH_CLS_CHH))
	         && s.n >= opt->min_cov;
	return s;
}

static int site_opt_ok(const bsx_meth_site_opt_t *opt)
{
	return opt && opt->type >= BSX_METH_TYPE_CG && opt->type <= BSX_METH_TYPE_C && opt->min_cov >= 1 && !(opt->merge && opt->type != BSX_METH_TYPE_CG);
}

int bsx_meth_host_sites(const bsx_index_t *idx, const uint32_t *cnt, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out,
                        int64_t cap, int64_t *n, int64_t *f_next)
{
	int64_t tb, f, got = 0;
	if (!site_opt_ok(opt) || !n || !f_next || !out || f_lo < 0 || f_lo > f_hi || f_hi > idx->ref.l_pac || cap < BSX_COV_TILE) return BSX_E_ARG;
	for (tb = f_lo / BSX_COV_TILE * BSX_COV_TILE; tb < f_hi; tb += BSX_COV_TILE) { /* whole tiles: one that does not fit is left to the next call */
		const int64_t a = tb > f_lo ? tb : f_lo, e = tb + BSX_COV_TILE < f_hi ? tb + BSX_COV_TILE : f_hi, got0 = got;
		for (f = a; f < e; ++f) {
			const msite_t s = host_site(idx, cnt, opt, f);
			bsx_meth_site_t r;
			if (!s.kept) continue;
			memset(&r, 0, sizeof(r));
			r.fpos = f;
			if (!opt->merge) {
				if (s.isg) { r.ret_g = s.ret; r.n_g = s.n; } else { r.ret_c = s.ret; r.n_c = s.n; }
				r.flags = (uint32_t)s.cls | (s.isg ? BSX_METH_SITE_G : BSX_METH_SITE_C);
			} else if (!s.isg) { /* mergecg.c:206-215: the kept G behind a kept C goes into the C's line */
				const msite_t g = host_site(idx, cnt, opt, f + 1);
				r.ret_c = s.ret; r.n_c = s.n; r.flags = BSX_METH_CLS_CG | BSX_METH_SITE_C;
				if (g.kept && g.isg) { r.ret_g = g.ret; r.n_g = g.n; r.flags |= BSX_METH_SITE_G; }
			} else {
				const msite_t p = host_site(idx, cnt, opt, f - 1);
				if (p.kept && !p.isg) continue;
				r.ret_g = s.ret; r.n_g = s.n; r.flags = (uint32_t)s.cls | BSX_METH_SITE_G;
			}
			if (got == cap) { *n = got0; *f_next = tb; return BSX_OK; }
			out[got++] = r;
		}
	}
	*n = got; *f_next = f_hi;
	return BSX_OK;
}

int bsx_meth_state_sites(bsx_meth_state_t *c, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n,
                         int64_t *f_next)
{
	int rc = BSX_OK;
	if (!c->on || !site_opt_ok(opt) || !n || !f_next || !out || f_lo < 0 || f_lo > f_hi || cap < BSX_COV_TILE) return BSX_E_ARG;
	pthread_mutex_lock(&c->mu);
	if (!c->attached) { *n = 0; *f_next = f_hi; }   /* no chunk was aligned: no site */
	else if (c->fn) rc = c->sites ? c->sites(c->ctx, opt, f_lo, f_hi, out, cap, n, f_next) : BSX_E_INTERNAL;
	else rc = bsx_meth_host_sites(c->idx, c->cnt, opt, f_lo, f_hi, out, cap, n, f_next);
	pthread_mutex_unlock(&c->mu);
	return rc;
}

/* ------------------------------------------------------------------ the BED file (vcf2bed.c:150-185, mergecg.c:90-137) */
static char *put_u64(char *p, uint64_t v)
{
	char t[24];
	int k = 0;
	do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (k) *p++ = t[--k];
	return p;
}
static char *put_milli(char *p, uint32_t m)   /* %1.3f of m thousandths */
{
	p = put_u64(p, m / 1000);
	*p++ = '.'; *p++ = (char)('0' + m / 100 % 10); *p++ = (char)('0' + m / 10 % 10); *p++ = (char)('0' + m % 10);
	return p;
}
/* mergecg.c:116-118 on one side: the beta as printed and read back (atof of d.ddd is the double nearest to milli / 1000), times the depth in
 * double, rounded to an integer as a float */
static float merged_side(uint32_t ret, uint32_t n)
{
	if (!n) return 0.0f;
	return rintf((float)((double)bsx_meth_milli(ret, n) / 1000.0 * (double)(int)n));
}

BSX_API size_t bsx_meth_bed_line(char *buf, const char *name, int64_t ctg_off, const bsx_meth_site_opt_t *opt, const bsx_meth_site_t *r)
{
	const size_t l = strlen(name);
	const int64_t f = r->fpos - ctg_off;
	char *p = buf + l;
	memcpy(buf, name, l);
	*p++ = '\t';
	if (!opt->merge) {
		const uint32_t ret = r->flags & BSX_METH_SITE_G ? r->ret_g : r->ret_c, n = r->flags & BSX_METH_SITE_G ? r->n_g : r->n_c;
		p = put_u64(p, (uint64_t)f); *p++ = '\t'; p = put_u64(p, (uint64_t)f + 1); *p++ = '\t';
		p = put_milli(p, bsx_meth_milli(ret, n)); *p++ = '\t'; p = put_u64(p, n);
	} else {
		const int has_c = (r->flags & BSX_METH_SITE_C) != 0;
		const uint32_t n_c = has_c ? r->n_c : 0, n_g = r->flags & BSX_METH_SITE_G ? r->n_g : 0, cov = n_c + n_g;
		const int M = (int)(merged_side(r->ret_c, n_c) + merged_side(r->ret_g, n_g));
		p = put_u64(p, (uint64_t)(has_c ? f : f - 1)); *p++ = '\t'; p = put_u64(p, (uint64_t)(has_c ? f + 2 : f + 1)); *p++ = '\t';
		p = put_milli(p, bsx_meth_milli((uint32_t)M, cov)); *p++ = '\t'; p = put_u64(p, cov);
		memcpy(p, "\tC:", 3); p += 3;
		if (n_c) { p = put_milli(p, bsx_meth_milli(r->ret_c, n_c)); *p++ = ':'; p = put_u64(p, n_c); } else { memcpy(p, ".:0", 3); p += 3; }
		memcpy(p, ",G:", 3); p += 3;
		if (n_g) { p = put_milli(p, bsx_meth_milli(r->ret_g, n_g)); *p++ = ':'; p = put_u64(p, n_g); } else { memcpy(p, ".:0", 3); p += 3; }
	}
	*p++ = '\n';
	return (size_t)(p - buf);
}

BSX_API int bsx_meth_bed_write(FILE *fp, const bsx_index_t *idx, const int32_t *order, const bsx_meth_site_opt_t *opt, bsx_meth_sites_fn sites, void *ud,
                               int64_t cap, uint64_t *n_lines)
{
	bsx_meth_site_t *recs;
	char *text;
	size_t max_name = 0, line_cap;
	uint64_t lines = 0;
	int rc = BSX_OK, i;
	if (!fp || !idx || !site_opt_ok(opt) || !sites || cap < 0 || (cap && cap < BSX_COV_TILE)) return BSX_E_ARG;
	if (!cap) cap = 1 << 20;
	for (i = 0; i < idx->ref.n_seqs; ++i) { const size_t l = strlen(idx->ref.anns[i].name); if (l > max_name) max_name = l; }
	line_cap = max_name + 160;
	recs = (bsx_meth_site_t*)malloc((size_t)cap * sizeof(*recs));
	text = (char*)malloc(line_cap * 4096);   /* 4096 lines at a time */
	if (!recs || !text) { free(recs); free(text); return BSX_E_NOMEM; }
	for (i = 0; i < idx->ref.n_seqs && rc == BSX_OK; ++i) {
		const bsx_ann_t *a = &idx->ref.anns[order ? order[i] : i];
		int64_t f = a->offset, end = a->offset + a->len;
		if (order && (order[i] < 0 || order[i] >= idx->ref.n_seqs)) { rc = BSX_E_ARG; break; }
		while (f < end && rc == BSX_OK) {
			int64_t n = 0, next = end, k;
			size_t used = 0;
			if ((rc = sites(ud, opt, f, end, recs, cap, &n, &next)) != BSX_OK) break;
			if (n < 0 || n > cap || next <= f || next > end) { rc = BSX_E_INTERNAL; break; }
			for (k = 0; k < n; ++k) {
				if (recs[k].fpos < a->offset || recs[k].fpos >= end) { rc = BSX_E_INTERNAL; break; }
				used += bsx_meth_bed_line(text + used, a->name, a->offset, opt, &recs[k]);
				if (((k + 1) & 4095) == 0 || k + 1 == n) { if (fwrite(text, 1, used, fp) != used) { rc = BSX_E_IO; break; } used = 0; }
			}
			lines += (uint64_t)n;
			f = next;
		}
	}
	free(recs); free(text);
	if (n_lines) *n_lines = lines;
	return rc;
}

typedef struct { const char *name; int32_t idx; } order_name_t;
static int order_name_cmp(const void *a, const void *b)
{
	const order_name_t *x = (const order_name_t*)a, *y = (const order_name_t*)b;
	const int c = strcmp(x->name, y->name);
	return c ? c : (x->idx > y->idx) - (x->idx < y->idx);
}
BSX_API int32_t *bsx_meth_bed_order(const bsx_index_t *idx, const char *hdr)
{
	const int ns = idx->ref.n_seqs;
	int32_t *order = (int32_t*)malloc(sizeof(int32_t) * (size_t)(ns ? ns : 1));
	order_name_t *by_name = (order_name_t*)malloc(sizeof(order_name_t) * (size_t)(ns ? ns : 1));
	char *taken = (char*)calloc((size_t)(ns ? ns : 1), 1);
	const char *p;
	int i, n = 0;
	if (!order || !by_name || !taken) { free(order); free(by_name); free(taken); return 0; }
	for (i = 0; i < ns; ++i) { by_name[i].name = idx->ref.anns[i].name; by_name[i].idx = i; }
	qsort(by_name, (size_t)ns, sizeof(*by_name), order_name_cmp);
	for (p = hdr; p && *p; ) { /* the @SQ lines as written; the first of two equal names counts */
		const char *eol = strchr(p, '\n'), *end = eol ? eol : p + strlen(p), *f = p + 3;
		if (strncmp(p, "@SQ\t", 4) == 0) while (f < end) { /* the SN field */
			const char *g = (const char*)memchr(f + 1, '\t', (size_t)(end - f - 1));
			if (!g) g = end;
			if (strncmp(f + 1, "SN:", 3) == 0 && f + 4 <= g) {
				const size_t l = (size_t)(g - (f + 4));
				int lo = 0, hi = ns;   /* the first contig of the index, in name order, whose name is not below this one */
				while (lo < hi) { const int mid = (lo + hi) >> 1; if (strncmp(by_name[mid].name, f + 4, l) < 0) lo = mid + 1; else hi = mid; }
				if (lo < ns && strncmp(by_name[lo].name, f + 4, l) == 0 && by_name[lo].name[l] == 0 && !taken[by_name[lo].idx]) {
					taken[by_name[lo].idx] = 1; order[n++] = by_name[lo].idx;   /* (of the names that begin with it the equal one comes first; equal ones by index) */
				}
				break;
			}
			f = g;
		}
		p = eol ? eol + 1 : 0;
	}
	for (i = 0; i < ns; ++i) if (!taken[i]) order[n++] = i;   /* no @SQ line: behind the others, in the index's order */
	free(by_name); free(taken);
	return order;
}
