/* meth.c -- BISCUITqc's base-averaged conversion table while aligning: what scripts/QC.sh:423-450 derives with `biscuit pileup`, `biscuit vcf2bed
 * -e -t c` and awk from a sorted BAM, from four counters per forward reference position kept while the records are written.  Per slice the jobs
 * qc.c built go to the backend's counters (k_meth.hip); a backend without the seam (the CPU checker's) keeps the same counters here and makes
 * the sums here.  Also the beta in thousandths without printf, and the file. */
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
		if (be->meth_batch) { rc = be->meth_batch(be->ctx, BSX_METH_OP_RESET, 0, 0, 0, 0, 0); c->fn = be->meth_batch; c->ctx = be->ctx; }
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
