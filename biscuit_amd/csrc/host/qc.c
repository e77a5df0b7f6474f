/* qc.c -- the BISCUITqc tables while aligning: process_qc (src/qc.c:112-179) applied to each record as it is written.  The final pass
 * (sam.c) notes every record; per slice the record fields are counted here (MAPQ and insert-size histograms, read totals, the strand table)
 * and the mapped records go to the backend as one batch of jobs (k_qc.hip keeps the column counts on the device).  A backend without
 * qc_batch (the CPU checker's): bsx_qc_walk_host does a job's columns here.  bsx_qc_write has the formatters of src/qc.c:29-110. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qc.h"

void bsx_qc_state_set(bsx_qc_state_t *q, int on)
{
	bsx_cov_state_set(&q->cov, 0);   /* (frees what an earlier run's state holds) */
	bsx_meth_state_set(&q->meth, 0);
	memset(q, 0, sizeof(*q));
	pthread_mutex_init(&q->mu, 0);
	pthread_mutex_init(&q->cov.mu, 0);
	pthread_mutex_init(&q->meth.mu, 0);
	q->on = on ? 1 : 0;
}

static void counts_add(bsx_qc_counts_t *dst, const bsx_qc_counts_t *src)
{
	uint64_t *d = (uint64_t*)dst;
	const uint64_t *s = (const uint64_t*)src;
	size_t i;
	for (i = 0; i < sizeof(*dst) / 8; ++i) d[i] += s[i];
}

/* forward base at forward coordinate f, 4 outside [cb, ce) (the record's contig) or in an N hole */
static int base_or_n(const bsx_index_t *idx, int64_t cb, int64_t ce, int64_t f)
{
	const bsx_amb_t *h = idx->ref.ambs;
	int lo = 0, hi = idx->ref.n_holes;   /* the last hole that starts at or before f */
	if (f < cb || f >= ce) return 4;
	while (lo < hi) { int mid = (lo + hi) >> 1; if (h[mid].offset <= f) lo = mid + 1; else hi = mid; }
	if (lo > 0 && f < h[lo - 1].offset + h[lo - 1].len) return 4;
	return bsx_pac_get(idx->pac, f);
}

void bsx_qc_walk_host(const bsx_index_t *idx, const uint8_t *reads, size_t reads_len, const bsx_qc_job_t *j, const uint32_t *cig, bsx_qc_counts_t *acc)
{
	const int rev = j->flags & BSX_QC_REVERSE ? 1 : 0, read2 = j->flags & BSX_QC_READ2 ? 1 : 0, tag = (int)BSX_QC_TAG(j->flags);
	const int cin = j->flags & BSX_QC_CINREAD ? 1 : 0, bsc = j->flags & BSX_QC_BSCONV ? 1 : 0, rlen = (int)j->rlen;
	int64_t cb = 0, ce = idx->ref.l_pac;
	int rid, pass, strand = tag == 1 ? 1 : 0, nC2T = 0, nG2A = 0;
	for (rid = 0; rid < idx->ref.n_seqs; ++rid)
		if (j->fpos >= idx->ref.anns[rid].offset && j->fpos < idx->ref.anns[rid].offset + idx->ref.anns[rid].len) { cb = idx->ref.anns[rid].offset; ce = cb + idx->ref.anns[rid].len; break; }
	/* first the record's own nC2T / nG2A (bsstrand.c:80-111), then the marks with the strand they may have decided (bisc_utils.c:208-238) */
	for (pass = 0; pass < 2; ++pass) {
		uint32_t k;
		int x = 0, i;
		int64_t y = 0;
		if (pass == 1 && !cin && !bsc) break;
		for (k = 0; k < j->n_cigar; ++k) {
			const int op = (int)(cig[k] & 0xf), len = (int)(cig[k] >> 4);
			if (op == 0) {
				for (i = 0; i < len; ++i) {
					const int qp = x + i, r = base_or_n(idx, cb, ce, j->fpos + y + i);
					const int64_t at = (int64_t)j->roff + (rev ? rlen - 1 - qp : qp) - j->rskip;
					int q = at >= 0 && (size_t)at < reads_len ? reads[at] : 4, nf, nb, ret, conv, pos;
					if (rev) q = q < 4 ? 3 - q : 4;
					if (pass == 0) { nC2T += r == 1 && q == 3; nG2A += r == 2 && q == 0; continue; }
					if (r != (strand ? 2 : 1)) continue;
					nf = base_or_n(idx, cb, ce, j->fpos + y + i + (strand ? -1 : 1));
					nb = strand ? (nf < 4 ? 3 - nf : 4) : nf;   /* fivenuc[3] (bisc_utils.c:33-52) */
					ret = q == r; conv = strand ? q == 0 : q == 3;
					if (!ret && !conv) continue;
					if (bsc && nb < 4) ++acc->conv[nb * 2 + conv];
					pos = rev ? rlen - qp : qp;
					if (cin && pos >= 0 && pos < BSX_QC_READ_LEN) ++acc->readpos[nb == 2 ? 0 : 1][read2][pos][conv ? 0 : 1];
				}
				x += len; y += len;
			} else if (op == 2) y += len;
			else x += len;
		}
		if (pass == 0) {
			if (j->flags & BSX_QC_STRAND) ++acc->confusion[tag * 4 + (nC2T == 0 && nG2A == 0 ? 3 : nC2T > nG2A ? 0 : nC2T < nG2A ? 1 : 2)];   /* bsstrand.c:115-132 */
			if (tag != 0 && tag != 1) strand = nC2T >= nG2A ? 0 : 1;
		}
	}
}

/* the records of the slice that count towards the base-averaged conversion table (sam.c has applied the record filters) as jobs of their own:
 * what the QC job has, the strand tag, the quality mask behind the CIGAR words in one pool, the mate overlap */
static int meth_slice(bsx_qc_state_t *q, const bsx_backend_t *be, const bsx_index_t *idx, const uint8_t *reads, size_t reads_len, const samctx_t *ctx, size_t n_units)
{
	bsx_meth_job_t *jobs;
	uint32_t *pool;
	size_t u, k, n_recs = 0, n_words = 0, nj = 0, nw = 0;
	int rc;
	for (u = 0; u < n_units; ++u) { n_recs += ctx[u].qc_recs.n; n_words += ctx[u].qc_cig.n + ctx[u].qc_qm.n; }
	jobs = (bsx_meth_job_t*)malloc(sizeof(*jobs) * (n_recs ? n_recs : 1));
	pool = (uint32_t*)malloc(4 * n_words + 4);
	for (u = 0; u < n_units; ++u) {
		const size_t cig0 = nw, qm0 = nw + ctx[u].qc_cig.n;
		for (k = 0; k < ctx[u].qc_recs.n; ++k) {
			const bsx_qc_rec_t *r = &ctx[u].qc_recs.a[k];
			bsx_meth_job_t *j = &jobs[nj];
			if (!r->mapped || !r->meth) continue;
			memset(j, 0, sizeof(*j));
			j->fpos = r->job.fpos; j->roff = r->job.roff; j->rskip = r->job.rskip; j->rlen = r->job.rlen;
			j->cig_off = (uint32_t)cig0 + r->job.cig_off; j->n_cigar = r->job.n_cigar;
			j->flags = r->job.flags & (BSX_QC_REVERSE | BSX_QC_READ2 | 3u << 2);
			j->qm_off = (uint32_t)qm0 + r->qm_off;
			j->ov_beg = r->ov_beg; j->ov_end = r->ov_end;
			++nj;
		}
		if (ctx[u].qc_cig.n) memcpy(pool + cig0, ctx[u].qc_cig.a, 4 * ctx[u].qc_cig.n);
		if (ctx[u].qc_qm.n) memcpy(pool + qm0, ctx[u].qc_qm.a, 4 * ctx[u].qc_qm.n);
		nw = qm0 + ctx[u].qc_qm.n;
	}
	rc = bsx_meth_slice(&q->meth, be, idx, reads, reads_len, (int64_t)nj, jobs, pool, nw);
	free(jobs); free(pool);
	return rc;
}

int bsx_qc_slice(bsx_qc_state_t *q, const bsx_backend_t *be, const bsx_index_t *idx, const uint8_t *reads, size_t reads_len,
                 const samctx_t *ctx, size_t n_units)
{
	bsx_qc_totals_t *t;
	bsx_qc_job_t *jobs;
	uint32_t *pool;
	size_t u, k, n_recs = 0, n_words = 0, nj = 0, nw = 0;
	int rc = BSX_OK, i;
	for (u = 0; u < n_units; ++u) { n_recs += ctx[u].qc_recs.n; n_words += ctx[u].qc_cig.n; }
	if (q->cov.on && (rc = bsx_cov_attach(&q->cov, be, idx)) != BSX_OK) return rc;
	if (q->meth.on && (rc = bsx_meth_attach(&q->meth, be, idx)) != BSX_OK) return rc;
	if (n_recs == 0) return BSX_OK;
	t = (bsx_qc_totals_t*)calloc(1, sizeof(*t));
	jobs = (bsx_qc_job_t*)malloc(sizeof(*jobs) * n_recs);
	pool = (uint32_t*)malloc(4 * n_words + 4);
	for (u = 0; u < n_units; ++u) {
		for (k = 0; k < ctx[u].qc_recs.n; ++k) { /* process_qc, src/qc.c:125-160 */
			const bsx_qc_rec_t *r = &ctx[u].qc_recs.a[k];
			++t->all_tot;
			if (r->flag & 0x400) ++t->all_dup;   /* (only --markdup sets it) */
			if (r->mapq >= 40) { ++t->q40_tot; if (r->flag & 0x400) ++t->q40_dup; }
			if (!(r->flag & 0x100)) {
				if (r->flag & 0x4) ++t->mapq[BSX_QC_N_MAPQ];
				else if (r->mapq <= BSX_QC_N_MAPQ) ++t->mapq[r->mapq];
				if ((r->flag & 0x2) && r->mapq >= 40 && r->tlen >= 0 && r->tlen <= BSX_QC_ISIZE) { ++t->n_isize; ++t->isize[r->tlen]; }
			}
			if (!r->mapped) continue;
			++t->strandcnt[(r->flag & 0x40 ? 0 : 1) * 8 + (r->flag & 0x10 ? 1 : 0) * 4 + (int)BSX_QC_TAG(r->job.flags)];   /* bsstrand.c:154-155 */
			jobs[nj] = r->job;
			jobs[nj].cig_off = (uint32_t)nw + r->job.cig_off;
			if (q->cov.on) jobs[nj].flags |= BSX_QC_COV | (r->mapq >= 40 ? BSX_QC_COV_Q40 : 0);   /* every record without 0x4 (`genomecov -ibam`); q40: `samtools view -q 40` */
			++nj;
		}
		if (ctx[u].qc_cig.n) memcpy(pool + nw, ctx[u].qc_cig.a, 4 * ctx[u].qc_cig.n);
		nw += ctx[u].qc_cig.n;
	}
	if (nj && be->qc_batch && q->cov.on && be->cov_batch) rc = be->cov_batch(be->ctx, BSX_COV_OP_QC_BATCH, (int64_t)nj, jobs, pool, nw, 0, 0);   /* one upload, k_qc and k_cov_add */
	else if (nj && be->qc_batch) rc = be->qc_batch(be->ctx, (int64_t)nj, jobs, pool, nw, 0, 0);
	else for (k = 0; k < nj; ++k) bsx_qc_walk_host(idx, reads, reads_len, &jobs[k], pool + jobs[k].cig_off, &t->dev);
	if (rc == BSX_OK && q->cov.on && !(be->qc_batch && be->cov_batch)) rc = bsx_cov_slice(&q->cov, be, idx, (int64_t)nj, jobs, pool, nw);
	if (rc == BSX_OK && q->meth.on) rc = meth_slice(q, be, idx, reads, reads_len, ctx, n_units);
	if (rc == BSX_OK) {
		pthread_mutex_lock(&q->mu);
		counts_add(&q->tot.dev, &t->dev);
		for (i = 0; i <= BSX_QC_N_MAPQ; ++i) q->tot.mapq[i] += t->mapq[i];
		for (i = 0; i <= BSX_QC_ISIZE; ++i) q->tot.isize[i] += t->isize[i];
		for (i = 0; i < 16; ++i) q->tot.strandcnt[i] += t->strandcnt[i];
		q->tot.n_isize += t->n_isize; q->tot.all_tot += t->all_tot; q->tot.q40_tot += t->q40_tot; q->tot.all_dup += t->all_dup; q->tot.q40_dup += t->q40_dup;
		if (nj && be->qc_batch) { /* this backend's table has counts of ours now */
			for (i = 0; i < q->n_be; ++i) if (q->be[i].ctx == be->ctx && q->be[i].fn == be->qc_batch) break;
			if (i == q->n_be && q->n_be < BSX_QC_MAX_BE) { q->be[i].fn = be->qc_batch; q->be[i].ctx = be->ctx; ++q->n_be; }
			else if (i == q->n_be) rc = BSX_E_INTERNAL;
		}
		pthread_mutex_unlock(&q->mu);
	}
	free(t); free(jobs); free(pool);
	return rc;
}

int bsx_qc_collect(bsx_qc_state_t *q)
{
	bsx_qc_counts_t *c = (bsx_qc_counts_t*)malloc(sizeof(*c));
	int i, rc = BSX_OK;
	pthread_mutex_lock(&q->mu);
	for (i = 0; i < q->n_be; ++i) {
		int r = q->be[i].fn(q->be[i].ctx, 0, 0, 0, 0, c, 1);
		if (r == BSX_OK) counts_add(&q->tot.dev, c);
		else rc = r;
	}
	q->n_be = 0;
	pthread_mutex_unlock(&q->mu);
	free(c);
	return rc;
}

/* ------------------------------------------------------------------ the files (src/qc.c:29-110) */
static FILE *qc_open(const char *prefix, const char *suffix)
{
	size_t l = strlen(prefix) + strlen(suffix) + 1;
	char *fn = (char*)malloc(l);
	FILE *f;
	snprintf(fn, l, "%s%s", prefix, suffix);
	f = fopen(fn, "w");
	if (!f) fprintf(stderr, "[E::%s] cannot write %s\n", "bsx_qc_write", fn);
	free(fn);
	return f;
}
static void readpos_report(FILE *f, const uint64_t counts[2][BSX_QC_READ_LEN][2], const char *type)
{
	int i, j, k;
	fprintf(f, "BISCUITqc %s Retention by Read Position Table\n", type);
	fprintf(f, "ReadInPair\tPosition\tConversion/Retention\tCount\n");
	for (i = 0; i < 2; ++i) for (j = 0; j < BSX_QC_READ_LEN; ++j) for (k = 0; k < 2; ++k)
		if (counts[i][j][k] > 0) fprintf(f, "%d\t%d\t%c\t%llu\n", i + 1, j, k ? 'R' : 'C', (unsigned long long)counts[i][j][k]);
}
BSX_API int bsx_qc_write(const char *prefix, const bsx_qc_totals_t *t, int paired)
{
	FILE *f;
	int i, bad = 0;
	if (!prefix || !t) return BSX_E_ARG;
	if (!(f = qc_open(prefix, "_mapq_table.txt"))) return BSX_E_IO;
	fprintf(f, "BISCUITqc Mapping Quality Table\nMapQ\tCount\n");
	fprintf(f, "unmapped\t%llu\n", (unsigned long long)t->mapq[BSX_QC_N_MAPQ]);
	for (i = 0; i < BSX_QC_N_MAPQ; ++i) fprintf(f, "%d\t%llu\n", i, (unsigned long long)t->mapq[i]);
	bad |= fclose(f) != 0;
	if (!(f = qc_open(prefix, "_dup_report.txt"))) return BSX_E_IO;
	fprintf(f, "BISCUITqc Read Duplication Table\n");
	fprintf(f, "Number of duplicate reads:\t%llu\n", (unsigned long long)t->all_dup);
	fprintf(f, "Number of reads:\t%llu\n", (unsigned long long)t->all_tot);
	fprintf(f, "Number of duplicate q40-reads:\t%llu\n", (unsigned long long)t->q40_dup);
	fprintf(f, "Number of q40-reads:\t%llu\n", (unsigned long long)t->q40_tot);
	bad |= fclose(f) != 0;
	if (!(f = qc_open(prefix, "_strand_table.txt"))) return BSX_E_IO;
	fprintf(f, "BISCUITqc Strand Table");
	fprintf(f, "\nStrand Distribution:\n");
	fprintf(f, "strand\\BS      BSW (f)      BSC (r)\n");
	for (i = 0; i < 4; ++i) { /* (a newline after every value: the tool's own layout) */
		static const char *row[4] = {"     R1 (f):   ", "     R1 (r):   ", "     R2 (f):   ", "     R2 (r):   "};
		fprintf(f, "%s%-13lld\n%-13lld\n", row[i], (long long)t->strandcnt[4 * i], (long long)t->strandcnt[4 * i + 1]);
	}
	bad |= fclose(f) != 0;
	if (!(f = qc_open(prefix, "_totalReadConversionRate.txt"))) return BSX_E_IO;
	fprintf(f, "BISCUITqc Conversion Rate by Read Average Table\nCpA\tCpC\tCpG\tCpT\n");
	for (i = 0; i < 4; ++i) { /* (retained over retained + converted; 0 / 0 prints as the C library prints it, as in the tool) */
		if (i) fprintf(f, "\t");
		fprintf(f, "%.8lf", (double)t->dev.conv[2 * i] / (t->dev.conv[2 * i] + t->dev.conv[2 * i + 1]));
	}
	fprintf(f, "\n");
	bad |= fclose(f) != 0;
	if (!(f = qc_open(prefix, "_CpGRetentionByReadPos.txt"))) return BSX_E_IO;
	readpos_report(f, t->dev.readpos[0], "CpG");
	bad |= fclose(f) != 0;
	if (!(f = qc_open(prefix, "_CpHRetentionByReadPos.txt"))) return BSX_E_IO;
	readpos_report(f, t->dev.readpos[1], "CpH");
	bad |= fclose(f) != 0;
	if (paired) {
		if (!(f = qc_open(prefix, "_isize_table.txt"))) return BSX_E_IO;
		fprintf(f, "BISCUITqc Insert Size Table\nInsertSize\tFraction\tReadCount\n");
		for (i = 0; i <= BSX_QC_ISIZE; ++i)
			if (t->isize[i] > 0) fprintf(f, "%d\t%.8lf\t%llu\n", i, t->isize[i] / (double)t->n_isize, (unsigned long long)t->isize[i]);
		bad |= fclose(f) != 0;
	}
	return bad ? BSX_E_IO : BSX_OK;
}
