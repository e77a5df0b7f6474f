/* extend.c -- C4: chains -> alignment regions, as a resumable per-task state machine.
 *
 * mem_chain2region / mem_chain2region1 (lib/aln/memchain.c:742-904) walk the seeds of every chain
 * best-first; whether a seed is extended depends on the regions produced so far by the same strand
 * search, so the work of one task is a strictly ordered sequence of ksw_extend2 calls (left then
 * right, each with up to MAX_BAND_TRY=2 band widths).  Across tasks there is no dependency.  The
 * pipeline therefore advances all tasks in lock-step rounds: every task that needs a DP call posts
 * ONE job, the whole round runs as one device batch (K4), and the results are fed back.
 */
#include "align_types.h"
#include "pipeline.h"

#include "c2r_rule.h"

#define MAX_BAND_TRY 2   /* memchain.c:611 */

/* asymmetric_flt_seed, memchain.c:138-149: reference T under a read C, or reference A under a read G */
static int seed_violates_conversion(const bsx_index_t *idx, const uint8_t *query, const seed_t *s)
{
	int i;
	for (i = 0; i < s->len; ++i) {
		int r = bsx_ref_base(idx->ref.l_pac, idx->pac, s->rbeg + i);
		int q = query[s->qbeg + i];
		if ((r == 3 && q == 1) || (r == 0 && q == 2)) return 1;
	}
	return 0;
}

static void c2r_open_list(c2r_t *t, const seed_v *seeds)
{
	size_t i;
	if (t->m_srt < (int)seeds->n) { bsx_cfree(t->srt); t->m_srt = (int)seeds->n + 8; t->srt = (uint64_t*)bsx_crealloc(0, 0, sizeof(uint64_t) * t->m_srt); }
	for (i = 0; i < seeds->n; ++i) t->srt[i] = (uint64_t)seeds->a[i].score << 32 | i;
	t->n_srt = (int)seeds->n;
	bsx_introsort_u64(seeds->n, t->srt);   /* ks_introsort_64, memchain.c:752 */
	t->k = t->n_srt - 1;
}

/* the job of side t->stage - 1 (0 left, 1 right) at band width opt->w << t->tryi */
static void c2r_post_job(const bsx_opt_t *opt, c2r_t *t, const seed_t *s)
{
	bsx_ext_job_t *j = &t->job;
	const c2r_job_t f = c2r_side_job(t->stage - 1, t->qoff, s->rbeg, s->qbeg, s->len, t->l_query, t->rmax[0], t->rmax[1], opt->a, t->sc0, opt->pen_clip5, opt->pen_clip3);
	memset(j, 0, sizeof(*j));
	j->qoff = f.qoff; j->qdir = (int8_t)f.qdir; j->qlen = f.qlen;
	j->tpos = f.tpos; j->tdir = (int8_t)f.tdir; j->tlen = f.tlen;
	j->h0 = f.h0; j->w = opt->w << t->tryi; j->end_bonus = f.end_bonus; j->parent = (uint8_t)t->parent;
	t->has_job = 1;
}

/* region complete: strand-boundary check, seed coverage, book-keeping (memchain.c:842-868) */
static void c2r_finish_region(const bsx_index_t *idx, c2r_t *t, const chain_t *c, const seed_v *seeds, const seed_t *s)
{
	reg_t *r = &t->cur;
	int64_t l_pac = idx->ref.l_pac;
	size_t i;
	r->bss = (uint8_t)c2r_bss(t->parent, l_pac, r->rb);
	r->parent = (uint8_t)t->parent;
	if (c2r_bss(t->parent, l_pac, r->re) == r->bss) {
		for (i = 0, r->seedcov = 0; i < seeds->n; ++i) {
			const seed_t *q = &seeds->a[i];
			if (c2r_covers(r->qb, r->qe, r->rb, r->re, q->rbeg, q->qbeg, q->len)) r->seedcov += q->len;
		}
		r->w = t->aw[0] > t->aw[1] ? t->aw[0] : t->aw[1];
		r->seedlen0 = s->len;
		r->frac_rep = c->frac_rep;
		bsx_cvec_push(t->regs, *r);
	}
	--t->k;
	t->stage = 0;
}

/* From side `side` on: a side that needs no extension is settled here, the first one that needs one posts its job (t->has_job); with
 * both sides settled the region is finished. */
static void c2r_begin_side(const bsx_opt_t *opt, const bsx_index_t *idx, c2r_t *t, const chain_t *c, const seed_v *seeds, const seed_t *s, int side)
{
	reg_t *r = &t->cur;
	for (; side < 2; ++side) {
		if (c2r_side_trivial(side, s->rbeg, s->qbeg, s->len, t->l_query, opt->a, &r->qb, &r->rb, &r->qe, &r->re, &r->score, &r->truesc)) continue;
		t->sc0 = r->score;
		t->tryi = 0;
		t->stage = side + 1;
		c2r_post_job(opt, t, s);
		return;
	}
	c2r_finish_region(idx, t, c, seeds, s);
}

/* Run the task until it posts a job (returns 1) or is finished (returns 0). */
int bsx_c2r_advance(const bsx_opt_t *opt, const bsx_index_t *idx, c2r_t *t)
{
	int64_t l_pac = idx->ref.l_pac;
	t->has_job = 0;
	if (t->done) return 0;
	for (;;) {
		chain_t *c;
		const seed_v *seeds;
		if (t->ci >= (int)t->chains.n) { t->done = 1; return 0; }
		c = &t->chains.a[t->ci];
		if (!t->chain_open) {
			if (c->seeds.n == 0) { ++t->ci; continue; }
			bsx_chain_ref_span(opt, t->l_query, l_pac, c, t->rmax);
			t->rid = bsx_fetch_span(&idx->ref, &t->rmax[0], c->seeds.a[0].rbeg, &t->rmax[1]);
			t->n0 = (int)t->regs.n;
			t->pass = 0;
			c2r_open_list(t, &c->seeds);
			t->chain_open = 1;
			t->stage = 0;
		}
		seeds = t->pass ? &c->seeds_extra : &c->seeds;
		if (t->stage != 0) return 0; /* a job is outstanding; nothing to do until its result arrives */
		while (t->k >= 0) {
			const seed_t *s = &seeds->a[(uint32_t)t->srt[t->k]];
			size_t u;
			if (seed_violates_conversion(idx, t->query, s)) { --t->k; continue; }
			/* is the seed inside a region this strand search already produced? (memchain.c:761-790) */
			for (u = 0; u < t->regs.n; ++u) {
				const reg_t *reg = &t->regs.a[u];
				int end;
				if (!c2r_in_box(s->rbeg, s->qbeg, s->len, t->l_query, reg->rb, reg->re, reg->qb, reg->qe, reg->seedlen0)) continue;
				for (end = 0; end < 2; ++end) {
					int64_t rd;
					int qd;
					c2r_end_dist(end, s->rbeg, s->qbeg, s->len, reg->rb, reg->re, reg->qb, reg->qe, &qd, &rd);
					if (c2r_near_diagonal(qd, rd, bsx_cal_max_gap(opt, c2r_gap_len(qd, rd)), reg->w)) break;
				}
				if (end < 2) break;
			}
			if (u < t->regs.n) { /* contained: extend anyway only if an overlapping long seed disagrees (memchain.c:794-819) */
				int i;
				for (i = t->k + 1; i < t->n_srt; ++i) {
					const seed_t *o;
					if (t->srt[i] == 0) continue;
					o = &seeds->a[(uint32_t)t->srt[i]];
					if (c2r_disagrees(s->rbeg, s->qbeg, s->len, o->rbeg, o->qbeg, o->len)) break;
				}
				if (i == t->n_srt) { t->srt[t->k] = 0; --t->k; continue; }
			}
			/* extend this seed (memchain.c:822-836) */
			memset(&t->cur, 0, sizeof(t->cur));
			t->cur.w = t->aw[0] = t->aw[1] = opt->w;
			t->cur.score = t->cur.truesc = -1;
			t->cur.rid = t->rid;
			c2r_begin_side(opt, idx, t, c, seeds, s, 0);   /* (a seed that spans the read is a region without a job) */
			if (t->has_job) return 1;
		}
		/* list exhausted: fall back to the contained seeds if the chain produced nothing (memchain.c:898-901) */
		if (t->pass == 0 && (int)t->regs.n == t->n0 && c->seeds_extra.n > 0) {
			t->pass = 1;
			c2r_open_list(t, &c->seeds_extra);
			continue;
		}
		++t->ci; t->chain_open = 0;
	}
}

/* Feed the result of the posted job back (left: memchain.c:641-671, right: memchain.c:700-729). */
void bsx_c2r_consume(const bsx_opt_t *opt, const bsx_index_t *idx, c2r_t *t, const bsx_ext_res_t *res)
{
	chain_t *c = &t->chains.a[t->ci];
	const seed_v *seeds = t->pass ? &c->seeds_extra : &c->seeds;
	const seed_t *s = &seeds->a[(uint32_t)t->srt[t->k]];
	reg_t *r = &t->cur;
	const int side = t->stage - 1, prev = r->score, aw = opt->w << t->tryi;
	t->has_job = 0;
	r->score = res->score;
	t->aw[side] = aw;
	if (c2r_band_again(r->score, prev, res->max_off, aw) && t->tryi + 1 < MAX_BAND_TRY) {
		++t->tryi; c2r_post_job(opt, t, s); return;
	}
	c2r_side_settle(side, r->score, res->qle, res->tle, res->gtle, res->gscore, t->job.end_bonus, t->sc0,
	                s->rbeg, s->qbeg, s->len, t->l_query, &r->qb, &r->rb, &r->qe, &r->re, &r->truesc);
	c2r_begin_side(opt, idx, t, c, seeds, s, side + 1);
}

void bsx_c2r_release(c2r_t *t)
{
	bsx_chain_free(&t->chains);
	bsx_cvec_free(t->chains);
	bsx_cfree(t->srt); t->srt = 0; t->m_srt = 0;
}
