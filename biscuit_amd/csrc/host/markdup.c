/* markdup.c -- duplicate templates marked while aligning (--markdup; include/bsx.h has the rule).  emit_sam (pipeline.c) builds a key per
 * template from the finished primary records of its ends and hands a slice's keys over here; the batches of a stream reach the table in
 * input order (a ticket per slice), so that "the first in input order stays unmarked" holds whatever the threads do.  The table itself is
 * the backend's (k_markdup.hip); for a backend without markdup_batch -- the CPU checker's -- bsx_md_table_batch keeps the same table, with
 * the same claim words and salts, on the host. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "markdup.h"
#include "markdup_hash.h"
#include "tune.h"

#define MD_NONE (~(uint64_t)0)
#define MD_MAX_SALTS 8

BSX_API uint64_t bsx_markdup_hash(const bsx_markdup_key_t *key, uint32_t salt, int bits) { return key ? bsx_md_hash(key->w[0], key->w[1], salt, bits) : 0; }

/* ------------------------------------------------------------------ the key */
uint64_t bsx_md_end_key(int rid, int64_t pos, int is_rev, int yd_r, int n_cigar, const uint32_t *cigar)
{
	int64_t u5 = pos + 1;   /* POS */
	int k;
	if (!is_rev) {
		for (k = 0; k < n_cigar && (cigar[k] & 0xf) >= 3; ++k) u5 -= (int64_t)(cigar[k] >> 4);   /* leading S and H */
	} else {
		for (k = 0; k < n_cigar; ++k) { const int op = (int)(cigar[k] & 0xf); if (op == 0 || op == 2) u5 += (int64_t)(cigar[k] >> 4); }
		u5 -= 1;
		for (k = n_cigar - 1; k >= 0 && (cigar[k] & 0xf) >= 3; --k) u5 += (int64_t)(cigar[k] >> 4);   /* trailing S and H */
	}
	return BSX_MD_END(rid, u5, is_rev, yd_r);
}

/* ------------------------------------------------------------------ the host's table */
void bsx_md_table_free(bsx_md_table_t *t) { free(t->slot); memset(t, 0, sizeof(*t)); }

static bsx_md_slot_t *table_new(uint64_t n_slots)
{
	bsx_md_slot_t *s = (bsx_md_slot_t*)malloc(sizeof(*s) * n_slots);
	uint64_t i;
	if (!s) { fprintf(stderr, "[E::markdup] no room for a table of %llu slots (%llu bytes)\n", (unsigned long long)n_slots, (unsigned long long)(n_slots * sizeof(*s))); return 0; }
	for (i = 0; i < n_slots; ++i) { s[i].claim = 0; s[i].ord = s[i].k0 = s[i].k1 = MD_NONE; }
	return s;
}
/* the slot of claim word h: the first on its probe sequence that is empty or holds h */
static bsx_md_slot_t *table_find(bsx_md_slot_t *slot, uint64_t n_slots, uint64_t h)
{
	uint64_t s = bsx_md_start(h, n_slots), p;
	for (p = 0; p < n_slots; ++p, s = (s + 1) & (n_slots - 1))
		if (slot[s].claim == 0 || slot[s].claim == h) return &slot[s];
	return 0;
}
static int table_room(bsx_md_table_t *t, uint64_t more)
{
	uint64_t want = t->n_slots, i;
	bsx_md_slot_t *s;
	if (!t->slot) {
		const long v = bsx_tune_long("markdup_slots", 0);
		want = v > 0 ? (uint64_t)v : 65536;
		while (want & (want - 1)) want += want & (~want + 1);
		if (want < 2) want = 2;
		t->bits = (int)bsx_tune_long("markdup_hash_bits", 64);
	}
	while ((t->n_used + more) * 2 > want) want *= 2;
	if (t->slot && want == t->n_slots) return BSX_OK;
	if (!(s = table_new(want))) return BSX_E_NOMEM;
	for (i = 0; i < t->n_slots; ++i)
		if (t->slot[i].claim) *table_find(s, want, t->slot[i].claim) = t->slot[i];   /* claim words are unique: an empty slot */
	free(t->slot);
	t->slot = s; t->n_slots = want;
	return BSX_OK;
}
int bsx_md_table_batch(bsx_md_table_t *t, int64_t n, const bsx_markdup_key_t *keys, uint64_t first_ordinal, uint8_t *dup_out)
{
	int64_t i;
	int rc;
	for (i = 0; i < n; ++i) {
		const uint64_t k0 = keys[i].w[0], k1 = keys[i].w[1];
		uint32_t salt;
		dup_out[i] = 0;
		if (k0 == MD_NONE && k1 == MD_NONE) continue;
		if ((rc = table_room(t, 1)) != BSX_OK) return rc;
		for (salt = 0; salt < MD_MAX_SALTS; ++salt) {
			const uint64_t h = bsx_md_hash(k0, k1, salt, t->bits);
			bsx_md_slot_t *s = table_find(t->slot, t->n_slots, h);
			if (!s) return BSX_E_INTERNAL;
			if (s->claim == 0) { s->claim = h; s->ord = first_ordinal + (uint64_t)i; s->k0 = k0; s->k1 = k1; ++t->n_used; break; }
			if (s->k0 == k0 && s->k1 == k1) { dup_out[i] = s->ord != first_ordinal + (uint64_t)i; break; }
		}
		if (salt == MD_MAX_SALTS) { fprintf(stderr, "[E::markdup] a key met other keys with its claim word at %d salts\n", MD_MAX_SALTS); return BSX_E_INTERNAL; }
	}
	return BSX_OK;
}

/* ------------------------------------------------------------------ state, tickets */
void bsx_md_state_set(bsx_md_state_t *q, int on)
{
	if (!q->inited) { pthread_mutex_init(&q->mu, 0); pthread_cond_init(&q->cv, 0); q->inited = 1; }
	pthread_mutex_lock(&q->mu);
	bsx_md_table_free(&q->host);
	memset(&q->tot, 0, sizeof(q->tot));
	q->next_ordinal = 0; q->next_seq = 0; q->turn_seq = 0; q->turn_slice = 0; q->failed = 0;
	q->on = on ? 1 : 0;
	pthread_mutex_unlock(&q->mu);
}

void bsx_md_state_end(bsx_md_state_t *q)
{
	bsx_md_table_free(&q->host);
	if (q->inited) { pthread_mutex_destroy(&q->mu); pthread_cond_destroy(&q->cv); q->inited = 0; }
	q->on = 0;
}

void bsx_md_chunk_begin(bsx_md_state_t *q, int n_units, int64_t *seq, uint64_t *first_ordinal)
{
	pthread_mutex_lock(&q->mu);
	*seq = q->next_seq++;
	*first_ordinal = q->next_ordinal;
	q->next_ordinal += (uint64_t)n_units;
	pthread_mutex_unlock(&q->mu);
}

static int turn_wait(bsx_md_state_t *q, int64_t seq, int slice)   /* returns with q->mu held */
{
	pthread_mutex_lock(&q->mu);
	while (!q->failed && (q->turn_seq != seq || q->turn_slice != slice)) pthread_cond_wait(&q->cv, &q->mu);
	return q->failed ? BSX_E_INTERNAL : BSX_OK;
}
static void turn_pass(bsx_md_state_t *q, int slice, int n_slices)   /* with q->mu held; releases it */
{
	if (slice + 1 >= n_slices) { ++q->turn_seq; q->turn_slice = 0; }
	else ++q->turn_slice;
	pthread_cond_broadcast(&q->cv);
	pthread_mutex_unlock(&q->mu);
}

int bsx_md_slice(bsx_md_state_t *q, const bsx_backend_t *be, int64_t seq, int slice, int n_slices, int64_t n, const bsx_markdup_key_t *keys,
                 uint64_t first_ordinal, uint8_t *dup_out)
{
	int rc = turn_wait(q, seq, slice);
	int64_t i;
	if (rc != BSX_OK) { pthread_mutex_unlock(&q->mu); return rc; }
	/* the batch runs inside the turn (the next slice's keys must find this slice's in the table), but not under the lock */
	pthread_mutex_unlock(&q->mu);
	rc = be->markdup_batch ? be->markdup_batch(be->ctx, n, keys, first_ordinal, dup_out) : bsx_md_table_batch(&q->host, n, keys, first_ordinal, dup_out);
	pthread_mutex_lock(&q->mu);
	if (rc == BSX_OK) {
		q->tot.n_templates += (uint64_t)n;
		for (i = 0; i < n; ++i) { q->tot.n_keyed += !(keys[i].w[0] == MD_NONE && keys[i].w[1] == MD_NONE); q->tot.n_dup += dup_out[i]; }
	} else q->failed = 1;
	turn_pass(q, slice, n_slices);
	return rc;
}

void bsx_md_slice_skip(bsx_md_state_t *q, int64_t seq, int slice, int n_slices)
{
	if (turn_wait(q, seq, slice) != BSX_OK) { pthread_mutex_unlock(&q->mu); return; }
	turn_pass(q, slice, n_slices);
}

void bsx_md_fail(bsx_md_state_t *q)
{
	pthread_mutex_lock(&q->mu);
	q->failed = 1;
	pthread_cond_broadcast(&q->cv);
	pthread_mutex_unlock(&q->mu);
}
