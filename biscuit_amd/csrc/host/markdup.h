/* markdup.h -- duplicate templates marked while aligning (markdup.c): state of a stream or of the process, a template's key from its finished
 * primary records, the ordered hand-over of a slice's keys to the backend's table, and the host's own table for a backend without one */
#ifndef BSX_MARKDUP_H
#define BSX_MARKDUP_H

#include <pthread.h>
#include "bsx_core.h"

typedef struct { uint64_t claim, ord, k0, k1; } bsx_md_slot_t;   /* as k_markdup.hip's: claim 0 = empty */
typedef struct {
	bsx_md_slot_t *slot;
	uint64_t n_slots, n_used;   /* n_slots: a power of two; the load stays at one half or less */
	int bits;                   /* low bits kept of the claim word (64: all) */
} bsx_md_table_t;

typedef struct {
	int on;
	int inited;                 /* mu and cv exist (made once, by the static initialiser or by the first bsx_md_state_set; gone after bsx_md_state_end) */
	pthread_mutex_t mu;
	pthread_cond_t cv;
	bsx_markdup_totals_t tot;
	uint64_t next_ordinal;      /* templates of the chunks pushed so far */
	int64_t next_seq;           /* chunks pushed so far */
	int64_t turn_seq; int turn_slice;   /* the batch that is submitted next: slice turn_slice of chunk turn_seq */
	int failed;                 /* a chunk gave up before all its batches: nobody waits any more */
	bsx_md_table_t host;        /* the table of a backend without markdup_batch */
} bsx_md_state_t;
#define BSX_MD_STATE_INIT {0, 1, PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, {0, 0, 0}, 0, 0, 0, 0, 0, {0, 0, 0, 0}}

/* on / off with ordinals, totals and the host table from zero; q is either BSX_MD_STATE_INIT or all zero before its first call */
void bsx_md_state_set(bsx_md_state_t *q, int on);
void bsx_md_state_end(bsx_md_state_t *q);   /* before q's memory goes away */
/* a chunk of n_units templates is pushed: its sequence number and the ordinal of its first template */
void bsx_md_chunk_begin(bsx_md_state_t *q, int n_units, int64_t *seq, uint64_t *first_ordinal);
/* the keys of slice `slice` (of n_slices) of chunk `seq`: waits until every earlier slice's batch has been submitted, submits this one (the
 * backend's markdup_batch, else the host table), lets the next one go, adds to the totals */
int  bsx_md_slice(bsx_md_state_t *q, const bsx_backend_t *be, int64_t seq, int slice, int n_slices, int64_t n, const bsx_markdup_key_t *keys,
                  uint64_t first_ordinal, uint8_t *dup_out);
/* the slice ended without a batch (an error on its way): the next one may go */
void bsx_md_slice_skip(bsx_md_state_t *q, int64_t seq, int slice, int n_slices);
void bsx_md_fail(bsx_md_state_t *q);

/* one end's word of the key (include/bsx.h): pos = 0-based leftmost reference position of the record, cigar = its final operations, S and H
 * included, in reference order (len << 4 | op, op 0..4 = MIDSH) */
uint64_t bsx_md_end_key(int rid, int64_t pos, int is_rev, int yd_r, int n_cigar, const uint32_t *cigar);

/* the rule over a table on the host, one key after the other */
void bsx_md_table_free(bsx_md_table_t *t);
int  bsx_md_table_batch(bsx_md_table_t *t, int64_t n, const bsx_markdup_key_t *keys, uint64_t first_ordinal, uint8_t *dup_out);

#endif
