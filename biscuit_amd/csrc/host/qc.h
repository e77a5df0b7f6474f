/* qc.h -- the BISCUITqc tables while aligning (qc.c): state of a stream or of the process, the per-slice hand-over, the files */
#ifndef BSX_QC_H
#define BSX_QC_H

#include <pthread.h>
#include "pipeline.h"
#include "cov.h"
#include "meth.h"

#define BSX_QC_MAX_BE 48
typedef struct {
	int on;
	pthread_mutex_t mu;
	bsx_qc_totals_t tot;   /* record fields, host-walked columns, and what has been collected from the backends' tables */
	/* backends whose table holds counts of this state that have not been collected yet (a device's lanes share one table) */
	struct { int (*fn)(void*, int64_t, const bsx_qc_job_t*, const uint32_t*, size_t, bsx_qc_counts_t*, int); void *ctx; } be[BSX_QC_MAX_BE];
	int n_be;
	bsx_cov_state_t cov;   /* the coverage tables over the same records (cov.c): off unless set after this state was set on */
	bsx_meth_state_t meth; /* the base-averaged conversion table over the same records (meth.c): likewise */
} bsx_qc_state_t;

void bsx_qc_state_set(bsx_qc_state_t *q, int on);
/* the records the final pass noted for one slice's units (ctx[u].qc_recs, .qc_cig): record fields counted here, one batch of jobs to the
 * backend (or, without qc_batch, walked here) */
int  bsx_qc_slice(bsx_qc_state_t *q, const bsx_backend_t *be, const bsx_index_t *idx, const uint8_t *reads, size_t reads_len,
                  const samctx_t *ctx, size_t n_units);
/* read (and zero) the backends' tables into the totals; the backends must still be open */
int  bsx_qc_collect(bsx_qc_state_t *q);
/* one record's columns on the host: what k_qc.hip does for a job */
void bsx_qc_walk_host(const bsx_index_t *idx, const uint8_t *reads, size_t reads_len, const bsx_qc_job_t *j, const uint32_t *cig, bsx_qc_counts_t *acc);

#endif
