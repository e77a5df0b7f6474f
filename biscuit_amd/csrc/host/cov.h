/* cov.h -- the BISCUITqc coverage tables while aligning (cov.c): state of a stream or of the process (part of its QC state), the per-slice
 * hand-over, the depth rule on the host for a backend without the seam, the BED reader, the files */
#ifndef BSX_COV_H
#define BSX_COV_H

#include <pthread.h>
#include "bsx_core.h"

typedef struct {
	int on;
	pthread_mutex_t mu;
	int64_t n_iv[2]; int64_t *iv[2]; int have_iv[2];   /* the masks as they were set (forward intervals), handed to the backend it attaches to */
	/* the backend whose depth state holds this state's records: the first one seen (the lanes of a device share one state), emptied then */
	int attached;
	int (*fn)(void*, int, int64_t, const bsx_qc_job_t*, const uint32_t*, size_t, const int64_t*, bsx_cov_tables_t*); void *ctx;
	/* without the seam: the state here -- (l_pac + 1) x 2 differences, as on the device */
	const bsx_index_t *idx;
	int32_t *diff;
} bsx_cov_state_t;

void bsx_cov_state_set(bsx_cov_state_t *c, int on);   /* (a zeroed struct is a valid `off` state with mu initialised by the caller) */
int  bsx_cov_state_mask(bsx_cov_state_t *c, int which, int64_t n, const int64_t *beg_end);
/* before a slice's records: the backend's state emptied and given the masks when it is the first one this state sees */
int  bsx_cov_attach(bsx_cov_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx);
/* the jobs of one slice (those with BSX_QC_COV count) */
int  bsx_cov_slice(bsx_cov_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *pool, size_t pool_len);
int  bsx_cov_state_tables(bsx_cov_state_t *c, bsx_cov_tables_t *out);

/* the depth rule on plain arrays (what k_cov.hip does on the device): diff = (l_pac + 1) x 2 ints, masks = bit arrays of (l_pac + 63) / 32 words or NULL */
int  bsx_cov_host_add(const bsx_index_t *idx, int32_t *diff, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *pool, size_t pool_len);
int  bsx_cov_host_paint(const bsx_index_t *idx, uint32_t *mask, int64_t n, const int64_t *beg_end);
int  bsx_cov_host_tables(const bsx_index_t *idx, const int32_t *diff, const uint32_t *m_top, const uint32_t *m_bot, bsx_cov_tables_t *out);

#endif
