/* meth.h -- BISCUITqc's base-averaged conversion table while aligning (meth.c): state of a stream or of the process (part of its QC state), the
 * per-slice hand-over, the counting rule, the table pass and the site list on the host for a backend without the seam, the files */
#ifndef BSX_METH_H
#define BSX_METH_H

#include <pthread.h>
#include "bsx_core.h"

typedef struct {
	int on;
	pthread_mutex_t mu;
	/* the backend whose counters hold this state's records: the first one seen (the lanes of a device share one state), emptied then */
	int attached;
	int (*fn)(void*, int, int64_t, const bsx_meth_job_t*, const uint32_t*, size_t, bsx_meth_tables_t*); void *ctx;
	int (*sites)(void*, const bsx_meth_site_opt_t*, int64_t, int64_t, bsx_meth_site_t*, int64_t, int64_t*, int64_t*);   /* the same backend's meth_sites */
	/* without the seam: the counters here -- l_pac x (ret, conv, opp_ref, opp_alt), as bsx_meth_read gives them */
	const bsx_index_t *idx;
	uint32_t *cnt;
} bsx_meth_state_t;

void bsx_meth_state_set(bsx_meth_state_t *c, int on);   /* (a zeroed struct is a valid `off` state with mu initialised by the caller) */
/* before a slice's records: the backend's counters emptied when it is the first one this state sees */
int  bsx_meth_attach(bsx_meth_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx);
/* the jobs of one slice; reads: the chunk's read buffer, as the backend has it */
int  bsx_meth_slice(bsx_meth_state_t *c, const bsx_backend_t *be, const bsx_index_t *idx, const uint8_t *reads, size_t reads_len, int64_t n,
                    const bsx_meth_job_t *jobs, const uint32_t *pool, size_t pool_len);
int  bsx_meth_state_tables(bsx_meth_state_t *c, bsx_meth_tables_t *out);

/* the rule on plain arrays (what k_meth.hip does on the device): cnt = l_pac x 4 counters.  Nothing is added unless every job is valid. */
int  bsx_meth_host_add(const bsx_index_t *idx, uint32_t *cnt, const uint8_t *reads, size_t reads_len, int64_t n, const bsx_meth_job_t *jobs,
                       const uint32_t *pool, size_t pool_len);
int  bsx_meth_host_tables(const bsx_index_t *idx, const uint32_t *cnt, bsx_meth_tables_t *out);
/* the methylation sites of the counters (--meth-bed; what k_msite.hip does on the device): bsx_meth_sites on plain arrays */
int  bsx_meth_host_sites(const bsx_index_t *idx, const uint32_t *cnt, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out,
                         int64_t cap, int64_t *n, int64_t *f_next);
int  bsx_meth_state_sites(bsx_meth_state_t *c, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n,
                          int64_t *f_next);

#endif
