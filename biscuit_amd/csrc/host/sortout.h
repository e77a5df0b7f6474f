/* sortout.h -- coordinate-sorted SAM while aligning (--sort): the host side.  include/bsx.h has the public bsx_sorter_* calls and the rule. */
#ifndef BSX_SORTOUT_H
#define BSX_SORTOUT_H
#include "bsx_core.h"

/* bsx_sorter_open over an arbitrary backend: be == NULL or be->sort_batch == NULL: the host's own stable merge sort (bsx_sort_host_perm), the
 * same permutation and schedule.  The backend is copied. */
BSX_API int bsx_sorter_open_backend(const bsx_backend_t *be, const char *header, const char *tmp_dir, bsx_sorter_t **out);
/* perm[i] = index of the i-th key in stable order; tmp: n words of scratch */
BSX_API void bsx_sort_host_perm(int64_t n, const uint64_t *keys, uint32_t *perm, uint32_t *tmp);
/* one record's key (fields 2 to 4 of the line) under the sorter's name -> rank table */
BSX_API uint64_t bsx_sorter_key(const bsx_sorter_t *s, const char *line, size_t len);

#endif
