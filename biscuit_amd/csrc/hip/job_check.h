/* job_check.h -- what the output passes' batches (shim_tables.hip) check of a job's CIGAR before a kernel indexes with it.  Plain C, no HIP:
 * tests/job_check_host_main.c runs it on the CPU. */
#ifndef BSX_JOB_CHECK_H
#define BSX_JOB_CHECK_H
#include <stddef.h>
#include <stdint.h>

enum { JOB_CIGAR_OK = 0, JOB_CIGAR_OUTSIDE = 1, JOB_CIGAR_BAD_OP = 2 };

/* The n_cigar words (len << 4 | op) at cig_off of a pool of pool_len words.  Refused: a range that is not inside the pool (nothing is read
 * then), an op above 4 (MIDSH are 0..4).  Otherwise *all = the sum of every length, *ref = that of the ops that advance on the reference
 * (M and D); both are 0 for an empty CIGAR, and neither means anything after a refusal.  What a sum may be at most is the caller's condition. */
static inline int job_cigar_spans(const uint32_t *pool, size_t pool_len, uint32_t cig_off, uint32_t n_cigar, uint64_t *all, uint64_t *ref)
{
	*all = *ref = 0;
	if ((uint64_t)cig_off + n_cigar > pool_len) return JOB_CIGAR_OUTSIDE;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t c = pool[(size_t)cig_off + k], op = c & 0xf;
		if (op > 4) return JOB_CIGAR_BAD_OP;
		*all += c >> 4;
		if (op == 0 || op == 2) *ref += c >> 4;
	}
	return JOB_CIGAR_OK;
}
#endif
