/* The CIGAR walk of the output passes' job checks (biscuit_amd/csrc/hip/job_check.h) on the CPU, under AddressSanitizer and
 * UndefinedBehaviorSanitizer (tests/test_job_check_host.py builds and runs this).  The pools are heap blocks of exactly their length, so a
 * word read past the end is reported.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "job_check.h"

#define W(len, op) ((uint32_t)(len) << 4 | (uint32_t)(op))
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main(void)
{
	enum { N = 12 };
	/*                      0: M I D S H of one CIGAR        5: an op too many   7: the pool's last five words  */
	const uint32_t words[N] = {W(100, 0), W(3, 1), W(7, 2), W(20, 3), W(5, 4), W(9, 5), W(1, 0), W(11, 4), W(40, 0), W(2, 2), W(8, 0), W(6, 3)};
	uint32_t *pool = (uint32_t*)malloc(N * 4);
	uint64_t all = 99, ref = 99;
	CHECK(pool);
	memcpy(pool, words, N * 4);

	/* an empty CIGAR at the pool's end (and one of an empty pool that does not exist) */
	CHECK(job_cigar_spans(pool, N, N, 0, &all, &ref) == JOB_CIGAR_OK && all == 0 && ref == 0);
	all = ref = 99;
	CHECK(job_cigar_spans(NULL, 0, 0, 0, &all, &ref) == JOB_CIGAR_OK && all == 0 && ref == 0);
	/* ends exactly at the pool's end: H M D M S = 11 + 40 + 2 + 8 + 6, on the reference 40 + 2 + 8 */
	CHECK(job_cigar_spans(pool, N, 7, 5, &all, &ref) == JOB_CIGAR_OK && all == 67 && ref == 50);
	/* one word past the end; a start past the end with no word at all */
	CHECK(job_cigar_spans(pool, N, 7, 6, &all, &ref) == JOB_CIGAR_OUTSIDE);
	CHECK(job_cigar_spans(pool, N, N + 1, 0, &all, &ref) == JOB_CIGAR_OUTSIDE);
	/* cig_off + n_cigar wraps 32 bits: to 3, to 0, to N */
	CHECK(job_cigar_spans(pool, N, 4, 0xffffffffu, &all, &ref) == JOB_CIGAR_OUTSIDE);
	CHECK(job_cigar_spans(pool, N, 0xffffffffu, 1, &all, &ref) == JOB_CIGAR_OUTSIDE);
	CHECK(job_cigar_spans(pool, N, 0xfffffff0u, 16 + N, &all, &ref) == JOB_CIGAR_OUTSIDE);
	/* op 4 is the last one accepted; op 5 is refused wherever it stands in the CIGAR */
	CHECK(job_cigar_spans(pool, N, 4, 1, &all, &ref) == JOB_CIGAR_OK && all == 5 && ref == 0);
	CHECK(job_cigar_spans(pool, N, 5, 1, &all, &ref) == JOB_CIGAR_BAD_OP);
	CHECK(job_cigar_spans(pool, N, 3, 4, &all, &ref) == JOB_CIGAR_BAD_OP);
	pool[5] = W(9, 15);
	CHECK(job_cigar_spans(pool, N, 5, 1, &all, &ref) == JOB_CIGAR_BAD_OP);
	/* M I D S H: every length 100 + 3 + 7 + 20 + 5, on the reference M + D */
	CHECK(job_cigar_spans(pool, N, 0, 5, &all, &ref) == JOB_CIGAR_OK && all == 135 && ref == 107);
	free(pool);

	/* lengths that add up to more than 2^32: a length has 28 bits, so that takes 17 words and a pool of its own */
	{
		enum { M = 17 };
		const uint32_t top = (1u << 28) - 1;
		uint32_t *big = (uint32_t*)malloc(M * 4);
		CHECK(big);
		for (int i = 0; i < M; ++i) big[i] = W(top, i == 0 ? 1 : (i & 1) ? 0 : 2);   /* I, then M and D in turn */
		CHECK(job_cigar_spans(big, M, 0, M, &all, &ref) == JOB_CIGAR_OK);
		CHECK(all == (uint64_t)M * top && all > (uint64_t)1 << 32 && ref == (uint64_t)(M - 1) * top);
		free(big);
	}
	printf("ok\n");
	return 0;
}
