/* markdup_hash.h -- the claim word of a duplicate-marking key: one definition for the device's table (k_markdup.hip) and the host's (markdup.c).
 * include/bsx.h (bsx_markdup_key_t) states it in words. */
#ifndef BSX_MARKDUP_HASH_H
#define BSX_MARKDUP_HASH_H

#include <stdint.h>

#ifdef __HIPCC__
#define BSX_MD_HD __host__ __device__ static inline
#else
#define BSX_MD_HD static inline
#endif

BSX_MD_HD uint64_t bsx_md_mix(uint64_t x)   /* the finalizer of splitmix64 */
{
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	x ^= x >> 31;
	return x;
}
/* never 0 (0 is the empty slot); bits < 64 keeps the low bits only (tests: keys that share a claim word) */
BSX_MD_HD uint64_t bsx_md_hash(uint64_t w0, uint64_t w1, uint32_t salt, int bits)
{
	uint64_t h = bsx_md_mix(bsx_md_mix(w0 ^ (uint64_t)salt * 0x9E3779B97F4A7C15ull) ^ w1);
	if (bits > 0 && bits < 64) h &= ((uint64_t)1 << bits) - 1;
	return h ? h : 1;
}
/* where the probe sequence of a claim word starts in a table of n_slots (a power of two) */
BSX_MD_HD uint64_t bsx_md_start(uint64_t h, uint64_t n_slots) { return bsx_md_mix(h) & (n_slots - 1); }

#endif
