// refn.hpp -- where the forward reference has no base: its N holes (DevIndex::hole_off / hole_end) and the contig ends, found by a whole wavefront
// (k_global.hip's counts by context, k_qc.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.hpp"

// is forward coordinate f inside one of the reference's N holes?  h0: the first hole that can matter (the ones before it end at or before the window)
__device__ __forceinline__ bool ctx_in_hole(const DevIndex &ix, int h0, int64_t f)
{
	for (int h = h0; h < ix.n_holes && ix.hole_off[h] <= f; ++h) if (f < ix.hole_end[h]) return true;
	return false;
}

// how many of the n sorted values a[] are <= key, found by the whole wave: 64 probes a step (two dependent loads for 4096 entries where a
// binary search by one lane makes twelve); every lane returns the same number
__device__ __forceinline__ int wave_count_le(const int64_t *a, int n, int64_t key, int lane)
{
	int lo = 0, hi = n;   // the answer lies in [lo, hi]
	while (hi > lo) {
		const int step = (hi - lo + 63) >> 6, idx = lo + lane * step;
		const bool le = idx < hi && a[idx] <= key;
		const int c = __popcll(__ballot(le));   // a[] is sorted: the lanes that say yes are the first c
		if (c == 0) hi = lo;
		else { const int nhi = lo + c * step; lo = lo + (c - 1) * step + 1; hi = nhi < hi ? nhi : hi; }
	}
	return lo;
}
