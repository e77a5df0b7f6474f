// k_markdup.hip -- duplicate templates found while aligning (--markdup): an open-addressing table of template keys that stays in HBM for the
// life of the device.  include/bsx.h (bsx_markdup_key_t, bsx_markdup_batch) has the rule and the key; this file has the table.
//
// A slot is 32 bytes: a 64-bit claim word (0: empty, else bsx_md_hash of the key that took it), the lowest ordinal seen for it, and the 128-bit
// key (all ones until published).  A batch is three launches, a lane per key, one after the other on the same stream:
//   k_md_claim    probes linearly from bsx_md_start(h): an empty slot is taken with one 64-bit compare-and-swap per slot visited, a slot whose
//                 claim word is h already is shared; then an atomic min of the lane's ordinal into the slot.  A compare-and-swap that loses
//                 moves on to the next slot or stops: no lane ever waits for another (the lanes of a wave run in lockstep; a spin on a slot a
//                 neighbour owns would never end).
//   k_md_publish  the one lane whose ordinal the slot now holds writes the key into a slot that has none yet.
//   k_md_decide   a lane whose key is the slot's is a duplicate unless the slot's ordinal is its own; a lane whose key is not (two keys, one
//                 64-bit claim word) stays unresolved and goes through the three launches again with the next salt.
// Keys are compared in full, so two different keys never merge; the lowest ordinal wins a slot however the lanes interleave, so the flags
// do not depend on scheduling.  Kernel boundaries order the phases: no fences, no flags.  k_md_rehash moves every slot into a larger table
// by its stored claim word (claim words are unique within a table, so every lane takes an empty slot).
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "kernels.h"
extern "C" {
#include "markdup_hash.h"
}

static_assert(sizeof(MdSlot) == 32, "MdSlot");
static_assert(sizeof(bsx_markdup_key_t) == 16, "bsx_markdup_key_t");
#define MD_NONE (~0ull)

__global__ void __launch_bounds__(256) k_md_init(MdSlot *T, unsigned long long n_slots)
{
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_slots) { MdSlot s; s.claim = 0; s.ord = MD_NONE; s.k0 = MD_NONE; s.k1 = MD_NONE; T[i] = s; }
}

// adds the number of lanes of the wave with `flag` set to *ctr: one atomic per wave (called by every lane of the wave)
__device__ __forceinline__ void md_count(bool flag, unsigned long long *ctr)
{
	const unsigned long long m = __ballot(flag);
	if (m && wave_lane() == __ffsll((long long)m) - 1) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256)
k_md_claim(MdSlot *T, unsigned long long n_slots, const bsx_markdup_key_t *keys, long long n, unsigned long long first, unsigned salt, int bits,
           uint8_t *res, unsigned long long *slot, unsigned long long *ctr)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	bool took = false;
	if (i < n && res[i] == MD_RES_OPEN) {
		const unsigned long long k0 = keys[i].w[0], k1 = keys[i].w[1];
		if (k0 == MD_NONE && k1 == MD_NONE) res[i] = MD_RES_SKIP;
		else {
			const unsigned long long h = bsx_md_hash(k0, k1, salt, bits), mask = n_slots - 1;
			unsigned long long s = bsx_md_start(h, n_slots), p;
			for (p = 0; p < n_slots; ++p, s = (s + 1) & mask) {
				const unsigned long long old = atomicCAS(&T[s].claim, 0ull, h);
				if (old == 0) { took = true; break; }
				if (old == h) break;
			}
			if (p == n_slots) res[i] = MD_RES_FULL;   // (the host keeps the load at one half or less: not reached)
			else {
				// the key words change only in k_md_publish: a slot published by an earlier batch or round that holds another key is not ours to lower
				const unsigned long long s0 = T[s].k0, s1 = T[s].k1;
				if ((s0 == MD_NONE && s1 == MD_NONE) || (s0 == k0 && s1 == k1)) atomicMin(&T[s].ord, first + (unsigned long long)i);
				slot[i] = s;
			}
		}
	}
	md_count(took, &ctr[0]);
}

__global__ void __launch_bounds__(256)
k_md_publish(MdSlot *T, const bsx_markdup_key_t *keys, long long n, unsigned long long first, const uint8_t *res, const unsigned long long *slot)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || res[i] != MD_RES_OPEN) return;
	MdSlot *S = &T[slot[i]];
	if (S->ord == first + (unsigned long long)i && S->k0 == MD_NONE && S->k1 == MD_NONE) { S->k0 = keys[i].w[0]; S->k1 = keys[i].w[1]; }
}

__global__ void __launch_bounds__(256)
k_md_decide(const MdSlot *T, const bsx_markdup_key_t *keys, long long n, unsigned long long first, uint8_t *res, const unsigned long long *slot,
            unsigned long long *ctr)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	bool open = false;
	if (i < n && res[i] == MD_RES_OPEN) {
		const MdSlot *S = &T[slot[i]];
		if (S->k0 == keys[i].w[0] && S->k1 == keys[i].w[1]) res[i] = S->ord != first + (unsigned long long)i ? MD_RES_DUP : MD_RES_FIRST;
		else open = true;   // another key has this claim word: the next salt
	}
	md_count(open, &ctr[1]);
}

__global__ void __launch_bounds__(256) k_md_rehash(const MdSlot *old, unsigned long long n_old, MdSlot *T, unsigned long long n_slots, unsigned long long *ctr)
{
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	bool lost = false;
	if (i < n_old && old[i].claim != 0) {
		const MdSlot o = old[i];
		const unsigned long long mask = n_slots - 1;
		unsigned long long s = bsx_md_start(o.claim, n_slots), p;
		for (p = 0; p < n_slots; ++p, s = (s + 1) & mask)
			if (atomicCAS(&T[s].claim, 0ull, o.claim) == 0) break;
		if (p == n_slots) lost = true;
		else { T[s].ord = o.ord; T[s].k0 = o.k0; T[s].k1 = o.k1; }
	}
	md_count(lost, &ctr[2]);
}

static inline unsigned md_grid(unsigned long long n) { return (unsigned)((n + 255) / 256); }

void launch_md_init(hipStream_t st, MdSlot *T, unsigned long long n_slots)
{
	hipLaunchKernelGGL(k_md_init, dim3(md_grid(n_slots)), dim3(256), 0, st, T, n_slots);
}
void launch_md_round(hipStream_t st, MdSlot *T, unsigned long long n_slots, const bsx_markdup_key_t *keys, long long n, unsigned long long first,
                     unsigned salt, int bits, uint8_t *res, unsigned long long *slot, unsigned long long *ctr)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(k_md_claim, dim3(md_grid((unsigned long long)n)), dim3(256), 0, st, T, n_slots, keys, n, first, salt, bits, res, slot, ctr);
	hipLaunchKernelGGL(k_md_publish, dim3(md_grid((unsigned long long)n)), dim3(256), 0, st, T, keys, n, first, res, slot);
	hipLaunchKernelGGL(k_md_decide, dim3(md_grid((unsigned long long)n)), dim3(256), 0, st, T, keys, n, first, res, slot, ctr);
}
void launch_md_rehash(hipStream_t st, const MdSlot *old, unsigned long long n_old, MdSlot *T, unsigned long long n_slots, unsigned long long *ctr)
{
	hipLaunchKernelGGL(k_md_rehash, dim3(md_grid(n_old)), dim3(256), 0, st, old, n_old, T, n_slots, ctr);
}
