// rg_common.hpp -- what more than one of the region units reads (k_regions.hip: the chaining tiers; k_c2r.hip: chains -> regions;
// k_seedsw.hip: the seed filter of long reads; k_occ.hip: K3 ahead of the tiers): the capacities and the table types of a strand
// search, the per-wave scratch with its $BSX_PHASES sums, the contig look-ups, bwt_sa, the publishing of a task's regions and
// the launchers' argument lists.  Every function here is a template or __forceinline__: several units include this.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "kernels.h"

#define RG_QCAP 256
#define RG_NC 4          // extension rows live in registers: 64 * RG_NC entries >= qlen + 1

struct RgChain {         // mem_chain_t reduced to what chaining, the filter and the region loop read: first seed = (pos, first_q), last seed,
                         // and mem_chain_weight's two running sums (query and reference coverage) with their high-water marks
	long long pos, last_r;
	int rid, endr_off;                                        // endr_off: end of the reference coverage so far, relative to pos
	short first_q, last_q, last_len, wq, wr, endq, first, w;  // w = min(wq, wr) once chaining is over; first: mem_chain_flt's
	unsigned short n_seeds, seed0;                            // seeds on the main list (not seeds_extra), and the first of them
	signed char kept; unsigned char is_alt; unsigned short n_extra;   // n_extra: seeds on seeds_extra (contained in the chain on both axes)
};

// Working set of one strand search.  Two sizes: the common case lives in LDS; what does not fit there is
// redone by a second launch whose tables are a per-wave slab in HBM.
// B-tree node of the chain index (kbtree.h with t = 3: up to 5 keys); keys are chain ids, compared through their start positions
struct RgNode { unsigned char n, internal; unsigned short id[5], child[6]; };

// PCAP_ > 0 (the LDS tiers): only chains with more than one seed (or with contained seeds) have a record, at most PCAP_ of them; a chain
// of one seed IS that seed (every field of its record follows from it).  Against an hg38-sized genome a strand search has ~100 chains and
// all but a handful are such: the chain table was half of a wave's LDS, and LDS is what bounds these tiers' occupancy.
// Chain ids: with PCAP_ == 0 the record index; else < RG_REC the seed index of a one-seed chain, >= RG_REC record id - RG_REC.
#define RG_REC 0x4000
template <int ICAP_, int SCAP_, int CCAP_, int RCAP_, int NODES_, typename Idx, typename SIdx, int PCAP_ = 0>
struct RgStore {
	static constexpr int ICAP = ICAP_, SCAP = SCAP_, CCAP = CCAP_, RCAP = RCAP_, NODES = NODES_, PCAP = PCAP_;
	typedef Idx idx_t;
	// intervals (sorted by info): read until the last occurrence has been chained; the sort keys of the chains and of a chain's seeds
	// (srt) are first written after that, so the two share their bytes (2 KB of the 13.7 KB a wave of the larger LDS tier had: a
	// sixth workgroup per CU)
	union {
		struct { unsigned long long iv_x0[ICAP_]; int iv_n[ICAP_]; short iv_beg[ICAP_], iv_end[ICAP_];
		         unsigned long long iv_rank[NODES_ ? ICAP_ : 1]; };   // iv_n: count | more beyond << 29 | over-represented << 30; iv_rank (HBM tiers): first SA rank
		unsigned long long srt[SCAP_];    // score<<32|i, ascending (memchain.c:748-752)
	};
	// seeds in arrival order
	long long s_rbeg[SCAP_];
	int s_rid[SCAP_];
	short s_qbeg[SCAP_], s_len[SCAP_]; SIdx s_chain[SCAP_]; signed char s_extra[SCAP_];
	RgChain ch[PCAP_ ? PCAP_ : CCAP_];
	Idx ord[CCAP_];                   // chain indices: by position, then in filter order
	Idx keep[CCAP_];                  // mem_chain_flt's kept list (indices into ord)
	Idx lst[SCAP_];                   // seed indices of the current chain / list
	bsx_region_t regs[RCAP_ ? RCAP_ : 1];
	int n_chains, n_regs;
	int boost_iv;                     // status 10: the interval (sorted index) that has to be walked further
	// NODES > 0: chains are indexed by the reference's B-tree, so that chains starting at the same position are found
	// and ordered as kb_intervalp / __kb_traverse would (the first tier declines such tasks instead)
	RgNode node[NODES_ ? NODES_ : 1];
	int n_nodes, root;
};
typedef RgStore<64, 128, 128, 0, 0, unsigned short, short, 32> RgSmall;
typedef RgStore<128, 256, 256, 0, 0, unsigned short, short, 64> RgMid;             // still LDS: 24 KB per wave, two waves per workgroup: the
                                                                                // strand search of a read against an hg38-sized index (~50 intervals, ~125 seeds, ~100 chains)
// chunks with long reads (a kilobase against an hg38-sized index: ~360 intervals, ~830 seeds, most of them alone in their piece): still
// LDS, 62 KB per wave, two workgroups of one wave per CU -- every table access of the HBM tiers below is a memory round trip
typedef RgStore<640, 1152, 1152, 0, 0, unsigned short, short, 160> RgLongS;   // 49 KB: three workgroups per CU; four fifths of the kilobase reads' strand searches fit
typedef RgStore<768, 1536, 1536, 0, 0, unsigned short, short, 288> RgLongB;   // 67 KB, two per CU: most of the rest (288 chain records since round 6: 192 sent 6.7 k strand searches a chunk on to the HBM tier for their chains of several seeds, five times the time each: its launch 110 -> 43 ms, this one's 488 -> 522)
// ordinary reads inside repeat families (an hg38-like genome: 7 % of the strand searches outgrow RgMid): 23 KB per wave, six workgroups of one wave per CU
typedef RgStore<256, 512, 512, 0, 0, unsigned short, short, 96> RgMid2;
typedef RgStore<512, 1024, 1024, 1024, 1024, unsigned short, short> RgBig;
// the same capacity chained as the LDS tiers do it (pieces, chain starts in registers, records for multi-seed chains only), tables in an HBM
// slab, exporting: for the repeat reads that outgrow the LDS tiers but have no tied chain starts
typedef RgStore<4096, 8192, 8192, 8192, 8192, unsigned short, short> RgHuge;   // reads inside tandem repeats: thousands of short seeds
#define RG_WIN 768       // reference window of a chain kept in LDS while its seeds are extended (longer windows: extension reads HBM)
// $BSX_PHASES: where a strand search's wave cycles go.  The sums live in the wave's LDS and every lane writes them alike (uniform values): no
// divergent region inside the stages.  Round 5: `if (P.prof) { ...; if (lane == 0) atomicAdd(&counters[..], ..); }` ahead of the (not inlined)
// call of rg_export made the compiler place a copy of the lane index for the call AHEAD of the s_or_b64 that restores EXEC at the end of the
// lane-0 region -- 63 lanes entered rg_export with a stale lane index and exported garbage (tools/dbg/exec_join_check.py looks for that shape
// in the assembly; tests/test_isa_exec_join.py).  Flushed to counters[CTR_STAGE + k] once, when the wave leaves the kernel.
#define RG_NPF 16            // 0-7 stage cycles, 8 extensions, 9 extension rows
#define RG_PF_ZERO(D) do { if (P.prof) { (D).pf[lane & (RG_NPF - 1)] = 0; WAVE_SYNC(); } } while (0)
#define RG_PF_ADD(D, k, v) do { const unsigned long long s_ = (D).pf[k] + (unsigned long long)(v); (D).pf[k] = s_; } while (0)
#define RG_PF_STAGE(D, k, pf_t) do { if (P.prof) { const long long now_ = (long long)__builtin_readcyclecounter(); RG_PF_ADD(D, k, now_ - (pf_t)); (pf_t) = now_; } } while (0)   // the cycles since the last stamp go to sum k
#define RG_PF_FLUSH(D) do { if (P.prof) { WAVE_SYNC(); if (lane < RG_NPF) { const unsigned long long v_ = (D).pf[lane]; if (v_) atomicAdd(&counters[CTR_STAGE + lane], v_); } } } while (0)
struct RgDp {            // per-wave LDS scratch
	static const int QCAP = RG_QCAP;
	unsigned long long pf[RG_NPF];
	int32_t H[64], E[64];        // the one-lane passes (introsort stack, tree traversal stack)
	uint8_t q[RG_QCAP];          // the read
	uint8_t win[RG_WIN];         // reference bases [rmax0, rmax1) of the chain being extended, one byte each
};
struct RgDpLite { static const int QCAP = RG_QCAP; unsigned long long pf[RG_NPF]; int32_t H[64], E[64]; uint8_t q[RG_QCAP]; uint8_t win[4]; };   // the LDS tiers stop before the extensions: no window
#define RG_QCAP_LONG 1024   // the launches for chunks with longer reads (a read of a kilobase; anything longer is chained by the caller)
struct RgDpLiteL { static const int QCAP = RG_QCAP_LONG; unsigned long long pf[RG_NPF]; int32_t H[64], E[64]; uint8_t q[RG_QCAP_LONG]; uint8_t win[4]; };

// wave-uniform values live in scalar registers: say so for what comes out of LDS, shuffles and reductions
__device__ __forceinline__ long long uni64(long long v)
{
	return (long long)((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)v));
}

__device__ __forceinline__ long long wave_max_i64(long long v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		const long long o = (long long)((unsigned long long)(unsigned)__shfl_xor((int)(v >> 32), off) << 32 | (unsigned)__shfl_xor((int)v, off));
		v = v > o ? v : o;
	}
	return v;
}

#define RG_CTG_LDS 128   // contig offset tables up to this many entries are copied to LDS once per workgroup
__device__ __forceinline__ int rg_pos2rid(const DevIndex &ix, const long long *ctg, long long pos_f)   // bns_pos2rid, bntseq.c:356-369
{
	int left = 0, mid = 0, right = ix.n_seqs;
	if (pos_f >= ix.l_pac) return -1;
	while (left < right) {
		mid = (left + right) >> 1;
		if (pos_f >= ctg[mid]) {
			if (mid == ix.n_seqs - 1) break;
			if (pos_f < ctg[mid + 1]) break;
			left = mid + 1;
		} else right = mid;
	}
	return mid;
}
__device__ __forceinline__ long long rg_depos(long long l_pac, long long p) { return p >= l_pac ? (l_pac << 1) - 1 - p : p; }
__device__ __forceinline__ int rg_intv2rid(const DevIndex &ix, const long long *ctg, long long rb, long long re)   // bns_intv2rid, bntseq.c:371-379
{
	if (rb < ix.l_pac && re > ix.l_pac) return -2;
	const int a = rg_pos2rid(ix, ctg, rg_depos(ix.l_pac, rb));
	const int b = rb < re ? rg_pos2rid(ix, ctg, rg_depos(ix.l_pac, re - 1)) : a;
	return a == b ? a : -1;
}
#define RG_BSS(parent, l_pac, rb) ((((rb) > (l_pac)) == (parent)) ? 1 : 0)

// bwt_sa (bwt.c:87-97) on one strand's own index
__device__ __forceinline__ long long rg_sa(const DevIndex &ix, int parent, unsigned long long k, uint32_t &n_steps)
{
	const unsigned long long prim = dev_ix_primary(ix, parent);
	const uint32_t *bw = dev_ix_bwt(ix, parent);
	const uint64_t *sa = parent ? ix.fmi[1].sa : ix.fmi[0].sa;
	const uint32_t sa_mask = ix.fmi[0].sa_mask, sa_shift = ix.fmi[0].sa_shift;
	unsigned long long steps = 0;
	while (k & sa_mask) {
		if (k == prim) { k = 0; ++steps; continue; }
		const unsigned long long x = k - (k > prim);
		const DevBlock B = dev_load_block4(bw, x);
		const int c = dev_planes_symbol(B, (int)(x & 127));
		uint32_t ca, cc, cg, ct;
		dev_planes_count4(B, (int)(x & 127), ca, cc, cg, ct);
		const unsigned long long base = c == 0 ? ((unsigned long long)B.v0.y << 32 | B.v0.x) : c == 1 ? ((unsigned long long)B.v0.w << 32 | B.v0.z) :
		                                c == 2 ? ((unsigned long long)B.v1.y << 32 | B.v1.x) : ((unsigned long long)B.v1.w << 32 | B.v1.z);
		k = dev_ix_L2(ix, parent, c) + base + (c == 0 ? ca : c == 1 ? cc : c == 2 ? cg : ct);
		++steps;
	}
	n_steps += (uint32_t)steps;
	return (long long)(steps + sa[k >> sa_shift]);
}

// publish the regions of task t (or the reason it was declined)
template <typename Store>
__device__ __forceinline__ int rg_publish(Store &S, int t, int status, bsx_region_t *out, unsigned long long out_cap, unsigned long long *out_cursor,
                                          long long *reg_off, int *reg_n, int lane)
{
	WAVE_SYNC();
	if (lane == 0) {
		const int n = status ? 0 : S.n_regs;
		unsigned long long base = 0;
		if (n > 0) {
			base = atomicAdd(out_cursor, (unsigned long long)n);
			if (base + n <= out_cap) for (int k = 0; k < n; ++k) out[base + k] = S.regs[k];
			else status = 7;
		}
		reg_off[t] = (long long)base;
		reg_n[t] = status ? -status : n;
	}
	status = uni(__shfl(status, 0));
	WAVE_SYNC();
	return status;
}

// the launchers unpack the common arguments (RgLaunch) into the kernels' parameter lists
#define RG_COMMON_ *G.ix, *G.sc, *G.P, G.reads, G.tasks
#define RG_LISTS_  G.seeds_dense, G.task_off, G.task_n
#define RG_OUT_    G.out, G.out_cap, G.out_cursor, G.reg_off, G.reg_n
#define RG_POS_    G.counters, (const long long*)G.pos_off, (const unsigned long long*)G.pos
