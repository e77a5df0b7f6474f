// rg_task.hpp -- the chaining body of the region tiers, included by k_regions.hip alone (rg_introsort_keys and rg_export are real
// functions: one includer).  One wavefront takes one strand search from its SA intervals to chains (and, in the tiers that
// do not export, on to regions):
//   K3  bwt_sa for every occurrence (lanes in parallel)                       lib/aln/bwt.c:87-97
//   C1  mem_chain: seeds clustered into chains in reference order             lib/aln/memchain.c:268-393
//   C2  mem_chain_flt (weights, klib introsort permutation, overlap filter)   lib/aln/memchain.c:406-488
//   C4  mem_chain2region(1): best-first seed extension with the containment   lib/aln/memchain.c:742-904
//       tests, left/right ksw_extend2 (wave-wide, ext_dp.hpp) and band retries
#pragma once
#include "parsort.hpp"
#include "ext_dp.hpp"
#include "ext_pk.hpp"
#include "rgx.hpp"
#include "rg_common.hpp"
#include "rg_ext_seed.hpp"

// asymmetric_flt_seed (memchain.c:138-149) for the seed of `ln` bases at reference position rb (forward-reverse space) whose read bases are q[0, ln): a
// reference T under a read C or a reference A under a read G.  The reference bases come 32 at a time (one unaligned 8-byte load of pac: a chance
// match of 19-22 bases is one load); a seed lies on one strand, the reverse one read backwards and complemented
__device__ __forceinline__ int rg_seed_conv_test(const DevIndex &ix, long long rb, int ln, const uint8_t *q)
{
	const long long l_pac = ix.l_pac;
	int bad = 0;
	const bool rev = rb >= l_pac;
	const long long f0 = rev ? (l_pac << 1) - rb - ln : rb;   // forward coordinate of the seed's lowest base
	for (int done = 0; done < ln; ) {
		const long long f = f0 + done;
		unsigned long long w;
		__builtin_memcpy(&w, ix.pac + (f >> 2), 8);   // (pac is padded: upload_ref)
		const int k0 = (int)(f & 3);
		int m = 32 - k0; if (m > ln - done) m = ln - done;
		for (int k = k0; k < k0 + m; ++k) {
			const int b = (int)(w >> (((k >> 2) << 3) + ((~k & 3) << 1))) & 3;
			const int at = done + (k - k0);   // position along the forward strand
			const int i = rev ? ln - 1 - at : at, r = rev ? 3 - b : b, qq = q[i];
			bad |= (r == 3 && qq == 1) || (r == 0 && qq == 2);
		}
		done += m;
	}
	return bad;
}

// klib introsort (ksort.h:184-236) of the chains by weight, descending, with the control flow of
// csrc/host/util.c:bsx_introsort so that equal weights end in the reference's order.  One lane runs it; the elements are
// packed keys (weight << RG_KEY_BITS | chain index) so that a comparison is two independent LDS reads and a swap two stores.
__device__ void rg_introsort_keys(unsigned int *a, int n, int *stk)
{
#define LT(x, y) (((x) >> RG_KEY_BITS) > ((y) >> RG_KEY_BITS))
#define SWP(i, j) do { const unsigned int t_ = a[i]; a[i] = a[j]; a[j] = t_; } while (0)
	if (n < 2) return;
	if (n == 2) { if (LT(a[1], a[0])) SWP(0, 1); return; }
	int d, s = 0, t = n - 1, i, j, k, top = 0;
	int *stk_l = stk, *stk_r = stk + 16, *stk_d = stk + 32;   // the longer side is stacked, and only when longer than 16: depth <= log2(n)
	for (d = 2; (1 << d) < n; ++d);
	d <<= 1;
	for (;;) {
		if (s < t) {
			if (--d == 0) { // comb sort fallback (ksort.h:162-183)
				const double shrink = 1.2473309501039786540366528676643;
				int m = t - s + 1, gap = m, swapped;
				do {
					if (gap > 2) { gap = (int)(gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
					swapped = 0;
					for (i = 0; i + gap < m; ++i) if (LT(a[s + i + gap], a[s + i])) { SWP(s + i, s + i + gap); swapped = 1; }
				} while (swapped || gap > 2);
				if (gap != 1) for (i = s + 1; i <= t; ++i) for (j = i; j > s && LT(a[j], a[j - 1]); --j) SWP(j, j - 1);
				t = s;
				continue;
			}
			i = s; j = t; k = i + ((j - i) >> 1) + 1;
			if (LT(a[k], a[i])) { if (LT(a[k], a[j])) k = j; }
			else k = LT(a[j], a[i]) ? i : j;
			const unsigned int rp = a[k];
			if (k != t) SWP(k, t);
			for (;;) {
				do ++i; while (LT(a[i], rp));
				do --j; while (i <= j && LT(rp, a[j]));
				if (j <= i) break;
				SWP(i, j);
			}
			SWP(i, t);
			if (i - s > t - i) {
				if (i - s > 16) { stk_l[top] = s; stk_r[top] = i - 1; stk_d[top] = d; ++top; }
				s = t - i > 16 ? i + 1 : t;
			} else {
				if (t - i > 16) { stk_l[top] = i + 1; stk_r[top] = t; stk_d[top] = d; ++top; }
				t = i - s > 16 ? i - 1 : s;
			}
		} else {
			if (top == 0) { for (i = 1; i < n; ++i) for (j = i; j > 0 && LT(a[j], a[j - 1]); --j) SWP(j, j - 1); return; }
			--top; s = stk_l[top]; t = stk_r[top]; d = stk_d[top];
		}
	}
#undef LT
#undef SWP
}

// ---- the chain index as the reference keeps it: kbtree.h instantiated with t = 3 (pre-emptive split on the way down,
// lower-bound search inside a node, duplicates allowed); same structure as csrc/host/util.c:bsx_bt_*.  One lane runs it.
template <typename Store>
__device__ int rg_bt_find(const Store &S, const RgNode &x, long long pos, int &r)
{
	int begin = 0, end = x.n;
	r = 0;
	if (x.n == 0) return -1;
	while (begin < end) { const int mid = (begin + end) >> 1; if (S.ch[x.id[mid]].pos < pos) begin = mid + 1; else end = mid; }
	if (begin == x.n) { r = 1; return x.n - 1; }
	const long long kb = S.ch[x.id[begin]].pos;
	r = (kb < pos) - (pos < kb);
	if (r < 0) --begin;
	return begin;
}
template <typename Store>
__device__ int rg_bt_alloc(Store &S, int internal)
{
	RgNode &x = S.node[S.n_nodes];
	x.n = 0; x.internal = (unsigned char)internal;
	return S.n_nodes++;
}
template <typename Store>
__device__ void rg_bt_split(Store &S, int xi, int i, int yi)
{
	const int zi = rg_bt_alloc(S, S.node[yi].internal);
	RgNode &x = S.node[xi], &y = S.node[yi], &z = S.node[zi];
	z.n = 2;
	z.id[0] = y.id[3]; z.id[1] = y.id[4];
	if (y.internal) { z.child[0] = y.child[3]; z.child[1] = y.child[4]; z.child[2] = y.child[5]; }
	y.n = 2;
	for (int k = x.n; k > i; --k) x.child[k + 1] = x.child[k];
	x.child[i + 1] = (unsigned short)zi;
	for (int k = x.n; k > i; --k) x.id[k] = x.id[k - 1];
	x.id[i] = y.id[2];
	++x.n;
}
template <typename Store>
__device__ void rg_bt_put(Store &S, long long pos, int id)
{
	if (S.node[S.root].n == 5) {
		const int r = S.root, s = rg_bt_alloc(S, 1);
		S.node[s].child[0] = (unsigned short)r;
		S.root = s;
		rg_bt_split(S, s, 0, r);
	}
	int xi = S.root, r;
	for (;;) {
		RgNode &x = S.node[xi];
		if (!x.internal) {
			const int i = rg_bt_find(S, x, pos, r);
			for (int k = x.n - 1; k > i; --k) x.id[k + 1] = x.id[k];
			x.id[i + 1] = (unsigned short)id;
			++x.n;
			return;
		}
		int i = rg_bt_find(S, x, pos, r) + 1;
		if (S.node[x.child[i]].n == 5) {
			rg_bt_split(S, xi, i, x.child[i]);
			if (pos > S.ch[x.id[i]].pos) ++i;
		}
		xi = x.child[i];
	}
}
template <typename Store>
__device__ int rg_bt_lower(const Store &S, long long pos)
{
	int xi = S.root, lower = -1, r;
	for (;;) {
		const RgNode &x = S.node[xi];
		const int i = rg_bt_find(S, x, pos, r);
		if (i >= 0 && r == 0) return x.id[i];
		if (i >= 0) lower = x.id[i];
		if (!x.internal) return lower;
		xi = x.child[i + 1];
	}
}
// in-order traversal (__kb_traverse, kbtree.h:340-366) into ord[]
template <typename Store>
__device__ int rg_bt_traverse(Store &S, int *stk)
{
	int n = 0, top = 0;
	int *st_x = stk, *st_i = stk + 32;
	st_x[0] = S.root; st_i[0] = 0;
	while (top >= 0) {
		const RgNode &x = S.node[st_x[top]];
		const int i = st_i[top];
		if (!x.internal) { for (int k = 0; k < x.n; ++k) S.ord[n++] = (typename Store::idx_t)x.id[k]; --top; continue; }
		if (i > x.n) { --top; continue; }
		if (i > 0) S.ord[n++] = (typename Store::idx_t)x.id[i - 1];
		st_i[top] = i + 1;
		++top; st_x[top] = x.child[i]; st_i[top] = 0;
	}
	return n;
}

// overlap test of mem_chain_flt (memchain.c:436-452) for chain ci against kept chain ck: bit 0 = large overlap, bit 1 = ci is dropped
__device__ __forceinline__ int rg_flt_vals(const RegParams &P, int ci_beg, int ci_end, int ci_w, int ci_alt, int ck_beg, int ck_end, int ck_w, int ck_alt)
{
	const int b_max = ck_beg > ci_beg ? ck_beg : ci_beg, e_min = ck_end < ci_end ? ck_end : ci_end;
	if (e_min > b_max && (!ck_alt || ci_alt)) {
		const int li = ci_end - ci_beg, lj = ck_end - ck_beg, min_l = li < lj ? li : lj;
		if ((float)(e_min - b_max) >= (float)min_l * P.mask_level && min_l < P.max_chain_gap)
			return 1 | (((float)ci_w < (float)ck_w * P.drop_ratio && ck_w - ci_w >= P.min_seed_len << 1) ? 2 : 0);
	}
	return 0;
}
__device__ __forceinline__ int rg_flt_test(const RegParams &P, const RgChain &ci, const RgChain &ck)
{
	return rg_flt_vals(P, ci.first_q, ci.last_q + ci.last_len, ci.w, ci.is_alt, ck.first_q, ck.last_q + ck.last_len, ck.w, ck.is_alt);
}

// ---- The LDS tiers stop after the chain filter and hand the surviving chains to k_c2r: chaining needs its tables (24 KB of LDS per
// wave at the larger size, six waves per CU), the chain-to-region loop needs registers and latency hiding (extension rows are
// dependent DPP chains) but almost no tables.  One launch each, with the occupancy each can have.  What is exported per strand
// search: the kept chains in processing order, each with its seeds (main list, then seeds_extra) in arrival order.
// the record of chain `id` (by value); for a chain of one seed, made up from the seed (s_extra bit 2 = its contig is an ALT)
template <typename Store>
__device__ __forceinline__ RgChain rg_chain(const Store &S, int id)
{
	if (Store::PCAP == 0) return S.ch[id];
	if (id >= RG_REC) return S.ch[id - RG_REC];
	RgChain c;
	const short qb = S.s_qbeg[id], ln = S.s_len[id];
	c.pos = c.last_r = S.s_rbeg[id]; c.rid = S.s_rid[id]; c.endr_off = ln;
	c.first_q = c.last_q = qb; c.last_len = ln; c.wq = c.wr = ln; c.endq = (short)(qb + ln); c.first = -1; c.w = ln;
	c.n_seeds = 1; c.seed0 = (unsigned short)id; c.kept = 0; c.is_alt = (unsigned char)((S.s_extra[id] >> 2) & 1); c.n_extra = 0;
	return c;
}

// returns 11 (exported), 0 (nothing left to extend: the strand search has no regions) or 6 (no room: the next tier takes it)
template <typename Store>
__device__ int rg_export(Store &S, int t, int tot, float frac_rep, const RgXPool &X, int lane, int flt)
{
	typedef typename Store::idx_t idx_t;
	const int nk = uni(S.n_chains);
	const unsigned long long lt_mask = (1ull << lane) - 1;
	// a chain of one seed that fails asymmetric_flt_seed, with no contained seeds to fall back to, comes and goes without a trace
	int n_surv = 0, n_sd = 0;
	for (int base = 0; base < nk; base += 64) {
		const int ci = base + lane;
		bool surv = false; int cnt = 0;
		if (ci < nk) {
			const RgChain c = rg_chain(S, (int)S.ord[ci]);
			surv = !(c.n_seeds == 1 && c.n_extra == 0 && (S.s_extra[c.seed0] & 2));
			cnt = surv ? c.n_seeds + c.n_extra : 0;
		}
		const unsigned long long b = __ballot(surv);
		WAVE_SYNC();
		if (surv) S.ord[n_surv + __popcll(b & lt_mask)] = S.ord[ci];   // compacted in place, order kept (targets never pass the sources)
		n_surv += __popcll(b);
		n_sd += wave_sum_i32(cnt);
		WAVE_SYNC();
	}
	if (n_surv == 0) return 0;
	// room for the extensions made ahead of k_c2r (k_ext4.hip); the seed-SW filter rewrites the lists after the export.  X.ext = 1: a slot per chain (the
	// seed the loop reaches first); 2: a slot per seed (every seed of every main list is extended ahead: the HBM tiers' strand searches, where the
	// loop skips one seed in fourteen)
	const int ext = flt == RG_NOFLT ? X.ext : 0;
	const unsigned long long bytes = sizeof(RgXHdr) + (unsigned long long)n_surv * sizeof(RgXChain) + (unsigned long long)n_sd * sizeof(RgXSeed) + (ext ? (unsigned long long)(ext == 2 ? n_sd : n_surv) * sizeof(RgXExt) : 0ull);
	unsigned long long at = 0;
	if (lane == 0) at = atomicAdd(X.cursor, bytes);
	at = (unsigned long long)uni64((long long)at);
	if (at + bytes > X.cap) return 6;
	RgXHdr *H = (RgXHdr*)(X.base + at);
	RgXChain *XC = (RgXChain*)(H + 1);
	RgXSeed *XS = (RgXSeed*)(XC + n_surv);
	if (lane == 0) { H->n_chains = n_surv; H->n_seeds = n_sd; H->frac_rep = frac_rep; H->flt = flt; H->has_ext = ext; H->pad = Store::SCAP; }   // (pad: which tier's tables made the record, for the debug checks)
	int so = 0;
	for (int ci = 0; ci < n_surv; ++ci) {
		const int c = uni(S.ord[ci]);
		const RgChain chn = rg_chain(S, c);
		const int n_main = uni(chn.n_seeds), n_extra = uni(chn.n_extra);
		if (lane == 0) { RgXChain x; x.pos = chn.pos; x.rid = chn.rid; x.seed_off = so; x.n_main = (unsigned short)n_main; x.n_extra = (unsigned short)n_extra; x.pad = 0; XC[ci] = x; }
		if (n_main == 1 && n_extra == 0) {
			if (lane == 0) { const int o = chn.seed0; RgXSeed x; x.rbeg = S.s_rbeg[o]; x.qbeg = S.s_qbeg[o]; x.len = S.s_len[o]; x.sb = (int)x.len << 1 | ((S.s_extra[o] >> 1) & 1); XS[so] = x; }
			so += 1;
			continue;
		}
		for (int pass = 0; pass < 2; ++pass) {
			if (pass == 1 && n_extra == 0) break;
			int nl = 0;
			for (int base = 0; base < tot; base += 64) {
				const int o = base + lane;
				const bool in = o < tot && S.s_chain[o] == c && (int)(S.s_extra[o] & 1) == pass;
				const unsigned long long b = __ballot(in);
				if (in) { RgXSeed x; x.rbeg = S.s_rbeg[o]; x.qbeg = S.s_qbeg[o]; x.len = S.s_len[o]; x.sb = (int)x.len << 1 | ((S.s_extra[o] >> 1) & 1); XS[so + nl + __popcll(b & lt_mask)] = x; }
				nl += __popcll(b);
			}
			so += nl;
		}
	}
	if (lane == 0) { X.xoff[t] = (long long)at; X.xlist[atomicAdd(X.xcount, 1u)] = t; }
	return 11;
}

// One strand search, SA intervals -> regions, by one wavefront.  Returns 0 or the reason the task is declined:
//   1 seeding overflowed   9 read longer than RG_QCAP or long enough for the seed-SW filter (memchain.c:544)   8 intervals > ICAP
//   2 occurrences > SCAP or an interval beyond max_occ      3 chains > CCAP      4 two chains start at the same position
//   6 regions > RCAP      10 an over-represented interval has to be walked past max_occ (memchain.c:325-326)
template <typename Store, bool SPLIT = false, typename DP = RgDp, bool PK = false>   // PK: extension rows of 64 columns and more in packed 16-bit (ext_pk.hpp); the launcher has checked ext_pk_exact_reads()
__device__ int rg_task(Store &S, DP &D, const DevIndex &ix, const DevScoring &sc, const RegParams &P, const uint8_t *reads,
                       int l_query, int parent, uint32_t qoff, const DevIntv *src, int n_iv, const unsigned long long *posl, int lane,
                       unsigned long long *counters, const int *gap, const long long *ctg, const RgXPool *X = nullptr, int task_id = 0,
                       int n_boost = 0, const int *boost_iv = nullptr, const int *boost_lvl = nullptr)
{
	typedef typename Store::idx_t idx_t;
	const long long l_pac = ix.l_pac;
	const uint8_t *query = reads + qoff;
	// per-stage wave cycles (P.prof, set under $BSX_PHASES) into the wave's sums D.pf, see RG_PF_ADD
	long long pf_t = P.prof ? (long long)__builtin_readcyclecounter() : 0;
	unsigned int pf_ext = 0, pf_rows = 0;
#define RG_STAGE(k) RG_PF_STAGE(D, k, pf_t)
	if (lane == 0) {
		S.n_chains = 0; S.n_regs = 0;
		if (Store::NODES) { S.n_nodes = 0; S.root = rg_bt_alloc(S, 0); }
	}
	WAVE_SYNC();
	if (n_iv < 0) return 1;
	if (l_query > DP::QCAP) return 9;
	if (n_iv > Store::ICAP) return 8;
	// mem_flt_chained_seeds (memchain.c:537-568) runs for reads of this length?  Then the chains are exported with the threshold and
	// k_seedsw scores their seeds before k_c2r; the tiers that make regions themselves leave such a strand search to the caller
	const int flt = (P.flt_tab && l_query <= P.flt_len) ? uni(P.flt_tab[l_query]) : RG_NOFLT;
	if (!SPLIT && flt != RG_NOFLT) return 9;
	if (n_iv == 0 || l_query < P.min_seed_len) return 0;
	for (int i = lane; i < l_query; i += 64) D.q[i] = query[i];   // the read, for the seed tests and the extensions (ordered by the stage barriers below)

	// ---- A. intervals, ordered by info (ks_introsort(mem_intv), memchain.c:105; equal keys are identical records)
	// With positions looked up beforehand (k_occ), posl holds them interval by interval in the order the seeding kernel
	// left the list: iv_x0 then carries each interval's offset into posl instead of its first SA rank.
	long long run = 0;
	for (int base = 0; base < n_iv; base += 64) {
		const int i = base + lane;
		DevIntv mine; mine.x0 = mine.x1 = mine.x2 = 0; mine.info = 0;
		if (i < n_iv) mine = src[i];
		// occurrences this strand search will visit: all of them, or the first max_occ of an over-represented interval (memchain.c:325-326)
		const int big = mine.x2 > (unsigned long long)P.max_occ;
		const int lk = big ? P.max_occ : (int)mine.x2;   // what k_occ looked up ahead
		long long incl = lk;
		if (P.max_occ <= 1 << 24) incl = wave_scan_sum_incl(lk);   // (64 intervals of at most max_occ: the sum fits; DPP instead of twelve ds_bpermute)
		else {
#pragma unroll
			for (int off = 1; off < 64; off <<= 1) {
				const long long o = (long long)((unsigned long long)(unsigned)__shfl_up((int)(incl >> 32), off) << 32 | (unsigned)__shfl_up((int)incl, off));
				if (lane >= off) incl += o;
			}
		}
		// the other keys come 64 at a time with one coalesced load and are handed round with v_readlane
		int rank = 0;
		constexpr bool K32 = Store::ICAP <= 1024 && DP::QCAP < 2048;   // begin (11 bits), end (11) and the list index (10) as ONE 32-bit key: unique, a readlane and a compare per pair
		if (K32) {
			const unsigned int mykey = i < n_iv ? ((unsigned int)(mine.info >> 32) << 21 | ((unsigned int)mine.info & 0x7ffu) << 10 | (unsigned int)i) : 0xffffffffu;
			for (int cb = 0; cb < n_iv; cb += 64) {
				const int kk = cb + lane;
				unsigned int okey = mykey;
				if (cb != base) { const unsigned long long oinfo = kk < n_iv ? src[kk].info : ~0ull; okey = kk < n_iv ? ((unsigned int)(oinfo >> 32) << 21 | ((unsigned int)oinfo & 0x7ffu) << 10 | (unsigned int)kk) : 0xffffffffu; }
				const int lim = n_iv - cb < 64 ? n_iv - cb : 64;
				for (int j = 0; j < lim; ++j) rank += (unsigned int)__builtin_amdgcn_readlane((int)okey, j) < mykey;
			}
		} else
		for (int cb = 0; cb < n_iv; cb += 64) {
			const int kk = cb + lane;
			const unsigned long long oinfo = kk < n_iv ? src[kk].info : ~0ull;
			const int lim = n_iv - cb < 64 ? n_iv - cb : 64;
			for (int j = 0; j < lim; ++j) {
				const unsigned long long oi = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(oinfo >> 32), j) << 32 | (unsigned)__builtin_amdgcn_readlane((int)oinfo, j);
				rank += (oi < mine.info) || (oi == mine.info && cb + j < i);
			}
		}
		if (i < n_iv) {
			// The reference walks an over-represented interval past its first max_occ occurrences while it has started at most five chains
			// (memchain.c:325-326).  The HBM tiers do too: when the rule asks for more of an interval the strand search is run again with that
			// interval's share multiplied (boost_*), the further positions walked here
			long long want = lk;
			if (Store::NODES && big) for (int b = 0; b < n_boost; ++b) if (boost_iv[b] == rank) want = (long long)P.max_occ * boost_lvl[b];
			if (want > (long long)mine.x2) want = (long long)mine.x2;
			if (want > 0x0fffffff) want = 0x0fffffff;
			const int cnt = (int)want;
			S.iv_x0[rank] = posl ? (unsigned long long)(run + incl - lk) : mine.x0;
			if (Store::NODES) S.iv_rank[rank] = mine.x0;
			S.iv_n[rank] = cnt | ((big && (unsigned long long)cnt < mine.x2) ? 1 << 29 : 0) | big << 30;
			S.iv_beg[rank] = (short)(mine.info >> 32); S.iv_end[rank] = (short)(uint32_t)mine.info;
		}
		run += uni64((long long)((unsigned long long)(unsigned)__shfl((int)(incl >> 32), 63) << 32 | (unsigned)__shfl((int)incl, 63)));
	}
	WAVE_SYNC();
	RG_STAGE(0);
	// ---- B. occurrences: every k < x[2] of every interval (the caps of memchain.c:325-326 cannot bind while x[2] <= max_occ)
	int tot = 0, over = 0, any_big = 0;
	for (int base = 0; base < n_iv; base += 64) { // totals with one pass over the table, 64 intervals at a time
		const int i = base + lane;
		const int v = i < n_iv ? S.iv_n[i] : 0;
		const int c = v & 0x1fffffff;
		if (__ballot(c > Store::SCAP)) over = 1;
		if (__ballot(v >> 30)) any_big = 1;
		tot += wave_sum_i32(c > Store::SCAP ? Store::SCAP : c);
		if (tot > Store::SCAP) { over = 1; break; }
	}
	if (over || tot > Store::SCAP) return 2;
	float frac_rep = 0.f;
	if (any_big) { // read length covered by over-represented seeds (memchain.c:294-301)
		int b = 0, e = 0, l_rep = 0;
		for (int i = 0; i < n_iv; ++i) {
			if (!(uni(S.iv_n[i]) >> 30)) continue;
			const int sb = uni(S.iv_beg[i]), se = uni(S.iv_end[i]);
			if (sb > e) { l_rep += e - b; b = sb; e = se; } else e = e > se ? e : se;
		}
		l_rep += e - b;
		frac_rep = (float)l_rep / l_query;
	}
	{
		int i = 0, acc = 0;   // occurrences are visited in increasing order by each lane: the interval cursor only moves forward
		uint32_t lf = 0;
		if (Store::SCAP > 256 && n_iv > 256) { // thousands of intervals with a few occurrences each: a lane per interval, 64 intervals at a time
			int run_o = 0;
			for (int base = 0; base < n_iv; base += 64) {
				const int ii = base + lane;
				const int cnt = ii < n_iv ? (S.iv_n[ii] & 0x1fffffff) : 0;
				const int incl = wave_scan_sum_incl(cnt);
				const int o0 = run_o + incl - cnt;
				if (cnt) {
					const unsigned long long x0 = S.iv_x0[ii];
					const int qb = S.iv_beg[ii], slen = S.iv_end[ii] - qb;
					const int lkc = (S.iv_n[ii] >> 30) && cnt > P.max_occ ? P.max_occ : cnt;   // looked up ahead; the rest is walked here
					const unsigned long long rk0 = Store::NODES ? S.iv_rank[ii] : x0;
					for (int c = 0; c < cnt; ++c) {
						const long long pos = (posl && c < lkc) ? (long long)posl[x0 + (unsigned long long)c] : rg_sa(ix, parent, (posl ? rk0 : x0) + (unsigned long long)c, lf);
						const int o = o0 + c;
						S.s_rbeg[o] = pos; S.s_qbeg[o] = (short)qb; S.s_len[o] = (short)slen;
						S.s_rid[o] = rg_intv2rid(ix, ctg, pos, pos + slen);
						S.s_chain[o] = -1; S.s_extra[o] = 0;
					}
				}
				run_o += uni(__builtin_amdgcn_readlane(incl, 63));
			}
		} else
		for (int o = lane; o < tot; o += 64) {
			while (acc + (S.iv_n[i] & 0x1fffffff) <= o) { acc += S.iv_n[i] & 0x1fffffff; ++i; }
			const int kk_ = o - acc, vv_ = S.iv_n[i], lkc_ = (vv_ >> 30) && (vv_ & 0x1fffffff) > P.max_occ ? P.max_occ : (vv_ & 0x1fffffff);
			const long long pos = (posl && kk_ < lkc_) ? (long long)posl[S.iv_x0[i] + (unsigned long long)kk_]
			                                            : rg_sa(ix, parent, ((posl && Store::NODES) ? S.iv_rank[Store::NODES ? i : 0] : S.iv_x0[i]) + (unsigned long long)kk_, lf);
			const int slen = S.iv_end[i] - S.iv_beg[i];
			S.s_rbeg[o] = pos; S.s_qbeg[o] = S.iv_beg[i]; S.s_len[o] = (short)slen;
			const int rid_ = rg_intv2rid(ix, ctg, pos, pos + slen);
			S.s_rid[o] = rid_;
			S.s_chain[o] = -1; S.s_extra[o] = (Store::PCAP && rid_ >= 0 && ix.ctg_alt[rid_]) ? 4 : 0;
		}
		// work counters of the algorithmic-bytes model: FM blocks touched by the LF walks, SA samples read
		lf = (uint32_t)wave_sum_i32((int)lf);
		if (lane == 0 && !posl) { atomicAdd(&counters[CTR_LF_STEPS], (unsigned long long)lf); atomicAdd(&counters[CTR_LF_CALLS], (unsigned long long)tot); }
	}
	WAVE_SYNC();
	// asymmetric_flt_seed (memchain.c:138-149) for every seed at once, a lane per seed: a reference T under a read C or a reference A
	// under a read G.  Bit 1 of s_extra; the seed loop of stage E only tests the bit (one dependent trip to HBM per seed there
	// was a quarter of this kernel's time on a genome where most seeds are chance matches).
	for (int o = lane; o < tot; o += 64) {
		if (S.s_rid[o] < 0) continue;
		const int bad = rg_seed_conv_test(ix, S.s_rbeg[o], (int)S.s_len[o], D.q + S.s_qbeg[o]);
		if (bad) S.s_extra[o] |= 2;
	}
	WAVE_SYNC();
	RG_STAGE(1);
	// ---- C. chaining in arrival order (mem_chain's loop over occurrences, memchain.c:313-366)
	// Without the B-tree (LDS tiers): the chain starts live sorted across the wave's registers, entry e in lane e & 63 of register set
	// e >> 6.  kb_intervalp's `lower` (the largest start <= rbeg) is a compare, a ballot and a population count per register set; a
	// new chain shifts the entries above it up one lane (DPP).  Unique starts make the sorted order the tree's in-order traversal.
	constexpr int TCAP = Store::CCAP < 512 ? Store::CCAP : 512;   // chain starts of one piece (the whole strand search in the HBM tiers' tree)
	constexpr int NR = Store::NODES ? 1 : (TCAP + 63) / 64;
	unsigned int st_lo[NR], st_hi[NR]; int st_id[NR];
#pragma unroll
	for (int r = 0; r < NR; ++r) { st_lo[r] = st_hi[r] = 0xffffffffu; st_id[r] = -1; }
	int nc = 0, n_prom = 0;   // chains; those of them with a record (PCAP stores)
	int cur_iv = -1, iv_stop = 0, iv_big = 0, count = 0;   // the interval the occurrence belongs to, and the chains it has started
	int iv_more = 0, iv_o0 = 0;                            // (HBM tiers) the interval has occurrences beyond the ones listed; its first seed
	// The LDS tiers first set aside the seeds that cannot meet any other: merge_seed_to_chain (memchain.c:227-256) only ever joins a
	// seed to a chain whose last seed lies less than l_query + min(w, max_chain_gap) before it on the reference (rdist <= qdist + w,
	// rdist - last->len < max_chain_gap) or whose span contains it, and every step inside a chain is that short too.  So cut the seeds,
	// sorted by reference position, wherever two neighbours are at least that far apart: a seed alone in its piece starts a chain of
	// its own whatever else the strand search holds, no later seed joins it, and it never changes the outcome of a test between two
	// other seeds (the chain below a seed is either in the seed's own piece or too far to be joined) -- against an hg38-sized genome
	// that is ~95 of the ~100 chains of a strand search, the chance matches of a 3-letter 19-mer.  Only the seeds of the other pieces
	// go through the sequential loop below, in arrival order, over a table of their own chain starts.
	int n_iso = 0, n_live = tot, n_pieces = 0;
	if (!Store::NODES) {
		constexpr int NS = Store::SCAP / 64;
		constexpr int KB = Store::SCAP <= 512 ? 9 : 12;   // bits of the arrival index below the position in the sort keys
		const long long dgap = (long long)l_query + 1 + (long long)(P.w < P.max_chain_gap ? P.w : P.max_chain_gap);
		unsigned long long key[NS]; int rk[NS];
		int n_dead = 0;
#pragma unroll
		for (int c = 0; c < NS; ++c) { // seeds that take no part (memchain.c:339-346) sort last
			const int o = (c << 6) + lane;
			key[c] = ~0ull; rk[c] = 0;
			bool dead = false;
			if (o < tot) {
				const long long rb = S.s_rbeg[o];
				dead = S.s_rid[o] < 0 || ((P.bsstrand & 1) && RG_BSS(parent, l_pac, rb) != P.bsstrand >> 1);
				if (dead) S.s_rbeg[o] = (1ll << 40) + o;   // nothing reads the position of such a seed again
				key[c] = (unsigned long long)(dead ? (1ll << 40) + o : rb) << KB | (unsigned)o;
			}
			n_dead += __popcll(__ballot(dead));
		}
		n_live = tot - n_dead;
		WAVE_SYNC();
		for (int k = 0; k < tot; ++k) { // rank by counting: the keys (position, arrival index) are unique
			const unsigned long long kk = (unsigned long long)uni64(S.s_rbeg[k]) << KB | (unsigned)k;
#pragma unroll
			for (int c = 0; c < NS; ++c) rk[c] += kk < key[c];
		}
#pragma unroll
		for (int c = 0; c < NS; ++c) { const int o = (c << 6) + lane; if (o < tot) S.lst[rk[c]] = (idx_t)o; }
		WAVE_SYNC();
		int iso = 0;
#pragma unroll
		for (int c = 0; c < NS; ++c) {
			const int r = (c << 6) + lane;
			bool opens = false; int o = 0;
			if (r < n_live) {
				o = S.lst[r];
				const long long rb = S.s_rbeg[o];
				const bool far_l = r == 0 || rb - S.s_rbeg[S.lst[r > 0 ? r - 1 : 0]] >= dgap;
				const bool far_r = r == n_live - 1 || S.s_rbeg[S.lst[r + 1 < n_live ? r + 1 : r]] - rb >= dgap;
				if (far_l && far_r) { S.s_chain[o] = (decltype(S.s_chain[0] + 0))o; S.s_extra[o] |= 8; ++iso; }   // bit 3: the seed starts a chain
				else { S.s_extra[o] |= 16; opens = far_l; }                                                          // bit 4: it goes through the loop
			}
			// the piece a seed with neighbours lies in (pieces numbered along the reference): keep[] is free until the chains are filtered
			const unsigned long long om = __ballot(opens);
			if (r < n_live && (S.s_extra[o] & 16)) S.keep[o] = (idx_t)(n_pieces + __popcll(om & ((2ull << lane) - 1)) - 1);
			n_pieces += __popcll(om);
		}
		n_iso = wave_sum_i32(iso);
		WAVE_SYNC();
	}
	// The pieces do not interact, so each is chained on its own, its seeds in arrival order over a table of its own chain starts: a read
	// inside a repeat family has hundreds of seeds in a hundred pieces of a few seeds each, and a search over one register set instead of
	// one per 64 chains of the whole strand search
	int o = -1, cbase = -64, piece = 0, nc_tot = 0;
	unsigned long long cmask = 0;
	for (;;) {
		if (Store::NODES) { // every occurrence, in arrival order
			if (++o >= tot) break;
			while (o >= iv_stop) { // next interval with occurrences
				// an over-represented interval is walked past its first max_occ occurrences while it has started at most 5 chains
				// (memchain.c:325-326): those further occurrences were not looked up, the host takes the strand search
				if (iv_more && count < P.max_occ && count <= 5) { if (lane == 0) S.boost_iv = cur_iv; return 10; }
				++cur_iv;
				const int v = uni(S.iv_n[cur_iv]);
				iv_o0 = iv_stop;
				iv_stop += v & 0x1fffffff; iv_big = v >> 30; iv_more = (v >> 29) & 1; count = 0;
			}
			// the loop condition of memchain.c:325-326: no more than max_occ chains from one interval; past the first max_occ occurrences only
			// while it has started at most five
			if (iv_big && (count >= P.max_occ || (count > 5 && o - iv_o0 >= P.max_occ))) { o = iv_stop - 1; continue; }
		} else { // the seeds of the current piece, in arrival order; then the next piece with an empty table
			while (cmask == 0 && piece < n_pieces) {
				cbase += 64;
				if (cbase >= tot) {
					++piece; cbase = -64;
					nc_tot += nc; nc = 0;
#pragma unroll
					for (int r = 0; r < NR; ++r) { st_lo[r] = st_hi[r] = 0xffffffffu; st_id[r] = -1; }
					continue;
				}
				const int oo = cbase + lane < tot ? cbase + lane : 0;
				cmask = __ballot(cbase + lane < tot && (S.s_extra[oo] & 16) && (int)S.keep[oo] == piece);
			}
			if (cmask == 0) break;
			o = cbase + (int)__builtin_ctzll(cmask);
			cmask &= cmask - 1;
		}
		const int rid = uni(S.s_rid[o]);
		if (rid < 0) continue;
		const long long rbeg = uni64(S.s_rbeg[o]);
		const int qbeg = uni(S.s_qbeg[o]), len = uni(S.s_len[o]);
		if (Store::NODES && (P.bsstrand & 1) && RG_BSS(parent, l_pac, rbeg) != P.bsstrand >> 1) continue;
		int lower = -1, at = 0;   // at: sorted index the new chain would take
		bool tied = false;
		if (Store::NODES) {
			if (lane == 0 && nc > 0) lower = rg_bt_lower(S, rbeg);
			lower = uni(__shfl(lower, 0));
		} else {
			const unsigned int rlo = (unsigned int)rbeg, rhi = (unsigned int)((unsigned long long)rbeg >> 32);
#pragma unroll
			for (int r = 0; r < NR; ++r)
				if (r * 64 < nc) at += __popcll(__ballot(st_hi[r] < rhi || (st_hi[r] == rhi && st_lo[r] <= rlo)));
			if (at > 0) {
				const int e = at - 1, el = e & 63;
				unsigned int plo = 0, phi = 0;
#pragma unroll
				for (int r = 0; r < NR; ++r)
					if (r == e >> 6) { lower = __builtin_amdgcn_readlane(st_id[r], el); plo = (unsigned int)__builtin_amdgcn_readlane((int)st_lo[r], el); phi = (unsigned int)__builtin_amdgcn_readlane((int)st_hi[r], el); }
				tied = plo == rlo && phi == rhi;
			}
		}
		int merged = 0;
		if (lower >= 0) { // merge_seed_to_chain, memchain.c:227-256
			const RgChain c = rg_chain(S, lower);
			int kind = 0;   // 1: contained in the chain (goes on seeds_extra), 2: appended
			if (rid == c.rid) {
				if (qbeg >= c.first_q && qbeg + len <= c.last_q + c.last_len && rbeg >= c.pos && rbeg + len <= c.last_r + c.last_len) kind = 1;
				else if (!((c.last_r < l_pac || c.pos < l_pac) && rbeg >= l_pac)) {
					const long long qdist = qbeg - c.last_q, rdist = rbeg - c.last_r;
					if (rdist >= 0 && qdist - rdist <= P.w && rdist - qdist <= P.w && qdist - c.last_len < P.max_chain_gap && rdist - c.last_len < P.max_chain_gap) kind = 2;
				}
			}
			kind = uni(kind);
			if (kind) {
				int rec = lower;   // where the chain's record is (made now if the chain was a single seed so far)
				if (Store::PCAP) {
					if (lower < RG_REC) {
						if (n_prom == Store::PCAP) return 3;
						rec = n_prom++;
						if (lane == 0) { S.ch[rec] = c; S.s_chain[c.seed0] = (decltype(S.s_chain[0] + 0))(RG_REC + rec); }
						const int e = at - 1, el = e & 63;   // its entry in the sorted table names the record from now on
#pragma unroll
						for (int r = 0; r < NR; ++r) if (r == e >> 6 && lane == el) st_id[r] = RG_REC + rec;
					} else rec = lower - RG_REC;
				}
				if (lane == 0) {
					RgChain &d = S.ch[rec];
					S.s_chain[o] = (decltype(S.s_chain[0] + 0))(Store::PCAP ? RG_REC + rec : rec);
					if (kind == 1) { S.s_extra[o] |= 1; d.n_extra = (unsigned short)(c.n_extra + 1); }
					else {
						d.last_q = (short)qbeg; d.last_r = rbeg; d.last_len = (short)len;
						// mem_chain_weight (memchain.c:158-180) as a running sum: seeds join a chain in the order that loop visits them
						int wq = c.wq, wr = c.wr;
						if (qbeg >= c.endq) wq += len; else if (qbeg + len > c.endq) wq += qbeg + len - c.endq;
						const long long endr = c.pos + c.endr_off;
						if (rbeg >= endr) wr += len; else if (rbeg + len > endr) wr += (int)(rbeg + len - endr);
						d.wq = (short)wq; d.wr = (short)(wr < 32767 ? wr : 32767);   // only min(wq, wr) is read, and wq <= read length
						if (qbeg + len > c.endq) d.endq = (short)(qbeg + len);
						if (rbeg + len > endr) d.endr_off = (int)(rbeg + len - c.pos);
						d.n_seeds = (unsigned short)(c.n_seeds + 1);
					}
				}
				merged = 1;
			}
		}
		if (!merged) {
			if (nc == (Store::NODES ? Store::CCAP : TCAP)) return 3;
			if (!Store::NODES && tied) return 4;   // duplicate key: the B-tree shape matters, the HBM tiers keep one
			const int new_id = Store::PCAP ? o : nc;   // a chain of one seed has no record in the LDS tiers
			if (lane == 0) {
				if (!Store::PCAP) {
					RgChain c;
					c.pos = c.last_r = rbeg; c.rid = rid; c.endr_off = len; c.first_q = c.last_q = (short)qbeg; c.last_len = (short)len;
					c.wq = c.wr = (short)len; c.endq = (short)(qbeg + len); c.first = -1; c.w = 0; c.n_seeds = 1; c.seed0 = (unsigned short)o;
					c.kept = 0; c.is_alt = ix.ctg_alt[rid] ? 1 : 0; c.n_extra = 0;
					S.ch[nc] = c;
				}
				S.s_chain[o] = (decltype(S.s_chain[0] + 0))new_id;
				if (!Store::NODES) S.s_extra[o] |= 8;
				if (Store::NODES) rg_bt_put(S, rbeg, nc);
			}
			if (!Store::NODES) { // open slot `at` of the sorted table
				const int ar = at >> 6, al = at & 63;
#pragma unroll
				for (int r = NR - 1; r >= 0; --r) {
					if (r >= ar && r * 64 <= nc) {
						const unsigned int e_lo = r > 0 ? (unsigned int)__builtin_amdgcn_readlane((int)st_lo[r > 0 ? r - 1 : 0], 63) : 0u;
						const unsigned int e_hi = r > 0 ? (unsigned int)__builtin_amdgcn_readlane((int)st_hi[r > 0 ? r - 1 : 0], 63) : 0u;
						const int e_id = r > 0 ? __builtin_amdgcn_readlane(st_id[r > 0 ? r - 1 : 0], 63) : 0;
						const unsigned int s_lo = (unsigned int)wave_prev((int)st_lo[r], (int)e_lo), s_hi = (unsigned int)wave_prev((int)st_hi[r], (int)e_hi);
						const int s_id = wave_prev(st_id[r], e_id);
						const bool keep = r == ar && lane < al, put = r == ar && lane == al;
						st_lo[r] = keep ? st_lo[r] : put ? (unsigned int)rbeg : s_lo;
						st_hi[r] = keep ? st_hi[r] : put ? (unsigned int)((unsigned long long)rbeg >> 32) : s_hi;
						st_id[r] = keep ? st_id[r] : put ? new_id : s_id;
					}
				}
			}
			++nc; ++count;
		}
		WAVE_SYNC();
	}
	if (Store::NODES && iv_more && count < P.max_occ && count <= 5) { if (lane == 0) S.boost_iv = cur_iv; return 10; }   // the last interval with occurrences, same rule
	const unsigned long long lt_mask_c = (1ull << lane) - 1;
	if (!Store::NODES) {
		WAVE_SYNC();
		if (any_big) { // the same rule: an over-represented interval that started at most 5 chains would be walked further
			int acc = 0;
			for (int i = 0; i < n_iv; ++i) {
				const int v = uni(S.iv_n[i]), cnt = v & 0x1fffffff;
				if (v >> 30) {
					int heads = 0;
					for (int b = acc; b < acc + cnt; b += 64) heads += __popcll(__ballot(b + lane < acc + cnt && (S.s_extra[b + lane < acc + cnt ? b + lane : acc] & 8)));
					if (heads < P.max_occ && heads <= 5) return 10;
				}
				acc += cnt;
			}
		}
		nc_tot += nc;
		if (nc_tot + n_iso > Store::CCAP) return 3;
		// chains in the order of their start positions (the in-order traversal of the reference's tree, memchain.c:372-379)
		int n_heads = 0;
		for (int base = 0; base < n_live; base += 64) {
			const int r = base + lane;
			bool hd = false; int id = 0;
			if (r < n_live) { const int oo = S.lst[r]; hd = (S.s_extra[oo] & 8) != 0; id = (int)S.s_chain[oo]; }
			const unsigned long long b = __ballot(hd);
			if (hd) S.ord[n_heads + __popcll(b & lt_mask_c)] = (idx_t)id;
			n_heads += __popcll(b);
		}
		nc = n_heads;
		WAVE_SYNC();
	}
	RG_STAGE(2);
	// ---- D. chain order = by start position; weights; filter (mem_chain_flt, memchain.c:406-488)
	if (nc > 0) {
		for (int c = lane; c < (Store::PCAP ? n_prom : nc); c += 64) { RgChain &d = S.ch[c]; const int w = d.wq < d.wr ? d.wq : d.wr; d.w = (short)w; }
		WAVE_SYNC();
		if (Store::NODES && lane == 0) rg_bt_traverse(S, D.E);
		WAVE_SYNC();
		RG_STAGE(3);
		// chains heavy enough, in that order, as sort keys; srt[] is free until stage E: first half keys, second half the kept list
		unsigned int *keys = (unsigned int*)S.srt, *keepc = keys + Store::SCAP;
		int n = 0;
		const unsigned long long lt_mask = (1ull << lane) - 1;
		for (int base = 0; base < nc; base += 64) {
			const int i = base + lane;
			const int c = i < nc ? (int)S.ord[i] : 0;
			const int w = i < nc ? (Store::PCAP ? (c >= RG_REC ? (int)S.ch[c - RG_REC].w : (int)S.s_len[c]) : (int)S.ch[c].w) : -1;
			const bool ok = i < nc && w >= P.min_chain_weight;
			const unsigned long long b = __ballot(ok);
			// the key carries the chain (its record index, or with PCAP its position in the order by start: ids do not fit the key there)
			if (ok) keys[n + __popcll(b & lt_mask)] = (unsigned int)w << RG_KEY_BITS | (unsigned int)(Store::PCAP ? i : c);
			if (Store::PCAP && i < nc) S.keep[i] = (idx_t)c;
			n += __popcll(b);
		}
		WAVE_SYNC();
		bool sorted = false;
		constexpr int SORT_MS = Store::CCAP <= 64 ? 1 : Store::CCAP <= 128 ? 2 : Store::CCAP <= 256 ? 4 : (Store::CCAP + 63) / 64;
		if (!Store::NODES && n <= 64 * SORT_MS) { // every partition at once (rg_introsort_par): the second half of srt[] holds the partners' lists
			// (the kilobase-read tiers: lst[] is free until the kept flags are written, E[] is the tree traversal's stack, which these tiers do not have)
			rg_introsort_par<SORT_MS>(keys, n, keys + Store::SCAP, keys + Store::SCAP + Store::SCAP / 2, D.H, lane, (short*)S.lst, D.E);
			sorted = true;
		}
		WAVE_SYNC();
		if (!sorted && lane == 0) rg_introsort_keys(keys, n, D.H);
		WAVE_SYNC();
		for (int i = lane; i < n; i += 64) { const unsigned int v = keys[i] & ((1u << RG_KEY_BITS) - 1); S.ord[i] = Store::PCAP ? S.keep[v] : (idx_t)v; }
		WAVE_SYNC();
		RG_STAGE(4);
		if (n > 0 && !Store::NODES) {
			// The overlap filter (mem_chain_flt, memchain.c:430-470) with the KEPT chains' numbers in registers: kept chain k lives in lane
			// k & 63 of register set k >> 6, in the order it was kept
			constexpr int NH = (Store::CCAP + 63) / 64;
			int kb[NH], kw[NH], kpos[NH], kst[NH], kfi[NH];
#pragma unroll
			for (int h = 0; h < NH; ++h) { kb[h] = kw[h] = 0; kpos[h] = -1; kst[h] = 0; kfi[h] = -1; }
			int n_kept = 1;
			{
				// A LANE PER CANDIDATE, 64 chains of the sorted order at a time, the kept list walked entry by entry (round 4): what chain i does to
				// a kept chain k, and k to i, depends on the two alone, and i meets the kept chains in the order they were kept.  So every lane
				// first tests its chain against the list as it stands (a drop ends the lane); then the lowest lane left is the next kept chain,
				// the lanes above it meet it straight from its lane's registers, and so on until no lane is left.  chn->first of a kept chain =
				// the lowest chain that overlaps it significantly having got that far = the lowest lane that says so in the one round it is met.
				// The test itself (memchain.c:436-452) in integers: "overlap >= min_l * mask_level" in float is overlap >= T(min_l) with
				// T(l) = ceil of the float product, T grows with l so T(min(li, lk)) = min(T(li), T(lk)); T >= 1 carries "e_min > b_max" and
				// T = 0xffff "min_l >= max_chain_gap"; "w_i < w_k * drop_ratio && w_k - w_i >= 2 * min_seed_len" is w_i < D(w_k).  T and D are
				// computed once per chain, a test is a max, two min, a subtraction and two compares, and who is alive, who overlapped somebody
				// and who is met are masks of the wave in scalar registers.
				// Kept chains: kb = begin | end << 16, kw = T | D << 16 | alt << 31, km = position | state << 12 | (first + 1) << 16.
				int km[NH];
#pragma unroll
				for (int h = 0; h < NH; ++h) km[h] = 0;
				const auto flt_T = [&](int l) -> int { if (!(l < P.max_chain_gap)) return 0xffff; const int t = (int)ceilf((float)l * P.mask_level); return t < 1 ? 1 : t; };
				const auto flt_D = [&](int w) -> int { int d = (int)ceilf((float)w * P.drop_ratio); const int e = w - (P.min_seed_len << 1) + 1; d = d < e ? d : e; return d < 0 ? 0 : d > 0x7fff ? 0x7fff : d; };
				// The chains no kept chain can drop are kept whatever the list holds: a drop needs w_i < w_k * drop_ratio and w_k - w_i >= 2 *
				// min_seed_len (memchain.c:449), no kept chain is heavier than the first, and the order is by weight -- so they are a PREFIX of the
				// sorted order (all of it for a strand search on the strand the read does not come from: a hundred chance matches of weight 19-22).
				// They enter the list up front, each from its own lane (entry = sorted position); what is left to find out about them -- whether
				// they overlap an earlier one significantly (kept = 2 instead of 3) and the first chain that does so to them -- are tests of
				// pairs that do not depend on each other: a pass over the list per 64 of them, no round per kept chain.
				int U = 0;
				{
					const int d0 = flt_D((int)(uni((int)keys[0]) >> RG_KEY_BITS));
					for (int base = 0; base < n; base += 64) {
						const int i = base + lane;
						const int wi = i < n ? (int)(keys[i] >> RG_KEY_BITS) : 0;
						const unsigned long long can = __ballot(i >= n || wi < d0);
						if (can) { U = base + (int)__builtin_ctzll(can); break; }
						U = base + 64;
					}
					if (U > n) U = n;
				}
#pragma unroll
				for (int h = 0; h < NH; ++h) {
					const int i = h * 64 + lane;
					if (h * 64 < U && i < U) {
						const RgChain cu = rg_chain(S, (int)S.ord[i]);
						const int b = cu.first_q, e = (int)cu.last_q + (int)cu.last_len;
						kb[h] = b | e << 16; kw[h] = flt_T(e - b) | flt_D((int)cu.w) << 16 | (int)((unsigned int)(cu.is_alt ? 1 : 0) << 31); km[h] = i | 3 << 12;
					}
				}
				n_kept = U;
				// When that prefix is the whole list nothing is left to find out: what the tests would add -- kept = 2 for 3, and the first
				// chain overlapping each (which mem_chain_flt turns into kept = 1, memchain.c:461-464) -- only ever tells kept chains apart
				// from each other, which nothing reads unless max_chain_extend is in force (memchain.c:467-475).  That is every strand search
				// on the strand its read does not come from: half of all, and the ones with the longest lists.
				const bool all_kept = U == n && P.max_chain_extend >= (unsigned int)n;
				for (int base = 0; base < n && !all_kept; base += 64) {
					const int i = base + lane;
					const bool valid = i >= 1 && i < n;
					int ib = 0, ie = 0, iw = 0, ia = 0;
					if (valid) { const RgChain ci = rg_chain(S, (int)S.ord[i]); ib = ci.first_q; ie = (int)ci.last_q + (int)ci.last_len; iw = ci.w; ia = ci.is_alt ? 1 : 0; }
					const int ti = flt_T(ie - ib);
					const int q0v = ib | ie << 16, q1v = ti | flt_D(iw) << 16 | (int)((unsigned int)ia << 31);
					unsigned long long live_m = __ballot(valid), large_m = 0;
					const unsigned long long pre_m = __ballot(i < U), alt_m = __ballot(ia != 0);   // pre: in the list already, meets the entries before its own
					const int k_end = base + 64 <= U ? base + 64 : n_kept;
					for (int k = 0; k < k_end; ++k) { // the list as it stands
						unsigned int p0 = 0, p1 = 0;
						const int kh = k >> 6, kl = k & 63;
#pragma unroll
						for (int h = 0; h < NH; ++h) if (h == kh) { p0 = (unsigned int)__builtin_amdgcn_readlane(kb[h], kl); p1 = (unsigned int)__builtin_amdgcn_readlane(kw[h], kl); }
						const int kbk = (int)(p0 & 0xffff), kek = (int)(p0 >> 16), tk = (int)(p1 & 0xffff), dk = (int)((p1 >> 16) & 0x7fff);
						const int ov = (kek < ie ? kek : ie) - (kbk > ib ? kbk : ib), tm = ti < tk ? ti : tk;
						unsigned long long hm = __ballot(ov >= tm) & live_m;
						if (k >= base) hm &= ~pre_m | (k - base < 63 ? ~0ull << (k - base + 1) : 0ull);
						if (p1 >> 31) hm &= alt_m;
						large_m |= hm;
						if (hm) {
							const int f = base + (int)__builtin_ctzll(hm);
#pragma unroll
							for (int h = 0; h < NH; ++h) if (h == kh) { if (lane == kl && !(km[h] >> 16)) km[h] |= (f + 1) << 16; }
							live_m &= ~(hm & __ballot(iw < dk));
						}
					}
					if (base < U) { // the entries of this batch's own lanes: kept = 2 when they overlap an earlier one
						const bool two = ((pre_m & live_m & large_m) >> lane) & 1;
#pragma unroll
						for (int h = 0; h < NH; ++h) if (h == base >> 6) { if (two) km[h] = (km[h] & ~(3 << 12)) | 2 << 12; }
					}
					unsigned long long um = live_m & ~pre_m;
					while (um) {
						const int l = (int)__builtin_ctzll(um);   // kept: the next entry of the list
						const unsigned int p0 = (unsigned int)__builtin_amdgcn_readlane(q0v, l), p1 = (unsigned int)__builtin_amdgcn_readlane(q1v, l);
						const int kbk = (int)(p0 & 0xffff), kek = (int)(p0 >> 16), tk = (int)(p1 & 0xffff), dk = (int)((p1 >> 16) & 0x7fff);
						const int ov = (kek < ie ? kek : ie) - (kbk > ib ? kbk : ib), tm = ti < tk ? ti : tk;
						unsigned long long hm = __ballot(ov >= tm) & live_m & (l < 63 ? ~0ull << (l + 1) : 0ull);
						if (p1 >> 31) hm &= alt_m;
						large_m |= hm;
						const unsigned long long dm = hm ? hm & __ballot(iw < dk) : 0ull;
						live_m &= ~dm;
						const int meta = (base + l) | (((large_m >> l) & 1) ? 2 : 3) << 12 | (hm ? base + (int)__builtin_ctzll(hm) + 1 : 0) << 16;
						const int sl = n_kept & 63, hi = n_kept >> 6;
#pragma unroll
						for (int h = 0; h < NH; ++h) if (h == hi) { if (lane == sl) { kb[h] = (int)p0; kw[h] = (int)p1; km[h] = meta; } }
						++n_kept;
						um &= ~dm & ~(1ull << l);
					}
				}
#pragma unroll
				for (int h = 0; h < NH; ++h) { kpos[h] = km[h] & 0xfff; kst[h] = (km[h] >> 12) & 3; kfi[h] = (km[h] >> 16) - 1; }
			}
			// kept flags by sorted position (PCAP: lst is free here), then the first chain each kept one shadows (chn->first, memchain.c:455-460)
			for (int j = lane; j < n; j += 64) { if (Store::PCAP) S.lst[j] = 0; else S.ch[S.ord[j]].kept = 0; }
			WAVE_SYNC();
#pragma unroll
			for (int h = 0; h < NH; ++h) if (lane + 64 * h < n_kept) { if (Store::PCAP) S.lst[kpos[h]] = (idx_t)kst[h]; else S.ch[S.ord[kpos[h]]].kept = (signed char)kst[h]; }
			WAVE_SYNC();
#pragma unroll
			for (int h = 0; h < NH; ++h) if (lane + 64 * h < n_kept && kfi[h] >= 0) { if (Store::PCAP) S.lst[kfi[h]] = 1; else S.ch[S.ord[kfi[h]]].kept = 1; }
			WAVE_SYNC();
		} else if (n > 0) {
			int nk = 1;
			if (lane == 0) { S.ch[S.ord[0]].kept = 3; S.keep[0] = 0; keepc[0] = S.ord[0]; }
			WAVE_SYNC();
			// no chain light enough for the heaviest one to drop it (memchain.c:449): then none is dropped by anybody, every chain is kept, and
			// the pair tests would only tell kept chains apart (2 for 3, `first`), which nothing reads unless max_chain_extend is in force
			bool all_kept = false;
			if (P.max_chain_extend >= (unsigned int)n) {
				const int w0 = (int)(uni((int)keys[0]) >> RG_KEY_BITS), wl = (int)(uni((int)keys[n - 1]) >> RG_KEY_BITS);
				all_kept = !((float)wl < (float)w0 * P.drop_ratio && w0 - wl >= P.min_seed_len << 1);
				if (all_kept) { for (int j = lane; j < n; j += 64) S.ch[S.ord[j]].kept = 3; WAVE_SYNC(); }
			}
			for (int i = 1; i < n && !all_kept; ++i) {
				// chain i against the kept chains, 64 at a time; the reference's loop stops at the first kept chain that drops it
				const int cidx = uni(S.ord[i]);
				const RgChain ci = S.ch[cidx];
				int stop = nk;
				for (int base = 0; base < nk && stop == nk; base += 64) {
					const int k = base + lane;
					const int r = k < nk ? rg_flt_test(P, ci, S.ch[keepc[k]]) : 0;
					const unsigned long long d = __ballot(r & 2);
					if (d) stop = base + __ffsll((long long)d) - 1;
				}
				int large = 0;
				for (int base = 0; base < nk && base <= stop; base += 64) {
					const int k = base + lane;
					int hit = 0;
					if (k < nk && k <= stop) { RgChain &ck = S.ch[keepc[k]]; hit = rg_flt_test(P, ci, ck) & 1; if (hit && ck.first < 0) ck.first = (short)i; }
					if (__ballot(hit)) large = 1;
				}
				if (stop == nk) {
					if (lane == 0) { S.keep[nk] = (idx_t)i; keepc[nk] = (unsigned int)cidx; S.ch[cidx].kept = large ? 2 : 3; }
					++nk;
				}
				WAVE_SYNC();
			}
			for (int k = lane; k < nk; k += 64) { const int f = S.ch[keepc[k]].first; if (f >= 0) S.ch[S.ord[f]].kept = 1; }
			WAVE_SYNC();
		}
		if (n > 0) {
			if (P.max_chain_extend < (unsigned int)n) { // at most max_chain_extend shadowed chains survive (memchain.c:474-482); off by default
				if (lane == 0) {
					int i; unsigned int k = 0;
					for (i = 0; i < n; ++i) { const int kp = Store::PCAP ? (int)S.lst[i] : (int)S.ch[S.ord[i]].kept; if (kp == 0 || kp == 3) continue; if (++k >= P.max_chain_extend) break; }
					for (; i < n; ++i) { if (Store::PCAP) { if (S.lst[i] < 3) S.lst[i] = 0; } else if (S.ch[S.ord[i]].kept < 3) S.ch[S.ord[i]].kept = 0; }
				}
				WAVE_SYNC();
			}
			int m = 0;   // surviving chains, in processing order, compacted in place (targets never pass the sources)
			for (int base = 0; base < n; base += 64) {
				const int i = base + lane;
				const int c = i < n ? (int)S.ord[i] : 0;
				const bool ok = i < n && (Store::PCAP ? S.lst[i] != 0 : S.ch[c].kept != 0);
				const unsigned long long b = __ballot(ok);
				WAVE_SYNC();
				if (ok) S.ord[m + __popcll(b & lt_mask)] = (idx_t)c;
				m += __popcll(b);
				WAVE_SYNC();
			}
			if (lane == 0) S.n_chains = m;
			WAVE_SYNC();
		}
	}
	RG_STAGE(5);
	if (SPLIT) { // the chain-to-region loop runs in k_c2r
		const int st = rg_export(S, task_id, tot, frac_rep, *X, lane, flt);
		RG_STAGE(6);
		return st;
	}
	// ---- E. chains -> regions (mem_chain2region, memchain.c:873-904)
	const int nk = uni(S.n_chains), ns = tot;
	unsigned int pf_seen = 0, pf_skip = 0, pf_inl = 0;
	for (int ci = 0; ci < nk; ++ci) {
		const int c = uni(S.ord[ci]);
		const RgChain chn = S.ch[c];
		const long long ch_pos = uni64(chn.pos);
		const int ch_has_extra = uni(chn.n_extra) != 0;
		const int single = uni(chn.n_seeds) == 1;
		const int seed0 = uni(chn.seed0);
		// a chain of one seed that fails asymmetric_flt_seed, with no contained seeds to fall back to, comes and goes without a trace:
		// most chains of a strand search against the wrong conversion are such
		if (single && !ch_has_extra && (uni(S.s_extra[seed0]) & 2)) continue;
		// mem_chain_reference_span (memchain.c:585-605) + bns_fetch_seq's contig clamp; one lane per seed
		int64_t rmax0 = l_pac << 1, rmax1 = 0;
		if (single) {
			const long long rb = uni64(S.s_rbeg[seed0]); const int qb = uni(S.s_qbeg[seed0]), ln = uni(S.s_len[seed0]);
			c2r_seed_span(rb, qb, ln, l_query, rg_gap(gap, P, qb), rg_gap(gap, P, l_query - qb - ln), &rmax0, &rmax1);
		} else {
			for (int o = lane; o < ns; o += 64) if (S.s_chain[o] == c && !(S.s_extra[o] & 1)) {
				const long long rb = S.s_rbeg[o]; const int qb = S.s_qbeg[o], ln = S.s_len[o];
				int64_t b, e;
				c2r_seed_span(rb, qb, ln, l_query, rg_gap(gap, P, qb), rg_gap(gap, P, l_query - qb - ln), &b, &e);
				rmax0 = rmax0 < b ? rmax0 : b; rmax1 = rmax1 > e ? rmax1 : e;
			}
			rmax0 = uni64(-wave_max_i64(-rmax0)); rmax1 = uni64(wave_max_i64(rmax1));
		}
		const int rid = uni(chn.rid);   // a chain's seeds share the contig of its first one (memchain.c:232)
		c2r_clamp_window(&rmax0, &rmax1, l_pac, ch_pos, uni64(ctg[rid]), uni64(ctg[rid + 1]));
		const int n0 = uni(S.n_regs);
		int win_ok = 0;   // 0: not loaded yet, 1: in LDS, -1: too long for it
		for (int pass = 0; pass < 2; ++pass) {
			if (pass == 1 && !(uni(S.n_regs) == n0 && ch_has_extra)) break;
			// the list (seeds or seeds_extra) in arrival order, and its best-first order
			int nl = 0;
			if (single && pass == 0) {
				if (lane == 0) { S.lst[0] = (idx_t)seed0; S.srt[0] = (unsigned long long)(unsigned)S.s_len[seed0] << 32; }
				nl = 1;
				WAVE_SYNC();
			} else {
				for (int base = 0; base < ns; base += 64) {
					const int o = base + lane;
					const bool in = o < ns && S.s_chain[o] == c && (int)(S.s_extra[o] & 1) == pass;
					const unsigned long long b = __ballot(in);
					if (in) S.lst[nl + __popcll(b & ((1ull << lane) - 1))] = (idx_t)o;
					nl += __popcll(b);
				}
				WAVE_SYNC();
				for (int i = lane; i < nl; i += 64) { // keys score<<32|i are unique: rank by counting
					const unsigned long long key = (unsigned long long)(unsigned)S.s_len[S.lst[i]] << 32 | (unsigned)i;
					int r = 0;
					for (int k = 0; k < nl; ++k) r += ((unsigned long long)(unsigned)S.s_len[S.lst[k]] << 32 | (unsigned)k) < key;
					S.srt[r] = key;
				}
				WAVE_SYNC();
			}
			for (int k = nl - 1; k >= 0; --k) {
				const int si = uni((int)(uint32_t)S.srt[k]);
				const int o = uni(S.lst[si]);
				if (uni(S.s_extra[o]) & 2) continue;   // asymmetric_flt_seed (memchain.c:138-149), tested for every seed after stage B
				const long long s_rbeg = uni64(S.s_rbeg[o]); const int s_qbeg = uni(S.s_qbeg[o]), s_len = uni(S.s_len[o]);
				++pf_seen;
				// contained in a region of this strand search, and no later seed of the list disagrees? (memchain.c:761-819)
				const auto seed_at = [&](int i, long long &t_rbeg, int &t_qbeg, int &t_len) { const int oo = S.lst[i]; t_rbeg = S.s_rbeg[oo]; t_qbeg = S.s_qbeg[oo]; t_len = S.s_len[oo]; };
				const int nr = uni(S.n_regs);
				const int u = rg_first_container(S.regs, nr, s_rbeg, s_qbeg, s_len, l_query, gap, P, lane);
				if (u < nr && !rg_later_disagrees(S.srt, k, nl, s_rbeg, s_qbeg, s_len, lane, seed_at)) { ++pf_skip; WAVE_SYNC(); if (lane == 0) S.srt[k] = 0; WAVE_SYNC(); continue; }
				++pf_inl;
				if (win_ok == 0) { // the chain's reference window (bns_fetch_seq, memchain.c:889) into LDS, once, when a seed of it is first extended
					const int span = (int)(rmax1 - rmax0);
					if (span > 0 && span <= RG_WIN) {
						dev_fetch_window(D.win, ix.pac, l_pac, rmax0, span, lane);
						win_ok = 1;
						WAVE_SYNC();
					} else win_ok = -1;
				}
				// (the stopping rule is counted in every instantiation of the tiers, which have no tallying form: the counter block's address is
				// null unless $BSX_PHASES is on, and counting costs these kernels no register, profiles/ext_stop_measurements.md)
				bsx_region_t R; int aw0, aw1;
				rg_region_open(R, aw0, aw1, P.w, rid);
				rg_ext_seed<PK, RG_QCAP, false, XS_FAM_TIER>(R, aw0, aw1, D, ix, sc, P, reads, qoff, l_query, parent, s_rbeg, s_qbeg, s_len, rmax0, rmax1, win_ok, lane, pf_t, pf_ext, pf_rows);
				if (rg_push_region(R, aw0, aw1, s_len, frac_rep, parent, l_pac, nl, seed_at, S.regs, S.n_regs, Store::RCAP, lane)) return 6;
			}
		}
	}
	RG_STAGE(6);
	if (P.prof) { RG_PF_ADD(D, 8, pf_ext); RG_PF_ADD(D, 9, pf_rows); RG_PF_ADD(D, 11, pf_seen); RG_PF_ADD(D, 12, pf_skip); RG_PF_ADD(D, 14, pf_inl); }
	return 0;
#undef RG_STAGE
}
