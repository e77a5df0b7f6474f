// ctr_layout.hpp -- the one layout of a lane's counter block (Lane::small in shim.hip: SMALL_BYTES of HBM, addressed as 64-bit slots).
// Two kinds of tenant.  Profiling and work slots: kernels add to counters[NAME] (the launchers hand them the block's base, or the base of
// one of the two later seeding passes' blocks); the values below are part of the device code.  Cursors and counts: the host passes each as a
// pointer of its own, so they are fields of the plain structs at the end, placed in the gaps between the profiling ranges.
// The static_asserts at the bottom show that no two tenants overlap and that everything ends below SMALL_BYTES.
#pragma once
#include <stddef.h>

#define SMALL_BYTES 4096

enum CtrSlot {
	CTR_FM_SLOW = 0, CTR_FM_FAST = 1,                 // FM blocks read by the seeding kernels (two per slow step, one per fast one)
	CTR_LF_STEPS = 2, CTR_LF_CALLS = 3,               // suffix-array lookups: LF steps walked, lookups made
	CTR_STAGE = 32, CTR_STAGE_N = 16,                 // $BSX_PHASES: wave cycles by stage of the region kernels (RG_PF_FLUSH: CTR_STAGE + k) ...
	CTR_STAGE_SEEDSW = 42,                            // ... of which [10]: alignments of the seed filter
	CTR_SEED_CYC = 48, CTR_SEED_COLD = 49, CTR_SEED_PUB = 50, CTR_SEED_TRIPS = 51, CTR_SEED_COLD_N = 52,   // seeding: wave cycles, in the full machine, publishing; wave trips; passes
	CTR_SEED_N = 8,                                   // (read and zeroed as eight slots)
	CTR_EXT = 56, CTR_EXT_N = 11,                     // k_ext4 ([0..5]) and k_extl ([6..10]) add to prof[k], prof = counters + CTR_EXT
	CTR_SEED_HIST = 60, CTR_SEED_HIST_N = 20,         // second pass only (block CTR_SEED2): strand searches by requests made, CTR_SEED_HIST + k; that block has no CTR_EXT
	CTR_TIER2_TIME = 110, CTR_TIER3_TIME = 114,       // the HBM tiers' strand searches: [0] longest [1] sum [2] number [3] busiest wave
	CTR_TIER_TIME_N = 4,
	CTR_OVERFLOW = 119,                               // strand searches a seeding pass leaves with a negative count
	CTR_TAB_LOOKUPS = 120,                            // entries of the k-mer table read
	CTR_SEEDT_HOT = 121, CTR_SEEDT_FETCH = 122, CTR_SEEDT_POST = 123, CTR_SEEDT_REQ = 124, CTR_SEEDT_N = 4,   // k_seedt's phases
	CTR_T3_LONGEST = 128, CTR_T3_HIST = 130, CTR_T3_HIST_N = 22,   // the last tier: its longest strand search (packed), strand searches by duration
	CTR_T3_N = 24,                                    // (the record, a spare slot, the histogram: read and zeroed together)
	CTR_HANDON = 160, CTR_HANDON_N = 12,              // $BSX_PHASES=2: why a tier hands a strand search on, CTR_HANDON + status
	CTR_X4W = 176, CTR_X4W_N = 8,                     // $BSX_PHASES: extensions made ahead that the seed loop never read, CTR_X4W + 4 * kernel + CtrX4w
	CTR_SEED2 = 256, CTR_SEED3 = 384,                 // bases of the blocks of the second seeding pass inside the sequence / of the one on the side stream
	CTR_SEED_BLOCK_N = 125,                           // a seeding pass reaches up to CTR_SEEDT_REQ of its block
	// where the cursor structs below live
	CTR_SHARED = 4, CTR_MAIN = 11, CTR_SIDE = 80,
	CTR_MD_CURSOR = 30                                // the back half's MD pool cursor (bsx_global_batch with tags), a slot of its own
};

// what k_ext4 / k_extl add to, relative to CTR_EXT
enum CtrExt { EXT4_JOBS = 0, EXT4_ROWS = 1, EXT4_TRIPS = 2, EXT4_COLD = 3, EXT4_SLOTS = 4, EXT4_NARROW_ROWS = 5,
              EXTL_JOBS = 6, EXTL_ROWS = 7, EXTL_TRIPS = 8, EXTL_COLD = 9, EXTL_SENT_ON = 10 };

// what rg_c2r adds to when the first seed it reaches in a chain's main list is skipped as contained while a valid extension made ahead lay in
// the chain's slot: relative to CTR_X4W + 4 * k, k = 0 the job ran in k_ext4, 1 in k_extl
enum CtrX4w { X4W_JOBS = 0, X4W_ROWS = 1, X4W_JOBS_R0 = 2, X4W_ROWS_R0 = 3 };   // _R0: of which contained in the strand search's first region

// the cursors every launch of a chunk shares
struct CtrShared {
	struct Seed { unsigned long long intv_cursor; unsigned int task_cursor, pad_; } seed;   // the interval pool's bump cursor; the first seeding pass's task cursor (lane_seed_batch zeroes the pair)
	unsigned int seed2_task_cursor, pad2_;   // the merged second pass's (it used to borrow the side sequence's)
	unsigned long long region_cursor;        // the region pool's
	unsigned long long k3_cursor;            // the position pool's (launch_occ); what it reaches is the chunk's occurrence count
	unsigned long long xpool_cursor;         // the export pool's
	struct Early3 { unsigned int count, cursor; } early3;   // the last HBM tier beside the others: what launch_occ lists for it (zeroed apart: everything before it goes in one)
};

// one tier sequence's own counts and cursors; two instances, the chunk's (CTR_MAIN) and the side stream's (CTR_SIDE)
struct TierCtr {
	struct Front {   // zeroed before the sequence starts
		unsigned long long k3_start;         // side sequence: where its ranks start in the position pool
		unsigned int seed_task_cursor;       // side sequence: the cursor of the seeding pass that feeds it
		unsigned int t1_cursor;
		unsigned int ra_count, t1b_cursor;   // what tier 1 hands on, and the cursor of the tier that takes it
		unsigned int rm_count, t1c_cursor;   // ... tier 1b
		unsigned int rl_count;               // ... tier 1c
		unsigned int t2_cursor;
		unsigned int rb_count, t3_cursor;    // what tier 2 hands on
		unsigned int ssw_prep_cursor, ssw_jobs, ssw_apply_cursor;   // the seed filter (the job count and the apply cursor are handed over as a pair)
		unsigned int x_count, c2r_cursor;    // exported strand searches, and the chains -> regions launch over them
		unsigned int rc_count, c2r2_cursor;  // what that launch declines, and the second launch's cursor
		unsigned int pad_;
	} front;
	struct Late {    // zeroed apart: the launches between the second chains -> regions launch and the last HBM tier
		unsigned int rh_count, c2r3_cursor;  // what the second declines, the third's cursor
		unsigned int x2_count, c2r_t2_cursor;   // tier2_export: what the first HBM tier exports, and chains -> regions over that
		unsigned int rf_count, t2_full_cursor;  // ... what takes the tier's full form
		unsigned int t2_export_cursor, pad_;    // ... the exporting launch
	} late;
	unsigned int x4[4], x4_t2[4];            // launch_x4's job counters (zeroed by the launcher): for the LDS tiers' exports, for tier 2's
};

// ---- nothing overlaps -------------------------------------------------------------------------------------------------------------------
struct CtrRange { int lo, hi; };   // u64 slots [lo, hi)
constexpr int ctr_slots(size_t bytes) { return (int)((bytes + 7) / 8); }
constexpr CtrRange ctr_ranges[] = {
	{CTR_FM_SLOW, CTR_LF_CALLS + 1},
	{CTR_SHARED, CTR_SHARED + ctr_slots(sizeof(CtrShared))},
	{CTR_MAIN, CTR_MAIN + ctr_slots(sizeof(TierCtr))},
	{CTR_MD_CURSOR, CTR_MD_CURSOR + 1},
	{CTR_STAGE, CTR_STAGE + CTR_STAGE_N},
	{CTR_SEED_CYC, CTR_SEED_CYC + CTR_SEED_N},
	{CTR_EXT, CTR_EXT + CTR_EXT_N},
	{CTR_SIDE, CTR_SIDE + ctr_slots(sizeof(TierCtr))},
	{CTR_TIER2_TIME, CTR_TIER2_TIME + CTR_TIER_TIME_N},
	{CTR_TIER3_TIME, CTR_TIER3_TIME + CTR_TIER_TIME_N},
	{CTR_OVERFLOW, CTR_OVERFLOW + 1},
	{CTR_TAB_LOOKUPS, CTR_TAB_LOOKUPS + 1},
	{CTR_SEEDT_HOT, CTR_SEEDT_HOT + CTR_SEEDT_N},
	{CTR_T3_LONGEST, CTR_T3_LONGEST + CTR_T3_N},
	{CTR_HANDON, CTR_HANDON + CTR_HANDON_N},
	{CTR_X4W, CTR_X4W + CTR_X4W_N},
	{CTR_SEED2, CTR_SEED2 + CTR_SEED_BLOCK_N},
	{CTR_SEED3, CTR_SEED3 + CTR_SEED_BLOCK_N},
};
constexpr bool ctr_ranges_ok()
{
	constexpr int n = (int)(sizeof(ctr_ranges) / sizeof(ctr_ranges[0]));
	for (int i = 0; i < n; ++i) {
		if (ctr_ranges[i].lo < 0 || ctr_ranges[i].lo >= ctr_ranges[i].hi || ctr_ranges[i].hi * 8 > SMALL_BYTES) return false;
		for (int j = 0; j < i; ++j) if (ctr_ranges[i].lo < ctr_ranges[j].hi && ctr_ranges[j].lo < ctr_ranges[i].hi) return false;
	}
	return true;
}
static_assert(ctr_ranges_ok(), "the lane's counter block: two tenants overlap, or one ends beyond SMALL_BYTES");
static_assert(sizeof(CtrShared) % 8 == 0 && sizeof(TierCtr) % 8 == 0 && sizeof(TierCtr::Front) % 8 == 0, "cursor structs are whole 64-bit slots");
static_assert(CTR_SEED_HIST + CTR_SEED_HIST_N <= CTR_TIER2_TIME && CTR_SEEDT_REQ < CTR_SEED_BLOCK_N, "a later seeding pass's block holds its histogram and phases");
static_assert(CTR_T3_HIST + CTR_T3_HIST_N <= CTR_T3_LONGEST + CTR_T3_N && CTR_STAGE_SEEDSW < CTR_STAGE + CTR_STAGE_N && CTR_SEED_COLD_N < CTR_SEED_CYC + CTR_SEED_N, "sub-slots lie inside their ranges");
// the values are what the kernels were built with: moving one changes device code
static_assert(CTR_FM_SLOW == 0 && CTR_FM_FAST == 1 && CTR_LF_STEPS == 2 && CTR_LF_CALLS == 3, "");
static_assert(CTR_STAGE == 32 && CTR_STAGE_SEEDSW == 42 && CTR_STAGE + CTR_STAGE_N - 1 == 47, "");
static_assert(CTR_SEED_CYC == 48 && CTR_SEED_COLD == 49 && CTR_SEED_PUB == 50 && CTR_SEED_TRIPS == 51 && CTR_SEED_COLD_N == 52, "");
static_assert(EXT4_JOBS == 0 && EXT4_NARROW_ROWS == 5 && EXTL_JOBS == 6 && EXTL_SENT_ON + 1 == CTR_EXT_N, "");
static_assert(CTR_EXT == 56 && CTR_EXT + CTR_EXT_N - 1 == 66 && CTR_SEED_HIST == 60, "");
static_assert(CTR_TIER2_TIME == 110 && CTR_TIER3_TIME == 114 && CTR_TIER3_TIME + CTR_TIER_TIME_N - 1 == 117, "");
static_assert(CTR_OVERFLOW == 119 && CTR_TAB_LOOKUPS == 120, "");
static_assert(CTR_SEEDT_HOT == 121 && CTR_SEEDT_FETCH == 122 && CTR_SEEDT_POST == 123 && CTR_SEEDT_REQ == 124, "");
static_assert(CTR_X4W == 176 && CTR_X4W_N == 8 && X4W_JOBS == 0 && X4W_ROWS == 1 && X4W_JOBS_R0 == 2 && X4W_ROWS_R0 == 3, "");
static_assert(CTR_T3_LONGEST == 128 && CTR_T3_HIST == 130 && CTR_HANDON == 160 && CTR_SEED2 == 256 && CTR_SEED3 == 384, "");
