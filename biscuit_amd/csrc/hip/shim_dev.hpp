// shim_dev.hpp -- what the units of the shim share, private to the library: shim.hip (the device, the index, the transfers, the counters, the
// seeding / regions / alignment batches, the vtable) and shim_tables.hip (the output passes that run while aligning).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <mutex>
#include "devbuf.hpp"
#include "kernels.h"
#include "tune.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "[bsx-hip] %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return BSX_E_NODEVICE; } } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != BSX_OK) return rc_; } while (0)

// One lane = one HIP stream with its own staging: a chunk is bound to a lane for its whole life, so the front half
// (seeding .. regions) of one chunk and the back half (merge .. SAM) of the previous one can be in flight together.
#define BSX_LANES 6
// the slots of bsx_device_kernel_time: the chunk-wide seeding pass, the suffix-array lookups, the DP batches (extensions, local alignments,
// global alignments), tier 1, the later tiers, seeding outside the chunk-wide launch (the batch form, the merged second pass)
enum KTime { KT_SEED = 0, KT_K3 = 1, KT_EXTEND = 2, KT_SW = 3, KT_GLOBAL = 4, KT_TIER1 = 5, KT_TIERS_LATER = 6, KT_SEED_OTHER = 7, KT_N = 8 };
struct Lane {
	hipStream_t st = nullptr;      // front-half kernels (low priority)
	hipEvent_t ev_seed_done = nullptr, ev_regions_done = nullptr;   // what the next chunk's launches of the same stage wait for
	hipStream_t st_hi = nullptr;   // back-half kernels (K5, K6): high priority, so that they get compute units while another chunk's front half runs
	hipEvent_t ev_timed_begin = nullptr, ev_timed_end = nullptr;   // around the launch finish_timed times; in a regions batch: around the chunk-wide seeding pass
	hipEvent_t ev_seed2_begin = nullptr, ev_seed2_end = nullptr;   // regions batch: around the second seeding pass inside the main sequence (recorded back to back when there is none)
	hipEvent_t ev_occ_end = nullptr, ev_tier1_end = nullptr, ev_tiers_end = nullptr;   // ... behind the suffix-array lookups, behind tier 1, behind everything of the main sequence
	hipEvent_t tier_ev[12] = {};   // $BSX_PHASES: between the region launches
	hipStream_t st_cp = nullptr;   // unmasked: the front half's small copies (xfer)
	hipEvent_t ev_cp = nullptr;
	hipStream_t st3 = nullptr;     // the last HBM tier of what is known to need it when the occurrences are counted: beside the chunk's other tiers
	hipEvent_t ev_t3a = nullptr, ev_t3b = nullptr;
	hipStream_t st2 = nullptr;     // side stream of the front half: seeding redone with larger lists while the region kernels run
	DevScoring sc;         // set by set_opt on this lane; read by every launch of this lane
	DevBuf reads; size_t n_reads = 0;
	DevBuf gath;             // lists gathered for the download of strand searches the caller takes back
	DevBuf qpack;            // the chunk's reads as base-3 digits for the seeding kernel (k_seedt.hip)
	int64_t rb_tasks = 0;    // strand searches of the last regions batch (their regions, offsets and counts are still in regs / regmeta)
	int flt_key[3] = {-1, -1, -1};   // what fltab was made for
	DevBuf fltab, jobs, res, scratch, scratch2, out, aux, pool, regs, regmeta, slabs, slabs3, slabflags, redo, pos, posoff, xpool, xmeta, x4jobs, tags, mdpool, gctx, qcjobs, qcpool, mdkeys, mdres, mdslot, dd, sswjobs, c2rslab;
	DevBuf xstop;          // the counters of the extensions' stopping rule (ext_stop.hpp), XS_N words per launch family
	DevBuf small;          // the counter block: SMALL_BYTES laid out by ctr_layout.hpp
	HostBuf hstage;        // pinned staging for bulk results
	HostBuf pin;           // two pinned halves through which large host<->device copies are streamed
	hipEvent_t pev[2] = {nullptr, nullptr};
	// strand searches being seeded again on the side stream while the caller goes on (lane_regions_finish collects them)
	struct {
		bool active = false;
		std::vector<int64_t> tasks;            // their indices in the chunk
		std::vector<bsx_seed_task_t> sub;      // kept alive for the asynchronous upload
		unsigned int n2u = 0;
		HostBuf hres;                          // pinned: region offsets (8 B each) then counts (4 B each)
		hipEvent_t ev = nullptr, ev_tiers = nullptr;
		unsigned long long used_main = 0;      // regions the caller already holds
		unsigned long long regs_cap = 0;       // size of the device's region pool for this chunk
	} rs;
	double k_ms[KT_N] = {0, 0, 0, 0, 0, 0, 0, 0};   // by KTime
	int64_t k_launch[KT_N] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint64_t work[5] = {0, 0, 0, 0, 0};   // the region kernels' work since the last reset: strand searches, SA intervals, occurrences, regions, read bases
	// what the last de-duplication of this lane left in `dd` (k_msw.hip reads the reads' lists from there): layout and validity
	struct { bool valid = false; int64_t n_reads = 0; int per_read = 0; size_t o_idx = 0, o_off = 0, o_pool = 0; bool with_long = false; } ddl;
	DevBuf msw_jobs, msw_res, msw_meta, msw_roff; int64_t msw_token = -1;
	std::mutex hi_mu;      // the back half's batches (K5, K6) of this lane, one at a time: the slices of a chunk's back half call them from two threads
	long last_overflow = -1;   // strand searches the first seeding pass of this lane's last chunk left to the second (-1: no chunk yet)
	double seed2_ms = 0; int64_t seed2_launches = 0; uint64_t seed2_tasks = 0;   // the second seeding pass inside the chunk's sequence (its own launch, its own counters: CTR_SEED2)
	void release_buffers()   // every buffer of the lane but rs.hres; a buffer that is not in this list leaks when the device is closed
	{
		DevBuf *b[] = {&reads, &gath, &qpack, &fltab, &jobs, &res, &scratch, &scratch2, &out, &aux, &pool, &regs, &regmeta, &slabs, &slabs3, &slabflags, &redo, &pos, &posoff, &xpool, &xmeta,
		               &x4jobs, &tags, &mdpool, &gctx, &qcjobs, &qcpool, &mdkeys, &mdres, &mdslot, &dd, &sswjobs, &c2rslab, &small, &xstop, &msw_jobs, &msw_res, &msw_meta, &msw_roff};
		for (DevBuf *x : b) x->release();
		hstage.release(); pin.release(); flt_key[0] = -1;
	}
};
// The seeding launches of a chunk count their FM blocks and table entries in blocks of their own, so that each pass's bytes can be put over
// that pass's time (bsx_device_seed_passes): CTR_FM_SLOW, CTR_FM_FAST, CTR_TAB_LOOKUPS of the lane's counter block (ctr_layout.hpp) for the chunk-wide
// first pass (and the batch form), the same three from CTR_SEED2 for the second pass inside the sequence, from CTR_SEED3 for the few seeded again
// on the side stream.

// The state of each output pass (shim_tables.hip), one struct per pass: what it keeps on the device between calls, its mutex (taken after the
// lane's hi_mu where both are held) and release(), the only place that frees the pass's memory, destroys its stream and resets its bookkeeping.
// The pass's reset calls it under the mutex once the device is idle, bsx_device_close without.
static inline void dev_free(void *p) { if (p) (void)hipFree(p); }
static inline void stream_release(hipStream_t &st) { if (st) (void)hipStreamDestroy(st); st = nullptr; }
struct QcState {   // the BISCUITqc column counts of every lane's batches (k_qc.hip): a bsx_qc_counts_t, zeroed when made and by bsx_qc_read(reset)
	DevBuf counts; std::mutex mu;
	void release() { counts.release(); }
};
struct CovState {   // the depth state of the coverage tables (k_cov.hip): the difference array (made and zeroed on first use) and the two optional masks
	void *diff = nullptr; uint32_t *mask[2] = {nullptr, nullptr}; std::mutex mu;
	void release() { dev_free(diff); dev_free(mask[0]); dev_free(mask[1]); diff = nullptr; mask[0] = mask[1] = nullptr; }
};
struct MethState {   // the counters of the base-averaged conversion table (k_meth.hip): two 64-bit words per position, made and zeroed on first use
	void *st = nullptr; std::mutex mu;
	void release() { dev_free(st); st = nullptr; }
};
struct MarkdupState {   // the table of template keys (k_markdup.hip): made by the first bsx_markdup_batch, doubled as it fills
	MdSlot *tab = nullptr; uint64_t slots = 0, used = 0; std::mutex mu;
	void release() { dev_free(tab); tab = nullptr; slots = used = 0; }
};
struct SortState {   // the sorted runs of record keys (k_sort.hip), one block per bsx_sort_run; the sort's own stream (the writer thread sorts a finished
	// chunk while the lanes align the next ones) and its working buffers
	std::vector<std::pair<uint64_t*, int64_t>> runs;
	hipStream_t st = nullptr;
	DevBuf k[2], p[2], counts, btot;
	std::mutex mu;
	void release() { for (auto &r : runs) dev_free(r.first); runs.clear(); for (DevBuf *x : {&k[0], &k[1], &p[0], &p[1], &counts, &btot}) x->release(); stream_release(st); }
};
struct BamState {   // --bam (k_bam.hip, k_bgzf.hip): the writer's stream (the writer thread encodes a finished chunk while the lanes align the next ones),
	// the name table of the writer's header (uploaded once: tab_serial says whose it is) and the working buffers of both stages
	hipStream_t st = nullptr;
	uint64_t tab_serial = 0;
	DevBuf names, noff, nid, text, cnt, start, size, bad, pay, err;
	DevBuf bz_in, bz_tok, bz_cand, bz_slots, bz_sizes, bz_out, bz_ops; bool bz_ops_ok = false;
	std::mutex mu;
	void release()
	{
		for (DevBuf *x : {&names, &noff, &nid, &text, &cnt, &start, &size, &bad, &pay, &err, &bz_in, &bz_tok, &bz_cand, &bz_slots, &bz_sizes, &bz_out, &bz_ops}) x->release();
		tab_serial = 0; bz_ops_ok = false; stream_release(st);
	}
};

struct bsx_device {
	int ordinal = 0;
	char name[256];
	int n_cu = 0;
	DevIndex ix; bool has_index = false;
	DevBuf bwt[2], sa[2], pac, ctg, holes, seedtab[2];
	QcState qc; CovState cov; MethState meth; MarkdupState md; SortState sort; BamState bam;   // the output passes (shim_tables.hip)
	Lane lane[BSX_LANES];   // scoring matrices and penalties are per lane (Lane::sc): chunks with different options may be in flight together
	// Front halves of consecutive chunks are chained stage by stage (the seeding launch of chunk k+1 waits for that of chunk k, the
	// region launches likewise): four chunks that share the device evenly all finish at the same moment, and the device then idles
	// through the first of their back halves; chained, they are one stage apart and a chunk's seeding overlaps its predecessor's regions
	std::mutex chain_mu;
	hipEvent_t chain_seed = nullptr, chain_regions = nullptr;
};
struct LaneRef { bsx_device *d; int lane; };   // what the backend vtable carries as ctx
#define LR(c) ((LaneRef*)(c))->d, ((LaneRef*)(c))->lane

// host <-> device copies of a lane, complete on return (shim.hip, next to k_copy_bytes)
int xfer(Lane &L, hipStream_t st, void *dst, const void *src, size_t n, bool h2d);
#define H2D(st, dst, src, n) do { int rc_ = xfer(L, st, dst, src, n, true); if (rc_ != BSX_OK) return rc_; } while (0)
#define D2H(st, dst, src, n) do { int rc_ = xfer(L, st, dst, src, n, false); if (rc_ != BSX_OK) return rc_; } while (0)

void shim_tables_backend(bsx_backend_t *out);   // shim_tables.hip: the output passes' slots of the vtable
