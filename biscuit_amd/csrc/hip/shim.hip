// shim.hip -- the thin C-ABI shim between the C host code and the HIP kernels (include/bsx.h).
// Owns: device selection, the HBM-resident index (both converted FM indices + SA samples + pac),
// per-chunk read buffer, job/result staging, kernel timing (HIP events on the launch stream) and
// the work counters behind the algorithmic-bytes model.  No CPU fallback: every entry point
// returns BSX_E_NODEVICE when HIP is unusable.  The output passes that run while aligning are a unit of their own, shim_tables.hip; what the
// two share (Lane, bsx_device, the error macros, xfer) is in shim_dev.hpp.
#include <time.h>
#include <atomic>
#include "shim_dev.hpp"
#include "index_build.h"
#include "ext_pk_bound.h"
#include "ext_stop.hpp"
#include "rgx.hpp"

#include <sys/time.h>
static double bsx_now_s(void) { struct timeval tv; gettimeofday(&tv, 0); return tv.tv_sec + tv.tv_usec * 1e-6; }
// the device's suffix-array sample: every 2nd rank (the files keep every 32nd, bwtindex.c:328,340): bwt_sa walks one LF step on average.
// Measured at hg38 size, k_occ per chunk: 28 ms at every 4th (12.4 GB per index), 16.5 at every 2nd (24.8 GB), 8.9 with the whole array (49.6 GB)
#define BSX_DEVICE_SA_INTV_DEFAULT 2
static inline unsigned long long *dev_counters(Lane &L) { return (unsigned long long*)L.small.p; }
static inline CtrShared *ctr_shared(Lane &L) { return (CtrShared*)(dev_counters(L) + CTR_SHARED); }   // (device memory: for the addresses of its fields)
static inline TierCtr *ctr_tiers(Lane &L, bool main_seq) { return (TierCtr*)(dev_counters(L) + (main_seq ? CTR_MAIN : CTR_SIDE)); }
// a lane's slab of a seeding pass: mem_cap SMEMs of 32 bytes, one list of list_cap 16-byte entries
static inline size_t seed_lane_bytes(long long mem_cap, int list_cap) { return (size_t)mem_cap * 32 + (size_t)list_cap * 16; }

extern "C" BSX_API int bsx_device_open(int ordinal, bsx_device_t **out)
{
	int n = 0;
	*out = nullptr;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { fprintf(stderr, "[bsx-hip] no HIP device available\n"); return BSX_E_NODEVICE; }
	if (ordinal < 0 || ordinal >= n) return BSX_E_ARG;
	HIPCHK(hipSetDevice(ordinal));
	// host threads that wait for the device sleep instead of polling: a chunk stream has half a dozen threads waiting at any time (front
	// halves, K5/K6 batches), and on a 16-core quota their polling was a third of the host's CPU time (the runtime's default polls)
	if (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();
	bsx_device *d = new bsx_device();
	d->ordinal = ordinal;
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, ordinal));
	snprintf(d->name, sizeof(d->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
	d->n_cu = prop.multiProcessorCount;
	for (int l = 0; l < BSX_LANES; ++l) {
		Lane &L = d->lane[l];
		int lo = 0, hi = 0;
		HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least, hi = greatest priority (numerically lower)
		// The front-half streams leave a few compute units alone (one in every `reserve`): workgroups of k_seed live for tens of
		// milliseconds and are not preempted, so without free CUs the short high-priority batches of the back half (K5, K6)
		// would queue behind them no matter their priority.
		const int reserve = (int)bsx_tune_long("reserve_cu_every", 0);   // (0 since round 6: with the CUs that are left free spread over every XCD -- below -- the back half's batches start at once and everything else gets slower by more: 735 k reads/s against 776 k without a mask and 757-780 k with the old one)
		bool masked = false;
		if (reserve >= 2 && d->n_cu >= 16) {
			std::vector<uint32_t> mask((size_t)(d->n_cu + 31) / 32, 0u);
			// Which CUs a mask bit stands for (tools/ubench/mask_probe.hip, round 6): bit i is CU i / 32 of shader engine (i / 8) % 4 of XCD i % 8 -- consecutive
			// bits go round the XCDs, then the shader engines.  Workgroups go round the XCDs as well, and a kernel is done when its last workgroup is:
			// the CUs left free must be in EVERY XCD.  Rounds 4-6 cleared every `reserve`-th bit -- with 8, all of XCD 7 and nothing of the others, and
			// a batch of the back half waited a workgroup's lifetime of whatever filled the other seven (the probe: 21 ms against 0.05 ms).  Now the TOP
			// n_cu / reserve bits (whole rows of 32: one CU of every shader engine of every XCD per row) are the ones left out.
			int n_free = d->n_cu / reserve;
			if (d->n_cu >= 64) n_free = (n_free + 31) / 32 * 32;
			if (n_free >= d->n_cu) n_free = d->n_cu / 2;
			for (int cu = 0; cu < d->n_cu - n_free; ++cu) mask[cu >> 5] |= 1u << (cu & 31);
			masked = hipExtStreamCreateWithCUMask(&L.st, (uint32_t)mask.size(), mask.data()) == hipSuccess &&
			         hipExtStreamCreateWithCUMask(&L.st2, (uint32_t)mask.size(), mask.data()) == hipSuccess &&
			         hipExtStreamCreateWithCUMask(&L.st3, (uint32_t)mask.size(), mask.data()) == hipSuccess;
			if (!masked) { (void)hipGetLastError(); if (L.st) { (void)hipStreamDestroy(L.st); L.st = nullptr; } if (L.st2) { (void)hipStreamDestroy(L.st2); L.st2 = nullptr; } if (L.st3) { (void)hipStreamDestroy(L.st3); L.st3 = nullptr; } }
		}
		if (!masked) {
			HIPCHK(hipStreamCreateWithPriority(&L.st, hipStreamNonBlocking, lo));
			HIPCHK(hipStreamCreateWithPriority(&L.st2, hipStreamNonBlocking, lo));
			HIPCHK(hipStreamCreateWithPriority(&L.st3, hipStreamNonBlocking, lo));
		}
		for (hipEvent_t *e : {&L.ev_timed_begin, &L.ev_timed_end, &L.ev_seed2_begin, &L.ev_seed2_end, &L.ev_occ_end, &L.ev_tier1_end, &L.ev_tiers_end}) HIPCHK(hipEventCreate(e));
		HIPCHK(hipEventCreate(&L.ev_t3a));
		HIPCHK(hipEventCreate(&L.ev_t3b));
		HIPCHK(hipStreamCreateWithPriority(&L.st_hi, hipStreamNonBlocking, hi));
		if (masked && bsx_tune_long("small_copies_unmasked", 1)) { HIPCHK(hipStreamCreateWithPriority(&L.st_cp, hipStreamNonBlocking, hi)); HIPCHK(hipEventCreateWithFlags(&L.ev_cp, hipEventDisableTiming)); }
		HIPCHK(hipEventCreateWithFlags(&L.ev_seed_done, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&L.ev_regions_done, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&L.rs.ev, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&L.rs.ev_tiers, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&L.pev[0], hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&L.pev[1], hipEventDisableTiming));
		if (L.slabflags.reserve((size_t)d->n_cu * 16 * 4) != BSX_OK) return BSX_E_NOMEM;
		HIPCHK(hipMemset(L.slabflags.p, 0, (size_t)d->n_cu * 16 * 4));
		if (L.small.reserve(SMALL_BYTES) != BSX_OK) return BSX_E_NOMEM;
		HIPCHK(hipMemset(L.small.p, 0, SMALL_BYTES));
	}
	memset(&d->ix, 0, sizeof(d->ix));
	for (int l = 0; l < BSX_LANES; ++l) memset(&d->lane[l].sc, 0, sizeof(DevScoring));
	*out = d;
	return BSX_OK;
}

extern "C" BSX_API void bsx_device_close(bsx_device_t *d)
{
	if (!d) return;
	(void)hipSetDevice(d->ordinal);
	devbuf_drain(d->ordinal);   // the blocks this device's buffers left behind when they grew
	for (int i = 0; i < 2; ++i) { d->bwt[i].release(); d->sa[i].release(); d->seedtab[i].release(); }
	d->pac.release(); d->ctg.release(); d->holes.release();
	d->qc.release(); d->cov.release(); d->meth.release(); d->md.release(); d->sort.release(); d->bam.release();
	for (int l = 0; l < BSX_LANES; ++l) {
		Lane &L = d->lane[l];
		L.release_buffers();
		if (L.pev[0]) (void)hipEventDestroy(L.pev[0]);
		if (L.pev[1]) (void)hipEventDestroy(L.pev[1]);
		if (L.ev_seed_done) (void)hipEventDestroy(L.ev_seed_done);
		if (L.ev_regions_done) (void)hipEventDestroy(L.ev_regions_done);
		if (L.st) (void)hipStreamDestroy(L.st);
		if (L.st_hi) (void)hipStreamDestroy(L.st_hi);
		if (L.st2) (void)hipStreamDestroy(L.st2);
		if (L.st3) (void)hipStreamDestroy(L.st3);
		if (L.st_cp) (void)hipStreamDestroy(L.st_cp);
		if (L.ev_cp) (void)hipEventDestroy(L.ev_cp);
		for (hipEvent_t e : {L.ev_timed_begin, L.ev_timed_end, L.ev_seed2_begin, L.ev_seed2_end, L.ev_occ_end, L.ev_tier1_end, L.ev_tiers_end}) if (e) (void)hipEventDestroy(e);
		if (L.ev_t3a) (void)hipEventDestroy(L.ev_t3a);
		if (L.ev_t3b) (void)hipEventDestroy(L.ev_t3b);
		for (int k = 0; k < 12; ++k) if (L.tier_ev[k]) { (void)hipEventDestroy(L.tier_ev[k]); L.tier_ev[k] = nullptr; }
		if (L.rs.ev) (void)hipEventDestroy(L.rs.ev);
		if (L.rs.ev_tiers) (void)hipEventDestroy(L.rs.ev_tiers);
		L.rs.hres.release();
	}
	delete d;
}

extern "C" BSX_API const char *bsx_device_name(const bsx_device_t *d) { return d ? d->name : ""; }
extern "C" BSX_API int bsx_device_n_cu(const bsx_device_t *d) { return d ? d->n_cu : 0; }

// pac and the contig table: what the kernels need of the reference besides the FM indices
static int upload_ref(bsx_device_t *d, const bsx_index_t *idx)
{
	size_t npac = (size_t)(idx->ref.l_pac / 4 + 1);
	int rc;
	// ranks and interval sizes travel as 34-bit numbers in the seeding kernel's interval lists (seed_core.hpp: SeedEnt)
	if (idx->ref.l_pac >= (int64_t)1 << 33) { fprintf(stderr, "[bsx-hip] genomes of 2^33 bases (8.6 Gbp) or more are not supported on the device\n"); return BSX_E_ARG; }
	if ((rc = d->pac.reserve(npac + 16)) != BSX_OK) return rc;
	HIPCHK(hipMemcpy(d->pac.p, idx->pac, npac, hipMemcpyHostToDevice));
	d->ix.pac = (const uint8_t*)d->pac.p; d->ix.l_pac = idx->ref.l_pac;
	{ // contig table: offsets (n_seqs + 1, the last one = l_pac) then the is_alt bytes
		const int ns = idx->ref.n_seqs;
		std::vector<int64_t> off((size_t)ns + 1);
		std::vector<uint8_t> alt((size_t)ns + 8, 0);
		for (int i = 0; i < ns; ++i) { off[i] = idx->ref.anns[i].offset; alt[i] = idx->ref.anns[i].is_alt ? 1 : 0; }
		off[ns] = idx->ref.l_pac;
		if ((rc = d->ctg.reserve(((size_t)ns + 1) * 8 + (size_t)ns + 8)) != BSX_OK) return rc;
		HIPCHK(hipMemcpy(d->ctg.p, off.data(), ((size_t)ns + 1) * 8, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy((char*)d->ctg.p + ((size_t)ns + 1) * 8, alt.data(), (size_t)ns, hipMemcpyHostToDevice));
		d->ix.ctg_off = (const int64_t*)d->ctg.p; d->ix.ctg_alt = (const uint8_t*)d->ctg.p + ((size_t)ns + 1) * 8; d->ix.n_seqs = ns;
	}
	{ // the N holes of the forward strand (.bis.amb, or the builder's list): starts, then ends, in the file's order (sorted by position)
		const int nh = idx->ref.n_holes;
		std::vector<int64_t> he((size_t)nh * 2 + 1);
		for (int i = 0; i < nh; ++i) { he[i] = idx->ref.ambs[i].offset; he[(size_t)nh + i] = idx->ref.ambs[i].offset + idx->ref.ambs[i].len; }
		for (int i = 1; i < nh; ++i) if (he[i] < he[(size_t)nh + i - 1]) { fprintf(stderr, "[bsx-hip] the index's N holes are not sorted\n"); return BSX_E_FORMAT; }
		if ((rc = d->holes.reserve((size_t)nh * 16 + 16)) != BSX_OK) return rc;
		if (nh) HIPCHK(hipMemcpy(d->holes.p, he.data(), (size_t)nh * 16, hipMemcpyHostToDevice));
		d->ix.hole_off = (const int64_t*)d->holes.p; d->ix.hole_end = (const int64_t*)d->holes.p + nh; d->ix.n_holes = nh; d->ix.pad2_ = 0;
	}
	return BSX_OK;
}

// The table of k-mer intervals of both converted indices (seed_tab.hpp), built from the indices now resident: K levels, K chosen from the
// text's size (18 for an hg38-sized genome: 2 x 9.3 GB), $BSX_SEED_TAB_K overrides (0: no table, every seeding step an FM extension).
// What the index's optional structures may take of the device's memory: the chunks in flight need room too (their buffers grow with the chunk:
// ~25 GB a lane for 1 M reads against an hg38-sized genome), so a third of the device (at most 64 GB) is left alone.  On a 288 GB part
// nothing changes; on a smaller one the table loses levels and the suffix-array sample gets sparser instead of the upload failing.
static size_t hbm_budget(void)
{
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return ~(size_t)0; }
	const size_t keep = std::min<size_t>(tot / 3, (size_t)64 << 30);
	return fr > keep ? fr - keep : 0;
}
static int build_seed_tables(bsx_device_t *d)
{
	int K = seed_tab_depth(d->ix.fmi[0].seq_len);
	const int K_want = K;
	if (const char *e = bsx_tune_str("seed_tab_k")) { K = atoi(e); if (K < 2) K = 0; if (K > 19) K = 19; }
	d->ix.tab.K = 0; d->ix.tab.t[0] = d->ix.tab.t[1] = nullptr; d->ix.tab.pad_ = 0;
	d->seedtab[0].release(); d->seedtab[1].release();
	while (K >= 2 && 2 * (size_t)seed_tab_entries(K) * sizeof(SeedEnt) > hbm_budget()) --K;   // a level is a third of the table
	Lane &L = d->lane[0];
	for (; K >= 2; --K) { // (and one level fewer when the reservation fails all the same)
		int rc = BSX_OK;
		for (int i = 0; i < 2 && rc == BSX_OK; ++i) rc = d->seedtab[i].reserve_exact((size_t)seed_tab_entries(K) * sizeof(SeedEnt));
		if (rc == BSX_OK) break;
		d->seedtab[0].release(); d->seedtab[1].release();
		(void)hipGetLastError();
	}
	if (K != K_want && !bsx_tune_is_set("seed_tab_k")) fprintf(stderr, "[W::%s] device memory: table of k-mer intervals with %d levels instead of %d%s\n", "bsx-hip", K < 2 ? 0 : K, K_want, K < 2 ? " (none: every seeding step is an FM extension)" : "");
	if (K < 2) { d->seedtab[0].release(); d->seedtab[1].release(); return BSX_OK; }
	for (int i = 0; i < 2; ++i) {
		int rc;
		if ((rc = seedtab_build(L.st, d->ix, i, K, d->seedtab[i].p)) != BSX_OK) return rc;
	}
	HIPCHK(hipStreamSynchronize(L.st));
	HIPCHK(hipGetLastError());
	d->ix.tab.t[0] = (const uint4*)d->seedtab[0].p; d->ix.tab.t[1] = (const uint4*)d->seedtab[1].p; d->ix.tab.K = K;
	return BSX_OK;
}

extern "C" BSX_API int bsx_device_upload_index(bsx_device_t *d, const bsx_index_t *idx)
{
	if (!d || !idx) return BSX_E_ARG;
	if (!idx->fmi[0].bwt || !idx->fmi[1].bwt || !idx->fmi[0].sa || !idx->fmi[1].sa) return BSX_E_ARG;   // no FM indices on the host side: bsx_device_build_index makes them in place
	HIPCHK(hipSetDevice(d->ordinal));
	for (int i = 0; i < 2; ++i) {
		const bsx_fmi_t *f = &idx->fmi[i];
		int rc;
		if ((rc = d->bwt[i].reserve((size_t)f->bwt_size * 4 + 64)) != BSX_OK) return rc;
		if ((rc = d->sa[i].reserve((size_t)f->n_sa * 8)) != BSX_OK) return rc;
		HIPCHK(hipMemset((char*)d->bwt[i].p + (size_t)f->bwt_size * 4, 0, 64));   // the slack the last thread of k_bwt_planes reads and writes
		HIPCHK(hipMemcpy(d->bwt[i].p, f->bwt, (size_t)f->bwt_size * 4, hipMemcpyHostToDevice));
		launch_bwt_planes(d->lane[0].st, (uint32_t*)d->bwt[i].p, (unsigned long long)f->bwt_size);   // the device's block layout (dev_common.hpp); ahead of everything that reads symbols
		HIPCHK(hipStreamSynchronize(d->lane[0].st));
		HIPCHK(hipMemcpy(d->sa[i].p, f->sa, (size_t)f->n_sa * 8, hipMemcpyHostToDevice));
		DevFmi &g = d->ix.fmi[i];
		g.primary = f->primary; for (int k = 0; k < 5; ++k) g.L2[k] = f->L2[k];
		g.seq_len = f->seq_len; g.bwt = (const uint32_t*)d->bwt[i].p; g.sa = (const uint64_t*)d->sa[i].p;
		g.sa_mask = (uint32_t)f->sa_intv - 1; g.sa_shift = 0;
		while ((1 << g.sa_shift) < f->sa_intv) ++g.sa_shift;
		if ((1 << g.sa_shift) != f->sa_intv) return BSX_E_FORMAT;
	}
	int rc;
	if ((rc = upload_ref(d, idx)) != BSX_OK) return rc;
	{ // denser suffix-array sample for the device (the files' 1-in-32 stays what the loader and the host see)
		const char *e = bsx_tune_str("device_sa_intv");
		int want = e ? atoi(e) : BSX_DEVICE_SA_INTV_DEFAULT;
		const int file_intv = (int)d->ix.fmi[0].sa_mask + 1;
		if (want >= 1 && (want & (want - 1)) == 0) { // sparser when the device is short of memory (hbm_budget), down to the files' own sample
			const int asked = want;
			while (want < file_intv && 2 * ((size_t)(d->ix.fmi[0].seq_len / (unsigned)want) + 1) * 8 > hbm_budget()) want <<= 1;
			if (want != asked) fprintf(stderr, "[W::%s] device memory: suffix-array sample every %d ranks instead of every %d\n", "bsx-hip", want < file_intv ? want : file_intv, asked);
		}
		if (want >= 1 && want < file_intv && (want & (want - 1)) == 0 && d->ix.fmi[1].sa_mask == d->ix.fmi[0].sa_mask) {
			DevBuf dense[2];
			Lane &L = d->lane[0];
			for (int i = 0; i < 2; ++i) {
				const unsigned long long nd = d->ix.fmi[i].seq_len / (unsigned)want + 1;
				if ((rc = dense[i].reserve((size_t)nd * 8)) != BSX_OK) { dense[0].release(); dense[1].release(); return rc; }
				launch_sa_dense(L.st, d->n_cu, d->ix, i, (unsigned)want, nd, (unsigned long long*)dense[i].p);
			}
			HIPCHK(hipStreamSynchronize(L.st));
			HIPCHK(hipGetLastError());
			int shift = 0;
			while ((1 << shift) < want) ++shift;
			for (int i = 0; i < 2; ++i) {
				d->sa[i].release();
				d->sa[i] = dense[i];
				d->ix.fmi[i].sa = (const uint64_t*)d->sa[i].p; d->ix.fmi[i].sa_mask = (uint32_t)want - 1; d->ix.fmi[i].sa_shift = (uint32_t)shift;
			}
		}
	}
	if ((rc = build_seed_tables(d)) != BSX_OK) return rc;
	d->has_index = true;
	return BSX_OK;
}

// (f)1 on the device: both FM indices built in HBM from the genome's pac (k_index.hip) and left resident
extern "C" BSX_API int bsx_device_build_index(bsx_device_t *d, bsx_index_t *idx, int fill_host)
{
	if (!d || !idx || !idx->pac || idx->ref.l_pac <= 0) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	if ((rc = upload_ref(d, idx)) != BSX_OK) return rc;
	const char *e = bsx_tune_str("device_sa_intv");
	int dense = e ? atoi(e) : BSX_DEVICE_SA_INTV_DEFAULT;
	if (dense < 1 || dense > 32 || (dense & (dense - 1))) dense = BSX_DEVICE_SA_INTV_DEFAULT;
	Lane &L = d->lane[0];
	for (int i = 1; i >= 0; --i) {
		bsx_fmi_t *f = &idx->fmi[i], meta;
		memset(&meta, 0, sizeof(meta));
		free(f->bwt); free(f->sa); f->bwt = nullptr; f->sa = nullptr;
		d->bwt[i].release(); d->sa[i].release();
		const uint64_t n = (uint64_t)idx->ref.l_pac * 2;
		uint32_t *h_bwt = nullptr; uint64_t *h_sa = nullptr;
		if (fill_host) {
			const uint64_t n_occ = (n + 127) / 128 + 1, words = ((n + 15) >> 4) + n_occ * 8, n_sa = (n + 32) / 32;
			h_bwt = (uint32_t*)calloc(words + 16, 4); h_sa = (uint64_t*)calloc(n_sa, 8);
			if (!h_bwt || !h_sa) { free(h_bwt); free(h_sa); return BSX_E_NOMEM; }
		}
		rc = bsx_ix_build_fmi(L.st, d->n_cu, (const uint8_t*)d->pac.p, idx->ref.l_pac, i, dense, 32, &d->bwt[i], &d->sa[i], &meta, h_bwt, h_sa);
		if (rc != BSX_OK) { free(h_bwt); free(h_sa); return rc; }
		launch_bwt_planes(L.st, (uint32_t*)d->bwt[i].p, (unsigned long long)meta.bwt_size);   // (the host copy above is the file layout)
		HIPCHK(hipStreamSynchronize(L.st));
		*f = meta; f->bwt = h_bwt; f->sa = h_sa;   // bwt == NULL: the FM index lives on the device only
		DevFmi &g = d->ix.fmi[i];
		g.primary = meta.primary; for (int k = 0; k < 5; ++k) g.L2[k] = meta.L2[k];
		g.seq_len = meta.seq_len; g.bwt = (const uint32_t*)d->bwt[i].p; g.sa = (const uint64_t*)d->sa[i].p;
		g.sa_mask = (uint32_t)dense - 1; g.sa_shift = 0;
		while ((1 << g.sa_shift) < dense) ++g.sa_shift;
	}
	devbuf_drain(d->ordinal);   // the blocks the builder's growing buffers left behind on this device go now
	if ((rc = build_seed_tables(d)) != BSX_OK) return rc;
	d->has_index = true;
	return BSX_OK;
}

static int lane_set_opt(bsx_device_t *d, int lane, const bsx_opt_t *o)
{
	if (!d || !o) return BSX_E_ARG;
	DevScoring &sc = d->lane[lane].sc;
	memcpy(sc.ctmat, o->ctmat, 25); memcpy(sc.gamat, o->gamat, 25);
	sc.o_del = o->o_del; sc.e_del = o->e_del; sc.o_ins = o->o_ins; sc.e_ins = o->e_ins; sc.zdrop = o->zdrop; sc.a = o->a;
	sc.mx_ct = sc.mx_ga = 0;   // as ksw_extend2 computes it: the maximum starts from 0
	for (int k = 0; k < 25; ++k) { sc.mx_ct = std::max<int>(sc.mx_ct, sc.ctmat[k]); sc.mx_ga = std::max<int>(sc.mx_ga, sc.gamat[k]); }
	sc.ext_stop = 0; sc.xs_ctr = nullptr;   // (every launch sequence that reads them arms them first: ext_stop_arm)
	return BSX_OK;
}
extern "C" BSX_API int bsx_device_set_opt(bsx_device_t *d, const bsx_opt_t *o) { return lane_set_opt(d, 0, o); }   // the batch calls of include/bsx.h run on lane 0

// Large copies between pageable host memory and the device go through two pinned halves, copy and DMA overlapped:
// handing pageable memory to hipMemcpy makes the runtime pin and unpin the user pages on every call, which costs
// more system time per chunk than the copies themselves.  Synchronous: complete on return.
#define XFER_CHUNK ((size_t)8 << 20)
// The back half's batches (K5, K6: a megabyte of jobs up, a megabyte of results down, on the lane's high-priority stream) do not go through
// the copy engines: those serve every stream first come first served, and behind another chunk's region download (half a gigabyte) a
// one-megabyte copy waited half a second (measured: "download 0.656 s" of a 15 ms K5 batch).  A kernel on the batch's own stream moves the
// bytes between the lane's pinned halves (mapped into the device's address space) and HBM instead.
// the strand searches seeded again inside the main launch sequence: their new lists replace the first pass's in the chunk's offset / count arrays
__global__ void __launch_bounds__(256)
k_patch_lists(const int *which, int n, const long long *off2, const int *cnt2, long long *off, int *cnt)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n) { off[which[j]] = off2[j]; cnt[which[j]] = cnt2[j]; }
}
__global__ void __launch_bounds__(256)
k_copy_bytes(const unsigned char *src, unsigned char *dst, size_t n)
{
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
	if ((((size_t)src | (size_t)dst) & 15) == 0) {
		const size_t n16 = n >> 4;
		for (size_t i = tid; i < n16; i += nth) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
		for (size_t i = (n16 << 4) + tid; i < n; i += nth) dst[i] = src[i];
	} else if ((((size_t)src | (size_t)dst) & 3) == 0) {
		const size_t n4 = n >> 2;
		for (size_t i = tid; i < n4; i += nth) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
		for (size_t i = (n4 << 2) + tid; i < n; i += nth) dst[i] = src[i];
	} else for (size_t i = tid; i < n; i += nth) dst[i] = src[i];
}
static void copy_by_kernel(hipStream_t st, void *dst, const void *src, size_t n)
{
	const unsigned int blocks = (unsigned int)std::min<size_t>(std::max<size_t>(1, (n / 16 + 255) / 256), 2048);
	hipLaunchKernelGGL(k_copy_bytes, dim3(blocks), dim3(256), 0, st, (const unsigned char*)src, (unsigned char*)dst, n);
}
int xfer(Lane &L, hipStream_t st, void *dst, const void *src, size_t n, bool h2d)
{
	if (n == 0) return BSX_OK;
	const bool zc = st == L.st_hi;   // the back half's small batches move with a kernel on their own stream, not through the copy engines (round 4)
	if (!zc && n < ((size_t)256 << 10)) {
		// A small copy is a kernel of the runtime's (__amd_rocclr_copyBuffer: 1 400 of them per chunk in the trace), and on a front-half stream it is
		// dispatched to that stream's CUs only: with other chunks' long-lived workgroups on all of them it waits for one to leave -- tens of milliseconds
		// for eight bytes, at every point where the host reads a count.  It goes to the lane's unmasked stream instead, behind an event of `st`: the
		// CUs the front-half streams leave alone are in every XCD (bsx_device_open), so it runs at once.
		hipStream_t cs = L.st_cp && (st == L.st || st == L.st2 || st == L.st3) ? L.st_cp : st;
		if (cs != st) { HIPCHK(hipEventRecord(L.ev_cp, st)); HIPCHK(hipStreamWaitEvent(cs, L.ev_cp, 0)); }
		HIPCHK(hipMemcpyAsync(dst, src, n, h2d ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, cs));
		HIPCHK(hipStreamSynchronize(cs));
		return BSX_OK;
	}
	int rc;
	if ((rc = L.pin.reserve(2 * XFER_CHUNK)) != BSX_OK) return rc;
	char *pin = (char*)L.pin.p;
	size_t off = 0, prev_off = 0, prev_m = 0;
	int i = 0;
	for (; off < n; off += XFER_CHUNK, ++i) {
		const size_t m = std::min(XFER_CHUNK, n - off);
		char *p = pin + (size_t)(i & 1) * XFER_CHUNK;
		if (h2d) {
			if (i >= 2) HIPCHK(hipEventSynchronize(L.pev[i & 1]));   // the DMA that last read this half is done
			memcpy(p, (const char*)src + off, m);
			if (zc) copy_by_kernel(st, (char*)dst + off, p, m); else HIPCHK(hipMemcpyAsync((char*)dst + off, p, m, hipMemcpyHostToDevice, st));
			HIPCHK(hipEventRecord(L.pev[i & 1], st));
		} else {
			if (zc) copy_by_kernel(st, p, (const char*)src + off, m); else HIPCHK(hipMemcpyAsync(p, (const char*)src + off, m, hipMemcpyDeviceToHost, st));
			HIPCHK(hipEventRecord(L.pev[i & 1], st));
			if (i >= 1) { // drain the previous half while this one is in flight
				HIPCHK(hipEventSynchronize(L.pev[(i - 1) & 1]));
				memcpy((char*)dst + prev_off, pin + (size_t)((i - 1) & 1) * XFER_CHUNK, prev_m);
			}
			prev_off = off; prev_m = m;
		}
	}
	HIPCHK(hipStreamSynchronize(st));
	if (!h2d) memcpy((char*)dst + prev_off, pin + (size_t)((i - 1) & 1) * XFER_CHUNK, prev_m);
	return BSX_OK;
}

static int lane_set_reads(bsx_device_t *d, int lane, const uint8_t *buf, size_t n)
{
	if (!d) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	if ((rc = L.reads.reserve(n + 64)) != BSX_OK) return rc;
	H2D(L.st, L.reads.p, buf, n);
	L.n_reads = n;
	return BSX_OK;
}

extern "C" BSX_API int bsx_device_set_reads(bsx_device_t *d, const uint8_t *buf, size_t n) { return lane_set_reads(d, 0, buf, n); }

// time one kernel (already enqueued between ev_timed_begin / ev_timed_end on the lane's stream)
static int finish_timed(Lane &L, int k)
{
	float ms = 0;
	HIPCHK(hipEventSynchronize(L.ev_timed_end));
	HIPCHK(hipEventElapsedTime(&ms, L.ev_timed_begin, L.ev_timed_end));
	L.k_ms[k] += ms; L.k_launch[k] += 1;
	HIPCHK(hipGetLastError());
	return BSX_OK;
}

extern "C" BSX_API int bsx_device_counters(bsx_device_t *d, uint64_t c[4], int reset)
{
	if (!d) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	c[0] = c[1] = c[2] = c[3] = 0;
	for (int l = 0; l < BSX_LANES; ++l) {
		uint64_t t[4];
		unsigned long long *ctr = dev_counters(d->lane[l]);
		static_assert(CTR_FM_SLOW == 0 && CTR_LF_CALLS == 3, "c[0..3]: FM blocks (slow, fast), LF steps, LF calls");
		HIPCHK(hipMemcpy(t, ctr + CTR_FM_SLOW, 32, hipMemcpyDeviceToHost));
		for (int k = 0; k < 4; ++k) c[k] += t[k];
		if (reset) HIPCHK(hipMemset(ctr + CTR_FM_SLOW, 0, 32));
		for (int b = 0; b < 2; ++b) { // the later seeding passes' FM blocks (counted apart: bsx_device_seed_passes)
			unsigned long long *p = ctr + (b ? CTR_SEED3 : CTR_SEED2) + CTR_FM_SLOW;
			HIPCHK(hipMemcpy(t, p, 16, hipMemcpyDeviceToHost));
			c[0] += t[0]; c[1] += t[1];
			if (reset) HIPCHK(hipMemset(p, 0, 16));
		}
	}
	return BSX_OK;
}

// table entries read by the seeding kernel since the last reset (summed over the lanes), and the depth of the resident table
extern "C" BSX_API int bsx_device_seed_table(bsx_device_t *d, uint64_t *lookups, int *depth, int reset)
{
	if (!d) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	uint64_t tot = 0;
	for (int l = 0; l < BSX_LANES; ++l) {
		static const int at[3] = {CTR_TAB_LOOKUPS, CTR_SEED2 + CTR_TAB_LOOKUPS, CTR_SEED3 + CTR_TAB_LOOKUPS};
		for (int b = 0; b < 3; ++b) {
			uint64_t t = 0;
			HIPCHK(hipMemcpy(&t, dev_counters(d->lane[l]) + at[b], 8, hipMemcpyDeviceToHost));
			tot += t;
			if (reset) HIPCHK(hipMemset(dev_counters(d->lane[l]) + at[b], 0, 8));
		}
	}
	if (lookups) *lookups = tot;
	if (depth) *depth = d->has_index ? d->ix.tab.K : 0;
	return BSX_OK;
}

// The seeding passes of bsx_regions_batch one by one since the last reset (call it BEFORE bsx_device_counters / _seed_table with reset, which
// zero the same blocks): w[0], w[1] FM blocks and table entries read by the chunk-wide first pass (and by bsx_seed_batch launches), w[2], w[3]
// by the second pass inside the chunk's sequence, w[4] its launches, w[5] its strand searches; ms[0], ms[1]: their summed HIP-event times.
extern "C" BSX_API int bsx_device_seed_passes(bsx_device_t *d, uint64_t w[6], double ms[2], int reset)
{
	if (!d || !w || !ms) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	for (int k = 0; k < 6; ++k) w[k] = 0;
	ms[0] = ms[1] = 0;
	for (int l = 0; l < BSX_LANES; ++l) {
		Lane &L = d->lane[l];
		uint64_t t[2], u = 0;
		unsigned long long *ctr = dev_counters(L);
		HIPCHK(hipMemcpy(t, ctr + CTR_FM_SLOW, 16, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(&u, ctr + CTR_TAB_LOOKUPS, 8, hipMemcpyDeviceToHost));
		w[0] += t[0] + t[1]; w[1] += u;
		HIPCHK(hipMemcpy(t, ctr + CTR_SEED2 + CTR_FM_SLOW, 16, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(&u, ctr + CTR_SEED2 + CTR_TAB_LOOKUPS, 8, hipMemcpyDeviceToHost));
		w[2] += t[0] + t[1]; w[3] += u;
		w[4] += (uint64_t)L.seed2_launches; w[5] += L.seed2_tasks;
		ms[0] += L.k_ms[KT_SEED]; ms[1] += L.seed2_ms;
		if (reset) { L.seed2_ms = 0; L.seed2_launches = 0; L.seed2_tasks = 0; }
	}
	return BSX_OK;
}

// Which extension rows the launches took: the packed 16-bit ones (ext_pk.hpp) where the scoring options and the batch pass ext_pk_exact()
// (ext_pk_bound.h), else the 32-bit ones.  The setting ext_pk=0 forces the 32-bit forms.
static std::atomic<uint64_t> g_ext_forms[2];
static bool ext_pk_wanted(void) { return bsx_tune_long("ext_pk", 1) != 0; }
static bool ext_pk_scoring(const DevScoring &sc, long long hmax, int qmax, bool per_read)
{
	int mn = 0;
	for (int k = 0; k < 25; ++k) mn = std::min<int>(mn, std::min<int>(sc.ctmat[k], sc.gamat[k]));
	const int mx = std::max(sc.mx_ct, sc.mx_ga);
	if (per_read) return ext_pk_exact_reads(sc.a, mx, mn, sc.o_del, sc.e_del, sc.o_ins, sc.e_ins, qmax);
	return ext_pk_exact(mx, mn, sc.o_del, sc.e_del, sc.o_ins, sc.e_ins, hmax, qmax);
}
extern "C" BSX_API int bsx_ext_forms(uint64_t c[2], int reset)
{
	if (!c) return BSX_E_ARG;
	for (int k = 0; k < 2; ++k) { c[k] = g_ext_forms[k].load(); if (reset) g_ext_forms[k].store(0); }
	return BSX_OK;
}

// The extensions' stopping rule (ext_stop_rule.h).  The setting ext_stop (default 1) goes to the kernels in the lane's DevScoring, together with the
// rule's counter block where the rule is counted: the batch seam (always) and the region launches under $BSX_PHASES.  With the switch off and the
// counters on, the kernels evaluate the rule without obeying it and count the rows that run after it would have fired.
static std::atomic<uint64_t> g_ext_stops[XS_FAM_N * XS_N];
static int ext_stop_arm(Lane &L, hipStream_t st, bool count)
{
	L.sc.ext_stop = bsx_tune_long("ext_stop", 1) != 0 ? 1 : 0;
	L.sc.xs_ctr = nullptr;
	if (!count) return BSX_OK;
	if (!L.xstop.p) {
		int rc = L.xstop.reserve(sizeof(unsigned long long) * XS_FAM_N * XS_N);
		if (rc != BSX_OK) return rc;
		HIPCHK(hipMemsetAsync(L.xstop.p, 0, sizeof(unsigned long long) * XS_FAM_N * XS_N, st));
	}
	L.sc.xs_ctr = (unsigned long long*)L.xstop.p;
	return BSX_OK;
}
// the lane's counters, read, zeroed and added to the process-wide ones; c (may be null) gets this read-out
static int ext_stop_collect(Lane &L, hipStream_t st, unsigned long long *c)
{
	unsigned long long h[XS_FAM_N * XS_N] = {0};
	if (L.xstop.p) {
		D2H(st, h, L.xstop.p, sizeof(h));
		HIPCHK(hipMemsetAsync(L.xstop.p, 0, sizeof(h), st));
	}
	for (int k = 0; k < XS_FAM_N * XS_N; ++k) { g_ext_stops[k] += h[k]; if (c) c[k] = h[k]; }
	return BSX_OK;
}
// c[5 * family + {0: extensions stopped, 1: evaluations, 2: rows left at the stops, 3: rows run after a stop that was not obeyed, 4: extensions that
// would have stopped with the switch off}], families: k_ext4, k_extl, the HBM tiers, chains -> regions, the wavefront-per-job batch form
// (ext_stop.hpp); c[25] = extensions stopped over all of them
extern "C" BSX_API int bsx_ext_stops(uint64_t c[26], int reset)
{
	if (!c) return BSX_E_ARG;
	c[XS_FAM_N * XS_N] = 0;
	for (int k = 0; k < XS_FAM_N * XS_N; ++k) { c[k] = g_ext_stops[k].load(); if (k % XS_N == XS_STOPS) c[XS_FAM_N * XS_N] += c[k]; if (reset) g_ext_stops[k].store(0); }
	return BSX_OK;
}

extern "C" BSX_API int bsx_device_region_work(bsx_device_t *d, uint64_t w[5], int reset)
{
	if (!d || !w) return BSX_E_ARG;
	for (int k = 0; k < 5; ++k) w[k] = 0;
	for (int l = 0; l < BSX_LANES; ++l) for (int k = 0; k < 5; ++k) { w[k] += d->lane[l].work[k]; if (reset) d->lane[l].work[k] = 0; }
	return BSX_OK;
}

extern "C" BSX_API int bsx_device_kernel_time(bsx_device_t *d, int k, double *total_ms, int64_t *launches, int reset)
{
	if (!d || k < 0 || k >= KT_N) return BSX_E_ARG;
	double ms = 0; int64_t n = 0;
	for (int l = 0; l < BSX_LANES; ++l) {
		ms += d->lane[l].k_ms[k]; n += d->lane[l].k_launch[k];
		if (reset) { d->lane[l].k_ms[k] = 0; d->lane[l].k_launch[k] = 0; }
	}
	if (total_ms) *total_ms = ms;
	if (launches) *launches = n;
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K1+K2
// ------------------------------------------------------------------------------------------
static bool intv_info_lt(const bsx_intv_t &a, const bsx_intv_t &b) { return a.info < b.info; }

struct SeedAsm {
	const long long *off; const int *cnt; const bsx_intv_t *dense;   // round-0 results (dense, arbitrary task order)
	const int64_t *redo_of; const std::vector<std::vector<bsx_intv_t>> *redo;
	bsx_intv_t *out; const int64_t *out_off;
};
static void seed_asm_worker(void *data, long i, int tid)
{
	const SeedAsm *A = (const SeedAsm*)data;
	(void)tid;
	bsx_intv_t *dst = A->out + A->out_off[i];
	const int64_t n = A->out_off[i + 1] - A->out_off[i];
	if (n <= 0) return;
	if (A->redo_of && A->redo_of[i] >= 0) std::copy((*A->redo)[A->redo_of[i]].begin(), (*A->redo)[A->redo_of[i]].end(), dst);
	else memcpy(dst, A->dense + A->off[i], sizeof(bsx_intv_t) * (size_t)n);
	// ks_introsort(mem_intv) (memchain.c:105): records with equal info are identical, any sort gives the reference order
	if (n > 1) std::sort(dst, dst + n, intv_info_lt);
}

// The first seeding pass of a chunk: list lengths, where the lists go, budget, quota, grid and slabs -- what rg_plan gives the chunk-wide launch of
// bsx_regions_batch, and what bsx_seed_batch launches with under the setting seed_batch_form=chunk (tests: the production launch, list for list).
struct SeedPlan {
	int mem_cap, list_cap; bool direct;
	unsigned long long direct_n, dense_cap;
	int quota, trip_budget, budget2_mul, n_slabs, grid;
	size_t scratch_bytes;
};
static SeedPlan seed_plan(const bsx_device_t *d, int64_t n, int max_len)
{
	SeedPlan S;
	// $BSX_SEED_MEM_CAP (tests): a short first-pass list, so that ordinary reads take the seeded-again path too
	S.mem_cap = bsx_tune_is_set("seed_mem_cap") ? std::max(4, (int)bsx_tune_long("seed_mem_cap", 64)) : std::max(64, max_len); S.list_cap = max_len + 2;
	const unsigned long long lf = (unsigned long long)std::max(1, (max_len + 149) / 150);   // pools are sized per 150 bases of read
	// the interval lists: strand search t's own stretch of mem_cap entries (k_seedt writes them where they stay), then room for the lists of the
	// strand searches seeded again with longer lists, which go one behind the other from the cursor
	S.direct = bsx_tune_long("seed_direct", 1) != 0 && !bsx_tune_is_set("seed_form")
	           && (unsigned long long)n * (unsigned long long)S.mem_cap <= (768ull << 20);   // (24 GB of lists: a chunk of short reads with one very long one keeps the lists one behind the other)   // ($BSX_SEED_DIRECT=0: one list behind the other, copied there when a strand search is done)
	S.direct_n = S.direct ? (unsigned long long)n * (unsigned long long)S.mem_cap : 0;
	S.dense_cap = S.direct_n + (unsigned long long)n * (S.direct ? 16 : 96) * lf + (1u << 20);
	// workgroups with a bounded life (a few tasks per lane / wave), many more of them than fit on the chip
	S.quota = (int)bsx_tune_long("seed_quota", bsx_tune_is_set("seed_form") ? 1 : 0);   // strand searches per lane, 0 = lanes take them until none is left.  The table form (k_seedt.hip) runs persistent lanes: a lane that is done takes the next strand search in the same trip (measured at hg38 scale: 68 ms against 97 with one per lane and 86 with four); the kernel without the table does best with one (292 ms against 335 with two and 359 persistent: its lanes then move through the seeding passes together)
	// extensions after which the first seeding pass hands a strand search to the second one (0: never)
	// (4096 for reads of 150 bases, which need ~1.2 k; in proportion for longer ones)
	S.trip_budget = std::max(0, (int)bsx_tune_long("seed_trip_budget", 4096));   // (the kernel scales it per 256 bases of read)
	S.budget2_mul = std::max(1, (int)bsx_tune_long("seed_budget2", 8));   // the second pass's budget, in first-pass budgets
	S.n_slabs = d->n_cu * 16;
	const int seed_wpc = 16;   // quota 0 = persistent waves, sixteen per CU
	S.grid = S.quota > 0 ? (int)((n + 256LL * S.quota - 1) / (256LL * S.quota))
	                     : (int)((std::min<int64_t>((n + 63) / 64, (int64_t)d->n_cu * seed_wpc) + 3) / 4);
	S.scratch_bytes = (size_t)S.n_slabs * 64 * seed_lane_bytes(S.mem_cap, S.list_cap);
	return S;
}

// a seeding pass over n2 strand searches whose lists overflowed: a lane each, lists eight times as long
struct SeedAgain { int grid; long long cap; size_t scratch; bool fits; };
static SeedAgain seed_again_size(size_t n2, int mem_cap, int list_cap, int n_slabs)
{
	SeedAgain s;
	s.grid = (int)((n2 + 255) / 256);
	s.cap = std::max<long long>((long long)mem_cap * 8, 1024);
	s.scratch = (size_t)s.grid * 256 * seed_lane_bytes(s.cap, list_cap);
	s.fits = s.grid * 4 <= n_slabs && s.scratch <= ((size_t)24 << 30);   // (one slab per four waves of the pass: n_slabs bounds it)
	return s;
}

static int lane_seed_batch(bsx_device_t *d, int lane, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks,
                           bsx_intv_t **out, int64_t *out_cap, int64_t *out_off)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (n == 0) { out_off[0] = 0; return BSX_OK; }
	HIPCHK(hipSetDevice(d->ordinal));
	int rc, max_len = 0;
	for (int64_t i = 0; i < n; ++i) max_len = std::max(max_len, tasks[i].len);
	if (max_len >= 1 << 18) return BSX_E_ARG;   // a lane addresses its slab with 32-bit byte offsets (seed_core.hpp): 64 lanes x 32 B x (8 x max_len) entries of the second pass must stay below 2^32
	SeedParams P;
	P.min_seed_len = opt->min_seed_len;
	P.split_len = (int)(opt->min_seed_len * opt->split_factor + .499);
	P.split_width = opt->split_width;
	P.max_mem_intv = (int)opt->max_mem_intv;
	P.start_width = (opt->flag & BSX_F_SELF_OVLP) ? 2 : 1;

	std::vector<long long> h_off((size_t)n);
	std::vector<int> h_n((size_t)n);
	std::vector<int64_t> todo;           // tasks whose interval list did not fit: redone with more room
	std::vector<bsx_seed_task_t> sub;
	int mem_cap = std::max(64, max_len);
	unsigned long long dense_cap = (unsigned long long)n * 24 * (unsigned long long)((max_len + 149) / 150 > 1 ? (max_len + 149) / 150 : 1) + 4096;   // (in proportion to the read length)
	std::vector<std::vector<bsx_intv_t>> redo_results;
	std::vector<int64_t> redo_index;
	const bsx_intv_t *h_dense = nullptr;
	std::vector<bsx_intv_t> dense_sub;
	// seed_batch_form=chunk (tests): the first launch as the chunk-wide one of bsx_regions_batch (seed_plan: its list length, lists written where
	// they stay, budget, quota, grid and slabs), what it leaves seeded again as that call's later passes do it (a lane each, lists eight times as
	// long; the second pass with seed_budget2 first-pass budgets, the ones after it without a budget), the direct lists fetched through
	// launch_gather_lists
	const char *form = bsx_tune_str("seed_batch_form");
	if (form && strcmp(form, "chunk") && strcmp(form, "batch")) { fprintf(stderr, "[bsx-hip] seed_batch_form=%s: batch or chunk\n", form); return BSX_E_ARG; }
	const bool chunk = form && !strcmp(form, "chunk");
	const SeedPlan SP = seed_plan(d, n, max_len);
	unsigned long long *const ctr0 = dev_counters(L);

	for (int round = 0; round < 6; ++round) {
		const bsx_seed_task_t *cur = tasks; int64_t cn = n;
		const int prev_cap = mem_cap;
		if (round > 0) {
			if (todo.empty()) break;
			sub.resize(todo.size());
			for (size_t i = 0; i < todo.size(); ++i) sub[i] = tasks[todo[i]];
			cur = sub.data(); cn = (int64_t)sub.size();
			if (!chunk) { mem_cap *= 8; dense_cap = (unsigned long long)cn * mem_cap + 4096; }
		}
		int list_cap = max_len + 2;
		int grid, n_slabs, quota = 0, budget = 0; size_t scratch_bytes; bool direct = false; unsigned long long cursor0 = 0;
		if (!chunk) {
			int waves = (int)std::min<int64_t>((cn + 63) / 64, (int64_t)d->n_cu * 16);
			const size_t per_lane = seed_lane_bytes(mem_cap, list_cap);
			waves = (int)std::max<size_t>(4, std::min<size_t>((size_t)waves, ((size_t)8 << 30) / (64 * per_lane)));   // (long reads seeded again with long lists: fewer waves, not tens of GB)
			grid = (waves + 3) / 4; n_slabs = grid * 4;
			scratch_bytes = (size_t)grid * 256 * per_lane;
		} else if (round == 0) {
			mem_cap = SP.mem_cap; list_cap = SP.list_cap; dense_cap = SP.dense_cap; direct = SP.direct; cursor0 = SP.direct_n;
			grid = SP.grid; n_slabs = SP.n_slabs; quota = SP.quota; budget = SP.trip_budget; scratch_bytes = SP.scratch_bytes;
		} else {
			const SeedAgain sa = seed_again_size((size_t)cn, prev_cap, list_cap, SP.n_slabs);
			if (!sa.fits || sa.cap > 0x7fffffff) { fprintf(stderr, "[bsx-hip] seed_batch: %lld strand searches to be seeded again with lists of %lld entries do not fit\n", (long long)cn, sa.cap); return BSX_E_NOMEM; }
			mem_cap = (int)sa.cap; dense_cap = (unsigned long long)cn * mem_cap + 4096;
			grid = sa.grid; n_slabs = sa.grid * 4; scratch_bytes = sa.scratch;
			budget = round == 1 ? SP.trip_budget * SP.budget2_mul : 0;
		}
		if ((rc = L.scratch.reserve(scratch_bytes)) != BSX_OK) return rc;
		if ((rc = L.jobs.reserve((size_t)cn * sizeof(bsx_seed_task_t))) != BSX_OK) return rc;
		if ((rc = L.out.reserve((size_t)dense_cap * sizeof(DevIntv))) != BSX_OK) return rc;
		if ((rc = L.aux.reserve((size_t)cn * 12 + 64)) != BSX_OK) return rc;
		if ((rc = L.qpack.reserve(seedt_pack_bytes(cn))) != BSX_OK) return rc;
		long long *d_off = (long long*)L.aux.p; int *d_n = (int*)((char*)L.aux.p + (size_t)cn * 8);
		unsigned long long *ctr = ctr0; CtrShared::Seed *sc = &ctr_shared(L)->seed;
		HIPCHK(hipMemcpyAsync(L.jobs.p, cur, (size_t)cn * sizeof(bsx_seed_task_t), hipMemcpyHostToDevice, L.st));
		HIPCHK(hipMemsetAsync(sc, 0, sizeof(*sc), L.st));   // the interval cursor and the task cursor
		if (chunk) {
			HIPCHK(hipMemsetAsync(ctr + CTR_OVERFLOW, 0, 8, L.st));   // (this pass's count of strand searches to be seeded again)
			if (cursor0) H2D(L.st, &sc->intv_cursor, &cursor0, 8);   // the cursor starts behind the strand searches' own stretches
		}
		HIPCHK(hipEventRecord(L.ev_timed_begin, L.st));
		launch_seed(L.st, grid, d->ix, (const uint8_t*)L.reads.p, (const bsx_seed_task_t*)L.jobs.p, (int)cn, P,
		            (DevIntv*)L.scratch.p, list_cap, mem_cap, (DevIntv*)L.out.p, dense_cap, &sc->intv_cursor, d_off, d_n,
		            &sc->task_cursor, ctr, quota, (unsigned int*)L.slabflags.p, n_slabs, budget, 0, (uint32_t*)L.qpack.p, direct ? 0ull : ~0ull);
		HIPCHK(hipEventRecord(L.ev_timed_end, L.st));
		if ((rc = finish_timed(L, KT_SEED_OTHER)) != BSX_OK) return rc;   // the batch form, for what the host chains: not the chunk-wide launch of KT_SEED
		std::vector<long long> r_off((size_t)cn); std::vector<int> r_n((size_t)cn);
		unsigned long long used = 0;
		D2H(L.st, r_off.data(), d_off, (size_t)cn * 8);
		D2H(L.st, r_n.data(), d_n, (size_t)cn * 4);
		D2H(L.st, &used, &sc->intv_cursor, 8);
		if (used > dense_cap) used = dense_cap;
		if (chunk && bsx_phases()) {
			unsigned long long n_over = 0;
			D2H(L.st, &n_over, ctr + CTR_OVERFLOW, 8);
			fprintf(stderr, "[M::seed_batch] chunk form, pass %d: %lld strand searches, lists of %d entries%s, budget %d, quota %d, %d workgroups, %d slabs: %llu left to be seeded again\n",
			        round + 1, (long long)cn, mem_cap, direct ? " written where they stay" : "", budget, quota, grid, n_slabs, n_over);
		}
		if (direct) { // the lists lie a strand search's stretch apart: gathered on the device, one copy (rg_declined does the same)
			std::vector<long long> which, doff;
			long long tot = 0;
			for (int64_t i = 0; i < cn; ++i) if (r_n[i] > 0) { which.push_back(i); doff.push_back(tot); tot += r_n[i]; }
			if (tot > 0) {
				const size_t nb = which.size() * 8;
				if ((rc = L.gath.reserve(2 * nb + (size_t)tot * sizeof(bsx_intv_t) + 64)) != BSX_OK) return rc;
				H2D(L.st, L.gath.p, which.data(), nb);
				H2D(L.st, (char*)L.gath.p + nb, doff.data(), nb);
				DevIntv *gd = (DevIntv*)((char*)L.gath.p + 2 * nb);
				launch_gather_lists(L.st, (const DevIntv*)L.out.p, d_off, d_n, (const long long*)L.gath.p, (const long long*)((char*)L.gath.p + nb), (long long)which.size(), gd);
				if ((rc = L.hstage.reserve((size_t)tot * sizeof(bsx_intv_t) + 64)) != BSX_OK) return rc;
				D2H(L.st, L.hstage.p, gd, (size_t)tot * sizeof(bsx_intv_t));
				for (size_t j = 0; j < which.size(); ++j) r_off[which[j]] = doff[j];
			}
			h_dense = (const bsx_intv_t*)L.hstage.p;
			used = 0;   // (nothing more to fetch from the pool)
		}
		std::vector<int64_t> next;
		if (round == 0) {
			if (!direct) {
				if ((rc = L.hstage.reserve((size_t)used * sizeof(bsx_intv_t) + 64)) != BSX_OK) return rc;
				if (used) D2H(L.st, L.hstage.p, L.out.p, (size_t)used * sizeof(bsx_intv_t));
				h_dense = (const bsx_intv_t*)L.hstage.p;
			}
			for (int64_t i = 0; i < n; ++i) { h_off[i] = r_off[i]; h_n[i] = r_n[i]; if (r_n[i] < 0) next.push_back(i); }
		} else {
			dense_sub.resize((size_t)used);
			if (used) D2H(L.st, dense_sub.data(), L.out.p, (size_t)used * sizeof(bsx_intv_t));
			for (int64_t i = 0; i < cn; ++i) {
				if (r_n[i] < 0) { next.push_back(todo[i]); continue; }
				redo_index.push_back(todo[i]);
				redo_results.emplace_back(dense_sub.begin() + r_off[i], dense_sub.begin() + r_off[i] + r_n[i]);
				h_n[todo[i]] = r_n[i];
			}
		}
		todo.swap(next);
		if (todo.empty()) break;
	}
	if (!todo.empty()) { fprintf(stderr, "[bsx-hip] seed_batch: %zu tasks still overflow\n", todo.size()); return BSX_E_INTERNAL; }

	// CSR in task order, each list ordered by info; assembled by the host worker pool
	int64_t tot = 0;
	for (int64_t i = 0; i < n; ++i) { out_off[i] = tot; tot += h_n[i]; }
	out_off[n] = tot;
	if (*out_cap < tot) { *out_cap = tot + (tot >> 2) + 16; *out = (bsx_intv_t*)realloc(*out, sizeof(bsx_intv_t) * (size_t)*out_cap); }
	std::vector<int64_t> redo_of;
	if (!redo_index.empty()) { redo_of.assign((size_t)n, -1); for (size_t r = 0; r < redo_index.size(); ++r) redo_of[redo_index[r]] = (int64_t)r; }
	SeedAsm A;
	A.off = h_off.data(); A.cnt = h_n.data(); A.dense = h_dense; A.redo_of = redo_of.empty() ? nullptr : redo_of.data(); A.redo = &redo_results;
	A.out = *out; A.out_off = out_off;
	bsx_parallel_for(bsx_host_threads(opt), seed_asm_worker, &A, (long)n);
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K1+K2 -> K3 + chaining + chain filter + chain-to-region on the device; the interval lists never leave HBM
// ------------------------------------------------------------------------------------------
// arrays carved out of a device buffer one behind the other: take<T>(count) aligns for T
struct Bump {
	char *p, *end;
	explicit Bump(const DevBuf &b) : p((char*)b.p), end((char*)b.p + b.cap) {}
	template <class T> T *take(size_t n) { p = (char*)(((size_t)p + alignof(T) - 1) & ~(size_t)(alignof(T) - 1)); T *r = (T*)p; p += n * sizeof(T); return r; }
	bool ok() const { return p <= end; }
};

// One tier sequence: the launches from tier 1 to tier 3 over a task list.  There are two: the chunk's on the lane's stream, and the side
// stream's over the strand searches seeded again there.
struct TierSeq {
	hipStream_t st; bool main_seq;
	RgLaunch G;               // tasks and their number, interval offsets and counts, region offsets and counts, position offsets
	long long *offs; int *cnts;   // (G.task_off, G.task_n as the seeding passes write them)
	unsigned char *cls;       // launch_occ: the first tier whose tables hold the strand search
	// what each launch hands on: tier 1 -> ra -> tier 1b -> rm -> tier 1c -> rl -> tier 2 -> rb -> tier 3; rc, rh: what the first and second
	// chains -> regions launches decline; x2: what tier 2 exports (tier2_export); rf: what takes that tier's full form
	int *ra, *rm, *rl, *rb, *rc, *rh, *x2, *rf;
	RgXPoolArg X;
	TierCtr *c;               // its counts and cursors in the lane's counter block (device memory)
};
// The arrays of a sequence, n entries each.  The chunk's lie in four buffers; the side sequence's one behind the other in one (the same Bump four times).
static void seq_carve(TierSeq &S, size_t n, Bump &lists, Bump &meta, Bump &xmeta, Bump &posoff)
{
	S.offs = lists.take<long long>(n); S.cnts = lists.take<int>(n);
	S.G.reg_off = meta.take<long long>(n); S.G.reg_n = meta.take<int>(n);
	for (int **q : {&S.ra, &S.rm, &S.rl, &S.rb, &S.rc, &S.rh, &S.x2, &S.rf}) *q = meta.take<int>(n);
	S.X.xoff = xmeta.take<long long>(n); S.X.xlist = xmeta.take<int>(n);
	S.G.pos_off = posoff.take<long long>(n);
	S.cls = meta.take<unsigned char>(n);
	S.G.task_off = S.offs; S.G.task_n = S.cnts; S.G.n_tasks = (int)n;
}

// what the stages of one lane_regions_batch call pass along: the call's arguments, the plan (sizes, caps, grids, the tune settings read once),
// the two sequences, and what the second seeding pass and the marks leave behind
struct RgBatch {
	bsx_device_t *d; Lane &L; int lane; const bsx_opt_t *opt; int64_t n; const bsx_seed_task_t *tasks;
	SeedParams P; RegParams R;
	int max_len = 0; bool long_reads = false, any_flt = false, export_all = false;
	int mem_cap = 0, list_cap = 0; bool seed_direct = false;
	unsigned long long direct_n = 0, dense_cap = 0, regs_cap = 0, pos_cap = 0, xcap = 0, x4_cap = 0, ssw_cap = 0;
	int seed_quota = 0, trip_budget = 0, budget2_mul = 1, reg_quota = 1, mid_quota = 1, c2r_quota = 1, n_slabs = 0;
	int grid = 0, big_grid = 0, huge_grid = 0, c2rh_grid = 0;
	int chain = 0, use_mid = 0, use_x4 = 0, tier2_export = 0; long merge_min = 0;
	bool order3 = false, early3 = false, use_1c = false, trace = false, trace_tiers = false, per_tier = false;
	TierSeq main, side;
	int *retry_e = nullptr;   // what launch_occ lists for the last HBM tier ahead of everything else
	std::vector<int> first_n;   // the first pass's counts (negative: overflowed), when the host has fetched them
	std::vector<int> merged_which; const int *merged_cnt = nullptr; bool merged = false;   // the strand searches of the second pass inside the main sequence, and where their new counts are
	std::vector<int64_t> redo;  // the strand searches that go to the side stream
	int n_marks = 0; const char *mark_name[12];
	struct timespec ts_in, ts0, ts1, ts2, ts3, ts_out;
	unsigned long long used = 0;   // regions of the main sequence
};
static double ms_between(const struct timespec &a, const struct timespec &b) { return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6; }

// stage 1: the kernels' parameters, and the seed filter's table by read length
static int rg_params(RgBatch &B)
{
	Lane &L = B.L; const bsx_opt_t *opt = B.opt; const int64_t n = B.n;
	for (int64_t i = 0; i < n; ++i) B.max_len = std::max(B.max_len, B.tasks[i].len);
	const int max_len = B.max_len;
	if (max_len >= 1 << 18) return BSX_E_ARG;   // a lane addresses its slab with 32-bit byte offsets (seed_core.hpp): 64 lanes x 32 B x (8 x max_len) entries of the second pass must stay below 2^32
	SeedParams &P = B.P;
	P.min_seed_len = opt->min_seed_len;
	P.split_len = (int)(opt->min_seed_len * opt->split_factor + .499);
	P.split_width = opt->split_width;
	P.max_mem_intv = (int)opt->max_mem_intv;
	P.start_width = (opt->flag & BSX_F_SELF_OVLP) ? 2 : 1;
	RegParams &R = B.R;
	R.a = opt->a; R.w = opt->w; R.o_del = opt->o_del; R.e_del = opt->e_del; R.o_ins = opt->o_ins; R.e_ins = opt->e_ins;
	R.pen_clip5 = opt->pen_clip5; R.pen_clip3 = opt->pen_clip3; R.min_seed_len = opt->min_seed_len; R.min_chain_weight = opt->min_chain_weight;
	R.max_chain_gap = opt->max_chain_gap; R.max_occ = opt->max_occ; R.bsstrand = opt->bsstrand; R.max_chain_extend = (uint32_t)opt->max_chain_extend;
	R.mask_level = opt->mask_level; R.drop_ratio = opt->drop_ratio; R.prof = bsx_phases() ? 1 : 0;
	R.gap_cap = -1;
	R.walk_on = 1;
	R.ext_win = (int)bsx_tune_long("ext_win", 1);
	// mem_flt_chained_seeds (memchain.c:537-548) by read length: does the seed-SW filter run, and with which threshold.  Tabulated
	// here because the rule goes through log() and the float / double conversions of the reference's expression.
	std::vector<int32_t> ft((size_t)max_len + 1, INT32_MIN);
	for (int l = 1; l <= max_len; ++l) {
		const double min_l = opt->min_chain_weight ? 1.1f * opt->min_chain_weight : 5.5f * log((double)l);
		if (min_l > 0.05f * l) continue;
		ft[l] = (int32_t)(opt->a * min_l + .499);
	}
	for (int64_t i = 0; i < n && !B.any_flt; ++i) B.any_flt = B.tasks[i].len >= 0 && ft[B.tasks[i].len] != INT32_MIN;   // (for a read of this chunk, not for some length below its longest)
	// (the table follows from the longest read, -W and -A: uploaded again only when one of them changes)
	if (!(L.fltab.p && L.flt_key[0] == max_len && L.flt_key[1] == opt->min_chain_weight && L.flt_key[2] == opt->a)) {
		TRY(L.fltab.reserve(ft.size() * 4));
		H2D(L.st, L.fltab.p, ft.data(), ft.size() * 4);
		L.flt_key[0] = max_len; L.flt_key[1] = opt->min_chain_weight; L.flt_key[2] = opt->a;
	}
	R.flt_tab = (const int32_t*)L.fltab.p; R.flt_len = max_len;
	// Chunks with reads above the short kernels' 256 bases (up to regions_long_max_query(); longer ones are chained by the caller) or with
	// the seed-SW filter active take the instantiations with longer tables, every tier exports its chains, and the filter (k_seedsw)
	// runs ahead of chains -> regions.
	B.long_reads = max_len > 256;
	B.export_all = B.long_reads || B.any_flt;
	return BSX_OK;
}

// stage 2: sizes, caps, grids and tune settings; the buffers; the main sequence's arrays and cursors
static int rg_plan(RgBatch &B)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const int64_t n = B.n; const int max_len = B.max_len;
	// the first seeding pass (seed_plan): list lengths, where the lists go, budgets, quota, grid and slabs
	const SeedPlan SP = seed_plan(d, n, max_len);
	B.mem_cap = SP.mem_cap; B.list_cap = SP.list_cap;
	// room for the interval lists (32 B each) and regions (56 B each) of the whole chunk; repeat-rich genomes average
	// dozens of intervals per strand search, and HBM is not the scarce resource here
	const unsigned long long lf = (unsigned long long)std::max(1, (max_len + 149) / 150);   // pools are sized per 150 bases of read
	B.seed_direct = SP.direct; B.direct_n = SP.direct_n;
	B.dense_cap = SP.dense_cap; B.regs_cap = (unsigned long long)n * 24 + 65536;   // (a read inside a repeat family has dozens of regions: 6 per strand search overflowed on an hg38-like genome)
	B.seed_quota = SP.quota; B.trip_budget = SP.trip_budget; B.budget2_mul = SP.budget2_mul;
	B.merge_min = bsx_tune_long("redo_merge_min", 4096);   // (tests: 1 = always merged, a huge number or a negative one = never)
	B.reg_quota = std::max(1, (int)bsx_tune_long("regions_quota", 16));
	B.n_slabs = SP.n_slabs; B.grid = SP.grid;
	const size_t scratch_bytes = SP.scratch_bytes;
	// the HBM tiers: workgroups of four waves over per-wave slabs; they are bound by the latency of their slabs, so what counts is waves in flight:
	// three workgroups per CU for the first (its kernel is held to 168 VGPRs for that and spills: 710 -> 578 ms per chunk on the hg38-like genome
	// all the same), one per CU for the second (1.3 MB of slab a wave; 222 -> 167 ms: a launch lasts as long as its largest strand search)
	// (the last tier: one workgroup of four waves per CU, or two -- "tier3_wgs"; its list longest strand search first -- "tier3_order")
	B.big_grid = d->n_cu * 3; B.huge_grid = d->n_cu * std::max(1, std::min(3, (int)bsx_tune_long("tier3_wgs", 2)));
	B.order3 = bsx_tune_long("tier3_order", 1) != 0;
	B.c2rh_grid = d->n_cu * 5;   // workgroups of the chains -> regions launch with its tables in HBM (a slab each)
	B.chain = (int)bsx_tune_long("chain_stages", 3);   // 0: none, 1: seeding, 2: seeding and regions, 3: the same but the HBM tiers (a few long strand searches on a few waves) hold nobody back (measured A/B on one box, 16 chunks: 1.76 / 1.81 M reads/s with 2, 2.00 / 1.89 M with 3)
	// tier 1 -> ra -> LDS tier with larger tables -> rm -> tier 2 (HBM slabs) -> rb -> tier 3
	B.use_mid = (int)bsx_tune_long("regions_mid", 1);
	// strand searches a wave of the larger LDS tier / of the chains -> regions launch takes before it leaves (bounded workgroup life)
	B.mid_quota = std::max(1, (int)bsx_tune_long("mid_quota", 8));
	B.c2r_quota = std::max(1, (int)bsx_tune_long("c2r_quota", 16));
	B.use_1c = bsx_tune_long("tier1c", 1) != 0;   // ($BSX_TIER1C=0: the tier sequence of rounds 2-4, for the A/B)
	B.tier2_export = (int)bsx_tune_long("tier2_export", 0);   // 1: the first HBM tier in steps (run_tiers_ordinary) instead of its monolithic form (chains, filter and extensions inline in one launch)
	// $BSX_PHASES: the main sequence's launches one by one (events between them); $BSX_TIERS: the launch times alone (no cycle counters in the kernels)
	// $BSX_PHASES=2: the stage counters read (and zeroed) after every launch of the main sequence: where each tier's wave cycles go
	B.trace = bsx_phases() != 0; B.trace_tiers = B.trace || bsx_tune_long("tiers", 0) != 0; B.per_tier = bsx_phases() == 2;
	// The last HBM tier beside the others (rg_occ_and_early_tier3): not with the exporting tiers (kilobase reads, the seed filter), and not
	// under phases=2 (the stage counters are read tier by tier).
	B.early3 = bsx_tune_long("tier3_early", 1) != 0 && !B.export_all && !B.long_reads && bsx_phases() != 2 && L.st3;
	TRY(L.scratch.reserve(scratch_bytes));
	TRY(L.jobs.reserve((size_t)n * sizeof(bsx_seed_task_t)));
	TRY(L.out.reserve((size_t)B.dense_cap * sizeof(DevIntv)));
	TRY(L.aux.reserve((size_t)n * 12 + 64));
	TRY(L.qpack.reserve(seedt_pack_bytes(n)));
	TRY(L.regs.reserve((size_t)B.regs_cap * sizeof(bsx_region_t)));
	TRY(L.regmeta.reserve((size_t)n * 49 + 64));
	// (an exporting sequence's last chains -> regions launch, RG_C2R_HL on 2 workgroups per CU, has the larger slabs)
	TRY(L.c2rslab.reserve(std::max((size_t)B.c2rh_grid * c2r_hbm_slab_bytes(false), B.export_all ? (size_t)d->n_cu * 2 * c2r_hbm_slab_bytes(true) : (size_t)0)));
	TRY(L.slabs.reserve((size_t)B.big_grid * 6 * regions_slab_bytes(2)));   // (the exporting form runs three workgroups per CU)
	TRY(L.slabs3.reserve((size_t)B.huge_grid * 4 * regions_slab_bytes(3)));
	// one u64 per seed occurrence of the chunk: ~125 per strand search against an hg38-sized genome (a 3-letter 19-mer has random
	// copies there), a few dozen against small ones.  $BSX_POS_CAP (tests): a cap small enough for strand searches to find no room.
	B.pos_cap = bsx_tune_is_set("pos_cap") ? strtoull(bsx_tune_str("pos_cap"), 0, 10) : (unsigned long long)n * 384 * lf + (1u << 20);
	TRY(L.pos.reserve((size_t)B.pos_cap * 8));
	TRY(L.posoff.reserve((size_t)n * 8 + 64));
	// what the LDS tiers export for the chains -> regions launch: ~0.5 KB per strand search (a task that finds no room goes to the next tier)
	B.xcap = (unsigned long long)n * 2560 * lf + (64u << 20);   // (a dozen chains per strand search at hg38 size: 24 + 16 bytes each, 48 more for its extensions)
	TRY(L.xpool.reserve(B.trace ? (size_t)rgx_rows_offset(B.xcap) + rgx_rows_bytes(B.xcap) : (size_t)B.xcap));   // ($BSX_PHASES: behind the pool, the rows each extension made ahead ran, rgx.hpp)
	TRY(L.xmeta.reserve((size_t)n * 12 + 64));
	// the extensions of the exported chains' best seeds are made ahead of chains -> regions, four to a wavefront (k_ext4.hip); $BSX_X4=0: all
	// of them inline in k_c2r (the tests compare the two).  Not for chunks whose lists the seed-SW filter rewrites after the export.
	B.use_x4 = (int)bsx_tune_long("x4", 1);
	B.x4_cap = (unsigned long long)n * 12 * lf + (1u << 20);
	if (B.use_x4 && !B.export_all) TRY(L.x4jobs.reserve((size_t)B.x4_cap * x4_job_bytes()));
	// the seed filter's alignments (reads of 700 bases and more: memchain.c:501-535) are one batch per chunk: a few dozen per strand search
	// ($BSX_SSW_CAP, tests: a list too short for the chunk -- what finds no room in it is aligned a wavefront at a time)
	B.ssw_cap = !B.any_flt ? 0 : bsx_tune_is_set("ssw_cap") ? std::max(8ull, strtoull(bsx_tune_str("ssw_cap"), 0, 10))
	                                   : std::min<unsigned long long>((unsigned long long)n * 24 * lf + (1u << 20), 0x3ffffff0ull);
	if (B.any_flt) TRY(L.sswjobs.reserve((size_t)B.ssw_cap * seedsw_job_bytes()));

	TierSeq &M = B.main;
	M.st = L.st; M.main_seq = true; M.c = ctr_tiers(L, true);
	Bump lists(L.aux), meta(L.regmeta), xmeta(L.xmeta), posoff(L.posoff);
	seq_carve(M, (size_t)n, lists, meta, xmeta, posoff);
	B.retry_e = meta.take<int>((size_t)n);
	if (!lists.ok() || !meta.ok() || !xmeta.ok() || !posoff.ok()) return BSX_E_INTERNAL;
	CtrShared *SH = ctr_shared(L);
	RgLaunch &G = M.G;
	G.ix = &d->ix; G.sc = &L.sc; G.P = &B.R; G.reads = (const uint8_t*)L.reads.p; G.tasks = (const bsx_seed_task_t*)L.jobs.p;
	G.seeds_dense = (const DevIntv*)L.out.p;
	G.out = (bsx_region_t*)L.regs.p; G.out_cap = B.regs_cap; G.out_cursor = &SH->region_cursor;
	G.counters = dev_counters(L); G.pos = (unsigned long long*)L.pos.p;
	TRY(ext_stop_arm(L, L.st, B.trace));   // the stopping rule's switch, and its counters under $BSX_PHASES
	// once per chunk: reads of at most 256 bases under scoring options whose extension rows fit 16 bits take the packed instantiations
	G.ext_pk = !B.long_reads && ext_pk_wanted() && ext_pk_scoring(L.sc, 0, B.max_len, true);
	++g_ext_forms[G.ext_pk ? 0 : 1];
	M.X.base = (unsigned char*)L.xpool.p; M.X.cap = B.xcap; M.X.cursor = &SH->xpool_cursor; M.X.xcount = &M.c->front.x_count;
	M.X.ext = B.use_x4 && !B.export_all ? 1 : 0;
	M.X.rows = B.trace && M.X.ext ? (unsigned int*)((unsigned char*)L.xpool.p + rgx_rows_offset(B.xcap)) : nullptr;
	return BSX_OK;
}

// stage 3 (lane's stream): the tasks up, the cursors zeroed, the chunk-wide seeding pass behind the chunk before it
static int rg_seed_first(RgBatch &B)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const int64_t n = B.n; TierSeq &M = B.main;
	CtrShared *SH = ctr_shared(L); unsigned long long *ctr = dev_counters(L);
	L.rb_tasks = n;
	L.ddl.valid = false;
	H2D(L.st, L.jobs.p, B.tasks, (size_t)n * sizeof(bsx_seed_task_t));
	HIPCHK(hipMemsetAsync(SH, 0, offsetof(CtrShared, early3), L.st));
	HIPCHK(hipMemsetAsync(&M.c->front, 0, sizeof(M.c->front), L.st));
	HIPCHK(hipMemsetAsync(&SH->early3, 0, sizeof(SH->early3), L.st));
	HIPCHK(hipMemsetAsync(ctr + CTR_OVERFLOW, 0, 8, L.st));  // (the first seeding pass's count of strand searches to be seeded again)
	HIPCHK(hipMemsetAsync(&M.c->late, 0, sizeof(M.c->late), L.st));
	HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&SH->seed.intv_cursor, (int)(uint32_t)B.direct_n, 1, L.st));            // the cursor starts behind the strand searches' own stretches
	HIPCHK(hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)&SH->seed.intv_cursor + 1), (int)(uint32_t)(B.direct_n >> 32), 1, L.st));
	if (B.chain >= 1) {
		std::lock_guard<std::mutex> g(d->chain_mu);
		if (d->chain_seed && d->chain_seed != L.ev_seed_done) HIPCHK(hipStreamWaitEvent(L.st, d->chain_seed, 0));
		// 4: front halves one after the other -- a chunk's seeding also waits for the region kernels of the chunk before it
		if (B.chain >= 4 && d->chain_regions && d->chain_regions != L.ev_regions_done) HIPCHK(hipStreamWaitEvent(L.st, d->chain_regions, 0));
	}
	HIPCHK(hipEventRecord(L.ev_timed_begin, L.st));
	launch_seed(L.st, B.grid, d->ix, M.G.reads, M.G.tasks, (int)n, B.P,
	            (DevIntv*)L.scratch.p, B.list_cap, B.mem_cap, (DevIntv*)L.out.p, B.dense_cap, &SH->seed.intv_cursor, M.offs, M.cnts,
	            &SH->seed.task_cursor, ctr, B.seed_quota, (unsigned int*)L.slabflags.p, B.n_slabs, B.trip_budget, B.R.prof, (uint32_t*)L.qpack.p, B.seed_direct ? 0ull : ~0ull);
	HIPCHK(hipEventRecord(L.ev_timed_end, L.st));
	if (B.chain >= 1) {
		std::lock_guard<std::mutex> g(d->chain_mu);
		HIPCHK(hipEventRecord(L.ev_seed_done, L.st));
		d->chain_seed = L.ev_seed_done;
	}
	return BSX_OK;
}

// stage 4 (lane's stream): the merged second pass.
// Strand searches whose interval list overflowed are seeded again with lists eight times as long.  A few of them (reads inside tandem
// repeats: ~300 k dependent FM steps on one lane, tens of milliseconds) go to the side stream and through a tier sequence of their own
// while the main one runs (rg_side_sequence).  MANY of them -- an hg38-like genome: 4 % of the strand searches, reads inside young copies of a
// repeat family, 23 ms for 43 k -- are seeded again right here and rejoin the chunk's one tier sequence (round 5): the second sequence could
// only start when the first had ended (shared slabs and export lists), and the front half waited for it as long again as for the first
// whenever the chunks in flight were in step (the command line's steady state: 8.5 s front halves).  The price is a host round trip
// between seeding and the suffix-array lookups for every chunk (the counts, 8 MB).
static int rg_seed_merged(RgBatch &B)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const int64_t n = B.n; TierSeq &M = B.main;
	CtrShared *SH = ctr_shared(L); unsigned long long *ctr = dev_counters(L);
	// Whether there are that many is the kernel's own count (CTR_OVERFLOW: 8 bytes back, not every strand search's count), and the host waits
	// for it only when the lane's last chunk came anywhere near the threshold: on a clean genome, where a few dozen overflow, nothing stands
	// between a chunk's seeding and its suffix-array lookups after the lane's first chunk.
	unsigned long long n_over = 0;
	const bool may_merge = B.merge_min >= 0 && B.merge_min <= (long)n;
	if (may_merge && (L.last_overflow < 0 || L.last_overflow >= B.merge_min / 4)) {
		HIPCHK(hipEventSynchronize(L.ev_timed_end));
		D2H(L.st, &n_over, ctr + CTR_OVERFLOW, 8);
		L.last_overflow = (long)n_over;
	}
	if (may_merge && (long)n_over >= B.merge_min) {
		B.first_n.resize((size_t)n);
		D2H(L.st, B.first_n.data(), M.cnts, (size_t)n * 4);
		std::vector<int> which;
		for (int64_t i = 0; i < n; ++i) if (B.first_n[i] < 0) which.push_back((int)i);
		const size_t n2 = which.size();
		const SeedAgain sa = seed_again_size(n2, B.mem_cap, B.list_cap, B.n_slabs);
		if ((long)n2 >= B.merge_min && n2 > 0 && n2 <= 262144 && sa.fits) {
			TRY(L.scratch2.reserve(sa.scratch));
			TRY(L.redo.reserve(n2 * (sizeof(bsx_seed_task_t) + 8 + 4 + 4) + 1024));
			L.rs.sub.resize(n2);
			for (size_t j = 0; j < n2; ++j) L.rs.sub[j] = B.tasks[which[j]];
			Bump b(L.redo);
			bsx_seed_task_t *t2 = b.take<bsx_seed_task_t>(n2);
			long long *off2 = b.take<long long>(n2); int *cnt2 = b.take<int>(n2); int *which_d = b.take<int>(n2);
			if (!b.ok()) return BSX_E_INTERNAL;
			H2D(L.st, t2, L.rs.sub.data(), n2 * sizeof(bsx_seed_task_t));
			H2D(L.st, which_d, which.data(), n2 * sizeof(int));
			HIPCHK(hipMemsetAsync(&SH->seed2_task_cursor, 0, sizeof(SH->seed2_task_cursor), L.st));
			HIPCHK(hipEventRecord(L.ev_seed2_begin, L.st));
			// (with a budget of its own, eight times the first pass's: the launch lasts as long as its slowest lane, and the handful of reads
			// inside tandem repeats -- hundreds of thousands of dependent FM steps -- made it 90-170 ms for 23 ms of work; they go on to the
			// side stream like the few of a clean genome)
			launch_seed(L.st, sa.grid, d->ix, M.G.reads, t2, (int)n2, B.P, (DevIntv*)L.scratch2.p, B.list_cap, (int)sa.cap, (DevIntv*)L.out.p, B.dense_cap, &SH->seed.intv_cursor,
			            off2, cnt2, &SH->seed2_task_cursor, ctr + CTR_SEED2, 0, (unsigned int*)L.slabflags.p, sa.grid * 4, B.trip_budget * B.budget2_mul, bsx_phases() ? 2 : 0, (uint32_t*)L.qpack.p);
			hipLaunchKernelGGL(k_patch_lists, dim3((unsigned int)((n2 + 255) / 256)), dim3(256), 0, L.st, (const int*)which_d, (int)n2, (const long long*)off2, (const int*)cnt2, M.offs, M.cnts);
			HIPCHK(hipEventRecord(L.ev_seed2_end, L.st));
			B.merged = true; B.merged_which.swap(which); B.merged_cnt = cnt2;
			if (bsx_phases()) fprintf(stderr, "[M::regions_batch] %zu strand searches seeded again inside the main sequence\n", n2);
		}
	}
	if (!B.merged) { HIPCHK(hipEventRecord(L.ev_seed2_begin, L.st)); HIPCHK(hipEventRecord(L.ev_seed2_end, L.st)); }
	return BSX_OK;
}

// stage 5 (lane's stream, then the lane's third): the suffix-array lookups, and the last HBM tier beside the others (round 6).
// That tier's launch lasts as long as its longest strand search -- 190 ms for a read inside a tandem repeat, on a device it leaves almost
// empty -- and what it takes is known as soon as the occurrences are counted (more intervals or occurrences than the tier before it holds).
// launch_occ lists those, the first tier skips them, and the launch goes to a stream of its own right behind the suffix-array lookups; what
// the first HBM tier hands on later (a strand search that grew along the way) gets the launch at the end as before.
static int rg_occ_and_early_tier3(RgBatch &B)
{
	Lane &L = B.L; bsx_device_t *d = B.d; TierSeq &M = B.main; CtrShared *SH = ctr_shared(L);
	launch_occ(L.st, d->n_cu, M.G, B.opt->max_occ, B.pos_cap, &SH->k3_cursor, M.cls, nullptr,
	           B.early3 ? B.retry_e : nullptr, B.early3 ? &SH->early3.count : nullptr);
	HIPCHK(hipEventRecord(L.ev_occ_end, L.st));
	if (B.early3) {
		HIPCHK(hipStreamWaitEvent(L.st3, L.ev_occ_end, 0));
		HIPCHK(hipEventRecord(L.ev_t3a, L.st3));
		if (B.order3) launch_order_list(L.st3, B.retry_e, &SH->early3.count, M.G.seeds_dense, M.offs, M.cnts, B.opt->max_occ);
		launch_regions_slab(L.st3, 3, B.huge_grid, M.G, B.retry_e, &SH->early3.count, &SH->early3.cursor, L.slabs3.p, nullptr, nullptr);
		HIPCHK(hipEventRecord(L.ev_t3b, L.st3));
	}
	if (B.chain >= 2) {
		std::lock_guard<std::mutex> g(d->chain_mu);
		if (d->chain_regions && d->chain_regions != L.ev_regions_done) HIPCHK(hipStreamWaitEvent(L.st, d->chain_regions, 0));
	}
	return BSX_OK;
}

// A mark between two launches of the main sequence ($BSX_PHASES, $BSX_TIERS): an event, and under $BSX_PHASES=2 the stage counters read
// and zeroed, the host waiting for the stream
static int tier_mark(RgBatch &B, const TierSeq &S, const char *name)
{
	Lane &L = B.L; unsigned long long *ctr = dev_counters(L);
	if (!S.main_seq || !B.trace_tiers || B.n_marks >= 12) return BSX_OK;
	if (!L.tier_ev[B.n_marks]) HIPCHK(hipEventCreate(&L.tier_ev[B.n_marks]));
	HIPCHK(hipEventRecord(L.tier_ev[B.n_marks], S.st)); B.mark_name[B.n_marks++] = name;
	if (!B.per_tier) return BSX_OK;
	unsigned long long pf[CTR_STAGE_N], ds[CTR_HANDON_N];
	HIPCHK(hipStreamSynchronize(S.st)); HIPCHK(hipMemcpy(pf, ctr + CTR_STAGE, sizeof(pf), hipMemcpyDeviceToHost)); HIPCHK(hipMemset(ctr + CTR_STAGE, 0, sizeof(pf)));
	HIPCHK(hipMemcpy(ds, ctr + CTR_HANDON, sizeof(ds), hipMemcpyDeviceToHost)); HIPCHK(hipMemset(ctr + CTR_HANDON, 0, sizeof(ds)));
	if (ds[2] | ds[3] | ds[4] | ds[6] | ds[8] | ds[10]) fprintf(stderr, "[M::regions_batch] %s hands on: %llu for their intervals, %llu for their occurrences (or a list too long), %llu chains, %llu tied chain starts, %llu regions, %llu an interval to be walked further\n", name, ds[8], ds[2], ds[3], ds[4], ds[6], ds[10]);
	if (pf[11]) fprintf(stderr, "[M::regions_batch] %s: seed loops: %llu seeds reached, %llu skipped as contained, %llu took the extension made ahead, %llu extended in place (%llu extensions, %llu rows)\n", name, pf[11], pf[12], pf[13], pf[14], pf[8], pf[9]);
	if (pf[9]) fprintf(stderr, "[M::regions_batch] %s: extension rows in place by query length: %llu below 64 | %llu of 64..127 | %llu of 128 and more\n", name,
	                   pf[9] - (pf[15] & 0xffffffffull) - (pf[15] >> 32), pf[15] & 0xffffffffull, pf[15] >> 32);
	double tot = 0; for (int k = 0; k < 8; ++k) tot += (double)pf[k];
	if (tot > 0) fprintf(stderr, "[M::regions_batch] %s: intervals %.1f%% occurrences %.1f%% chaining %.1f%% weights+order %.1f%% sort %.1f%% filter %.1f%% prologues+seed tests %.1f%% extension %.1f%% of %.0f M wave cycles\n", name,
	                     100 * pf[0] / tot, 100 * pf[1] / tot, 100 * pf[2] / tot, 100 * pf[3] / tot, 100 * pf[4] / tot, 100 * pf[5] / tot, 100 * pf[6] / tot, 100 * pf[7] / tot, tot * 1e-6);
	return BSX_OK;
}

#ifdef BSX_DEBUG_XCHECK
// debug builds (tools/dbg/lds_variants.sh): every exported record of the main sequence looked at before k_c2r reads it
static int xcheck_exports(RgBatch &B, const TierSeq &S)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const hipStream_t st = S.st; const RgXPoolArg &XP = S.X; const int64_t nT = S.G.n_tasks;
	unsigned long long used = 0; unsigned int xn = 0;
	HIPCHK(hipStreamSynchronize(st));
	D2H(st, &used, XP.cursor, 8); D2H(st, &xn, XP.xcount, 4);
	HIPCHK(hipStreamSynchronize(st));
	fprintf(stderr, "[xcheck] %u records, %llu bytes of %llu\n", xn, used, XP.cap);
	if (used > XP.cap) used = XP.cap;
	std::vector<unsigned char> a((size_t)used);
	std::vector<long long> xo((size_t)nT); std::vector<int> xl((size_t)xn);
	D2H(st, a.data(), XP.base, (size_t)used); D2H(st, xo.data(), XP.xoff, (size_t)nT * 8); D2H(st, xl.data(), XP.xlist, (size_t)xn * 4);
	HIPCHK(hipStreamSynchronize(st));
	std::vector<std::pair<long long, long long>> span;
	long n_bad = 0;
	for (unsigned int k = 0; k < xn; ++k) {
		const int t = xl[k];
		if (t < 0 || t >= nT) { fprintf(stderr, "[xcheck] list entry %u names task %d\n", k, t); ++n_bad; continue; }
		const long long o = xo[t];
		if (o < 0 || (unsigned long long)o + 24 > used) { fprintf(stderr, "[xcheck] task %d offset %lld\n", t, o); ++n_bad; continue; }
		const int *H = (const int*)(a.data() + o);
		const int nk = H[0], nsd = H[1], has = H[4], tier = H[5];
		const long long bytes = 24 + (long long)nk * 24 + (long long)nsd * 16 + (has ? (long long)nk * 48 : 0);
		span.push_back(std::make_pair(o, o + bytes));
		bool bad = nk <= 0 || nsd < nk || (unsigned long long)(o + bytes) > used;
		long long so_expect = 0;
		for (int c = 0; c < nk && !bad; ++c) {
			const unsigned char *xc = a.data() + o + 24 + (size_t)c * 24;
			const long long pos = *(const long long*)xc; const int rid = *(const int*)(xc + 8), so = *(const int*)(xc + 12);
			const int nm = *(const unsigned short*)(xc + 16), ne = *(const unsigned short*)(xc + 18);
			if (rid < 0 || rid >= d->ix.n_seqs || pos < 0 || pos >= 2 * d->ix.l_pac || so < so_expect || so + nm + ne > nsd) {
				fprintf(stderr, "[xcheck] task %d (len %d, tier tables %d) record at %lld: %d chains %d seeds; chain %d: pos %lld rid %d seed_off %d (expected %lld) main %d extra %d\n",
				        t, B.tasks[t].len, tier, o, nk, nsd, c, pos, rid, so, so_expect, nm, ne);
				bad = true;
			}
			so_expect = so + nm + ne;   // (k_seedsw shortens a main list in place and moves the backup list up behind it: offsets stay those of the export)
		}
		if (bad) { ++n_bad; if (nk <= 0 || nsd < nk) fprintf(stderr, "[xcheck] task %d (tier tables %d) record at %lld: %d chains %d seeds %lld bytes\n", t, tier, o, nk, nsd, bytes); }
	}
	std::sort(span.begin(), span.end());
	for (size_t k = 1; k < span.size(); ++k) if (span[k].first < span[k - 1].second) { fprintf(stderr, "[xcheck] records overlap: [%lld, %lld) and [%lld, %lld)\n", span[k - 1].first, span[k - 1].second, span[k].first, span[k].second); ++n_bad; }
	fprintf(stderr, "[xcheck] %ld bad\n", n_bad);
	return BSX_OK;
}
#endif

// the rest of a sequence whose every tier exports (kilobase reads, the seed filter): the HBM tiers, then the seed-SW filter where it applies,
// then chains -> regions (what outgrows its tables is left to the caller).  to2 / n2c: what the LDS tiers handed on
static int run_tiers_exporting(RgBatch &B, TierSeq &S, int *to2, unsigned int *n2c)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const hipStream_t st = S.st; const RgLaunch &G = S.G;
	TierCtr::Front *c = &S.c->front; TierCtr::Late *h = &S.c->late;
	const int64_t nT = G.n_tasks;
	launch_regions_slab(st, 2, B.big_grid, G, to2, n2c, &c->t2_cursor, L.slabs.p, S.rb, &c->rb_count, &S.X);
	TRY(tier_mark(B, S, "tier 2 (exports)"));
	launch_regions_slab(st, 3, B.huge_grid, G, S.rb, &c->rb_count, &c->t3_cursor, L.slabs3.p, nullptr, nullptr, &S.X);
	TRY(tier_mark(B, S, "tier 3 (exports)"));
	if (B.any_flt)   // (the side stream's run comes after the main one's on the device -- it waits for the tiers -- and may use the same job list)
		launch_seedsw(st, (int)std::min<int64_t>(nT, (int64_t)d->n_cu * 32), d->n_cu, G, S.X, &c->ssw_prep_cursor, &c->ssw_jobs, L.sswjobs.p, (unsigned int)B.ssw_cap);
	TRY(tier_mark(B, S, "seed filter"));
#ifdef BSX_DEBUG_XCHECK
	if (S.main_seq) TRY(xcheck_exports(B, S));
#endif
	// (what outgrows the launch's tables -- 64 regions of a strand search, 256 seeds of a list -- gets a second one with up to 1024 of each, the
	// regions in HBM; round 6: those were forty strand searches per chunk of kilobase reads chained on the host, a second of its time each chunk)
	launch_c2r(st, (int)((nT + 4LL * B.c2r_quota - 1) / (4LL * B.c2r_quota)), G, S.X, &c->c2r_cursor, S.rh, &h->rh_count, B.c2r_quota, B.long_reads ? RG_C2R_L : RG_C2R);
	RgXPoolArg XB3 = S.X;
	XB3.xlist = S.rh; XB3.xcount = &h->rh_count;
	launch_c2r(st, d->n_cu * 2, G, XB3, &h->c2r3_cursor, nullptr, nullptr, 1 << 30, RG_C2R_HL, L.c2rslab.p);
	TRY(tier_mark(B, S, "chains -> regions"));
	return BSX_OK;
}

// the rest of an ordinary chunk's sequence: chains -> regions of everything the LDS tiers exported; what outgrows its tables joins the list of
// the HBM tiers.
// (The first HBM tier exporting its chains as well -- 156 instead of 225 VGPRs, its chains through k_c2r with everybody else's -- was
// measured in rounds 3 and 4 and removed: what k_c2r cannot hold, 64 regions and 128 seeds a chain, takes the full form afterwards anyway,
// 1468 against 1287 ms per chunk on the hg38-like genome.  Round 6 takes it up again with a chains -> regions launch that CAN hold them.)
static int run_tiers_ordinary(RgBatch &B, TierSeq &S, int *to2, unsigned int *n2c, bool tier1c)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const hipStream_t st = S.st; const RgLaunch &G = S.G;
	TierCtr::Front *c = &S.c->front; TierCtr::Late *h = &S.c->late;
	const int c2r_grid = (int)((G.n_tasks + 4LL * B.c2r_quota - 1) / (4LL * B.c2r_quota));
	const int t2x = tier1c && S.X.ext ? B.tier2_export : 0;
	if (S.X.ext) {
		launch_x4(st, d->n_cu, G, S.X, L.x4jobs.p, B.x4_cap, S.c->x4, B.R.prof ? G.counters + CTR_EXT : nullptr);
		TRY(tier_mark(B, S, "extensions"));
	}
	if (tier1c) { // ... and what the chains -> regions launch declines (more than 64 regions, lists of more than 128 seeds) gets a second one with larger tables
		launch_c2r(st, c2r_grid, G, S.X, &c->c2r_cursor, S.rc, &c->rc_count, B.c2r_quota);
		RgXPoolArg XB2 = S.X;
		XB2.xlist = S.rc; XB2.xcount = &c->rc_count;
		if (t2x) { // ... and what THAT declines (up to 1024 regions, 1024 seeds a list) a third, the regions it makes in HBM: the record and its extensions are there
			launch_c2r(st, d->n_cu * 2, G, XB2, &c->c2r2_cursor, S.rh, &h->rh_count, 1 << 30, RG_C2R_B);
			RgXPoolArg XB3 = S.X;
			XB3.xlist = S.rh; XB3.xcount = &h->rh_count;
			launch_c2r(st, B.c2rh_grid, G, XB3, &h->c2r3_cursor, S.rf, &h->rf_count, 1 << 30, RG_C2R_H, L.c2rslab.p);
		} else
			launch_c2r(st, d->n_cu * 2, G, XB2, &c->c2r2_cursor, to2, n2c, 1 << 30, RG_C2R_B);   // (few strand searches, long ones: persistent waves)
	} else
		launch_c2r(st, c2r_grid, G, S.X, &c->c2r_cursor, to2, n2c, B.c2r_quota);
	if (S.main_seq && B.chain == 3) { // the HBM tiers (a few long strand searches on a few waves) do not hold the next chunk's region launches back
		std::lock_guard<std::mutex> g(d->chain_mu);
		HIPCHK(hipEventRecord(L.ev_regions_done, st));
		d->chain_regions = L.ev_regions_done;
	}
	TRY(tier_mark(B, S, "chains -> regions"));
	if (t2x) {
		// The first HBM tier in steps (round 6, "tier2_export=1"; measured and not the default).  What outgrew the LDS tiers'
		// tables is chained and filtered over the tier's slabs and EXPORTED like the LDS tiers' strand searches; its chains' best seeds are extended
		// ahead, several jobs to a wavefront (k_extl / k_ext4) -- inline, a wavefront each, the extensions are 58 % of the tier's cycles --; the seed
		// loop is run by the chains -> regions launch that keeps up to 1024 regions in HBM.  Only what even that cannot hold takes the tier's
		// monolithic form; what outgrows the tier's tables goes on to the last tier as before.
		RgXPoolArg XT = S.X;
		XT.xlist = S.x2; XT.xcount = &h->x2_count;
		if (t2x >= 2) XT.ext = 2;   // every seed of every main list extended ahead (a slot per seed): the seed loops of these strand searches skip one seed in fourteen
		launch_regions_slab(st, 2, B.big_grid, G, to2, n2c, &h->t2_export_cursor, L.slabs.p, S.rb, &c->rb_count, &XT);
		TRY(tier_mark(B, S, "tier 2 (chains)"));
		launch_x4(st, d->n_cu, G, XT, L.x4jobs.p, B.x4_cap, S.c->x4_t2, nullptr);
		TRY(tier_mark(B, S, "tier 2 (extensions)"));
		launch_c2r(st, B.c2rh_grid, G, XT, &h->c2r_t2_cursor, S.rf, &h->rf_count, 1 << 30, RG_C2R_H, L.c2rslab.p);
		TRY(tier_mark(B, S, "tier 2 (chains -> regions)"));
		launch_regions_slab(st, 2, B.big_grid, G, S.rf, &h->rf_count, &h->t2_full_cursor, L.slabs.p, S.rb, &c->rb_count);
	} else
		launch_regions_slab(st, 2, B.big_grid, G, to2, n2c, &c->t2_cursor, L.slabs.p, S.rb, &c->rb_count);
	TRY(tier_mark(B, S, "tier 2"));
	if (S.main_seq && B.early3) HIPCHK(hipStreamWaitEvent(st, L.ev_t3b, 0));   // (the early launch: it shares the tier's slabs, and everything behind this point waits for its regions)
	if (B.order3) launch_order_list(st, S.rb, &c->rb_count, G.seeds_dense, G.task_off, G.task_n, B.opt->max_occ);
	launch_regions_slab(st, 3, B.huge_grid, G, S.rb, &c->rb_count, &c->t3_cursor, L.slabs3.p, nullptr, nullptr);
	TRY(tier_mark(B, S, "tier 3"));
	return BSX_OK;
}

// stage 6 (the sequence's stream): the tier sequence over a task list -- the chunk's, and once more the re-seeded strand searches' on the side stream
static int run_tiers(RgBatch &B, TierSeq &S)
{
	Lane &L = B.L; const hipStream_t st = S.st; const RgLaunch &G = S.G; TierCtr::Front *c = &S.c->front;
	const int64_t nT = G.n_tasks;
	const int mid_grid = (int)((nT + 2LL * B.mid_quota - 1) / (2LL * B.mid_quota));
	TRY(tier_mark(B, S, "start"));
	launch_regions(st, (int)((nT + 4LL * B.reg_quota - 1) / (4LL * B.reg_quota)), G, &c->t1_cursor, S.ra, &c->ra_count, B.reg_quota, S.cls, S.X, B.long_reads);
	if (S.main_seq) HIPCHK(hipEventRecord(L.ev_tier1_end, st));
	TRY(tier_mark(B, S, "tier 1"));
	if (B.use_mid) launch_regions_mid(st, mid_grid, G, S.ra, &c->ra_count, &c->t1b_cursor, S.rm, &c->rm_count, S.X, B.mid_quota, B.long_reads ? RG_MID_LONGS : RG_MID);
	TRY(tier_mark(B, S, "tier 1b"));
	int *to2 = B.use_mid ? S.rm : S.ra; unsigned int *n2c = B.use_mid ? &c->rm_count : &c->ra_count;
	// a third LDS tier.  Kilobase reads: larger tables (two workgroups per CU) for what outgrows the first (three).  Ordinary reads inside
	// repeat families: twice the tables of the tier before it (round 5)
	const bool tier1c = B.use_mid && !B.long_reads && !B.export_all && B.use_1c;
	if ((B.use_mid && B.long_reads) || tier1c) {
		launch_regions_mid(st, mid_grid, G, S.rm, &c->rm_count, &c->t1c_cursor, S.rl, &c->rl_count, S.X, B.mid_quota, B.long_reads ? RG_MID_LONGB_L : RG_MID2);
		to2 = S.rl; n2c = &c->rl_count;
		TRY(tier_mark(B, S, "tier 1c"));
	}
	return B.export_all ? run_tiers_exporting(B, S, to2, n2c) : run_tiers_ordinary(B, S, to2, n2c, tier1c);
}

// stage 7 (host, then the side stream): strand searches whose interval list overflowed (reads inside tandem repeats: ~300 k dependent FM
// steps on one lane) are seeded again on the side stream with much longer lists and no trip budget, then go through the same tiers as
// everything else.  None of that is waited for here: everything is enqueued, and lane_regions_finish collects the result when the caller
// gets to the chunk's back half.
// (on a genome with hg38's repeat content these are 4 % of the strand searches -- reads inside young copies of a repeat family -- not
// the few dozen tandem-repeat reads of a clean one)
static int rg_side_sequence(RgBatch &B)
{
	Lane &L = B.L; bsx_device_t *d = B.d; const int64_t n = B.n; TierSeq &M = B.main; std::vector<int64_t> &redo = B.redo;
	CtrShared *SH = ctr_shared(L);
	clock_gettime(CLOCK_MONOTONIC, &B.ts0);
	{
		std::vector<int> s_n;
		if (!B.first_n.empty()) s_n.swap(B.first_n);
		else { s_n.resize((size_t)n); HIPCHK(hipEventSynchronize(L.ev_timed_end)); D2H(L.st2, s_n.data(), M.cnts, (size_t)n * 4); }
		for (int64_t i = 0; i < n; ++i) if (s_n[i] < 0) redo.push_back(i); else L.work[1] += (uint64_t)s_n[i];
		L.last_overflow = (long)redo.size();
		if (B.merged) { // they are in the main sequence, but for those that the second pass gave up on as well (its budget, its list)
			std::vector<int> c2(B.merged_which.size());
			HIPCHK(hipEventSynchronize(L.ev_seed2_end));
			D2H(L.st2, c2.data(), B.merged_cnt, c2.size() * 4);
			redo.clear();
			for (size_t j = 0; j < c2.size(); ++j) if (c2[j] < 0) redo.push_back(B.merged_which[j]); else L.work[1] += (uint64_t)c2[j];
		}
		if (redo.size() > 262144) redo.clear();   // (seed_again_size: n_slabs bounds the pass) leave them to the caller
	}
	clock_gettime(CLOCK_MONOTONIC, &B.ts1);
	L.rs.active = false;
	const size_t n2 = redo.size();
	const SeedAgain sa = seed_again_size(n2, B.mem_cap, B.list_cap, B.n_slabs);
	if (n2 && !sa.fits) redo.clear();
	if (!redo.empty()) {
		TRY(L.scratch2.reserve(sa.scratch));
		L.rs.tasks = redo; L.rs.sub.resize(n2); L.rs.n2u = (unsigned int)n2;
		for (size_t j = 0; j < n2; ++j) L.rs.sub[j] = B.tasks[redo[j]];
		// device side, per re-seeded strand search: task | interval offset | region offset | position offset | export offset | interval
		// count | region count | eight tier lists | export list | tier class (seq_carve)
		TRY(L.redo.reserve(n2 * (sizeof(bsx_seed_task_t) + 8 + 8 + 8 + 8 + 4 + 4 + 16 + 4 + 4 + 12 + 1) + 1024));
		TRY(L.rs.hres.reserve(n2 * 12 + 64));
		TierSeq &S = B.side;
		S = M;   // the same index, reads, pools and shared cursors
		S.st = L.st2; S.main_seq = false; S.c = ctr_tiers(L, false);
		Bump b(L.redo);
		bsx_seed_task_t *t2 = b.take<bsx_seed_task_t>(n2);
		seq_carve(S, n2, b, b, b, b);
		if (!b.ok()) return BSX_E_INTERNAL;
		S.G.tasks = t2; S.X.xcount = &S.c->front.x_count;
		HIPCHK(hipMemcpyAsync(t2, L.rs.sub.data(), n2 * sizeof(bsx_seed_task_t), hipMemcpyHostToDevice, L.st2));
		HIPCHK(hipMemsetAsync(&S.c->front, 0, sizeof(S.c->front), L.st2));
		HIPCHK(hipMemsetAsync(&S.c->late, 0, sizeof(S.c->late), L.st2));
		launch_seed(L.st2, sa.grid, d->ix, S.G.reads, t2, (int)n2, B.P, (DevIntv*)L.scratch2.p, B.list_cap, (int)sa.cap, (DevIntv*)L.out.p, B.dense_cap, &SH->seed.intv_cursor,
		            S.offs, S.cnts, &S.c->front.seed_task_cursor, S.G.counters + CTR_SEED3, 0, (unsigned int*)L.slabflags.p, sa.grid * 4, 0, 0, (uint32_t*)L.qpack.p);   // (the main launch is over: its packed reads are no longer needed)
		HIPCHK(hipStreamWaitEvent(L.st2, L.rs.ev_tiers, 0));   // the slabs of the HBM tiers and the export pool's lists are shared with the main launch sequence
		launch_occ(L.st2, d->n_cu, S.G, B.opt->max_occ, B.pos_cap, &SH->k3_cursor, S.cls, &S.c->front.k3_start);
		TRY(run_tiers(B, S));
		HIPCHK(hipMemcpyAsync(L.rs.hres.p, S.G.reg_off, n2 * 8, hipMemcpyDeviceToHost, L.st2));
		HIPCHK(hipMemcpyAsync((char*)L.rs.hres.p + n2 * 8, S.G.reg_n, n2 * 4, hipMemcpyDeviceToHost, L.st2));
		HIPCHK(hipEventRecord(L.rs.ev, L.st2));
		L.rs.active = true;
	}
	clock_gettime(CLOCK_MONOTONIC, &B.ts2);
	return BSX_OK;
}

// stage 8 (host): wait for the main sequence, and put its launches' times into the lane's slots
static int rg_wait_and_time(RgBatch &B)
{
	Lane &L = B.L; unsigned long long *ctr = dev_counters(L);
	float ms0 = 0, ms1 = 0, ms2 = 0, ms3 = 0, ms_again = 0;
	HIPCHK(hipEventRecord(L.ev_tiers_end, L.st));
	HIPCHK(hipEventSynchronize(L.ev_tiers_end));
	clock_gettime(CLOCK_MONOTONIC, &B.ts3);
	if (B.trace_tiers && B.n_marks > 1) {
		fprintf(stderr, "[M::regions_batch] region launches (ms):");
		for (int k = 1; k < B.n_marks; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, L.tier_ev[k - 1], L.tier_ev[k]) == hipSuccess) fprintf(stderr, " %s %.1f |", B.mark_name[k], ms); }
		if (B.early3) { float ms = 0; unsigned int ne = 0; D2H(L.st, &ne, &ctr_shared(L)->early3.count, 4); if (hipEventElapsedTime(&ms, L.ev_t3a, L.ev_t3b) == hipSuccess) fprintf(stderr, " tier 3 beside them (%u strand searches) %.1f |", ne, ms); }
		fprintf(stderr, "\n");
	}
	if (B.trace) fprintf(stderr, "[M::regions_batch] seed kernel done +%.0f ms | redo of %zu strand searches enqueued +%.0f ms | all region tiers done +%.0f ms\n",
	                     ms_between(B.ts0, B.ts1), B.redo.size(), ms_between(B.ts0, B.ts2), ms_between(B.ts0, B.ts3));
	HIPCHK(hipEventElapsedTime(&ms0, L.ev_timed_begin, L.ev_timed_end));
	HIPCHK(hipEventElapsedTime(&ms_again, L.ev_seed2_begin, L.ev_seed2_end));   // the second seeding pass, when it ran inside this sequence
	if (B.merged && B.trace) { // requests per strand search of the second pass, by power of two (k_seedt, prof & 2)
		unsigned long long hh[CTR_SEED_HIST_N];
		HIPCHK(hipMemcpy(hh, ctr + CTR_SEED2 + CTR_SEED_HIST, sizeof(hh), hipMemcpyDeviceToHost)); HIPCHK(hipMemset(ctr + CTR_SEED2 + CTR_SEED_HIST, 0, sizeof(hh)));
		fprintf(stderr, "[M::regions_batch] second seeding pass %.1f ms (budget %d requests); strand searches by requests made, < 2^k:", ms_again, B.trip_budget * B.budget2_mul);
		for (int k = 0; k < CTR_SEED_HIST_N; ++k) if (hh[k]) fprintf(stderr, " k=%d: %llu |", k, hh[k]);
		fprintf(stderr, "\n");
	}
	if (B.merged) { L.k_ms[KT_SEED_OTHER] += ms_again; L.k_launch[KT_SEED_OTHER] += 1; L.seed2_ms += ms_again; L.seed2_launches += 1; L.seed2_tasks += (uint64_t)B.merged_which.size(); }
	HIPCHK(hipEventElapsedTime(&ms3, L.ev_seed2_end, L.ev_occ_end));   // K3 for the chunk (k_occ_expand + k_occ)
	L.k_ms[KT_K3] += ms3; L.k_launch[KT_K3] += 1;
	HIPCHK(hipEventElapsedTime(&ms1, L.ev_occ_end, L.ev_tier1_end));   // the first region tier alone
	HIPCHK(hipEventElapsedTime(&ms2, L.ev_tier1_end, L.ev_tiers_end));   // the later tiers and the wait for the early launch of the last one
	L.k_ms[KT_SEED] += ms0; L.k_launch[KT_SEED] += 1; L.k_ms[KT_TIER1] += ms1; L.k_launch[KT_TIER1] += 1; L.k_ms[KT_TIERS_LATER] += ms2; L.k_launch[KT_TIERS_LATER] += 1;
	HIPCHK(hipGetLastError());
	return BSX_OK;
}

// stage 9 (host): offsets, counts and regions of the main sequence down
static int rg_download(RgBatch &B, bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n)
{
	Lane &L = B.L; const int64_t n = B.n; TierSeq &M = B.main; CtrShared *SH = ctr_shared(L);
	unsigned long long used = 0;
	std::vector<long long> h_off((size_t)n);
	D2H(L.st, h_off.data(), M.G.reg_off, (size_t)n * 8);
	D2H(L.st, out_n, M.G.reg_n, (size_t)n * 4);
	D2H(L.st, &used, &SH->region_cursor, 8);
	if (used > B.regs_cap) used = B.regs_cap;
	{ // work of the chunk (bsx_device_region_work)
		unsigned long long n_occ = 0;
		D2H(L.st, &n_occ, &SH->k3_cursor, 8);
		L.work[0] += (uint64_t)n; L.work[2] += n_occ < B.pos_cap ? n_occ : B.pos_cap; L.work[3] += used;
		for (int64_t i = 0; i < n; ++i) L.work[4] += (uint64_t)(B.tasks[i].len > 0 ? B.tasks[i].len : 0);
	}
	for (int64_t i = 0; i < n; ++i) out_off[i] = h_off[i];
	L.rs.used_main = used; L.rs.regs_cap = B.regs_cap;
	for (size_t j = 0; j < B.redo.size(); ++j) out_n[B.redo[j]] = BSX_REGIONS_PENDING;   // lane_regions_finish fills these in
	if (*out_cap < (int64_t)used + 65536) { *out_cap = (int64_t)used + 65536; *out = (bsx_region_t*)realloc(*out, sizeof(bsx_region_t) * (size_t)*out_cap); }
	D2H(L.st, *out, L.regs.p, (size_t)used * sizeof(bsx_region_t));
	B.used = used;
	return BSX_OK;
}

// stage 10 (host, $BSX_PHASES): what the chunk's counters say, read and zeroed
static int rg_report(RgBatch &B)
{
	Lane &L = B.L; unsigned long long *ctr = dev_counters(L);
	CtrShared sh; TierCtr tc;
	D2H(L.st, &tc, B.main.c, sizeof(tc));
	D2H(L.st, &sh, ctr_shared(L), sizeof(sh));
	const TierCtr::Front &f = tc.front;
	fprintf(stderr, "[M::regions_batch] %lld strand searches: %llu intervals, %llu occurrences looked up ahead | left tier 1: %u, left tier 1b: %u, reached tier 2: %u, left tier 2: %u | second chains -> regions launch: %u | every tier exports: %d\n",
	        (long long)B.n, sh.seed.intv_cursor, sh.k3_cursor, f.ra_count, f.rm_count, B.long_reads || B.export_all ? f.rl_count : f.rl_count ? f.rl_count : f.rm_count, f.rb_count, f.rc_count, B.export_all ? 1 : 0);
	unsigned long long sp[CTR_SEED_N];
	D2H(L.st, sp, ctr + CTR_SEED_CYC, sizeof(sp));
	HIPCHK(hipMemsetAsync(ctr + CTR_SEED_CYC, 0, sizeof(sp), L.st));
	if (sp[0]) fprintf(stderr, "[M::regions_batch] k_seed: %.0f M wave cycles, %.1f%% in the full machine (%llu passes, %.0f cycles each), publishing %.1f%% | %llu wave trips, %.0f cycles per trip\n",
	                   sp[0] * 1e-6, 100.0 * sp[1] / sp[0], sp[4], sp[4] ? (double)sp[1] / sp[4] : 0.0, 100.0 * sp[2] / sp[0], sp[3], sp[3] ? (double)sp[0] / sp[3] : 0.0);
	unsigned long long tq[CTR_SEEDT_N];
	D2H(L.st, tq, ctr + CTR_SEEDT_HOT, sizeof(tq));
	HIPCHK(hipMemsetAsync(ctr + CTR_SEEDT_HOT, 0, sizeof(tq), L.st));
	if (sp[0] && tq[3]) fprintf(stderr, "[M::regions_batch] k_seedt: short machine %.1f%%, fetch %.1f%%, post %.1f%% of the wave cycles | %.1f requests per wave trip\n",
	                            100.0 * tq[0] / sp[0], 100.0 * tq[1] / sp[0], 100.0 * tq[2] / sp[0], sp[3] ? (double)tq[3] / sp[3] : 0.0);
	unsigned long long xp[CTR_EXT_N];
	D2H(L.st, xp, ctr + CTR_EXT, sizeof(xp));
	HIPCHK(hipMemsetAsync(ctr + CTR_EXT, 0, sizeof(xp), L.st));
	if (xp[EXT4_JOBS] || xp[EXTL_JOBS]) fprintf(stderr, "[M::regions_batch] k_ext4: %llu jobs, %llu rows in %llu wave trips (%.2f rows per trip), %llu passes between extensions, %.2f slots per trip, %llu rows of narrow jobs\n", xp[0], xp[1], xp[2], xp[2] ? (double)xp[1] / xp[2] : 0.0, xp[3], xp[2] ? (double)xp[4] / xp[2] : 0.0, xp[5]);
	if (xp[EXTL_JOBS]) fprintf(stderr, "[M::regions_batch] k_extl: %llu jobs (%llu sent on to k_ext4), %llu rows in %llu wave trips (%.1f rows per trip), %llu passes between extensions\n", xp[6], xp[10], xp[7], xp[8], xp[8] ? (double)xp[7] / xp[8] : 0.0, xp[9]);
	{ // the extensions' stopping rule (ext_stop_rule.h), per launch family
		unsigned long long xs[XS_FAM_N * XS_N];
		int rc = ext_stop_collect(L, L.st, xs);
		if (rc != BSX_OK) return rc;
		static const char *fam[XS_FAM_N] = {"k_ext4", "k_extl", "tiers", "k_c2r", "batch"};
		for (int k = 0; k < XS_FAM_N; ++k) if (xs[XS_N * k + XS_EVALS])
			fprintf(stderr, "[M::regions_batch] ext_stop=%d %s: %llu extensions stopped by the rule, %llu evaluations, %llu rows still to run at the stops | the switch off: %llu would have stopped, %llu rows run after the rule would have fired\n",
			        L.sc.ext_stop, fam[k], xs[XS_N * k + XS_STOPS], xs[XS_N * k + XS_EVALS], xs[XS_N * k + XS_LEFT], xs[XS_N * k + XS_WOULD], xs[XS_N * k + XS_DEAD]);
	}
	unsigned long long xw[CTR_X4W_N];
	D2H(L.st, xw, ctr + CTR_X4W, sizeof(xw));
	HIPCHK(hipMemsetAsync(ctr + CTR_X4W, 0, sizeof(xw), L.st));
	if (xp[EXT4_JOBS] || xp[EXTL_JOBS]) for (int k = 0; k < 2; ++k)   // the extensions made ahead that the seed loops never read (first seed of a chain skipped as contained)
		fprintf(stderr, "[M::regions_batch] %s: unread jobs %llu with %llu rows (%.3f%% of the kernel's rows) | of which inside the strand search's first region: %llu jobs, %llu rows (%.4f%%)\n",
		        k ? "k_extl" : "k_ext4", xw[4 * k + X4W_JOBS], xw[4 * k + X4W_ROWS], xp[k ? EXTL_ROWS : EXT4_ROWS] ? 100.0 * xw[4 * k + X4W_ROWS] / xp[k ? EXTL_ROWS : EXT4_ROWS] : 0.0,
		        xw[4 * k + X4W_JOBS_R0], xw[4 * k + X4W_ROWS_R0], xp[k ? EXTL_ROWS : EXT4_ROWS] ? 100.0 * xw[4 * k + X4W_ROWS_R0] / xp[k ? EXTL_ROWS : EXT4_ROWS] : 0.0);
	unsigned long long pf[CTR_STAGE_N];
	D2H(L.st, pf, ctr + CTR_STAGE, sizeof(pf));
	HIPCHK(hipMemsetAsync(ctr + CTR_STAGE, 0, sizeof(pf), L.st));
	double tot = 0; for (int k = 0; k < 8; ++k) tot += (double)pf[k];
	if (tot > 0) fprintf(stderr, "[M::regions_batch] wave cycles by stage (all tiers): intervals %.1f%% occurrences %.1f%% chaining %.1f%% weights+order %.1f%% sort %.1f%% filter %.1f%% chain prologues+seed tests %.1f%% extension %.1f%% | %.0f M cycles, %llu extensions, %llu rows\n",
	        100 * pf[0] / tot, 100 * pf[1] / tot, 100 * pf[2] / tot, 100 * pf[3] / tot, 100 * pf[4] / tot, 100 * pf[5] / tot, 100 * pf[6] / tot, 100 * pf[7] / tot, tot * 1e-6, pf[8], pf[9]);
	if (pf[10]) fprintf(stderr, "[M::regions_batch] seed filter: %llu alignments\n", pf[10]);
	if (pf[11]) fprintf(stderr, "[M::regions_batch] seed loops (mem_chain2region1): %llu seeds reached, %llu skipped as contained, %llu took the extension made ahead, %llu extended in place\n", pf[11], pf[12], pf[13], pf[14]);
	// the HBM tiers: how long their strand searches take (a wave each)
	unsigned long long tk[2 * CTR_TIER_TIME_N];
	D2H(L.st, tk, ctr + CTR_TIER2_TIME, sizeof(tk));
	HIPCHK(hipMemsetAsync(ctr + CTR_TIER2_TIME, 0, sizeof(tk), L.st));
	for (int k = 0; k < 2; ++k) if (tk[4 * k + 2])
		fprintf(stderr, "[M::regions_batch] tier %d: %llu strand searches, %.2f M cycles each on average, the longest %.1f M, the busiest wave %.1f M, all of them %.0f M\n",
		        2 + k, tk[4 * k + 2], 1e-6 * tk[4 * k + 1] / tk[4 * k + 2], 1e-6 * tk[4 * k], 1e-6 * tk[4 * k + 3], 1e-6 * tk[4 * k + 1]);
	unsigned long long th[CTR_T3_N];
	D2H(L.st, th, ctr + CTR_T3_LONGEST, sizeof(th));
	HIPCHK(hipMemsetAsync(ctr + CTR_T3_LONGEST, 0, sizeof(th), L.st));
	if (th[0]) {
		fprintf(stderr, "[M::regions_batch] tier 3: the longest strand search: %.1f M cycles, %llu intervals, %llu chains kept, %llu regions | strand searches by duration, < 2^k x 65536 cycles:",
		        (double)(th[0] >> 36) * 4096e-6, (th[0] >> 24) & 4095, (th[0] >> 14) & 16383, th[0] & 16383);
		for (int k = 0; k < CTR_T3_HIST_N; ++k) if (th[2 + k]) fprintf(stderr, " k=%d: %llu |", k, th[2 + k]);
		fprintf(stderr, "\n");
	}
	return BSX_OK;
}

// stage 11 (host): declined tasks: hand their interval lists back (ordered by info, as bsx_seed_batch returns them)
static int rg_declined(RgBatch &B, const int32_t *out_n, bsx_intv_t **decl_intv, int64_t *decl_cap, int64_t *decl_off)
{
	Lane &L = B.L; const int64_t n = B.n; TierSeq &M = B.main;
	std::vector<int64_t> decl;
	for (int64_t i = 0; i < n; ++i) if (out_n[i] < -1 && out_n[i] != BSX_REGIONS_PENDING) decl.push_back(i);
	decl_off[0] = 0;
	if (decl.empty()) return BSX_OK;
	std::vector<long long> s_off((size_t)n); std::vector<int> s_n((size_t)n);
	D2H(L.st, s_off.data(), M.offs, (size_t)n * 8);
	D2H(L.st, s_n.data(), M.cnts, (size_t)n * 4);
	int64_t tot = 0;
	for (size_t j = 0; j < decl.size(); ++j) { decl_off[j] = tot; tot += s_n[decl[j]]; }
	decl_off[decl.size()] = tot;
	if (*decl_cap < tot) { *decl_cap = tot + (tot >> 2) + 16; *decl_intv = (bsx_intv_t*)realloc(*decl_intv, sizeof(bsx_intv_t) * (size_t)*decl_cap); }
	const bsx_intv_t *dense = nullptr;
	if (decl.size() > 256 && tot > 0) { // many: their lists gathered on the device (they lie a strand search's stretch apart), one copy
		std::vector<long long> which(decl.begin(), decl.end()), doff(decl_off, decl_off + decl.size());
		for (size_t j = 0; j < decl.size(); ++j) if (s_n[decl[j]] < 0) { which.clear(); break; }   // (a list that did not fit has no entries to fetch: leave the one-by-one path to skip it)
		if (!which.empty()) {
			const size_t nb = decl.size() * 8;
			TRY(L.gath.reserve(2 * nb + (size_t)tot * sizeof(bsx_intv_t) + 64));
			H2D(L.st, L.gath.p, which.data(), nb);
			H2D(L.st, (char*)L.gath.p + nb, doff.data(), nb);
			DevIntv *gd = (DevIntv*)((char*)L.gath.p + 2 * nb);
			launch_gather_lists(L.st, (const DevIntv*)L.out.p, M.offs, M.cnts, (const long long*)L.gath.p, (const long long*)((char*)L.gath.p + nb), (long long)decl.size(), gd);
			TRY(L.hstage.reserve((size_t)tot * sizeof(bsx_intv_t) + 64));
			D2H(L.st, L.hstage.p, gd, (size_t)tot * sizeof(bsx_intv_t));
			dense = (const bsx_intv_t*)L.hstage.p;
		}
	}
	for (size_t j = 0; j < decl.size(); ++j) {
		const int64_t i = decl[j]; const int cnt = s_n[i];
		bsx_intv_t *dst = *decl_intv + decl_off[j];
		if (cnt <= 0) continue;
		if (dense) memcpy(dst, dense + decl_off[j], sizeof(bsx_intv_t) * (size_t)cnt);
		else D2H(L.st, dst, (const bsx_intv_t*)L.out.p + s_off[i], sizeof(bsx_intv_t) * (size_t)cnt);
		if (cnt > 1) std::sort(dst, dst + cnt, intv_info_lt);
	}
	return BSX_OK;
}

// The chunk's front half behind the seeding: the stages above in order.  The host waits at four points: for the seeding pass when the second
// may have to be merged in (rg_seed_merged) and for its counts (rg_side_sequence), for the main sequence (rg_wait_and_time), and -- in
// lane_regions_finish -- for the side stream.
static int lane_regions_batch(bsx_device_t *d, int lane, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks,
                              bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n,
                              bsx_intv_t **decl_intv, int64_t *decl_cap, int64_t *decl_off)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (n == 0) return BSX_OK;
	if (n > 0x7fffffff) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	RgBatch B = {d, d->lane[lane], lane, opt, n, tasks};
	Lane &L = B.L;
	clock_gettime(CLOCK_MONOTONIC, &B.ts_in);
	TRY(rg_params(B));
	TRY(rg_plan(B));
	TRY(rg_seed_first(B));
	TRY(rg_seed_merged(B));
	TRY(rg_occ_and_early_tier3(B));
	TRY(run_tiers(B, B.main));
	if (B.chain == 2 || B.chain >= 4) {
		std::lock_guard<std::mutex> g(d->chain_mu);
		HIPCHK(hipEventRecord(L.ev_regions_done, L.st));
		d->chain_regions = L.ev_regions_done;
	}
	HIPCHK(hipEventRecord(L.rs.ev_tiers, L.st));
	TRY(rg_side_sequence(B));
	TRY(rg_wait_and_time(B));
	TRY(rg_download(B, out, out_cap, out_off, out_n));
	if (B.trace) TRY(rg_report(B));
	clock_gettime(CLOCK_MONOTONIC, &B.ts_out);
	if (B.trace) fprintf(stderr, "[M::regions_batch] entry to kernels enqueued %.0f ms | tiers done to regions downloaded %.0f ms (%llu regions)\n",
	                     ms_between(B.ts_in, B.ts0), ms_between(B.ts3, B.ts_out), B.used);
	TRY(rg_declined(B, out_n, decl_intv, decl_cap, decl_off));
	if (B.trace) { // one line per call, with the lane: lines of chunks in flight together interleave
		struct timespec te; clock_gettime(CLOCK_MONOTONIC, &te);
		fprintf(stderr, "[M::regions_batch] lane %d from %.3f: %.0f ms = enqueue %.0f + seeding awaited %.0f + second pass enqueued %.0f + tiers awaited %.0f + counts and regions down %.0f + the rest %.0f\n",
		        lane, B.ts_in.tv_sec % 1000 + B.ts_in.tv_nsec * 1e-9, ms_between(B.ts_in, te), ms_between(B.ts_in, B.ts0), ms_between(B.ts0, B.ts1), ms_between(B.ts1, B.ts2), ms_between(B.ts2, B.ts3), ms_between(B.ts3, B.ts_out), ms_between(B.ts_out, te));
	}
	return BSX_OK;
}

// the strand searches lane_regions_batch left pending: their regions are appended to *out, out_off/out_n filled in
// (out_n = -1: even the longest lists or the largest tier did not hold them, the caller seeds and chains them itself)
static int lane_regions_finish(bsx_device_t *d, int lane, bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (!L.rs.active) return BSX_OK;
	HIPCHK(hipSetDevice(d->ordinal));
	struct timespec ta, tb;
	clock_gettime(CLOCK_MONOTONIC, &ta);
	HIPCHK(hipEventSynchronize(L.rs.ev));
	clock_gettime(CLOCK_MONOTONIC, &tb);
	if (bsx_phases()) fprintf(stderr, "[M::regions_finish] waited %.0f ms for %zu strand searches seeded again\n", (tb.tv_sec - ta.tv_sec) * 1e3 + (tb.tv_nsec - ta.tv_nsec) * 1e-6, L.rs.tasks.size());
	HIPCHK(hipGetLastError());
	const size_t n2 = L.rs.tasks.size();
	const long long *roff = (const long long*)L.rs.hres.p;
	const int *rn = (const int*)((const char*)L.rs.hres.p + n2 * 8);
	int64_t used = (int64_t)L.rs.used_main;
	// their regions lie behind the main sequence's in the device's pool: one copy of that stretch (a copy per strand search was tens
	// of thousands of small transfers per chunk on a repeat-rich genome), then each list is taken from it
	unsigned long long used_all = 0;
	D2H(L.st2, &used_all, &ctr_shared(L)->region_cursor, 8);
	if (used_all > L.rs.regs_cap) used_all = L.rs.regs_cap;   // (a cursor past the pool: the strand searches that found no room carry status 7)
	const unsigned long long lo = L.rs.used_main, hi = std::max<unsigned long long>(used_all, lo);
	std::vector<bsx_region_t> stretch;
	if (hi > lo) {
		bool any = false;
		for (size_t j = 0; j < n2 && !any; ++j) any = rn[j] > 0;
		if (any) { stretch.resize((size_t)(hi - lo)); D2H(L.st2, stretch.data(), (const bsx_region_t*)L.regs.p + lo, sizeof(bsx_region_t) * (size_t)(hi - lo)); }
	}
	long hist[16] = {0};
	for (size_t j = 0; j < n2; ++j) {
		const int64_t i = L.rs.tasks[j];
		if (rn[j] < 0) { out_n[i] = -1; out_off[i] = 0; ++hist[(-rn[j]) & 15]; continue; }
		if (*out_cap < used + rn[j]) { *out_cap = used + rn[j] + 1024 + (*out_cap >> 2); *out = (bsx_region_t*)realloc(*out, sizeof(bsx_region_t) * (size_t)*out_cap); }
		if (rn[j] > 0) {
			if (!stretch.empty() && (unsigned long long)roff[j] >= lo && (unsigned long long)roff[j] + (unsigned long long)rn[j] <= hi)
				memcpy(*out + used, stretch.data() + ((unsigned long long)roff[j] - lo), sizeof(bsx_region_t) * (size_t)rn[j]);
			else D2H(L.st2, *out + used, (const bsx_region_t*)L.regs.p + roff[j], sizeof(bsx_region_t) * (size_t)rn[j]);
		}
		out_off[i] = used; out_n[i] = rn[j];
		used += rn[j];
	}
	if (bsx_phases()) {
		fprintf(stderr, "[M::regions_finish] left to the caller after the second pass, by reason:");
		for (int k = 1; k < 16; ++k) if (hist[k]) fprintf(stderr, " %d: %ld", k, hist[k]);
		fprintf(stderr, "\n");
	}
	L.rs.active = false;
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K3
// ------------------------------------------------------------------------------------------
static int lane_sa_batch(bsx_device_t *d, int lane, int64_t n, const bsx_sa_job_t *jobs, uint64_t *pos)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (n == 0) return BSX_OK;
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_sa_job_t))) != BSX_OK) return rc;
	if ((rc = L.res.reserve((size_t)n * 8)) != BSX_OK) return rc;
	HIPCHK(hipMemcpyAsync(L.jobs.p, jobs, (size_t)n * sizeof(bsx_sa_job_t), hipMemcpyHostToDevice, L.st));
	int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)d->n_cu * 8);
	HIPCHK(hipEventRecord(L.ev_timed_begin, L.st));
	launch_sa(L.st, grid, d->ix, (const bsx_sa_job_t*)L.jobs.p, (long long)n, (uint64_t*)L.res.p, dev_counters(L));
	HIPCHK(hipEventRecord(L.ev_timed_end, L.st));
	if ((rc = finish_timed(L, KT_K3)) != BSX_OK) return rc;
	D2H(L.st, pos, L.res.p, (size_t)n * 8);
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K4
// ------------------------------------------------------------------------------------------
static int lane_extend_batch(bsx_device_t *d, int lane, int64_t n, const bsx_ext_job_t *jobs, bsx_ext_res_t *res)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (n == 0) return BSX_OK;
	HIPCHK(hipSetDevice(d->ordinal));
	if (bsx_tune_is_set("ext4")) { // tests: the batch through the quarter-wave kernel of the regions path (k_ext4.hip); jobs it declines fail the call
		int rc, max_q = 0;
		if ((rc = ext_stop_arm(L, L.st, true)) != BSX_OK) return rc;
		for (int64_t i = 0; i < n; ++i) max_q = std::max(max_q, jobs[i].qlen);
		if ((max_q > x4_max_query(16) && bsx_tune_long("ext4", 0) != 3) || n > 0x7fffffff) return BSX_E_ARG;
		if (bsx_tune_long("ext4", 0) == 4) { // ... or the wavefront-per-job form of the region kernels' inline extensions: packed 16-bit rows (ext_dp_pk) when the batch passes the guard, else 32-bit
			long long hmax = 0;
			for (int64_t i = 0; i < n; ++i) hmax = std::max(hmax, (long long)jobs[i].h0 + (long long)jobs[i].qlen * (jobs[i].parent ? L.sc.mx_ct : L.sc.mx_ga));
			const bool packed = ext_pk_wanted() && ext_pk_scoring(L.sc, hmax, max_q, false);
			if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_ext_job_t))) != BSX_OK) return rc;
			if ((rc = L.res.reserve((size_t)n * sizeof(bsx_ext_res_t))) != BSX_OK) return rc;
			HIPCHK(hipMemcpyAsync(L.jobs.p, jobs, (size_t)n * sizeof(bsx_ext_job_t), hipMemcpyHostToDevice, L.st));
			launch_extpk_batch(L.st, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (bsx_ext_res_t*)L.res.p, (long long)n, packed);
			++g_ext_forms[packed ? 0 : 1];
			HIPCHK(hipGetLastError());
			D2H(L.st, res, L.res.p, (size_t)n * sizeof(bsx_ext_res_t));
			if ((rc = ext_stop_collect(L, L.st, nullptr)) != BSX_OK) return rc;
			L.sc.xs_ctr = nullptr;
			for (int64_t i = 0; i < n; ++i) if (res[i].score == X4_DECLINED) return BSX_E_ARG;
			return BSX_OK;
		}
		if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_ext_job_t))) != BSX_OK) return rc;
		if ((rc = L.res.reserve((size_t)n * sizeof(bsx_ext_res_t))) != BSX_OK) return rc;
		if ((rc = L.aux.reserve(64)) != BSX_OK) return rc;
		HIPCHK(hipMemcpyAsync(L.jobs.p, jobs, (size_t)n * sizeof(bsx_ext_job_t), hipMemcpyHostToDevice, L.st));
		HIPCHK(hipMemsetAsync(L.aux.p, 0, 64, L.st));
		if (bsx_tune_long("ext4", 0) != 3) launch_ext4_batch(L.st, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (bsx_ext_res_t*)L.res.p, (unsigned int)n, (unsigned int*)L.aux.p, max_q);
		if (bsx_tune_long("ext4", 0) == 3) { // ... or the wavefront-per-job form whose rows follow the band in a register window (ext_dp_win: the long reads' chains -> regions launch)
			launch_extwin_batch(L.st, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (bsx_ext_res_t*)L.res.p, (long long)n);
		} else
		if (bsx_tune_long("ext4", 0) == 2) { // then the lane-per-job kernel (k_extl.hip) over the same jobs: its answers replace the others'
			HIPCHK(hipMemsetAsync(L.aux.p, 0, 64, L.st));
			launch_extl_batch(L.st, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (bsx_ext_res_t*)L.res.p, (unsigned int)n, (unsigned int*)L.aux.p);
			unsigned int c[4]; D2H(L.st, c, L.aux.p, 16);
			fprintf(stderr, "[M::extl] %lld jobs, %u left to k_ext4\n", (long long)n, c[0]);
		}
		HIPCHK(hipGetLastError());
		D2H(L.st, res, L.res.p, (size_t)n * sizeof(bsx_ext_res_t));
		if ((rc = ext_stop_collect(L, L.st, nullptr)) != BSX_OK) return rc;
		L.sc.xs_ctr = nullptr;
		for (int64_t i = 0; i < n; ++i) if (res[i].score == X4_DECLINED) return BSX_E_ARG;
		return BSX_OK;
	}
	// (the classes below run every row: ext_dp and ext_dp_win do not apply the stopping rule)
	// classes by LDS footprint (query length) and row width (band): {qcap, max band columns, NC}
	// The host chaining path calls this once per round of its strand searches' extensions -- a thousand rounds of a few hundred jobs for
	// the reads inside satellite arrays of a repeat-rich genome -- while the front-half kernels of other chunks fill the device.
	// $BSX_HOSTPATH_STREAM=1 puts the rounds on the lane's high-priority stream: measured, no difference (3.36-3.60 against 3.52 s per chunk).
	const int hp_hi = 0;
	hipStream_t S = hp_hi ? L.st_hi : L.st;
	// the last class: queries of any length, rows in HBM (reads of tens of kilobases).  What remains out of reach is a band of more
	// than 2048 columns, i.e. -w above 511 -- a limit of the option, not of the data
	static const int QCAP[4] = {256, 1024, 16384, 0x7fffffff}, BAND[4] = {256, 512, 2048, 2048}, NCS[4] = {4, 8, 32, 32};
	std::vector<int> order[4];
	int hbm_qmax = 0, rc0;
	for (int64_t i = 0; i < n; ++i) {
		const bsx_ext_job_t &j = jobs[i];
		if (j.qlen <= 0 || j.tlen < 0 || j.h0 <= 0) { fprintf(stderr, "[bsx-hip] extend job %lld: invalid (qlen=%d tlen=%d h0=%d)\n", (long long)i, j.qlen, j.tlen, j.h0); return BSX_E_ARG; }
		long long band = std::min<long long>(j.qlen, 2LL * j.w + 1);
		int c = 0;
		while (c < 4 && (j.qlen > QCAP[c] || band > BAND[c])) ++c;
		if (c == 4) { fprintf(stderr, "[bsx-hip] extend job %lld: a band of %lld columns is beyond the kernel's 2048 (-w above 511)\n", (long long)i, band); return BSX_E_ARG; }
		if (c == 3) hbm_qmax = std::max(hbm_qmax, j.qlen);
		order[c].push_back((int)i);
	}
	const int hbm_blocks = order[3].empty() ? 0 : (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((order[3].size() + 3) / 4, (size_t)d->n_cu), ((size_t)2 << 30) / (4 * extend_hbm_row_bytes(hbm_qmax))));
	if (hbm_blocks && (rc0 = L.scratch.reserve((size_t)hbm_blocks * 4 * extend_hbm_row_bytes(hbm_qmax))) != BSX_OK) return rc0;
	int rc;
	if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_ext_job_t))) != BSX_OK) return rc;
	if ((rc = L.res.reserve((size_t)n * sizeof(bsx_ext_res_t))) != BSX_OK) return rc;
	if ((rc = L.aux.reserve((size_t)n * 4 + 64)) != BSX_OK) return rc;
	HIPCHK(hipMemcpyAsync(L.jobs.p, jobs, (size_t)n * sizeof(bsx_ext_job_t), hipMemcpyHostToDevice, S));
	size_t off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		HIPCHK(hipMemcpyAsync((int*)L.aux.p + off, order[c].data(), order[c].size() * 4, hipMemcpyHostToDevice, S));
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_begin, S));
	off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		if (c == 3)
			launch_extend_hbm(S, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (const int*)L.aux.p + off,
			                  (long long)order[c].size(), (bsx_ext_res_t*)L.res.p, hbm_qmax, hbm_blocks, L.scratch.p);
		else
		launch_extend(S, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_ext_job_t*)L.jobs.p, (const int*)L.aux.p + off,
		              (long long)order[c].size(), (bsx_ext_res_t*)L.res.p, QCAP[c], NCS[c], d->n_cu);
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_end, S));
	if ((rc = finish_timed(L, KT_EXTEND)) != BSX_OK) return rc;
	D2H(S, res, L.res.p, (size_t)n * sizeof(bsx_ext_res_t));
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K5
// ------------------------------------------------------------------------------------------
static int lane_sw_batch(bsx_device_t *d, int lane, int64_t n, const bsx_sw_job_t *jobs, bsx_sw_res_t *res)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (n == 0) return BSX_OK;
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (bsx_tune_is_set("sw_form")) { // tests: score-only jobs of up to 199 x 199 through the seed filter's alignments (k_seedsw.hip), in the order given
		const char *form = bsx_tune_str("sw_form");
		const bool f16 = strcmp(form, "ssw16") == 0;
		if ((!f16 && strcmp(form, "ssw32") != 0) || n > 0x7fffffff || L.n_reads == 0) return BSX_E_ARG;
		for (int64_t i = 0; i < n; ++i) {
			const bsx_sw_job_t &j = jobs[i];
			if (j.qdir != 1 || j.tdir != 1 || j.qcomp != 0 || j.qlen < 0 || j.qlen > 199 || j.tlen < 0 || j.tlen > 199) return BSX_E_ARG;
			if (j.qlen == 0) continue;   // an empty job: nothing of it is read
			if (j.tpos < 0 || j.tpos + j.tlen > 2 * d->ix.l_pac || (j.qoff >> 31) || (size_t)j.qoff + (size_t)j.qlen > L.n_reads) return BSX_E_ARG;
		}
		int rc;
		if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_sw_job_t))) != BSX_OK) return rc;
		if ((rc = L.res.reserve((size_t)n * sizeof(bsx_sw_res_t))) != BSX_OK) return rc;
		if ((rc = L.scratch.reserve((size_t)n * seedsw_job_bytes() + 16)) != BSX_OK) return rc;
		H2D(L.st_hi, L.jobs.p, jobs, (size_t)n * sizeof(bsx_sw_job_t));
		if (!f16) launch_ssw32_batch(L.st_hi, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_sw_job_t*)L.jobs.p, (bsx_sw_res_t*)L.res.p, (unsigned int)n);
		else if (!launch_swl16_batch(L.st_hi, d->n_cu, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_sw_job_t*)L.jobs.p, (bsx_sw_res_t*)L.res.p, (unsigned int)n, L.scratch.p))
			return BSX_E_ARG;   // scoring options the packed kernel cannot hold (ssw16_bound.h): nothing was launched
		HIPCHK(hipGetLastError());
		D2H(L.st_hi, res, L.res.p, (size_t)n * sizeof(bsx_sw_res_t));
		return BSX_OK;
	}
	// byte-sized jobs (KSW_XBYTE, queries of up to 256 columns: mate rescue of ordinary reads) go four to a wavefront through the striped
	// kernel (k_swl.hip), ordered by stripe count and then by target length, longest first, so that the four jobs of a wavefront are alike;
	// the others a wavefront each (k_sw.hip), by padded query length: up to 256, 1024, 3072 columns
	std::vector<int> order[4];
	int max_tlen = 1, slen_max = 1;
	const bool use_swl = true;
	std::vector<int> key;
	for (int64_t i = 0; i < n; ++i) {
		const bsx_sw_job_t &j = jobs[i];
		if (j.qlen <= 0 || j.tlen < 0) { fprintf(stderr, "[bsx-hip] sw job %lld: invalid\n", (long long)i); return BSX_E_ARG; }
		const int p = (j.xtra & BSX_KSW_XBYTE) ? 16 : 8, Q = (j.qlen + p - 1) / p * p;
		if (Q > 3072) { fprintf(stderr, "[bsx-hip] sw job %lld: query %d beyond kernel limit (3072)\n", (long long)i, j.qlen); return BSX_E_ARG; }
		max_tlen = std::max(max_tlen, j.tlen);
		if (use_swl && p == 16 && Q <= 256) { order[3].push_back((int)i); slen_max = std::max(slen_max, Q / 16); }
		else order[Q <= 256 ? 0 : Q <= 1024 ? 1 : 2].push_back((int)i);
	}
	if (order[3].size() > 4) { // counting sort by (stripes, target length descending)
		const int NK = 17 * 2048;
		std::vector<int> cnt((size_t)NK + 1, 0), sorted(order[3].size());
		auto keyof = [&](int i) { const bsx_sw_job_t &j = jobs[i]; return ((j.qlen + 15) >> 4) * 2048 + (2047 - std::min(j.tlen, 2047)); };
		for (int i : order[3]) ++cnt[(size_t)keyof(i) + 1];
		for (int x = 0; x < NK; ++x) cnt[(size_t)x + 1] += cnt[(size_t)x];
		for (int i : order[3]) sorted[(size_t)cnt[(size_t)keyof(i)]++] = i;
		order[3].swap(sorted);
	}
	int rc;
	const int blocks_cap = d->n_cu * 8;
	if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_sw_job_t))) != BSX_OK) return rc;
	if ((rc = L.res.reserve((size_t)n * sizeof(bsx_sw_res_t))) != BSX_OK) return rc;
	if ((rc = L.aux.reserve((size_t)n * 4 + 64)) != BSX_OK) return rc;
	if ((rc = L.scratch.reserve((size_t)blocks_cap * 4 * 4 * (size_t)max_tlen * 8)) != BSX_OK) return rc;   // b[] of every job in flight: four jobs to a wave in k_swl
	const bool tr_sw = bsx_phases() != 0;
	const double ts0 = tr_sw ? bsx_now_s() : 0;
	H2D(L.st_hi, L.jobs.p, jobs, (size_t)n * sizeof(bsx_sw_job_t));
	size_t off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		H2D(L.st_hi, (int*)L.aux.p + off, order[c].data(), order[c].size() * 4);
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_begin, L.st_hi));
	off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		const long long m = (long long)order[c].size();
		if (c == 3) {
			const int blocks = (int)std::min<long long>((m + 15) / 16, blocks_cap);
			launch_swl(L.st_hi, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_sw_job_t*)L.jobs.p, (const int*)L.aux.p + off, m,
			           (bsx_sw_res_t*)L.res.p, (unsigned long long*)L.scratch.p, max_tlen, blocks, slen_max);
		} else {
			const int blocks = (int)std::min<long long>((m + 3) / 4, blocks_cap);
			launch_sw(L.st_hi, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_sw_job_t*)L.jobs.p, (const int*)L.aux.p + off, m,
			          (bsx_sw_res_t*)L.res.p, (unsigned long long*)L.scratch.p, max_tlen, blocks, c == 0 ? 4 : c == 1 ? 16 : 48);
		}
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_end, L.st_hi));
	const double ts1 = tr_sw ? bsx_now_s() : 0;
	if ((rc = finish_timed(L, KT_SW)) != BSX_OK) return rc;
	const double ts2 = tr_sw ? bsx_now_s() : 0;
	D2H(L.st_hi, res, L.res.p, (size_t)n * sizeof(bsx_sw_res_t));
	if (tr_sw) { float ms = 0; (void)hipEventElapsedTime(&ms, L.ev_timed_begin, L.ev_timed_end);
		fprintf(stderr, "[M::sw_batch] %lld jobs: upload %.3f s, waited %.3f s for the kernels (%.3f s on the device), download %.3f s\n", (long long)n, ts1 - ts0, ts2 - ts1, ms * 1e-3, bsx_now_s() - ts2); }
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// C5 over the regions of the last regions batch of this lane
// ------------------------------------------------------------------------------------------
static int lane_regions_dedup(bsx_device_t *d, int lane, const bsx_opt_t *opt, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx,
                              int64_t *long_off = nullptr, uint16_t **long_idx = nullptr, int64_t *long_cap = nullptr)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (!opt || !out_n || !out_idx || per_read < 1) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	if (n_reads == 0) return BSX_OK;
	if (n_reads * per_read != L.rb_tasks) { fprintf(stderr, "[bsx-hip] regions_dedup: %lld reads x %d strand searches, but the last regions batch had %lld\n", (long long)n_reads, per_read, (long long)L.rb_tasks); return BSX_E_ARG; }
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	const int64_t n = L.rb_tasks;
	const size_t cap = (size_t)dedup_cap();
	// the reads with more regions than a lane of k_dedup holds (long_off given): a wavefront each (k_dedup_long), their lists of 16-bit indices
	// one behind the other in a pool with room for every region the main sequence made
	const bool with_long = long_off && long_idx && long_cap && per_read <= 4 && bsx_tune_long("long_dedup", 1) != 0;
	const size_t pool_cap = with_long ? (size_t)L.rs.used_main + 64 : 0;
	// layout of L.dd: counts | short lists | [long: class lists (2 n_reads ints) | offsets (n_reads i64) | 2 counters + cursor (16 B) | pool]
	const size_t o_idx = (size_t)n_reads * 4, o_list = (o_idx + (size_t)n_reads * cap + 15) & ~(size_t)15, o_off = o_list + (size_t)n_reads * 8, o_cnt = o_off + (size_t)n_reads * 8, o_pool = o_cnt + 16;
	if ((rc = L.dd.reserve(with_long ? o_pool + pool_cap * 2 + 64 : o_idx + (size_t)n_reads * cap + 64)) != BSX_OK) return rc;
	const long long *r_off = (const long long*)L.regmeta.p; const int *r_n = (const int*)((const char*)L.regmeta.p + (size_t)n * 8);
	int *d_n = (int*)L.dd.p; unsigned char *d_idx = (unsigned char*)L.dd.p + o_idx;
	int *d_list = with_long ? (int*)((char*)L.dd.p + o_list) : nullptr;
	long long *d_off = (long long*)((char*)L.dd.p + o_off);
	unsigned int *d_cnt = with_long ? (unsigned int*)((char*)L.dd.p + o_cnt) : nullptr;
	if (with_long) {
		HIPCHK(hipMemsetAsync(d_cnt, 0, 16, L.st));
		HIPCHK(hipMemsetAsync(d_off, 0xff, (size_t)n_reads * 8, L.st));   // -1: the read's list (if it has one) is among the short ones
	}
	L.ddl.valid = true; L.ddl.n_reads = n_reads; L.ddl.per_read = per_read; L.ddl.o_idx = o_idx; L.ddl.o_off = o_off; L.ddl.o_pool = o_pool; L.ddl.with_long = with_long;
	launch_dedup(L.st, (const bsx_region_t*)L.regs.p, r_off, r_n, (int)n_reads, per_read, (long long)d->ix.l_pac, opt->max_chain_gap, opt->w, opt->mask_level_redun, d_n, d_idx, d_list, d_cnt);
	if (with_long)
		launch_dedup_long(L.st, d->n_cu, (const bsx_region_t*)L.regs.p, r_off, r_n, (int)n_reads, per_read, (long long)d->ix.l_pac, opt->max_chain_gap, opt->w, opt->mask_level_redun,
		                  d_list, d_cnt, d_n, d_off, (unsigned short*)((char*)L.dd.p + o_pool), (unsigned long long)pool_cap, (unsigned long long*)(d_cnt + 2));
	HIPCHK(hipGetLastError());
	D2H(L.st, out_n, d_n, (size_t)n_reads * 4);
	D2H(L.st, out_idx, d_idx, (size_t)n_reads * cap);
	if (with_long) {
		unsigned int hc[4];
		D2H(L.st, hc, d_cnt, 16);
		unsigned long long used = (unsigned long long)hc[2] | (unsigned long long)hc[3] << 32;
		if (used > pool_cap) used = pool_cap;   // (lists that found no room left their reads to the caller)
		D2H(L.st, long_off, d_off, (size_t)n_reads * 8);
		if (*long_cap < (int64_t)used + 16) { *long_cap = (int64_t)used + (int64_t)(used >> 2) + 1024; *long_idx = (uint16_t*)realloc(*long_idx, (size_t)*long_cap * 2); }
		if (used) D2H(L.st, *long_idx, (char*)L.dd.p + o_pool, (size_t)used * 2);
		if (bsx_phases()) fprintf(stderr, "[M::regions_dedup] a wavefront per read: %u reads of up to 256 regions, %u of up to %d; %llu regions kept\n", hc[0], hc[1], dedup_long_cap(), used);
	} else if (long_off) for (int64_t i = 0; i < n_reads; ++i) long_off[i] = -1;
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// mate rescue's plan + its K5 batch on the device (k_msw.hip), for the pairs [p0, p1) of the chunk whose reads the lane last de-duplicated.
// Returns BSX_OK and *n_jobs >= 0, or *n_jobs = -1 when the plan does not apply (the caller plans on the host as before): no
// de-duplication state for these reads, reads too long for the byte-sized kernel, more than 64 candidates a read.
// ------------------------------------------------------------------------------------------
static int lane_msw_plan(bsx_device_t *d, int lane, const bsx_opt_t *opt, const bsx_pestat_t *pes, int64_t token, int64_t n_reads, int per_read,
                         const uint32_t *roff, int max_len, int p0, int p1, void *table, bsx_sw_res_t **res, int64_t *res_cap, int64_t *n_jobs)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	*n_jobs = -1;
	if (p1 <= p0) { *n_jobs = 0; return BSX_OK; }
	if (!bsx_tune_long("msw_plan", 0)) return BSX_OK;   // (built, bit-identical, measured slower than the host's plan pass: off unless asked for -- DESIGN.md section 4)
	if (!L.ddl.valid || L.ddl.n_reads != n_reads || L.ddl.per_read != per_read || n_reads * per_read != L.rb_tasks) return BSX_OK;
	if (max_len <= 0 || max_len > 256 || (long long)max_len * opt->a >= 250 || opt->max_matesw > 64 || opt->max_matesw < 1 || (opt->flag & BSX_F_SELF_OVLP)) return BSX_OK;
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	const int np = p1 - p0, MM = opt->max_matesw;
	const size_t job_cap = (size_t)np * 2 * (size_t)MM;
	const size_t tb = (size_t)np * msw_pair_bytes(), o_hist = (tb + 255) & ~(size_t)255, o_cnt = o_hist + (size_t)msw_hist_bins() * 4, o_ord = o_cnt + 256;
	if ((rc = L.msw_jobs.reserve(job_cap * sizeof(bsx_sw_job_t) + 64)) != BSX_OK) return rc;
	if ((rc = L.msw_res.reserve(job_cap * sizeof(bsx_sw_res_t) + 64)) != BSX_OK) return rc;
	if ((rc = L.msw_meta.reserve(o_ord + job_cap * 4 + 64)) != BSX_OK) return rc;
	if (L.msw_token != token) { // the chunk's read offsets, once per chunk
		if ((rc = L.msw_roff.reserve(((size_t)n_reads + 1) * 4)) != BSX_OK) return rc;
		H2D(L.st_hi, L.msw_roff.p, roff, ((size_t)n_reads + 1) * 4);
		L.msw_token = token;
	}
	char *M = (char*)L.msw_meta.p;
	unsigned int *d_hist = (unsigned int*)(M + o_hist), *d_cnt = (unsigned int*)(M + o_cnt);
	int *d_ord = (int*)(M + o_ord);
	HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)msw_hist_bins() * 4 + 256, L.st_hi));
	const int64_t n = L.rb_tasks;
	const long long *r_off = (const long long*)L.regmeta.p; const int *r_n = (const int*)((const char*)L.regmeta.p + (size_t)n * 8);
	const char *DD = (const char*)L.dd.p;
	launch_msw_plan(L.st_hi, d->n_cu, d->ix, (const bsx_region_t*)L.regs.p, r_off, r_n, (const int*)DD, (const unsigned char*)DD + L.ddl.o_idx,
	                L.ddl.with_long ? (const long long*)(DD + L.ddl.o_off) : nullptr, L.ddl.with_long ? (const unsigned short*)(DD + L.ddl.o_pool) : nullptr, dedup_cap(), per_read,
	                (const unsigned int*)L.msw_roff.p, pes->low, pes->high, opt->pen_unpaired, MM, opt->min_seed_len, opt->a, p0, np,
	                (bsx_sw_job_t*)L.msw_jobs.p, (unsigned int)std::min<size_t>(job_cap, 0xfffffff0u), d_cnt, d_hist, M, d_ord);
	unsigned int nj = 0;
	D2H(L.st_hi, &nj, d_cnt, 4);
	if ((size_t)nj > job_cap) nj = (unsigned int)job_cap;
	if (nj) {
		const int blocks_cap = d->n_cu * 8;
		long long bound = (long long)pes->high - (long long)pes->low + max_len + 8;   // no window is longer: re - rb <= high - low + l_ms
		if (bound < 1) bound = 1;
		if (bound > (1 << 20)) { *n_jobs = -1; return BSX_OK; }                       // (absurd insert-size bounds: the host's path sizes its scratch from the jobs)
		if ((rc = L.scratch.reserve((size_t)blocks_cap * 4 * 4 * (size_t)bound * 8)) != BSX_OK) return rc;
		const int blocks = (int)std::min<long long>(((long long)nj + 15) / 16, blocks_cap);
		HIPCHK(hipEventRecord(L.ev_timed_begin, L.st_hi));
		launch_swl(L.st_hi, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_sw_job_t*)L.msw_jobs.p, (const int*)d_ord, (long long)nj,
		           (bsx_sw_res_t*)L.msw_res.p, (unsigned long long*)L.scratch.p, (int)bound, blocks, (max_len + 15) / 16);
		HIPCHK(hipEventRecord(L.ev_timed_end, L.st_hi));
		if ((rc = finish_timed(L, KT_SW)) != BSX_OK) return rc;
		if (*res_cap < (int64_t)nj) { *res_cap = (int64_t)nj + (nj >> 2) + 1024; *res = (bsx_sw_res_t*)realloc(*res, sizeof(bsx_sw_res_t) * (size_t)*res_cap); }
		D2H(L.st_hi, *res, L.msw_res.p, (size_t)nj * sizeof(bsx_sw_res_t));
	}
	D2H(L.st_hi, table, M, tb);
	HIPCHK(hipGetLastError());
	*n_jobs = (int64_t)nj;
	if (bsx_phases()) fprintf(stderr, "[M::msw_plan] pairs %d..%d: %u alignments planned and run on the device\n", p0, p1, nj);
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// K6
// ------------------------------------------------------------------------------------------
static int lane_global_batch(bsx_device_t *d, int lane, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res,
                             uint32_t *cigar_pool, size_t cigar_pool_len, bsx_glb_tag_t *tags = nullptr, char **md = nullptr, int64_t *md_cap = nullptr,
                             bsx_glb_ctx_t *ctx = nullptr)   // ctx (with tags): the k_global_ctx form, counts by context for both strand hypotheses
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	Lane &L = d->lane[lane];
	if (n == 0) return BSX_OK;
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	HIPCHK(hipSetDevice(d->ordinal));
	// the last class: queries of any length with their rows in HBM (as lane_extend_batch); a band above 2048 columns stays out of reach
	static const int QCAP[4] = {256, 1024, 16384, 0x7fffffff}, BAND[4] = {256, 1024, 2048, 2048}, NCS[4] = {4, 16, 32, 32}, WPB[4] = {4, 4, 1, 1};
	std::vector<int> order[4];
	size_t zmax[4] = {64, 64, 64, 64};
	int hbm_qmax = 0;
	// tags: the target bases of a job are staged in LDS for the MD walk when they fit next to the DP rows (the rare longer ones are
	// read from HBM); an MD string is at most two characters per target base plus the last count
	static const int TCAP[4] = {512, 2048, 0, 0};
	size_t md_bound = 64;
	const DevScoring &sc = L.sc;
	for (int64_t i = 0; i < n; ++i) {
		const bsx_glb_job_t &j = jobs[i];
		if (tags && j.want_cigar) md_bound += 2 * (size_t)j.tlen + 16;
		if (j.qlen <= 0 || j.tlen <= 0 || j.n_try < 1) { fprintf(stderr, "[bsx-hip] global job %lld: invalid\n", (long long)i); return BSX_E_ARG; }
		if (j.want_cigar && (size_t)j.cigar_off + j.cigar_cap > cigar_pool_len) return BSX_E_ARG;
		const int8_t *mat = j.use_ct ? sc.ctmat : sc.gamat;
		long long wtop = (long long)j.w0 << (j.n_try - 1);
		if (wtop > j.w_max) wtop = j.w_max;
		int dl = j.tlen - j.qlen; dl = dl < 0 ? -dl : dl;
		int max_ins = (int)((double)(((j.qlen + 1) >> 1) * mat[0] - sc.o_ins) / sc.e_ins + 1.);
		int max_del = (int)((double)(((j.qlen + 1) >> 1) * mat[0] - sc.o_del) / sc.e_del + 1.);
		int max_gap = std::max(std::max(max_ins, max_del), 1);
		long long wk = std::max<long long>(std::min<long long>((max_gap + dl + 1) >> 1, wtop), dl + 3);
		long long band = std::min<long long>(j.qlen, 2 * wk + 1);
		int c = 0;
		while (c < 4 && (j.qlen > QCAP[c] || band > BAND[c])) ++c;
		if (c == 4) { fprintf(stderr, "[bsx-hip] global job %lld: a band of %lld columns (query %d, target %d) is beyond the kernel's 2048\n", (long long)i, band, j.qlen, j.tlen); return BSX_E_ARG; }
		if (c == 3) hbm_qmax = std::max(hbm_qmax, j.qlen);
		order[c].push_back((int)i);
		if (j.want_cigar) zmax[c] = std::max(zmax[c], (size_t)band * (size_t)j.tlen + 64);
	}
	int rc, blocks[4];
	size_t ztot = 0;
	for (int c = 0; c < 4; ++c) {
		const long long m = (long long)order[c].size();
		blocks[c] = (int)std::min<long long>((m + WPB[c] - 1) / WPB[c], (long long)d->n_cu * 8);
		zmax[c] = (zmax[c] + 255) & ~(size_t)255;
		// every wave's traceback scratch is sized for the class's largest job (a kilobase read across a long deletion: megabytes): fewer
		// waves rather than tens of GB
		const size_t zbudget = (size_t)4 << 30;
		if ((size_t)blocks[c] * WPB[c] * zmax[c] > zbudget) blocks[c] = (int)std::max<size_t>(1, zbudget / (WPB[c] * zmax[c]));
		if (c == 3 && hbm_qmax) blocks[c] = (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks[c], ((size_t)2 << 30) / global_hbm_row_bytes(hbm_qmax)));
		ztot = std::max(ztot, (size_t)blocks[c] * WPB[c] * zmax[c]);
	}
	if ((rc = L.jobs.reserve((size_t)n * sizeof(bsx_glb_job_t))) != BSX_OK) return rc;
	if ((rc = L.res.reserve((size_t)n * sizeof(bsx_glb_res_t))) != BSX_OK) return rc;
	if ((rc = L.aux.reserve((size_t)n * 4 + 64)) != BSX_OK) return rc;
	// traceback slabs first, then (queries beyond LDS) the DP rows of the HBM class
	const size_t rows_off = (ztot + 256 + 255) & ~(size_t)255, rows_bytes = hbm_qmax ? (size_t)blocks[3] * global_hbm_row_bytes(hbm_qmax) : 0;
	if ((rc = L.scratch.reserve(rows_off + rows_bytes)) != BSX_OK) return rc;
	if ((rc = L.pool.reserve(cigar_pool_len * 4 + 64)) != BSX_OK) return rc;
	unsigned long long *md_cursor = dev_counters(L) + CTR_MD_CURSOR;
	if (tags) {
		if ((rc = L.tags.reserve((size_t)n * sizeof(bsx_glb_tag_t))) != BSX_OK) return rc;
		if ((rc = L.mdpool.reserve(md_bound)) != BSX_OK) return rc;
		HIPCHK(hipMemsetAsync(md_cursor, 0, 8, L.st_hi));
		HIPCHK(hipMemsetAsync(L.tags.p, 0xff, (size_t)n * sizeof(bsx_glb_tag_t), L.st_hi));   // l_md = -1: jobs that ask for no CIGAR
	}
	if (ctx) {
		if ((rc = L.gctx.reserve((size_t)n * sizeof(bsx_glb_ctx_t))) != BSX_OK) return rc;
		HIPCHK(hipMemsetAsync(L.gctx.p, 0, (size_t)n * sizeof(bsx_glb_ctx_t), L.st_hi));
	}
	H2D(L.st_hi, L.jobs.p, jobs, (size_t)n * sizeof(bsx_glb_job_t));
	size_t off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		H2D(L.st_hi, (int*)L.aux.p + off, order[c].data(), order[c].size() * 4);
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_begin, L.st_hi));
	off = 0;
	for (int c = 0; c < 4; ++c) if (!order[c].empty()) {
		if (c == 3)
			launch_global_hbm(L.st_hi, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_glb_job_t*)L.jobs.p, (const int*)L.aux.p + off,
			                  (long long)order[c].size(), (bsx_glb_res_t*)L.res.p, (uint32_t*)L.pool.p, (uint8_t*)L.scratch.p, zmax[c], hbm_qmax, blocks[c],
			                  tags ? (bsx_glb_tag_t*)L.tags.p : nullptr, (char*)L.mdpool.p, (unsigned long long)md_bound, md_cursor, (char*)L.scratch.p + rows_off,
			                  ctx ? (bsx_glb_ctx_t*)L.gctx.p : nullptr);
		else
		launch_global(L.st_hi, d->ix, L.sc, (const uint8_t*)L.reads.p, (const bsx_glb_job_t*)L.jobs.p, (const int*)L.aux.p + off,
		              (long long)order[c].size(), (bsx_glb_res_t*)L.res.p, (uint32_t*)L.pool.p, (uint8_t*)L.scratch.p, zmax[c],
		              QCAP[c], NCS[c], blocks[c], WPB[c], tags ? (bsx_glb_tag_t*)L.tags.p : nullptr, (char*)L.mdpool.p, (unsigned long long)md_bound, md_cursor, tags ? TCAP[c] : 0,
		              ctx ? (bsx_glb_ctx_t*)L.gctx.p : nullptr);
		off += order[c].size();
	}
	HIPCHK(hipEventRecord(L.ev_timed_end, L.st_hi));
	if ((rc = finish_timed(L, KT_GLOBAL)) != BSX_OK) return rc;
	D2H(L.st_hi, res, L.res.p, (size_t)n * sizeof(bsx_glb_res_t));
	D2H(L.st_hi, cigar_pool, L.pool.p, cigar_pool_len * 4);
	if (tags) {
		unsigned long long used = 0;
		D2H(L.st_hi, tags, L.tags.p, (size_t)n * sizeof(bsx_glb_tag_t));
		D2H(L.st_hi, &used, md_cursor, 8);
		if (used > md_bound) { fprintf(stderr, "[bsx-hip] MD pool overrun (%llu > %zu)\n", used, md_bound); return BSX_E_INTERNAL; }
		if ((int64_t)used + 1 > *md_cap) {
			char *g = (char*)realloc(*md, (size_t)used + 64);
			if (!g) return BSX_E_NOMEM;
			*md = g; *md_cap = (int64_t)used + 64;
		}
		D2H(L.st_hi, *md, L.mdpool.p, (size_t)used);
	}
	if (ctx) D2H(L.st_hi, ctx, L.gctx.p, (size_t)n * sizeof(bsx_glb_ctx_t));
	return BSX_OK;
}

// the C ABI of include/bsx.h: lane 0
extern "C" BSX_API int bsx_seed_batch(bsx_device_t *d, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks, bsx_intv_t **out, int64_t *out_cap, int64_t *out_off)
{ return lane_seed_batch(d, 0, opt, n, tasks, out, out_cap, out_off); }
extern "C" BSX_API int bsx_regions_batch(bsx_device_t *d, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks, bsx_region_t **out, int64_t *out_cap,
                                         int64_t *out_off, int32_t *out_n, bsx_intv_t **decl_intv, int64_t *decl_cap, int64_t *decl_off)
{ return lane_regions_batch(d, 0, opt, n, tasks, out, out_cap, out_off, out_n, decl_intv, decl_cap, decl_off); }
extern "C" BSX_API int bsx_regions_finish(bsx_device_t *d, bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n)
{ return lane_regions_finish(d, 0, out, out_cap, out_off, out_n); }
extern "C" BSX_API int bsx_regions_dedup_cap(void) { return dedup_cap(); }
extern "C" BSX_API int bsx_regions_dedup(bsx_device_t *d, const bsx_opt_t *opt, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx)
{ return lane_regions_dedup(d, 0, opt, n_reads, per_read, out_n, out_idx); }
extern "C" BSX_API int bsx_regions_dedup_long_cap(void) { return dedup_long_cap(); }
extern "C" BSX_API int bsx_regions_dedup2(bsx_device_t *d, const bsx_opt_t *opt, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx,
                                          int64_t *long_off, uint16_t **long_idx, int64_t *long_cap)
{ return lane_regions_dedup(d, 0, opt, n_reads, per_read, out_n, out_idx, long_off, long_idx, long_cap); }
// test hook (like the bsx_hook_* entries of csrc/host/hooks.c; not in include/bsx.h): the caller's regions, offsets and counts put into lane 0
// where lane_regions_batch leaves its own, so that bsx_regions_dedup* can be given lists made for it.  cnt[t] = -1: a strand search the
// device did not finish.
extern "C" BSX_API int bsx_hook_regions_put(bsx_device_t *d, int64_t n_tasks, const bsx_region_t *regs, int64_t n_regs, const int64_t *off, const int32_t *cnt)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (!regs || !off || !cnt || n_tasks < 0 || n_tasks > 0x7fffffff || n_regs < 0) return BSX_E_ARG;
	Lane &L = d->lane[0];
	if (L.rs.active) return BSX_E_ARG;
	for (int64_t t = 0; t < n_tasks; ++t)
		if (cnt[t] >= 0 && (off[t] < 0 || off[t] > n_regs || (int64_t)cnt[t] > n_regs - off[t])) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	const size_t n = (size_t)n_tasks;
	if ((rc = L.regs.reserve(((size_t)n_regs + 1) * sizeof(bsx_region_t))) != BSX_OK) return rc;
	if ((rc = L.regmeta.reserve(n * 49 + 64)) != BSX_OK) return rc;
	H2D(L.st, L.regs.p, regs, (size_t)n_regs * sizeof(bsx_region_t));
	H2D(L.st, L.regmeta.p, off, n * 8);
	H2D(L.st, (char*)L.regmeta.p + n * 8, cnt, n * 4);
	L.rb_tasks = n_tasks;
	L.rs.used_main = (unsigned long long)n_regs;
	L.ddl.valid = false;
	return BSX_OK;
}
extern "C" BSX_API int bsx_sa_batch(bsx_device_t *d, int64_t n, const bsx_sa_job_t *jobs, uint64_t *pos) { return lane_sa_batch(d, 0, n, jobs, pos); }
extern "C" BSX_API int bsx_extend_batch(bsx_device_t *d, int64_t n, const bsx_ext_job_t *jobs, bsx_ext_res_t *res) { return lane_extend_batch(d, 0, n, jobs, res); }
extern "C" BSX_API int bsx_sw_batch(bsx_device_t *d, int64_t n, const bsx_sw_job_t *jobs, bsx_sw_res_t *res) { return lane_sw_batch(d, 0, n, jobs, res); }
extern "C" BSX_API int bsx_global_batch(bsx_device_t *d, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_len)
{ return lane_global_batch(d, 0, n, jobs, res, cigar_pool, cigar_pool_len); }
extern "C" BSX_API int bsx_global_batch_tags(bsx_device_t *d, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_len,
                                             bsx_glb_tag_t *tags, char **md, int64_t *md_cap)
{ if (!tags || !md || !md_cap) return BSX_E_ARG; return lane_global_batch(d, 0, n, jobs, res, cigar_pool, cigar_pool_len, tags, md, md_cap); }
extern "C" BSX_API int bsx_global_batch_tags_ctx(bsx_device_t *d, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_len,
                                                 bsx_glb_tag_t *tags, char **md, int64_t *md_cap, bsx_glb_ctx_t *ctx)
{ if (!tags || !md || !md_cap || !ctx) return BSX_E_ARG; return lane_global_batch(d, 0, n, jobs, res, cigar_pool, cigar_pool_len, tags, md, md_cap, ctx); }


// the seams as one vtable for the host pipeline; ctx = (device, lane)
static int be_set_opt(void *c, const bsx_opt_t *o) { return lane_set_opt(LR(c), o); }
static int be_set_reads(void *c, const uint8_t *b, size_t n) { return lane_set_reads(LR(c), b, n); }
static int be_seed(void *c, const bsx_opt_t *o, int64_t n, const bsx_seed_task_t *t, bsx_intv_t **out, int64_t *cap, int64_t *off) { return lane_seed_batch(LR(c), o, n, t, out, cap, off); }
static int be_sa(void *c, int64_t n, const bsx_sa_job_t *j, uint64_t *p) { return lane_sa_batch(LR(c), n, j, p); }
static int be_ext(void *c, int64_t n, const bsx_ext_job_t *j, bsx_ext_res_t *r) { return lane_extend_batch(LR(c), n, j, r); }
static int be_sw(void *c, int64_t n, const bsx_sw_job_t *j, bsx_sw_res_t *r) { return lane_sw_batch(LR(c), n, j, r); }
static int be_regions(void *c, const bsx_opt_t *o, int64_t n, const bsx_seed_task_t *t, bsx_region_t **out, int64_t *cap, int64_t *off, int32_t *cnt,
                      bsx_intv_t **di, int64_t *dc, int64_t *doff)
{
	// The handful of strand searches seeded again (tandem repeats) are done by the time the region tiers are, so by default they are
	// collected before returning; $BSX_ASYNC_REDO=1 leaves them pending for regions_finish at the start of the chunk's back half.
	const int async_redo = (int)bsx_tune_long("async_redo", 0);
	int rc = lane_regions_batch(LR(c), o, n, t, out, cap, off, cnt, di, dc, doff);
	if (rc == BSX_OK && !async_redo) rc = lane_regions_finish(LR(c), out, cap, off, cnt);
	return rc;
}
static int be_regions_finish(void *c, bsx_region_t **out, int64_t *cap, int64_t *off, int32_t *cnt) { return lane_regions_finish(LR(c), out, cap, off, cnt); }
static int be_dedup(void *c, const bsx_opt_t *o, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx) { return lane_regions_dedup(LR(c), o, n_reads, per_read, out_n, out_idx); }
static int be_msw_plan(void *c, const bsx_opt_t *o, const bsx_pestat_t *pes, int64_t token, int64_t n_reads, int per_read, const uint32_t *roff, int max_len,
                       int p0, int p1, void *table, bsx_sw_res_t **res, int64_t *res_cap, int64_t *n_jobs)
{ return lane_msw_plan(LR(c), o, pes, token, n_reads, per_read, roff, max_len, p0, p1, table, res, res_cap, n_jobs); }
static int be_dedup2(void *c, const bsx_opt_t *o, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx, int64_t *long_off, uint16_t **long_idx, int64_t *long_cap)
{ return lane_regions_dedup(LR(c), o, n_reads, per_read, out_n, out_idx, long_off, long_idx, long_cap); }
static int be_glb(void *c, int64_t n, const bsx_glb_job_t *j, bsx_glb_res_t *r, uint32_t *pool, size_t len) { return lane_global_batch(LR(c), n, j, r, pool, len); }
static int be_glb_tags(void *c, int64_t n, const bsx_glb_job_t *j, bsx_glb_res_t *r, uint32_t *pool, size_t len, bsx_glb_tag_t *t, char **md, int64_t *cap)
{ return lane_global_batch(LR(c), n, j, r, pool, len, t, md, cap); }
static int be_glb_tags_ctx(void *c, int64_t n, const bsx_glb_job_t *j, bsx_glb_res_t *r, uint32_t *pool, size_t len, bsx_glb_tag_t *t, char **md, int64_t *cap, bsx_glb_ctx_t *x)
{ return lane_global_batch(LR(c), n, j, r, pool, len, t, md, cap, x); }


static LaneRef g_lane_ref[8][BSX_LANES];   // ctx storage for the vtables (by device ordinal)

extern "C" int bsx_hip_backend_lane(bsx_device_t *dev, int lane, bsx_backend_t *out)
{
	if (!dev) return BSX_E_NODEVICE;
	if (lane < 0 || lane >= BSX_LANES || dev->ordinal < 0 || dev->ordinal >= 8) return BSX_E_ARG;
	LaneRef *r = &g_lane_ref[dev->ordinal][lane];
	r->d = dev; r->lane = lane;
	memset(out, 0, sizeof(*out));
	out->ctx = r; out->name = "hip-gfx950";
	out->set_opt = be_set_opt; out->set_reads = be_set_reads; out->seed_batch = be_seed; out->sa_batch = be_sa;
	out->extend_batch = be_ext; out->sw_batch = be_sw; out->global_batch = be_glb; out->global_batch_tags = be_glb_tags; out->global_batch_tags_ctx = be_glb_tags_ctx;
	shim_tables_backend(out);
	out->regions_batch = bsx_tune_long("host_chain", 0) ? nullptr : be_regions;
	out->regions_finish = out->regions_batch ? be_regions_finish : nullptr;   // BSX_HOST_CHAIN=1: host chaining for every task (A/B checks)
	out->regions_dedup = out->regions_batch && !bsx_tune_long("host_dedup", 0) ? be_dedup : nullptr;   // BSX_HOST_DEDUP=1: C5 on the host for every read (A/B checks)
	out->dedup_cap = dedup_cap();
	out->regions_dedup2 = out->regions_dedup ? be_dedup2 : nullptr;
	out->msw_plan = out->regions_dedup ? be_msw_plan : nullptr;
	return BSX_OK;
}
extern "C" int bsx_hip_backend(bsx_device_t *dev, bsx_backend_t *out) { return bsx_hip_backend_lane(dev, 0, out); }
