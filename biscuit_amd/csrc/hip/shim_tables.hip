// shim_tables.hip -- the output passes that run while aligning, each off unless its flag is given: the BISCUITqc column counts (--qc), the coverage
// tables (--qc-cov), the base-averaged conversion table and the methylation sites (--qc-meth, --meth-bed), duplicate templates (--markdup),
// coordinate order (--sort) and BAM (--bam).  A pass keeps its state in its struct of bsx_device (shim_dev.hpp), has its entry points of
// include/bsx.h and its slots of the vtable here (shim_tables_backend, at the end), and shares the four helpers below.  Lock order: a lane's
// hi_mu, then the pass's mutex.
#include "shim_dev.hpp"
#include "job_check.h"
extern "C" {
#include "bam.h"
}

// Device memory that is not a lane's: `what` of the pass `pass`, as the message names them (`more`: what the pass adds behind the free bytes).
static int dev_room(const char *pass, const char *what, size_t bytes, const char *more, void **out)
{
	*out = nullptr;
	if (hipMalloc(out, bytes) == hipSuccess) return BSX_OK;
	size_t fr = 0, tot = 0; (void)hipGetLastError(); (void)hipMemGetInfo(&fr, &tot);
	fprintf(stderr, "[bsx-hip] %s: no room for %s, %zu bytes (%zu of %zu bytes free%s)\n", pass, what, bytes, fr, tot, more);
	*out = nullptr; return BSX_E_NOMEM;
}
// ... zeroed: the depth state, the masks, the tile sums, the bins, the conversion counters
static int dev_zeroed(const char *pass, const char *what, size_t bytes, void **out)
{
	TRY(dev_room(pass, what, bytes, "", out));
	// the lanes' streams do not wait for the null stream: the zeroes are there before anything is launched on one of them
	if (hipMemsetAsync(*out, 0, bytes, 0) != hipSuccess || hipStreamSynchronize(0) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(*out); *out = nullptr; return BSX_E_NODEVICE; }
	return BSX_OK;
}
#define COV_PASS "coverage tables"
// A block of device memory that lives as long as the call that made it: freed on every return, behind the synchronising copies that read it.
struct Scratch {
	void *p = nullptr;
	~Scratch() { dev_free(p); }
	int alloc(size_t bytes) { if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return BSX_E_NOMEM; } return BSX_OK; }
	void *keep() { void *q = p; p = nullptr; return q; }   // the block outlives the call: it is the caller's now
};
// A batch's jobs and the pool of words they point into (CIGARs, quality masks), staged in the lane's buffers on its high-priority stream.
static int stage_jobs(Lane &L, const void *jobs, size_t jobs_bytes, const uint32_t *pool, size_t pool_len)
{
	TRY(L.qcjobs.reserve(jobs_bytes));
	TRY(L.qcpool.reserve(pool_len * 4 + 64));
	H2D(L.st_hi, L.qcjobs.p, jobs, jobs_bytes);
	H2D(L.st_hi, L.qcpool.p, pool, pool_len * 4);
	return BSX_OK;
}
// The stream of a pass that works beside the lanes (sort, BAM), made on first use.
static int own_stream(hipStream_t *st) { if (!*st) HIPCHK(hipStreamCreateWithFlags(st, hipStreamNonBlocking)); return BSX_OK; }

// ------------------------------------------------------------------------------------------
// BISCUITqc column counts (k_qc.hip)
// ------------------------------------------------------------------------------------------
static int qc_table(bsx_device_t *d)   // the device's table, made on first use
{
	std::lock_guard<std::mutex> lock(d->qc.mu);
	if (d->qc.counts.p) return BSX_OK;
	TRY(d->qc.counts.reserve(sizeof(bsx_qc_counts_t)));
	HIPCHK(hipMemset(d->qc.counts.p, 0, sizeof(bsx_qc_counts_t)));
	return BSX_OK;
}
static int cov_state_locked(bsx_device_t *d);
// with_cov: the same upload also feeds k_cov_add (the jobs with BSX_QC_COV into the depth state of the coverage tables, below)
static int lane_qc_batch(bsx_device_t *d, int lane, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len, bool with_cov = false)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (n == 0) return BSX_OK;
	if (n < 0 || !jobs || (!cigar_pool && cigar_pool_len)) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	for (int64_t i = 0; i < n; ++i) { // what the kernel indexes with must lie inside what it is given (read bases are checked one by one there)
		const bsx_qc_job_t &j = jobs[i];
		uint64_t span, rspan;
		const int ck = job_cigar_spans(cigar_pool, cigar_pool_len, j.cig_off, j.n_cigar, &span, &rspan);
		// k_qc counts read columns in 32 bits (rlen and the CIGAR's columns at most 2^30 each) and looks up the base under the job's first column
		if (ck == JOB_CIGAR_OUTSIDE || j.rlen > (1u << 30) || j.fpos < 0 || j.fpos >= d->ix.l_pac) { fprintf(stderr, "[bsx-hip] qc job %lld: invalid\n", (long long)i); return BSX_E_ARG; }
		if (ck == JOB_CIGAR_BAD_OP || span > (1u << 30)) return BSX_E_ARG;
		// k_qc checks every reference position itself; only k_cov_add writes the depth state at the job's far end
		if (with_cov && (uint64_t)j.fpos + rspan > (uint64_t)d->ix.l_pac) { fprintf(stderr, "[bsx-hip] cov job %lld: beyond the reference\n", (long long)i); return BSX_E_ARG; }
	}
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	HIPCHK(hipSetDevice(d->ordinal));
	TRY(qc_table(d));
	TRY(stage_jobs(L, jobs, (size_t)n * sizeof(bsx_qc_job_t), cigar_pool, cigar_pool_len));
	launch_qc(L.st_hi, d->ix, (const uint8_t*)L.reads.p, (long long)L.n_reads, (const bsx_qc_job_t*)L.qcjobs.p, (long long)n, (const uint32_t*)L.qcpool.p,
	          (unsigned long long*)d->qc.counts.p, d->n_cu);
	HIPCHK(hipGetLastError());
	std::unique_lock<std::mutex> cov_lock(d->cov.mu, std::defer_lock);
	if (with_cov) { // (the depth state stays where it is until the launch is done: bsx_cov_reset takes the same lock)
		cov_lock.lock();
		const int rc = cov_state_locked(d);
		if (rc != BSX_OK) { (void)hipStreamSynchronize(L.st_hi); return rc; }
		launch_cov_add(L.st_hi, d->n_cu, d->cov.diff, d->ix.l_pac, (const bsx_qc_job_t*)L.qcjobs.p, (long long)n, (const uint32_t*)L.qcpool.p, (long long)cigar_pool_len);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(L.st_hi));   // the lane's read buffer belongs to the next chunk once the caller is done with this one
	return BSX_OK;
}
extern "C" BSX_API int bsx_qc_batch(bsx_device_t *d, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len)
{ return lane_qc_batch(d, 0, n, jobs, cigar_pool, cigar_pool_len); }
extern "C" BSX_API int bsx_qc_read(bsx_device_t *d, bsx_qc_counts_t *out, int reset)
{
	if (!d || !out) return BSX_E_ARG;
	HIPCHK(hipSetDevice(d->ordinal));
	TRY(qc_table(d));
	std::lock_guard<std::mutex> lock(d->qc.mu);
	HIPCHK(hipDeviceSynchronize());   // every lane's batches
	HIPCHK(hipMemcpy(out, d->qc.counts.p, sizeof(bsx_qc_counts_t), hipMemcpyDeviceToHost));
	if (reset) HIPCHK(hipMemset(d->qc.counts.p, 0, sizeof(bsx_qc_counts_t)));
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// BISCUITqc coverage tables (k_cov.hip)
// ------------------------------------------------------------------------------------------
static int cov_state_locked(bsx_device_t *d)   // the difference array, made on first use; the caller holds cov.mu
{
	if (d->cov.diff) return BSX_OK;
	return dev_zeroed(COV_PASS, "the depth state", cov_diff_entries(d->ix.l_pac) * 8, &d->cov.diff);
}
static int lane_cov_batch(bsx_device_t *d, int lane, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (n == 0) return BSX_OK;
	if (n < 0 || !jobs || (!cigar_pool && cigar_pool_len)) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	for (int64_t i = 0; i < n; ++i) { // every event of every job inside the array, every CIGAR word inside the pool
		const bsx_qc_job_t &j = jobs[i];
		uint64_t span, rspan;
		const int ck = job_cigar_spans(cigar_pool, cigar_pool_len, j.cig_off, j.n_cigar, &span, &rspan);
		// k_cov_add reads no read base, so rlen is free; the array has an entry at l_pac, where a job without a reference span may stand
		if (ck == JOB_CIGAR_OUTSIDE || j.fpos < 0 || j.fpos > d->ix.l_pac) { fprintf(stderr, "[bsx-hip] cov job %lld: invalid\n", (long long)i); return BSX_E_ARG; }
		if (ck == JOB_CIGAR_BAD_OP) return BSX_E_ARG;   // (no cap on the columns: only the reference span is walked, and that ends inside the genome)
		// the job's far end is where the depth goes down again
		if ((uint64_t)j.fpos + rspan > (uint64_t)d->ix.l_pac) { fprintf(stderr, "[bsx-hip] cov job %lld: beyond the reference\n", (long long)i); return BSX_E_ARG; }
	}
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	std::lock_guard<std::mutex> lock(d->cov.mu);   // until the launch is done: bsx_cov_reset frees the state under the same lock
	HIPCHK(hipSetDevice(d->ordinal));
	TRY(cov_state_locked(d));
	TRY(stage_jobs(L, jobs, (size_t)n * sizeof(bsx_qc_job_t), cigar_pool, cigar_pool_len));
	launch_cov_add(L.st_hi, d->n_cu, d->cov.diff, d->ix.l_pac, (const bsx_qc_job_t*)L.qcjobs.p, (long long)n, (const uint32_t*)L.qcpool.p, (long long)cigar_pool_len);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(L.st_hi));   // the staging buffers are the next batch's
	return BSX_OK;
}
extern "C" BSX_API int bsx_cov_batch(bsx_device_t *d, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len)
{ return lane_cov_batch(d, 0, n, jobs, cigar_pool, cigar_pool_len); }
extern "C" BSX_API int bsx_cov_set_mask(bsx_device_t *d, int which, int64_t n, const int64_t *beg_end)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (which < 0 || which > 1 || n < 0 || (n && !beg_end)) return BSX_E_ARG;
	for (int64_t i = 0; i < n; ++i) if (beg_end[2 * i] < 0 || beg_end[2 * i] > beg_end[2 * i + 1] || beg_end[2 * i + 1] > d->ix.l_pac) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->cov.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	HIPCHK(hipDeviceSynchronize());
	const size_t bytes = cov_mask_words(d->ix.l_pac) * 4;
	if (d->cov.mask[which]) HIPCHK(hipMemset(d->cov.mask[which], 0, bytes));
	else TRY(dev_zeroed(COV_PASS, "a mask", bytes, (void**)&d->cov.mask[which]));
	if (n == 0) return BSX_OK;
	Scratch iv;
	TRY(iv.alloc((size_t)n * 16));
	HIPCHK(hipMemcpy(iv.p, beg_end, (size_t)n * 16, hipMemcpyHostToDevice));
	launch_cov_paint(0, d->n_cu, d->cov.mask[which], d->ix.l_pac, (const long long*)iv.p, (long long)n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	return BSX_OK;
}
extern "C" BSX_API int bsx_cov_tables(bsx_device_t *d, bsx_cov_tables_t *out)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (!out) return BSX_E_ARG;
	memset(out, 0, sizeof(*out));
	HIPCHK(hipSetDevice(d->ordinal));
	long lds_bins = bsx_tune_long("cov_lds_bins", COV_LDS_BINS_MAX), flush_tiles = bsx_tune_long("cov_flush_tiles", 524287);
	if (lds_bins < 1 || lds_bins > COV_LDS_BINS_MAX || (lds_bins & (lds_bins - 1)) || flush_tiles < 1 || flush_tiles > 524287) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->cov.mu);
	TRY(cov_state_locked(d));
	if ((d->cov.mask[0] != nullptr) != (d->cov.mask[1] != nullptr)) { fprintf(stderr, "[bsx-hip] coverage tables: one GC mask without the other\n"); return BSX_E_ARG; }
	HIPCHK(hipDeviceSynchronize());   // every lane's batches
	const long long n_tiles = (long long)cov_n_tiles(d->ix.l_pac);
	Scratch tsum, bins;
	TRY(dev_zeroed(COV_PASS, "the tile sums", (size_t)n_tiles * 8 + 16, &tsum.p));
	int *gmax = (int*)((char*)tsum.p + (size_t)n_tiles * 8);
	int vmax = 0;
	launch_cov_sums(0, d->n_cu, d->cov.diff, n_tiles, tsum.p);
	launch_cov_max(0, d->n_cu, d->ix, d->cov.diff, tsum.p, n_tiles, gmax);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(&vmax, gmax, 4, hipMemcpyDeviceToHost));
	const uint64_t nb = (uint64_t)(vmax < 0 ? 0 : vmax) + 1;
	std::vector<uint64_t> host((size_t)BSX_COV_N_TABLES * nb);
	TRY(dev_zeroed(COV_PASS, "the bins", host.size() * 8, &bins.p));
	launch_cov_count(0, d->n_cu, d->ix, d->cov.diff, tsum.p, n_tiles, d->cov.mask[0], d->cov.mask[1], (int)lds_bins, (int)flush_tiles, (unsigned long long*)bins.p, (long long)nb);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(host.data(), bins.p, host.size() * 8, hipMemcpyDeviceToHost));
	out->have_gc = d->cov.mask[0] ? 1 : 0;
	for (int i = 0; i < (out->have_gc ? BSX_COV_N_TABLES : 4); ++i) {
		out->t[i].count = (uint64_t*)malloc(nb * 8);
		if (!out->t[i].count) { bsx_cov_tables_free(out); return BSX_E_NOMEM; }
		memcpy(out->t[i].count, host.data() + (size_t)i * nb, nb * 8);
		out->t[i].n_bins = nb;
	}
	return BSX_OK;
}
extern "C" BSX_API int bsx_cov_reset(bsx_device_t *d)
{
	if (!d) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->cov.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (d->cov.diff || d->cov.mask[0] || d->cov.mask[1]) HIPCHK(hipDeviceSynchronize());
	d->cov.release();
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// BISCUITqc base-averaged conversion table (k_meth.hip)
// ------------------------------------------------------------------------------------------
static int meth_state_locked(bsx_device_t *d)   // the counters, made on first use; the caller holds meth.mu
{
	if (d->meth.st) return BSX_OK;
	return dev_zeroed("base-averaged conversion table", "the counters", meth_state_entries(d->ix.l_pac) * 16, &d->meth.st);
}
static int lane_meth_batch(bsx_device_t *d, int lane, int64_t n, const bsx_meth_job_t *jobs, const uint32_t *pool, size_t pool_len)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (n == 0) return BSX_OK;
	if (n < 0 || !jobs || !pool) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	for (int64_t i = 0; i < n; ++i) { // every column of every job inside the genome, every CIGAR and mask word inside the pool
		const bsx_meth_job_t &j = jobs[i];
		uint64_t span, rspan;
		const int ck = job_cigar_spans(pool, pool_len, j.cig_off, j.n_cigar, &span, &rspan);
		// as k_qc, and the read has a quality mask of one bit per base in the same pool (so rlen is at least 1)
		if (ck == JOB_CIGAR_OUTSIDE || j.rlen < 1 || j.rlen > (1u << 30) || (size_t)j.qm_off + (j.rlen + 31) / 32 > pool_len || j.fpos < 0 || j.fpos >= d->ix.l_pac) {
			fprintf(stderr, "[bsx-hip] meth job %lld: invalid\n", (long long)i); return BSX_E_ARG;
		}
		if (ck == JOB_CIGAR_BAD_OP || span > (1u << 30)) return BSX_E_ARG;
		// k_meth_add writes a counter at every reference column of the job: always checked
		if ((uint64_t)j.fpos + rspan > (uint64_t)d->ix.l_pac) { fprintf(stderr, "[bsx-hip] meth job %lld: beyond the reference\n", (long long)i); return BSX_E_ARG; }
	}
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	std::lock_guard<std::mutex> lock(d->meth.mu);   // until the launch is done: bsx_meth_reset frees the state under the same lock
	HIPCHK(hipSetDevice(d->ordinal));
	TRY(meth_state_locked(d));
	TRY(stage_jobs(L, jobs, (size_t)n * sizeof(bsx_meth_job_t), pool, pool_len));
	launch_meth_add(L.st_hi, d->ix, (const uint8_t*)L.reads.p, (long long)L.n_reads, (const bsx_meth_job_t*)L.qcjobs.p, (long long)n, (const uint32_t*)L.qcpool.p,
	                (long long)pool_len, d->meth.st, d->n_cu);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(L.st_hi));   // the staging buffers are the next batch's, the lane's read buffer the next chunk's
	return BSX_OK;
}
extern "C" BSX_API int bsx_meth_batch(bsx_device_t *d, int64_t n, const bsx_meth_job_t *jobs, const uint32_t *pool, size_t pool_len) { return lane_meth_batch(d, 0, n, jobs, pool, pool_len); }
extern "C" BSX_API int bsx_meth_read(bsx_device_t *d, int64_t fpos, int64_t n, uint32_t *out)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (fpos < 0 || n < 0 || fpos > d->ix.l_pac || n > d->ix.l_pac - fpos || (n && !out)) return BSX_E_ARG;
	if (n == 0) return BSX_OK;
	std::lock_guard<std::mutex> lock(d->meth.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (!d->meth.st) { memset(out, 0, (size_t)n * 16); return BSX_OK; }
	HIPCHK(hipDeviceSynchronize());   // every lane's batches
	HIPCHK(hipMemcpy(out, (const char*)d->meth.st + (size_t)fpos * 16, (size_t)n * 16, hipMemcpyDeviceToHost));   // (little endian: ret, conv, opp_ref, opp_alt)
	return BSX_OK;
}
static_assert(sizeof(bsx_meth_tables_t) == 2 * BSX_METH_N_CTX * 8, "k_meth_walk's cells are bsx_meth_tables_t");
extern "C" BSX_API int bsx_meth_tables(bsx_device_t *d, bsx_meth_tables_t *out)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (!out) return BSX_E_ARG;
	memset(out, 0, sizeof(*out));
	const long flush_tiles = bsx_tune_long("meth_flush_tiles", METH_FLUSH_TILES_MAX);
	if (flush_tiles < 1 || flush_tiles > METH_FLUSH_TILES_MAX) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->meth.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (!d->meth.st) return BSX_OK;   // no batch yet: no site
	HIPCHK(hipDeviceSynchronize());   // every lane's batches
	Scratch cells;
	TRY(cells.alloc(sizeof(*out)));
	HIPCHK(hipMemset(cells.p, 0, sizeof(*out)));
	launch_meth_tables(0, d->n_cu, d->ix, d->meth.st, (long long)meth_n_tiles(d->ix.l_pac), (int)flush_tiles, (unsigned long long*)cells.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(out, cells.p, sizeof(*out), hipMemcpyDeviceToHost));
	return BSX_OK;
}
extern "C" BSX_API int bsx_meth_reset(bsx_device_t *d)
{
	if (!d) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->meth.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (d->meth.st) HIPCHK(hipDeviceSynchronize());
	d->meth.release();
	return BSX_OK;
}
// the methylation sites of the state (k_msite.hip): the tiles' counts come to the host, which sums them and cuts the window that fits cap; the
// records of that window are written on the device at their final places and come down in one copy
extern "C" BSX_API int bsx_meth_sites(bsx_device_t *d, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n, int64_t *f_next)
{
	if (!d || !d->has_index) return BSX_E_NODEVICE;
	if (!opt || !n || !f_next || f_lo < 0 || f_lo > f_hi || f_hi > d->ix.l_pac || cap < BSX_COV_TILE || !out) return BSX_E_ARG;
	if (opt->type < BSX_METH_TYPE_CG || opt->type > BSX_METH_TYPE_C || opt->min_cov < 1 || (opt->merge && opt->type != BSX_METH_TYPE_CG)) return BSX_E_ARG;
	*n = 0; *f_next = f_hi;
	if (f_lo == f_hi) return BSX_OK;
	if (cap > (1ll << 31) - 1) cap = (1ll << 31) - 1;   // 32-bit places
	std::lock_guard<std::mutex> lock(d->meth.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (!d->meth.st) return BSX_OK;   // no batch yet: no site
	HIPCHK(hipDeviceSynchronize());   // every lane's batches
	const long long t_lo = f_lo / BSX_COV_TILE, nt = (f_hi + BSX_COV_TILE - 1) / BSX_COV_TILE - t_lo;
	bsx_meth_site_opt_t o = *opt;
	o.merge = o.merge ? 1 : 0; o.pad = 0;
	Scratch cnt, recs;    // cnt: nt counts, then the window's nt + 1 exclusive sums
	TRY(cnt.alloc(((size_t)nt + 1) * 4));
	std::vector<uint32_t> h((size_t)nt + 1);
	launch_msite_count(0, d->n_cu, d->ix, d->meth.st, o, f_lo, f_hi, t_lo, nt, (uint32_t*)cnt.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(h.data(), cnt.p, (size_t)nt * 4, hipMemcpyDeviceToHost));
	long long w = 0;            // tiles of the window
	uint64_t total = 0;
	for (; w < nt; ++w) {
		const uint32_t c = h[(size_t)w];
		if (c > BSX_COV_TILE) return BSX_E_INTERNAL;
		if (total + c > (uint64_t)cap) break;
		h[(size_t)w] = (uint32_t)total; total += c;
	}
	h[(size_t)w] = (uint32_t)total;
	if (total) {
		TRY(recs.alloc((size_t)total * sizeof(bsx_meth_site_t)));
		HIPCHK(hipMemcpy(cnt.p, h.data(), ((size_t)w + 1) * 4, hipMemcpyHostToDevice));
		launch_msite_emit(0, d->n_cu, d->ix, d->meth.st, o, f_lo, f_hi, t_lo, w, (uint32_t*)cnt.p, (bsx_meth_site_t*)recs.p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpy(out, recs.p, (size_t)total * sizeof(bsx_meth_site_t), hipMemcpyDeviceToHost));
	}
	*n = (int64_t)total;
	*f_next = w == nt ? f_hi : (int64_t)(t_lo + w) * BSX_COV_TILE;
	return BSX_OK;
}

// ------------------------------------------------------------------------------------------
// duplicate templates (k_markdup.hip)
// ------------------------------------------------------------------------------------------
static int md_alloc(bsx_device_t *d, hipStream_t st, uint64_t n_slots, MdSlot **out)   // an empty table of n_slots
{
	char what[64], more[64];
	snprintf(what, sizeof(what), "a table of %llu slots", (unsigned long long)n_slots);
	snprintf(more, sizeof(more), "; the table in use has %llu slots", (unsigned long long)d->md.slots);
	TRY(dev_room("markdup", what, n_slots * sizeof(MdSlot), more, (void**)out));
	launch_md_init(st, *out, n_slots);
	HIPCHK(hipGetLastError());
	return BSX_OK;
}
// room for `more` new keys at a load of one half or less: the first table, or one of twice (four times, ...) the slots with every slot moved over
static int md_room(bsx_device_t *d, Lane &L, uint64_t more, unsigned long long *ctr)
{
	uint64_t want = d->md.slots;
	if (!d->md.tab) {
		const long t = bsx_tune_long("markdup_slots", 0);
		want = t > 0 ? (uint64_t)t : std::max<uint64_t>(65536, 32 * more);
		while (want & (want - 1)) want += want & (~want + 1);   // up to a power of two
		if (want < 2) want = 2;
	}
	while ((d->md.used + more) * 2 > want) want *= 2;
	if (d->md.tab && want == d->md.slots) return BSX_OK;
	Scratch T;   // (the new table: the device's once every slot has come over)
	TRY(md_alloc(d, L.st_hi, want, (MdSlot**)&T.p));
	if (d->md.tab) {
		unsigned long long lost = 0;
		launch_md_rehash(L.st_hi, d->md.tab, d->md.slots, (MdSlot*)T.p, want, ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(&lost, ctr + MD_CTR_LOST, 8, hipMemcpyDeviceToHost, L.st_hi));
		HIPCHK(hipStreamSynchronize(L.st_hi));
		if (lost) return BSX_E_INTERNAL;
		(void)hipFree(d->md.tab);
		if (bsx_phases()) fprintf(stderr, "[M::markdup] table grown from %llu to %llu slots (%llu taken)\n", (unsigned long long)d->md.slots, (unsigned long long)want, (unsigned long long)d->md.used);
	}
	d->md.tab = (MdSlot*)T.keep(); d->md.slots = want;
	return BSX_OK;
}
extern "C" BSX_API int bsx_markdup_reset(bsx_device_t *d)
{
	if (!d) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->md.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (d->md.tab) HIPCHK(hipDeviceSynchronize());
	d->md.release();
	return BSX_OK;
}
#define MD_MAX_SALTS 8
static int lane_markdup_batch(bsx_device_t *d, int lane, int64_t n, const bsx_markdup_key_t *keys, uint64_t first_ordinal, uint8_t *dup_out)
{
	if (!d) return BSX_E_NODEVICE;
	if (n < 0) return bsx_markdup_reset(d);
	if (n == 0) return BSX_OK;
	if (!keys || !dup_out || first_ordinal + (uint64_t)n < first_ordinal || first_ordinal + (uint64_t)n == ~0ull) return BSX_E_ARG;
	Lane &L = d->lane[lane];
	std::lock_guard<std::mutex> hi_lock(L.hi_mu);
	std::lock_guard<std::mutex> lock(d->md.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	const int bits = (int)bsx_tune_long("markdup_hash_bits", 64);
	const size_t res_bytes = ((size_t)n + 7) & ~(size_t)7, tail = 4 * 8;   // res[n], then ctr[4]: slots taken, keys left open, slots lost in a rehash
	TRY(L.mdkeys.reserve((size_t)n * sizeof(bsx_markdup_key_t)));
	TRY(L.mdres.reserve(res_bytes + tail));
	TRY(L.mdslot.reserve((size_t)n * 8));
	uint8_t *res = (uint8_t*)L.mdres.p;
	unsigned long long *ctr = (unsigned long long*)(res + res_bytes);
	std::vector<uint8_t> host(res_bytes + tail);
	HIPCHK(hipMemsetAsync(res, MD_RES_OPEN, res_bytes, L.st_hi));
	HIPCHK(hipMemsetAsync(ctr, 0, tail, L.st_hi));
	H2D(L.st_hi, L.mdkeys.p, keys, (size_t)n * sizeof(bsx_markdup_key_t));
	uint64_t open = (uint64_t)n;
	for (unsigned salt = 0; open; ++salt) {
		if (salt == MD_MAX_SALTS) { fprintf(stderr, "[bsx-hip] markdup: %llu keys met other keys with their claim word at %d salts\n", (unsigned long long)open, MD_MAX_SALTS); return BSX_E_INTERNAL; }
		TRY(md_room(d, L, open, ctr));
		HIPCHK(hipMemsetAsync(ctr, 0, tail, L.st_hi));
		launch_md_round(L.st_hi, d->md.tab, d->md.slots, (const bsx_markdup_key_t*)L.mdkeys.p, (long long)n, first_ordinal, salt, bits, res, (unsigned long long*)L.mdslot.p, ctr);
		HIPCHK(hipGetLastError());
		D2H(L.st_hi, host.data(), res, res_bytes + tail);
		const unsigned long long *c = (const unsigned long long*)(host.data() + res_bytes);
		d->md.used += c[0];
		open = c[1];
	}
	for (int64_t i = 0; i < n; ++i) {
		if (host[(size_t)i] == MD_RES_FULL || host[(size_t)i] == MD_RES_OPEN) return BSX_E_INTERNAL;
		dup_out[i] = host[(size_t)i] == MD_RES_DUP;
	}
	return BSX_OK;
}
extern "C" BSX_API int bsx_markdup_batch(bsx_device_t *d, int64_t n, const bsx_markdup_key_t *keys, uint64_t first_ordinal, uint8_t *dup_out)
{ if (n < 0) return BSX_E_ARG; return lane_markdup_batch(d, 0, n, keys, first_ordinal, dup_out); }
extern "C" BSX_API int bsx_markdup_table_info(bsx_device_t *d, uint64_t *n_slots, uint64_t *n_used)
{
	if (!d) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->md.mu);
	if (n_slots) *n_slots = d->md.slots;
	if (n_used) *n_used = d->md.used;
	return BSX_OK;
}

// ---- coordinate order (k_sort.hip) ----
// The passes over (sort_k[0], sort_p[0]) -- n keys; iota: the payload is the key's index and sort_p[0] holds nothing yet.  *cur = the buffer pair the
// sorted keys and their payloads are in; *have_pay = 0 only when iota and every key was equal (nothing ran: the payload is the identity).
static int sort_passes(bsx_device *d, int64_t n, bool iota, int *cur, int *have_pay, int *n_passes)
{
	hipStream_t st = d->sort.st;
	uint64_t *k[2] = {(uint64_t*)d->sort.k[0].p, (uint64_t*)d->sort.k[1].p};
	uint32_t *p[2] = {(uint32_t*)d->sort.p[0].p, (uint32_t*)d->sort.p[1].p};
	*cur = 0; *have_pay = !iota; *n_passes = 0;
	if (n <= BSX_SORT_TILE) {
		launch_sort_small(st, (const unsigned long long*)k[0], iota ? nullptr : p[0], (unsigned long long*)k[1], p[1], n);
		HIPCHK(hipGetLastError());
		*cur = 1; *have_pay = 1;
		return BSX_OK;
	}
	TRY(d->sort.counts.reserve(sort_n_tiles(n) * 256 * 4));
	TRY(d->sort.btot.reserve(sort_n_scan_blocks(n) * 4 + 16));
	unsigned long long *bits_d = (unsigned long long*)((char*)d->sort.btot.p + ((sort_n_scan_blocks(n) * 4 + 7) & ~(size_t)7)), bits = 0;
	HIPCHK(hipMemsetAsync(bits_d, 0, 8, st));
	launch_sort_bits(st, (const unsigned long long*)k[0], n, bits_d);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(&bits, bits_d, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	for (int shift = 0; shift < 64; shift += 8) {
		if (((bits >> shift) & 255) == 0) continue;   // every key has the same digit here: the pass would move nothing
		launch_sort_pass(st, (const unsigned long long*)k[*cur], *have_pay ? p[*cur] : nullptr, (unsigned long long*)k[*cur ^ 1], p[*cur ^ 1], n, shift,
		                 (unsigned int*)d->sort.counts.p, (unsigned int*)d->sort.btot.p);
		HIPCHK(hipGetLastError());
		*cur ^= 1; *have_pay = 1; ++*n_passes;
	}
	return BSX_OK;
}
static int sort_buffers(bsx_device *d, int64_t n)
{
	TRY(own_stream(&d->sort.st));
	for (int i = 0; i < 2; ++i) {
		TRY(d->sort.k[i].reserve((size_t)n * 8));
		TRY(d->sort.p[i].reserve((size_t)n * 4));
	}
	return BSX_OK;
}
extern "C" BSX_API int bsx_sort_run(bsx_device_t *d, int64_t n, const uint64_t *keys, uint32_t *perm_out)
{
	if (!d) return BSX_E_NODEVICE;
	if (n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!keys || !perm_out))) return BSX_E_ARG;
	if (n == 0) return BSX_OK;
	std::lock_guard<std::mutex> lock(d->sort.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	int cur, have_pay, n_passes;
	TRY(sort_buffers(d, n));
	Scratch run;   // the sorted keys: one of sort.runs once they are there
	if (run.alloc((size_t)n * 8) != BSX_OK) { fprintf(stderr, "[bsx-hip] sort: no device memory for a run of %lld keys\n", (long long)n); return BSX_E_NOMEM; }
	HIPCHK(hipMemcpyAsync(d->sort.k[0].p, keys, (size_t)n * 8, hipMemcpyHostToDevice, d->sort.st));
	TRY(sort_passes(d, n, true, &cur, &have_pay, &n_passes));
	HIPCHK(hipMemcpyAsync(run.p, d->sort.k[cur].p, (size_t)n * 8, hipMemcpyDeviceToDevice, d->sort.st));
	if (have_pay) HIPCHK(hipMemcpyAsync(perm_out, d->sort.p[cur].p, (size_t)n * 4, hipMemcpyDeviceToHost, d->sort.st));
	HIPCHK(hipStreamSynchronize(d->sort.st));
	if (!have_pay) for (int64_t i = 0; i < n; ++i) perm_out[i] = (uint32_t)i;
	if (bsx_phases()) fprintf(stderr, "[M::sort] run %zu: %lld keys, %d passes\n", d->sort.runs.size(), (long long)n, n_passes);
	d->sort.runs.push_back(std::make_pair((uint64_t*)run.keep(), n));
	return BSX_OK;
}
extern "C" BSX_API int bsx_sort_schedule(bsx_device_t *d, int64_t *n_total, uint32_t **run_of)
{
	if (!d) return BSX_E_NODEVICE;
	if (!n_total || !run_of) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->sort.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	int64_t n = 0;
	*n_total = 0; *run_of = nullptr;
	for (auto &r : d->sort.runs) n += r.second;
	if (n == 0) return BSX_OK;
	if (n >= ((int64_t)1 << 31)) { fprintf(stderr, "[bsx-hip] sort: %lld records; the schedule holds fewer than 2^31\n", (long long)n); return BSX_E_ARG; }
	int cur, have_pay, n_passes;
	TRY(sort_buffers(d, n));
	int64_t off = 0;
	for (size_t r = 0; r < d->sort.runs.size(); ++r) { // the concatenation in run order, each key's payload its run
		const int64_t m = d->sort.runs[r].second;
		HIPCHK(hipMemcpyAsync((uint64_t*)d->sort.k[0].p + off, d->sort.runs[r].first, (size_t)m * 8, hipMemcpyDeviceToDevice, d->sort.st));
		HIPCHK(hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)d->sort.p[0].p + off), (int)r, (size_t)m, d->sort.st));
		off += m;
	}
	TRY(sort_passes(d, n, false, &cur, &have_pay, &n_passes));
	uint32_t *out = (uint32_t*)malloc((size_t)n * 4);
	if (!out) return BSX_E_NOMEM;
	if (hipMemcpyAsync(out, d->sort.p[cur].p, (size_t)n * 4, hipMemcpyDeviceToHost, d->sort.st) != hipSuccess || hipStreamSynchronize(d->sort.st) != hipSuccess) {
		fprintf(stderr, "[bsx-hip] sort: %s\n", hipGetErrorString(hipGetLastError())); free(out); return BSX_E_NODEVICE;
	}
	if (bsx_phases()) fprintf(stderr, "[M::sort] schedule: %zu runs, %lld keys, %d passes\n", d->sort.runs.size(), (long long)n, n_passes);
	*n_total = n; *run_of = out;
	return BSX_OK;
}
extern "C" BSX_API int bsx_sort_reset(bsx_device_t *d)
{
	if (!d) return BSX_E_NODEVICE;
	std::lock_guard<std::mutex> lock(d->sort.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	if (d->sort.st) HIPCHK(hipStreamSynchronize(d->sort.st));
	d->sort.release();
	return BSX_OK;
}
extern "C" BSX_API int bsx_sort_info(bsx_device_t *d, uint64_t *n_runs, uint64_t *n_keys)
{
	if (!d) return BSX_E_NODEVICE;
	std::lock_guard<std::mutex> lock(d->sort.mu);
	uint64_t n = 0;
	for (auto &r : d->sort.runs) n += (uint64_t)r.second;
	if (n_runs) *n_runs = d->sort.runs.size();
	if (n_keys) *n_keys = n;
	return BSX_OK;
}

// ---- BAM output (k_bam.hip, k_bgzf.hip) ----
static int bam_host_grow(uint8_t **out, size_t *cap, size_t want)
{
	if (want <= *cap) return BSX_OK;
	size_t m = *cap ? *cap : 4096;
	while (m < want) m += m >> 1;
	uint8_t *p = (uint8_t*)realloc(*out, m);
	if (!p) return BSX_E_NOMEM;
	*out = p; *cap = m;
	return BSX_OK;
}
// text -> records: newlines counted per tile and summed on the device, line starts, a size pass (the first refused line comes back as one word per
// workgroup), the sizes summed on the device, the emit pass; 4 + 8 x workgroups + 4 bytes come to the host between the launches, then the payload
static int be_bam_encode(void *c, const bsx_bam_refs_t *refs, const char *text, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len,
                         int64_t *n_records, int64_t *bad_record, int *bad_why)
{
	bsx_device_t *d = ((LaneRef*)c)->d;
	if (!d) return BSX_E_NODEVICE;
	if (!refs || !out || !out_cap || !out_len || !n_records || !bad_record || !bad_why || (len && !text)) return BSX_E_ARG;
	*out_len = 0; *n_records = 0; *bad_record = -1; *bad_why = 0;
	if (len == 0) return BSX_OK;
	if (text[len - 1] != '\n' || len >= ((size_t)1 << 31)) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->bam.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	TRY(own_stream(&d->bam.st));
	hipStream_t st = d->bam.st;
	if (d->bam.tab_serial != refs->serial) { // the writer's name table, once
		if ((rc = d->bam.names.reserve(refs->names_len + 16)) != BSX_OK || (rc = d->bam.noff.reserve(((size_t)refs->n + 1) * 4)) != BSX_OK ||
		    (rc = d->bam.nid.reserve(((size_t)refs->n + 1) * 4)) != BSX_OK) return rc;
		if (refs->names_len) HIPCHK(hipMemcpyAsync(d->bam.names.p, refs->names, refs->names_len, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d->bam.noff.p, refs->off, ((size_t)refs->n + 1) * 4, hipMemcpyHostToDevice, st));
		if (refs->n) HIPCHK(hipMemcpyAsync(d->bam.nid.p, refs->id, (size_t)refs->n * 4, hipMemcpyHostToDevice, st));
		HIPCHK(hipStreamSynchronize(st));
		d->bam.tab_serial = refs->serial;
	}
	const long long nt = bam_n_tiles((long long)len);
	if ((rc = d->bam.text.reserve(len + 16)) != BSX_OK || (rc = d->bam.cnt.reserve(((size_t)nt + 1) * 4)) != BSX_OK) return rc;
	const char *d_text = (const char*)d->bam.text.p;
	uint32_t *cnt = (uint32_t*)d->bam.cnt.p;
	HIPCHK(hipMemcpyAsync(d->bam.text.p, text, len, hipMemcpyHostToDevice, st));
	launch_bam_count(st, d->n_cu, d_text, (long long)len, cnt);
	launch_bam_scan(st, cnt, cnt, nt);
	HIPCHK(hipGetLastError());
	uint32_t n_lines = 0;
	HIPCHK(hipMemcpyAsync(&n_lines, cnt + nt, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	const int grid = bam_lines_grid(n_lines);
	if ((rc = d->bam.start.reserve(((size_t)n_lines + 1) * 4)) != BSX_OK || (rc = d->bam.size.reserve(((size_t)n_lines + 1) * 4)) != BSX_OK ||
	    (rc = d->bam.bad.reserve((size_t)grid * 8)) != BSX_OK || (rc = d->bam.err.reserve(((size_t)n_lines + 1) * 4)) != BSX_OK) return rc;
	uint32_t *start = (uint32_t*)d->bam.start.p, *size = (uint32_t*)d->bam.size.p;
	int *errs = (int*)d->bam.err.p;
	launch_bam_starts(st, d->n_cu, d_text, (long long)len, cnt, start);
	launch_bam_size(st, d_text, start, n_lines, (const char*)d->bam.names.p, (const uint32_t*)d->bam.noff.p, (const int32_t*)d->bam.nid.p, refs->n, size, errs,
	                (unsigned long long*)d->bam.bad.p);
	HIPCHK(hipGetLastError());
	std::vector<unsigned long long> bad((size_t)grid);
	HIPCHK(hipMemcpyAsync(bad.data(), d->bam.bad.p, (size_t)grid * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	unsigned long long first = ~0ull;
	for (unsigned long long b : bad) first = std::min(first, b);
	const long long n_ok = first == ~0ull ? (long long)n_lines : (long long)(first >> 4);
	if (first != ~0ull) { *bad_record = n_ok; *bad_why = (int)(first & 15); }
	uint32_t total = 0;
	if (n_ok > 0) {
		launch_bam_scan(st, size, size, n_ok);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(&total, size + n_ok, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		if ((rc = d->bam.pay.reserve((size_t)total + 16)) != BSX_OK || (rc = bam_host_grow(out, out_cap, total)) != BSX_OK) return rc;
		launch_bam_emit(st, d_text, start, n_ok, (const char*)d->bam.names.p, (const uint32_t*)d->bam.noff.p, (const int32_t*)d->bam.nid.p, refs->n, errs, size,
		                (uint8_t*)d->bam.pay.p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(*out, d->bam.pay.p, total, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	*out_len = total; *n_records = n_ok;
	return BSX_OK;
}
// payload -> members: every block deflated into its 64 KiB slot, the sizes summed on the device, the members moved behind each other, one copy down
static int be_bgzf_deflate(void *c, const uint8_t *payload, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len)
{
	bsx_device_t *d = ((LaneRef*)c)->d;
	if (!d) return BSX_E_NODEVICE;
	if (!out || !out_cap || !out_len || (len && !payload)) return BSX_E_ARG;
	*out_len = 0;
	if (len == 0) return BSX_OK;
	if (len >= ((size_t)1 << 31)) return BSX_E_ARG;
	std::lock_guard<std::mutex> lock(d->bam.mu);
	HIPCHK(hipSetDevice(d->ordinal));
	int rc;
	TRY(own_stream(&d->bam.st));
	hipStream_t st = d->bam.st;
	const long long nb = ((long long)len + BSX_BGZF_BLOCK - 1) / BSX_BGZF_BLOCK;
	const int grid = bgzf_grid(nb);
	if ((rc = d->bam.bz_in.reserve(len + 16)) != BSX_OK || (rc = d->bam.bz_tok.reserve(bgzf_tok_bytes(grid))) != BSX_OK || (rc = d->bam.bz_cand.reserve(bgzf_cand_bytes(grid))) != BSX_OK ||
	    (rc = d->bam.bz_slots.reserve((size_t)nb * 65536)) != BSX_OK || (rc = d->bam.bz_sizes.reserve(((size_t)nb + 1) * 4)) != BSX_OK || (rc = d->bam.bz_ops.reserve(256 * 4)) != BSX_OK) return rc;
	if (!d->bam.bz_ops_ok) {
		uint32_t ops[256];
		bgzf_crc_ops(ops);
		HIPCHK(hipMemcpyAsync(d->bam.bz_ops.p, ops, sizeof(ops), hipMemcpyHostToDevice, st));
		HIPCHK(hipStreamSynchronize(st));
		d->bam.bz_ops_ok = true;
	}
	uint32_t *sizes = (uint32_t*)d->bam.bz_sizes.p, total = 0;
	HIPCHK(hipMemcpyAsync(d->bam.bz_in.p, payload, len, hipMemcpyHostToDevice, st));
	for (long long b0 = 0; b0 < nb; b0 += grid) // (launches on one stream: the second one's workgroups find the workspaces free)
		launch_bgzf_deflate(st, (const uint8_t*)d->bam.bz_in.p, (long long)len, b0, (int)std::min<long long>(grid, nb - b0), (const uint32_t*)d->bam.bz_ops.p, (uint32_t*)d->bam.bz_tok.p,
		                    (uint16_t*)d->bam.bz_cand.p, (uint8_t*)d->bam.bz_slots.p, sizes);
	launch_bam_scan(st, sizes, sizes, nb);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(&total, sizes + nb, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	if (total < 27 * (uint64_t)nb || (uint64_t)total > 65536ull * (uint64_t)nb) return BSX_E_INTERNAL;
	if ((rc = d->bam.bz_out.reserve(total)) != BSX_OK || (rc = bam_host_grow(out, out_cap, total)) != BSX_OK) return rc;
	launch_bgzf_compact(st, d->n_cu, (const uint8_t*)d->bam.bz_slots.p, sizes, nb, (uint8_t*)d->bam.bz_out.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(*out, d->bam.bz_out.p, total, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	*out_len = total;
	return BSX_OK;
}

// ---- the passes' slots of the vtable (bsx_hip_backend_lane, shim.hip); ctx = (device, lane) ----
static int be_qc(void *c, int64_t n, const bsx_qc_job_t *j, const uint32_t *pool, size_t len, bsx_qc_counts_t *read_out, int reset)
{
	int rc = lane_qc_batch(LR(c), n, j, pool, len);
	if (rc == BSX_OK && read_out) rc = bsx_qc_read(((LaneRef*)c)->d, read_out, reset);
	return rc;
}
static int be_markdup(void *c, int64_t n, const bsx_markdup_key_t *k, uint64_t first, uint8_t *out) { return lane_markdup_batch(LR(c), n, k, first, out); }
static int be_cov(void *c, int op, int64_t n, const bsx_qc_job_t *j, const uint32_t *pool, size_t len, const int64_t *beg_end, bsx_cov_tables_t *out)
{
	bsx_device_t *d = ((LaneRef*)c)->d;
	if (op == BSX_COV_OP_BATCH) return lane_cov_batch(LR(c), n, j, pool, len);
	if (op == BSX_COV_OP_QC_BATCH) return lane_qc_batch(LR(c), n, j, pool, len, true);
	if (op == BSX_COV_OP_MASK || op == BSX_COV_OP_MASK + 1) return bsx_cov_set_mask(d, op - BSX_COV_OP_MASK, n, beg_end);
	if (op == BSX_COV_OP_TABLES) return bsx_cov_tables(d, out);
	if (op == BSX_COV_OP_RESET) return bsx_cov_reset(d);
	return BSX_E_ARG;
}
static int be_meth(void *c, int op, int64_t n, const bsx_meth_job_t *j, const uint32_t *pool, size_t len, bsx_meth_tables_t *out)
{
	bsx_device_t *d = ((LaneRef*)c)->d;
	if (op == BSX_METH_OP_BATCH) return lane_meth_batch(LR(c), n, j, pool, len);
	if (op == BSX_METH_OP_TABLES) return bsx_meth_tables(d, out);
	if (op == BSX_METH_OP_RESET) return bsx_meth_reset(d);
	return BSX_E_ARG;
}
static int be_meth_sites(void *c, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n, int64_t *f_next)
{ return bsx_meth_sites(((LaneRef*)c)->d, opt, f_lo, f_hi, out, cap, n, f_next); }
static int be_sort(void *c, int op, int64_t n, const uint64_t *keys, uint32_t *perm_out, int64_t *n_total, uint32_t **run_of)
{
	bsx_device_t *d = ((LaneRef*)c)->d;
	if (op == BSX_SORT_OP_RUN) return bsx_sort_run(d, n, keys, perm_out);
	if (op == BSX_SORT_OP_SCHEDULE) return bsx_sort_schedule(d, n_total, run_of);
	if (op == BSX_SORT_OP_RESET) return bsx_sort_reset(d);
	return BSX_E_ARG;
}
void shim_tables_backend(bsx_backend_t *out)
{
	out->qc_batch = be_qc; out->markdup_batch = be_markdup; out->cov_batch = be_cov; out->sort_batch = be_sort; out->meth_batch = be_meth; out->meth_sites = be_meth_sites;
	out->bam_encode = be_bam_encode; out->bgzf_deflate = be_bgzf_deflate;
}

