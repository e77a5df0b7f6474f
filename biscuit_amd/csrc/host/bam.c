/* bam.c -- BAM output while aligning (--bam): the header part of the payload, the reference name table, the host's own statement of both
 * stages (records by bam_rec.h, the one rule the device compiles too; deflate by zlib level 1 raw + crc32) and the writer that carries the
 * tail of the record stream from call to call so that every block but the last holds exactly BSX_BGZF_BLOCK payload bytes.
 * DESIGN.md section 7 has the rule, tests/bam_model.py is its reference statement. */
#include <zlib.h>
#include "bsx_core.h"
#include "tune.h"
#include "bam.h"
#include "bam_rec.h"

static const uint8_t g_bgzf_eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

BSX_API const char *bsx_bam_strerror(int why)
{
	switch (why) {
	case BSX_BAM_E_LINE: return "not a SAM record (fewer than 11 columns, an empty column, or a number that is none or out of range)";
	case BSX_BAM_E_TAG: return "a field after column 11 is not XX:T:value with T in A, i, Z, f";
	case BSX_BAM_E_INT: return "an integer tag outside -2^31 .. 2^32 - 1";
	case BSX_BAM_E_NAME: return "a read name longer than 254 bytes";
	case BSX_BAM_E_CIGAR: return "more than 65535 CIGAR operations";
	case BSX_BAM_E_REF: return "an RNAME or RNEXT without an @SQ line in the header";
	case BSX_BAM_E_QUAL: return "SEQ and QUAL of different lengths";
	}
	return "unknown reason";
}

static int grow(uint8_t **out, size_t *cap, size_t want)
{
	if (want > *cap) {
		size_t m = *cap ? *cap : 4096;
		uint8_t *p;
		while (m < want) m += m >> 1;
		if ((p = (uint8_t*)realloc(*out, m)) == 0) return BSX_E_NOMEM;
		*out = p; *cap = m;
	}
	return BSX_OK;
}

/* ---- the header: its @SQ lines, in order ---- */
typedef struct { const char *name; uint32_t l_name; int64_t ln; int32_t idx; } sq_t;
typedef BSX_VEC(sq_t) sq_v;
static void header_refs(const char *text, sq_v *v)
{
	const char *p = text;
	bsx_vec_init(*v);
	while (*p) {
		const char *e = strchr(p, '\n'), *end = e ? e : p + strlen(p);
		if (end - p >= 4 && memcmp(p, "@SQ\t", 4) == 0) {
			sq_t s = {0, 0, 0, 0};
			int have_ln = 0;
			const char *f = p + 4;
			while (f < end) {
				const char *g = memchr(f, '\t', (size_t)(end - f));
				if (!g) g = end;
				if (g - f >= 3 && memcmp(f, "SN:", 3) == 0 && !s.name) { s.name = f + 3; s.l_name = (uint32_t)(g - f - 3); }
				else if (g - f >= 3 && memcmp(f, "LN:", 3) == 0 && !have_ln) { s.ln = strtoll(f + 3, 0, 10); have_ln = 1; }
				f = g + 1;
			}
			if (s.name) { s.idx = (int32_t)v->n; bsx_vec_push(*v, s); }
		}
		if (!e) break;
		p = e + 1;
	}
}
static int sq_cmp(const void *a_, const void *b_)
{
	const sq_t *a = (const sq_t*)a_, *b = (const sq_t*)b_;
	const uint32_t k = a->l_name < b->l_name ? a->l_name : b->l_name;
	const int c = memcmp(a->name, b->name, k);
	if (c) return c;
	if (a->l_name != b->l_name) return a->l_name < b->l_name ? -1 : 1;
	return a->idx < b->idx ? -1 : a->idx > b->idx;
}

BSX_API int bsx_bam_header(const char *text, uint8_t **out, size_t *out_len)
{
	sq_v v;
	size_t l_text, n = 0, i;
	uint8_t *o;
	if (!text || !out || !out_len) return BSX_E_ARG;
	l_text = strlen(text);
	if (l_text > 0x7fffffff) return BSX_E_ARG;
	header_refs(text, &v);
	n = 12 + l_text;
	for (i = 0; i < v.n; ++i) n += 8 + v.a[i].l_name + 1;
	if ((o = (uint8_t*)malloc(n)) == 0) { bsx_vec_free(v); return BSX_E_NOMEM; }
#define P32(at, x) do { const uint32_t x_ = (uint32_t)(x); o[at] = (uint8_t)x_; o[(at) + 1] = (uint8_t)(x_ >> 8); o[(at) + 2] = (uint8_t)(x_ >> 16); o[(at) + 3] = (uint8_t)(x_ >> 24); } while (0)
	memcpy(o, "BAM\1", 4);
	P32(4, l_text);
	memcpy(o + 8, text, l_text);
	n = 8 + l_text;
	P32(n, v.n); n += 4;
	for (i = 0; i < v.n; ++i) {
		P32(n, v.a[i].l_name + 1); n += 4;
		memcpy(o + n, v.a[i].name, v.a[i].l_name); n += v.a[i].l_name;
		o[n++] = 0;
		P32(n, v.a[i].ln); n += 4;
	}
#undef P32
	bsx_vec_free(v);
	*out = o; *out_len = n;
	return BSX_OK;
}

BSX_API int bsx_bam_refs_open(const char *text, bsx_bam_refs_t **out)
{
	static uint64_t serial = 0;
	sq_v v;
	bsx_bam_refs_t *r;
	size_t i, tot = 0;
	int32_t k = 0;
	if (!text || !out) return BSX_E_ARG;
	*out = 0;
	header_refs(text, &v);
	if (v.n) qsort(v.a, v.n, sizeof(sq_t), sq_cmp);
	for (i = 0; i < v.n; ++i) tot += v.a[i].l_name;
	if ((r = (bsx_bam_refs_t*)calloc(1, sizeof(*r))) == 0) { bsx_vec_free(v); return BSX_E_NOMEM; }
	r->names = (char*)malloc(tot + 1); r->off = (uint32_t*)malloc((v.n + 1) * sizeof(uint32_t)); r->id = (int32_t*)malloc((v.n + 1) * sizeof(int32_t));
	if (!r->names || !r->off || !r->id) { bsx_bam_refs_close(r); bsx_vec_free(v); return BSX_E_NOMEM; }
	tot = 0;
	for (i = 0; i < v.n; ++i) { /* of equal names the first line's (sorted first) stays */
		if (i && v.a[i].l_name == v.a[i - 1].l_name && memcmp(v.a[i].name, v.a[i - 1].name, v.a[i].l_name) == 0) continue;
		r->off[k] = (uint32_t)tot; r->id[k] = v.a[i].idx; ++k;
		memcpy(r->names + tot, v.a[i].name, v.a[i].l_name); tot += v.a[i].l_name;
	}
	r->off[k] = (uint32_t)tot; r->n = k; r->names_len = tot;
	r->serial = __atomic_add_fetch(&serial, 1, __ATOMIC_RELAXED);
	bsx_vec_free(v);
	*out = r;
	return BSX_OK;
}
BSX_API void bsx_bam_refs_close(bsx_bam_refs_t *r)
{
	if (!r) return;
	free(r->names); free(r->off); free(r->id); free(r);
}

/* ---- the host's statement of the two stages ---- */
BSX_API int bsx_bam_encode_host(const bsx_bam_refs_t *refs, const char *text, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len,
                                int64_t *n_records, int64_t *bad_record, int *bad_why)
{
	bam_reftab_t T;
	size_t at = 0, n = 0;
	int64_t rec = 0;
	if (!refs || !out || !out_cap || !out_len || !n_records || !bad_record || !bad_why || (len && !text)) return BSX_E_ARG;
	*out_len = 0; *n_records = 0; *bad_record = -1; *bad_why = 0;
	if (len && text[len - 1] != '\n') return BSX_E_ARG;
	T.names = refs->names; T.off = refs->off; T.id = refs->id; T.n = refs->n;
	while (at < len) {
		const char *e = (const char*)memchr(text + at, '\n', len - at);
		const size_t l = (size_t)(e - (text + at));
		int err = 0;
		uint32_t sz;
		if (l > 0x7ffffff0u) { *bad_record = rec; *bad_why = BSX_BAM_E_LINE; break; }
		sz = bam_rec_encode(text + at, (uint32_t)l, &T, 0, &err, 0);
		if (err) { *bad_record = rec; *bad_why = err; break; }
		if (grow(out, out_cap, n + sz) != BSX_OK) return BSX_E_NOMEM;
		bam_rec_encode(text + at, (uint32_t)l, &T, *out + n, &err, 0);
		n += sz; at += l + 1; ++rec;
	}
	*out_len = n; *n_records = rec;
	return BSX_OK;
}

/* one block's member around raw (its deflate stream) at o; returns its length */
static size_t bgzf_frame(uint8_t *o, const uint8_t *raw, size_t n_raw, const uint8_t *data, size_t n)
{
	static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
	const size_t total = 18 + n_raw + 8;
	const uint32_t crc = (uint32_t)crc32(crc32(0, 0, 0), data, (uInt)n);
	memcpy(o, head, 16);
	o[16] = (uint8_t)(total - 1); o[17] = (uint8_t)((total - 1) >> 8);
	if (raw != o + 18) memmove(o + 18, raw, n_raw);
	o += 18 + n_raw;
	o[0] = (uint8_t)crc; o[1] = (uint8_t)(crc >> 8); o[2] = (uint8_t)(crc >> 16); o[3] = (uint8_t)(crc >> 24);
	o[4] = (uint8_t)n; o[5] = (uint8_t)(n >> 8); o[6] = o[7] = 0;
	return total;
}
BSX_API int bsx_bgzf_deflate_host(const uint8_t *payload, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len)
{
	size_t at, w = 0;
	if (!out || !out_cap || !out_len || (len && !payload)) return BSX_E_ARG;
	*out_len = 0;
	for (at = 0; at < len; at += BSX_BGZF_BLOCK) {
		const size_t n = bsx_min(len - at, (size_t)BSX_BGZF_BLOCK);
		z_stream z;
		uint8_t *o;
		size_t n_raw;
		int zr;
		if (grow(out, out_cap, w + 65536 + 64) != BSX_OK) return BSX_E_NOMEM;
		o = *out + w;
		memset(&z, 0, sizeof(z));
		if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return BSX_E_INTERNAL;
		z.next_in = (Bytef*)(payload + at); z.avail_in = (uInt)n;
		z.next_out = o + 18; z.avail_out = (uInt)(n + 4);   /* anything that needs n + 5 or more is stored */
		zr = deflate(&z, Z_FINISH);
		n_raw = z.total_out;
		deflateEnd(&z);
		if (zr != Z_STREAM_END) { /* one stored block */
			o[18] = 1; o[19] = (uint8_t)n; o[20] = (uint8_t)(n >> 8); o[21] = (uint8_t)~n; o[22] = (uint8_t)(~n >> 8);
			memcpy(o + 23, payload + at, n);
			n_raw = 5 + n;
		}
		w += bgzf_frame(o, o + 18, n_raw, payload + at, n);
	}
	*out_len = w;
	return BSX_OK;
}

/* ---- the public seams: the device's kernels, or with dev == NULL the statements above ---- */
BSX_API int bsx_bam_encode(bsx_device_t *dev, const bsx_bam_refs_t *refs, const char *text, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len,
                           int64_t *n_records, int64_t *bad_record, int *bad_why)
{
	bsx_backend_t be;
	int rc;
	if (!dev) return bsx_bam_encode_host(refs, text, len, out, out_cap, out_len, n_records, bad_record, bad_why);
	if ((rc = bsx_hip_backend(dev, &be)) != BSX_OK) return rc;
	if (!refs || !out || !out_cap || !out_len || !n_records || !bad_record || !bad_why || (len && !text)) return BSX_E_ARG;
	return be.bam_encode(be.ctx, refs, text, len, out, out_cap, out_len, n_records, bad_record, bad_why);
}
BSX_API int bsx_bgzf_deflate(bsx_device_t *dev, const uint8_t *payload, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len)
{
	bsx_backend_t be;
	int rc;
	if (!dev) return bsx_bgzf_deflate_host(payload, len, out, out_cap, out_len);
	if ((rc = bsx_hip_backend(dev, &be)) != BSX_OK) return rc;
	if (!out || !out_cap || !out_len || (len && !payload)) return BSX_E_ARG;
	return be.bgzf_deflate(be.ctx, payload, len, out, out_cap, out_len);
}

/* ---- the writer ---- */
struct bsx_bam_writer {
	bsx_backend_t be; int have_enc, have_defl;
	bsx_bam_refs_t *refs;
	bsx_bam_sink_fn sink; void *ud;
	uint8_t *hdr; size_t hdr_len;          /* the header's block, until the sink has had it */
	uint8_t *pay; size_t pay_cap;          /* a piece's records */
	uint8_t *tail; size_t tail_len;        /* payload carried to the next piece: the tail behind the last whole block, then the new records */
	size_t tail_cap;
	uint8_t *blk; size_t blk_cap;
	int failed;                            /* BSX_E_* of the first failure: every later call returns it */
	int64_t bad_record; int bad_why;
	uint64_t n_records, n_payload, n_written;
};

static int w_sink(bsx_bam_writer_t *w, const uint8_t *data, size_t len)
{
	if (w->hdr) {
		if (w->sink(w->ud, w->hdr, w->hdr_len, 1) != 0) return BSX_E_IO;
		w->n_written += w->hdr_len;
		free(w->hdr); w->hdr = 0;
	}
	if (len) { if (w->sink(w->ud, data, len, 0) != 0) return BSX_E_IO; w->n_written += len; }
	return BSX_OK;
}
static int w_deflate(bsx_bam_writer_t *w, const uint8_t *p, size_t n, size_t *out_len)
{
	return w->have_defl ? w->be.bgzf_deflate(w->be.ctx, p, n, &w->blk, &w->blk_cap, out_len) : bsx_bgzf_deflate_host(p, n, &w->blk, &w->blk_cap, out_len);
}

BSX_API int bsx_bam_writer_open_backend(const bsx_backend_t *be, const char *header_text, bsx_bam_sink_fn sink, void *ud, bsx_bam_writer_t **out)
{
	bsx_bam_writer_t *w;
	uint8_t *h = 0, *blk = 0;
	size_t hl = 0, cap = 0, bl = 0;
	int rc;
	if (!header_text || !sink || !out) return BSX_E_ARG;
	*out = 0;
	if ((w = (bsx_bam_writer_t*)calloc(1, sizeof(*w))) == 0) return BSX_E_NOMEM;
	if (be) { w->be = *be; w->have_enc = be->bam_encode != 0; w->have_defl = be->bgzf_deflate != 0; }
	w->sink = sink; w->ud = ud; w->bad_record = -1;
	if ((rc = bsx_bam_refs_open(header_text, &w->refs)) != BSX_OK || (rc = bsx_bam_header(header_text, &h, &hl)) != BSX_OK) { bsx_bam_refs_close(w->refs); free(w); return rc; }
	/* the header part ends its block(s): the first record starts a new one */
	rc = w->have_defl ? w->be.bgzf_deflate(w->be.ctx, h, hl, &blk, &cap, &bl) : bsx_bgzf_deflate_host(h, hl, &blk, &cap, &bl);
	free(h);
	if (rc != BSX_OK) { free(blk); bsx_bam_refs_close(w->refs); free(w); return rc; }
	w->hdr = blk; w->hdr_len = bl;
	*out = w;
	return BSX_OK;
}
BSX_API int bsx_bam_writer_open(bsx_device_t *dev, const char *header_text, bsx_bam_sink_fn sink, void *ud, bsx_bam_writer_t **out)
{
	bsx_backend_t be;
	int rc;
	if (!dev) return bsx_bam_writer_open_backend(0, header_text, sink, ud, out);
	if ((rc = bsx_hip_backend(dev, &be)) != BSX_OK) return rc;
	return bsx_bam_writer_open_backend(&be, header_text, sink, ud, out);
}

static int w_piece(bsx_bam_writer_t *w, const char *text, size_t len)
{
	size_t n_pay = 0, whole, n_blk = 0;
	int64_t n_rec = 0, bad = -1;
	int why = 0, rc;
	rc = w->have_enc ? w->be.bam_encode(w->be.ctx, w->refs, text, len, &w->pay, &w->pay_cap, &n_pay, &n_rec, &bad, &why)
	                 : bsx_bam_encode_host(w->refs, text, len, &w->pay, &w->pay_cap, &n_pay, &n_rec, &bad, &why);
	if (rc != BSX_OK) return rc;
	if (bad >= 0) { w->bad_record = (int64_t)w->n_records + bad; w->bad_why = why; return BSX_E_FORMAT; }
	if (grow(&w->tail, &w->tail_cap, w->tail_len + n_pay) != BSX_OK) return BSX_E_NOMEM;
	memcpy(w->tail + w->tail_len, w->pay, n_pay);
	w->tail_len += n_pay; w->n_records += (uint64_t)n_rec; w->n_payload += n_pay;
	whole = w->tail_len / BSX_BGZF_BLOCK * BSX_BGZF_BLOCK;
	if (whole) {
		if ((rc = w_deflate(w, w->tail, whole, &n_blk)) != BSX_OK) return rc;
		if ((rc = w_sink(w, w->blk, n_blk)) != BSX_OK) return rc;
		memmove(w->tail, w->tail + whole, w->tail_len - whole);
		w->tail_len -= whole;
	}
	return BSX_OK;
}

BSX_API int bsx_bam_writer_add(bsx_bam_writer_t *w, const char *text, size_t len)
{
	size_t at = 0, piece;
	if (!w || (len && !text)) return BSX_E_ARG;
	if (w->failed) return w->failed;
	if (len && text[len - 1] != '\n') return BSX_E_ARG;
	piece = (size_t)bsx_tune_long("bam_piece_bytes", 32l << 20);
	if (piece < 1) piece = 1;
	while (at < len) { /* pieces of whole lines: as many as fit, at least one */
		size_t end = at + piece;
		int rc;
		if (end >= len) end = len;
		else {
			size_t e = end;
			while (e > at && text[e - 1] != '\n') --e;
			if (e == at) { const char *q = (const char*)memchr(text + end, '\n', len - end); e = (size_t)(q - text) + 1; }
			end = e;
		}
		if ((rc = w_piece(w, text + at, end - at)) != BSX_OK) { w->failed = rc; return rc; }
		at = end;
	}
	return BSX_OK;
}

BSX_API int bsx_bam_writer_close(bsx_bam_writer_t *w, int finish)
{
	int rc = BSX_OK;
	if (!w) return BSX_E_ARG;
	if (finish) {
		rc = w->failed;
		if (rc == BSX_OK && w->tail_len) { size_t n_blk = 0; if ((rc = w_deflate(w, w->tail, w->tail_len, &n_blk)) == BSX_OK) rc = w_sink(w, w->blk, n_blk); }
		if (rc == BSX_OK) rc = w_sink(w, g_bgzf_eof, sizeof(g_bgzf_eof));
	}
	bsx_bam_refs_close(w->refs);
	free(w->hdr); free(w->pay); free(w->tail); free(w->blk); free(w);
	return rc;
}
BSX_API void bsx_bam_writer_refused(const bsx_bam_writer_t *w, int64_t *record, int *why)
{
	if (record) *record = w ? w->bad_record : -1;
	if (why) *why = w ? w->bad_why : 0;
}
BSX_API void bsx_bam_writer_counts(const bsx_bam_writer_t *w, uint64_t *n_records, uint64_t *payload_bytes, uint64_t *bytes_written)
{
	if (n_records) *n_records = w ? w->n_records : 0;
	if (payload_bytes) *payload_bytes = w ? w->n_payload : 0;
	if (bytes_written) *bytes_written = w ? w->n_written : 0;
}
