/* sortout.c -- coordinate-sorted SAM while aligning (--sort), the host side: keys from the text of a finished chunk, the chunk's lines appended
 * to one temporary file in the order the backend computed (bsx_sort_run on the device; a stable merge sort here for a backend without the
 * seam), and at the end the runs streamed out in the order of the backend's schedule, a pread cursor and a buffer per run.  With a device the
 * host compares no two records: it copies bytes in an order it was given.  include/bsx.h has the rule. */
#include <unistd.h>
#include <errno.h>
#include <fcntl.h>
#include "sortout.h"
#include "tune.h"

#define RANK_NONE 0xffffffffu
typedef struct { int64_t off, len, n; } run_t;
struct bsx_sorter {
	bsx_backend_t be; int have_be;
	/* RNAME -> rank: open addressing over the names of the header's @SQ lines */
	char *names; size_t n_slots; int64_t *slot_name; uint32_t *slot_rank;
	int fd; int64_t file_len; int failed;
	run_t *runs; size_t n_runs, m_runs;
	uint64_t **hkeys;      /* host sort only: every run's sorted keys (the device keeps its own) */
	uint64_t n_records;
};

static uint64_t name_hash(const char *s, size_t l)
{
	uint64_t h = 1469598103934665603ull;
	size_t i;
	for (i = 0; i < l; ++i) h = (h ^ (unsigned char)s[i]) * 1099511628211ull;
	return h;
}
static uint32_t rank_of(const bsx_sorter_t *s, const char *name, size_t l)
{
	size_t k;
	if (s->n_slots == 0 || (l == 1 && name[0] == '*')) return RANK_NONE;
	for (k = name_hash(name, l) & (s->n_slots - 1); s->slot_name[k] >= 0; k = (k + 1) & (s->n_slots - 1)) {
		const char *q = s->names + s->slot_name[k];
		if (strcspn(q, "\t\n") == l && memcmp(q, name, l) == 0) return s->slot_rank[k];   /* (the names lie in the header text, ended by its separators) */
	}
	return RANK_NONE;   /* a name the header does not have: behind every contig, like '*' */
}
/* the names of the @SQ lines in the header's order; the first of two equal names keeps its rank */
static int rank_table(bsx_sorter_t *s, const char *hdr)
{
	const char *p;
	size_t n_sq = 0, k;
	uint32_t rank = 0;
	for (p = hdr; p && *p; p = strchr(p, '\n'), p = p ? p + 1 : 0) if (strncmp(p, "@SQ\t", 4) == 0) ++n_sq;
	for (s->n_slots = 16; s->n_slots < 2 * n_sq + 2; s->n_slots <<= 1);
	s->names = strdup(hdr ? hdr : "");
	s->slot_name = (int64_t*)malloc(s->n_slots * sizeof(int64_t));
	s->slot_rank = (uint32_t*)malloc(s->n_slots * sizeof(uint32_t));
	if (!s->names || !s->slot_name || !s->slot_rank) return BSX_E_NOMEM;
	for (k = 0; k < s->n_slots; ++k) s->slot_name[k] = -1;
	for (p = s->names; p && *p; ) {
		char *eol = strchr(p, '\n');
		if (strncmp(p, "@SQ\t", 4) == 0) {
			char *f = (char*)p + 3, *end = eol ? eol : (char*)p + strlen(p);
			while (f < end) { /* the SN field */
				char *g = (char*)memchr(f + 1, '\t', (size_t)(end - f - 1));
				if (!g) g = end;
				if (strncmp(f + 1, "SN:", 3) == 0 && f + 4 <= g) {
					const size_t l = (size_t)(g - (f + 4));
					if (rank_of(s, f + 4, l) == RANK_NONE && !(l == 1 && f[4] == '*')) {
						for (k = name_hash(f + 4, l) & (s->n_slots - 1); s->slot_name[k] >= 0; k = (k + 1) & (s->n_slots - 1));
						s->slot_name[k] = (int64_t)(f + 4 - s->names); s->slot_rank[k] = rank;
					}
					break;
				}
				f = g;
			}
			++rank;
		}
		p = eol ? eol + 1 : 0;
	}
	return BSX_OK;
}

BSX_API uint64_t bsx_sorter_key(const bsx_sorter_t *s, const char *line, size_t len)
{
	const char *end = line + len, *f1, *f2, *f3, *f4, *q;
	uint64_t flag = 0, pos = 0;
	if (!(f1 = (const char*)memchr(line, '\t', len))) return ~0ull;
	if (!(f2 = (const char*)memchr(f1 + 1, '\t', (size_t)(end - f1 - 1)))) return ~0ull;
	if (!(f3 = (const char*)memchr(f2 + 1, '\t', (size_t)(end - f2 - 1)))) return ~0ull;
	if (!(f4 = (const char*)memchr(f3 + 1, '\t', (size_t)(end - f3 - 1)))) f4 = end;
	for (q = f1 + 1; q < f2 && *q >= '0' && *q <= '9'; ++q) flag = flag * 10 + (uint64_t)(*q - '0');
	for (q = f3 + 1; q < f4 && *q >= '0' && *q <= '9'; ++q) pos = pos * 10 + (uint64_t)(*q - '0');
	return BSX_SORT_KEY(rank_of(s, f2 + 1, (size_t)(f3 - f2 - 1)), pos & 0x7fffffffull, flag & 0x10);
}

/* stable bottom-up merge sort of the indices by key */
BSX_API void bsx_sort_host_perm(int64_t n, const uint64_t *keys, uint32_t *perm, uint32_t *tmp)
{
	int64_t w, i;
	uint32_t *a = perm, *b = tmp;
	for (i = 0; i < n; ++i) a[i] = (uint32_t)i;
	for (w = 1; w < n; w <<= 1) {
		for (i = 0; i < n; i += 2 * w) {
			int64_t l = i, m = bsx_min(i + w, n), r = m, e = bsx_min(i + 2 * w, n), o = i;
			while (l < m && r < e) b[o++] = keys[a[r]] < keys[a[l]] ? a[r++] : a[l++];   /* (the right one only when strictly smaller: stable) */
			while (l < m) b[o++] = a[l++];
			while (r < e) b[o++] = a[r++];
		}
		{ uint32_t *t = a; a = b; b = t; }
	}
	if (a != perm) memcpy(perm, a, (size_t)n * sizeof(uint32_t));
}

/* (no $TMPDIR: the library reads the few environment variables tests/test_tune.py lists and no others; --sort-tmp "$TMPDIR" says the same) */
static const char *tmp_dir_of(const char *dir) { return dir && *dir ? dir : "/tmp"; }
/* a file in the directory that has no name any more: no exit leaves it behind */
static int tmp_open(const char *dir)
{
	const char *d = tmp_dir_of(dir);
	const size_t l = strlen(d) + 32;
	char *path = (char*)malloc(l);
	int fd;
	if (!path) return -1;
	snprintf(path, l, "%s/bsx_sort_XXXXXX", d);
	fd = mkstemp(path);
	if (fd >= 0) unlink(path);
	free(path);
	return fd;
}
BSX_API int bsx_sorter_dir_ok(const char *tmp_dir)
{
	const int fd = tmp_open(tmp_dir);
	if (fd < 0) return BSX_E_IO;
	close(fd);
	return BSX_OK;
}

BSX_API int bsx_sorter_open_backend(const bsx_backend_t *be, const char *header, const char *tmp_dir, bsx_sorter_t **out)
{
	bsx_sorter_t *s;
	int rc;
	*out = 0;
	if (!(s = (bsx_sorter_t*)calloc(1, sizeof(*s)))) return BSX_E_NOMEM;
	s->fd = -1;
	if (be && be->sort_batch) { s->be = *be; s->have_be = 1; }
	if ((rc = rank_table(s, header)) != BSX_OK) { bsx_sorter_close(s); return rc; }
	if ((s->fd = tmp_open(tmp_dir)) < 0) { bsx_sorter_close(s); return BSX_E_IO; }
	if (s->have_be && (rc = s->be.sort_batch(s->be.ctx, BSX_SORT_OP_RESET, 0, 0, 0, 0, 0)) != BSX_OK) { bsx_sorter_close(s); return rc; }
	*out = s;
	return BSX_OK;
}

BSX_API void bsx_sorter_close(bsx_sorter_t *s)
{
	size_t i;
	if (!s) return;
	if (s->have_be) (void)s->be.sort_batch(s->be.ctx, BSX_SORT_OP_RESET, 0, 0, 0, 0, 0);
	if (s->fd >= 0) close(s->fd);
	for (i = 0; s->hkeys && i < s->n_runs; ++i) free(s->hkeys[i]);
	free(s->hkeys); free(s->runs); free(s->names); free(s->slot_name); free(s->slot_rank);
	free(s);
}

BSX_API void bsx_sorter_counts(const bsx_sorter_t *s, uint64_t *n_runs, uint64_t *n_records)
{
	if (n_runs) *n_runs = s ? s->n_runs : 0;
	if (n_records) *n_records = s ? s->n_records : 0;
}

static int write_all(bsx_sorter_t *s, const char *buf, size_t n)
{
	while (n) {
		const ssize_t w = pwrite(s->fd, buf, n, (off_t)s->file_len);
		if (w < 0 && errno == EINTR) continue;
		if (w <= 0) {
			fprintf(stderr, "[E::%s] writing the temporary file of --sort failed: %s\n", "bsx_sorter", w < 0 ? strerror(errno) : "nothing written");
			s->failed = 1;
			return BSX_E_IO;
		}
		buf += w; n -= (size_t)w; s->file_len += w;
	}
	return BSX_OK;
}

BSX_API int bsx_sorter_add(bsx_sorter_t *s, const char *text, size_t len)
{
	BSX_VEC(int64_t) at;   /* line starts, and the end behind the last */
	uint64_t *keys = 0;
	uint32_t *perm = 0;
	char *ordered = 0;
	int64_t n, i;
	size_t o = 0;
	int rc = BSX_OK;
	if (!s) return BSX_E_ARG;
	if (s->failed) return BSX_E_IO;
	if (len == 0) return BSX_OK;
	bsx_vec_init(at);
	{
		const char *p = text, *end = text + len;
		while (p < end) {
			const char *nl = (const char*)memchr(p, '\n', (size_t)(end - p));
			bsx_vec_push(at, (int64_t)(p - text));
			p = nl ? nl + 1 : end;
		}
		bsx_vec_push(at, (int64_t)len);
	}
	n = (int64_t)at.n - 1;
	if (n >= ((int64_t)1 << 31)) { bsx_vec_free(at); return BSX_E_ARG; }
	keys = (uint64_t*)malloc((size_t)n * sizeof(uint64_t));
	perm = (uint32_t*)malloc((size_t)n * 2 * sizeof(uint32_t));
	ordered = (char*)malloc(len);
	if (!keys || !perm || !ordered || !at.a) { rc = BSX_E_NOMEM; goto done; }
	for (i = 0; i < n; ++i) keys[i] = bsx_sorter_key(s, text + at.a[i], (size_t)(at.a[i + 1] - at.a[i]));
	if (s->have_be) rc = s->be.sort_batch(s->be.ctx, BSX_SORT_OP_RUN, n, keys, perm, 0, 0);
	else bsx_sort_host_perm(n, keys, perm, perm + n);
	if (rc != BSX_OK) goto done;
	for (i = 0; i < n; ++i) {
		const int64_t a = at.a[perm[i]], l = at.a[perm[i] + 1] - a;
		memcpy(ordered + o, text + a, (size_t)l);
		o += (size_t)l;
	}
	if (s->n_runs == s->m_runs) {
		s->m_runs = s->m_runs ? s->m_runs * 2 : 16;
		s->runs = (run_t*)realloc(s->runs, s->m_runs * sizeof(run_t));
		if (!s->have_be) s->hkeys = (uint64_t**)realloc(s->hkeys, s->m_runs * sizeof(uint64_t*));
	}
	s->runs[s->n_runs].off = s->file_len; s->runs[s->n_runs].len = (int64_t)len; s->runs[s->n_runs].n = n;
	if (!s->have_be) { /* the run's keys in its order, for the schedule */
		uint64_t *sk = (uint64_t*)malloc((size_t)n * sizeof(uint64_t));
		if (!sk) { rc = BSX_E_NOMEM; goto done; }
		for (i = 0; i < n; ++i) sk[i] = keys[perm[i]];
		s->hkeys[s->n_runs] = sk;
	}
	++s->n_runs;
	s->n_records += (uint64_t)n;
	rc = write_all(s, ordered, len);
done:
	if (rc != BSX_OK) s->failed = 1;
	bsx_vec_free(at); free(keys); free(perm); free(ordered);
	return rc;
}

/* a backend without the seam: the stable order of the concatenation of the runs' keys, as run ids */
static int host_schedule(bsx_sorter_t *s, int64_t *n_total, uint32_t **run_of)
{
	int64_t n = 0, i, o = 0;
	size_t r;
	uint64_t *keys;
	uint32_t *perm, *runs;
	*n_total = 0; *run_of = 0;
	for (r = 0; r < s->n_runs; ++r) n += s->runs[r].n;
	if (n == 0) return BSX_OK;
	if (n >= ((int64_t)1 << 31)) return BSX_E_ARG;
	keys = (uint64_t*)malloc((size_t)n * 8); perm = (uint32_t*)malloc((size_t)n * 8); runs = (uint32_t*)malloc((size_t)n * 4);
	if (!keys || !perm || !runs) { free(keys); free(perm); free(runs); return BSX_E_NOMEM; }
	for (r = 0; r < s->n_runs; ++r) for (i = 0; i < s->runs[r].n; ++i, ++o) { keys[o] = s->hkeys[r][i]; runs[o] = (uint32_t)r; }
	bsx_sort_host_perm(n, keys, perm, perm + n);
	for (i = 0; i < n; ++i) perm[n + i] = runs[perm[i]];
	memcpy(runs, perm + n, (size_t)n * 4);
	free(keys); free(perm);
	*n_total = n; *run_of = runs;
	return BSX_OK;
}

typedef struct { int64_t at, end; char *buf; size_t have, used; } cursor_t;
#define OUT_PIECE ((size_t)4 << 20)

BSX_API int bsx_sorter_finish(bsx_sorter_t *s, int (*sink)(void *ud, const char *text, size_t len), void *ud)
{
	int64_t n_total = 0, i;
	uint32_t *run_of = 0;
	cursor_t *cur = 0;
	BSX_VEC(char) out;
	size_t r, buf_bytes;
	int rc;
	if (!s || !sink) return BSX_E_ARG;
	if (s->failed) return BSX_E_IO;
	rc = s->have_be ? s->be.sort_batch(s->be.ctx, BSX_SORT_OP_SCHEDULE, 0, 0, 0, &n_total, &run_of) : host_schedule(s, &n_total, &run_of);
	if (rc != BSX_OK) return rc;
	if ((uint64_t)n_total != s->n_records) { free(run_of); return BSX_E_INTERNAL; }
	if (n_total == 0) { free(run_of); return BSX_OK; }
	/* every run reads through a buffer of its own: all of them together about 1 GB at most, 8 MB each at most */
	buf_bytes = (size_t)bsx_tune_long("sort_buf_bytes", (long)bsx_min(((int64_t)1 << 30) / (int64_t)s->n_runs, (int64_t)8 << 20));
	if (buf_bytes < 1) buf_bytes = 1;
	bsx_vec_init(out);
	cur = (cursor_t*)calloc(s->n_runs, sizeof(cursor_t));
	if (!cur) { free(run_of); return BSX_E_NOMEM; }
	for (r = 0; r < s->n_runs; ++r) {
		cur[r].at = s->runs[r].off; cur[r].end = s->runs[r].off + s->runs[r].len;
		if (!(cur[r].buf = (char*)malloc(bsx_min(buf_bytes, (size_t)s->runs[r].len + 1)))) { rc = BSX_E_NOMEM; goto done; }
	}
	for (i = 0; i < n_total; ++i) {
		cursor_t *c;
		int line_done = 0;
		size_t line_len = 0;
		if (run_of[i] >= s->n_runs) { rc = BSX_E_INTERNAL; goto done; }
		c = &cur[run_of[i]];
		while (!line_done) { /* the next line of this run, through as many fills of its buffer as it is long */
			const char *p, *nl;
			size_t l;
			if (c->used == c->have) {
				const size_t want = (size_t)bsx_min((int64_t)buf_bytes, c->end - c->at);
				ssize_t got;
				if (want == 0) { if (line_len) break; rc = BSX_E_INTERNAL; goto done; }   /* (a last line without its newline ends with the run) */
				do got = pread(s->fd, c->buf, want, (off_t)c->at); while (got < 0 && errno == EINTR);
				if (got <= 0) { fprintf(stderr, "[E::%s] reading the temporary file of --sort failed: %s\n", "bsx_sorter", got < 0 ? strerror(errno) : "it ends early"); rc = BSX_E_IO; goto done; }
				c->at += got; c->have = (size_t)got; c->used = 0;
			}
			p = c->buf + c->used;
			nl = (const char*)memchr(p, '\n', c->have - c->used);
			l = nl ? (size_t)(nl + 1 - p) : c->have - c->used;
			bsx_vec_reserve(out, out.n + l + 1);
			if (!out.a) { rc = BSX_E_NOMEM; goto done; }
			memcpy(out.a + out.n, p, l);
			out.n += l; c->used += l; line_len += l;
			line_done = nl != 0;
		}
		if (out.n >= OUT_PIECE || i + 1 == n_total) {
			if (sink(ud, out.a, out.n) != 0) { rc = BSX_E_IO; goto done; }
			out.n = 0;
		}
	}
	for (r = 0; r < s->n_runs; ++r) if (cur[r].at != cur[r].end || cur[r].used != cur[r].have) { rc = BSX_E_INTERNAL; break; }   /* every run was read to its end */
done:
	for (r = 0; cur && r < s->n_runs; ++r) free(cur[r].buf);
	free(cur); free(run_of); bsx_vec_free(out);
	return rc;
}

/* the header of a sorted file (include/bsx.h) */
BSX_API char *bsx_sort_header(const char *header)
{
	static const char so[] = "SO:coordinate";
	const char *h = header ? header : "", *p, *hd = 0, *hd_end = 0;
	char *out = (char*)malloc(strlen(h) + 64), *o = out;
	if (!out) return 0;
	for (p = h; *p; ) {
		const char *eol = strchr(p, '\n'), *next = eol ? eol + 1 : p + strlen(p);
		if (strncmp(p, "@HD", 3) == 0 && (p[3] == '\t' || p[3] == '\n' || p[3] == 0)) { hd = p; hd_end = eol ? eol : next; break; }
		p = next;
	}
	if (!hd) o += sprintf(o, "@HD\tVN:1.6\t%s\n", so);
	else { /* its fields, SO: replaced or appended */
		int had = 0;
		for (p = hd; p < hd_end; ) {
			const char *t = (const char*)memchr(p, '\t', (size_t)(hd_end - p)), *e = t ? t : hd_end;
			if (p != hd) *o++ = '\t';
			if (p != hd && e - p >= 3 && strncmp(p, "SO:", 3) == 0) { memcpy(o, so, sizeof(so) - 1); o += sizeof(so) - 1; had = 1; }
			else { memcpy(o, p, (size_t)(e - p)); o += e - p; }
			p = t ? t + 1 : hd_end;
			if (t && p == hd_end) *o++ = '\t';   /* (a trailing tab stays) */
		}
		if (!had) { *o++ = '\t'; memcpy(o, so, sizeof(so) - 1); o += sizeof(so) - 1; }
		*o++ = '\n';
	}
	for (p = h; *p; ) { /* every other line as it is */
		const char *eol = strchr(p, '\n'), *next = eol ? eol + 1 : p + strlen(p);
		if (p != hd) { memcpy(o, p, (size_t)(next - p)); o += next - p; }
		p = next;
	}
	*o = 0;
	return out;
}
