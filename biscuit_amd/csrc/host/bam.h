/* bam.h -- BAM output while aligning (--bam): the host side.  include/bsx.h has the public calls and DESIGN.md section 7 the rule. */
#ifndef BSX_BAM_H
#define BSX_BAM_H
#include "bsx_core.h"

/* the reference names of a header as both backends search them (bam_rec.h): sorted, the first of two equal names counting */
struct bsx_bam_refs {
	char *names; uint32_t *off; int32_t *id; int32_t n;   /* bam_reftab_t's arrays; off has n + 1 entries */
	size_t names_len;
	uint64_t serial;                                      /* unique per object: what a backend keys its uploaded copy on */
};

/* the host's own statement of both stages (a backend without the seams; dev == NULL in the public calls): records by bam_rec.h, deflate by
 * zlib level 1 raw + crc32, stored when that is no smaller.  Both append to a caller-owned growable buffer (*out, *out_cap; realloc'd) from
 * offset 0 and say how much they wrote. */
BSX_API int bsx_bam_encode_host(const bsx_bam_refs_t *refs, const char *text, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len,
                                int64_t *n_records, int64_t *bad_record, int *bad_why);
BSX_API int bsx_bgzf_deflate_host(const uint8_t *payload, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len);
/* the writer over an arbitrary backend (copied); be == NULL or a backend without bam_encode / bgzf_deflate: the host's statement of that stage */
BSX_API int bsx_bam_writer_open_backend(const bsx_backend_t *be, const char *header_text, bsx_bam_sink_fn sink, void *ud, bsx_bam_writer_t **out);

#endif
