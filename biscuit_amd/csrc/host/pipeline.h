/* pipeline.h -- per-chunk working records of the batch pipeline (pipeline.c) */
#ifndef BSX_PIPELINE_H
#define BSX_PIPELINE_H

#include "align_types.h"

/* one strand search (mem_align1_core call, lib/aln/bwamem.c:183-208) being turned into regions */
typedef struct {
	/* header: every strand search */
	int read_idx, parent;
	uint32_t qoff;            /* of the clipped read in the chunk read buffer */
	int l_query;
	const uint8_t *query;     /* clipped raw read on the host */
	chain_v chains;
	BSX_VEC(reg_t) regs;
	int has_job, done;
	/* state machine (extend.c): only touched for the strand searches the host chains itself (bsx_c2r_init) */
	int ci, chain_open, pass, n0;
	uint64_t *srt; int n_srt, m_srt, k;
	int stage, tryi;
	int64_t rmax[2]; int rid;
	reg_t cur; int aw[2]; int sc0;
	bsx_ext_job_t job;
} c2r_t;
#define C2R_HEADER_BYTES offsetof(c2r_t, ci)
static inline void bsx_c2r_init(c2r_t *t) { memset((char*)t + C2R_HEADER_BYTES, 0, sizeof(c2r_t) - C2R_HEADER_BYTES); }

int  bsx_c2r_advance(const bsx_opt_t *opt, const bsx_index_t *idx, c2r_t *t);
void bsx_c2r_consume(const bsx_opt_t *opt, const bsx_index_t *idx, c2r_t *t, const bsx_ext_res_t *res);
void bsx_c2r_release(c2r_t *t);

/* ---------------- sam.c ---------------- */
/* one computed CIGAR (what mem_alnreg_setSAM leaves in a region, lib/aln/mem_alnreg_format.c:40-123) */
typedef struct {
	int valid;
	int pos, n_cigar, NM, bss_u;
	uint32_t is_rev, ZC, ZR;
	uint32_t *cigar;          /* ops + MD text, malloc'd */
} samrec_t;

/* one written record as the final pass notes it (BISCUITqc while aligning, qc.c): the fields the host counts, and the device's job when the record is mapped */
typedef struct {
	bsx_qc_job_t job;     /* cig_off: into the unit's own CIGAR words */
	int32_t tlen;
	uint16_t flag;
	uint8_t mapq, mapped;
	/* the base-averaged conversion table (--qc-meth, meth.c): does the record count, where its quality mask starts in the unit's mask words,
	 * the forward interval a read 2 leaves to its mate (empty otherwise) */
	uint8_t meth;
	uint32_t qm_off;
	int64_t ov_beg, ov_end;
} bsx_qc_rec_t;
typedef BSX_VEC(bsx_qc_rec_t) bsx_qc_rec_v;
typedef BSX_VEC(uint32_t) bsx_qc_cig_v;

typedef struct {
	/* plan mode: collect the regions whose CIGAR will be needed instead of formatting */
	int plan;
	BSX_VEC(int) want[2];     /* region indices per read of the pair (or [0] for SE) */
	samrec_t *table[2];       /* per region, filled between plan and final pass */
	/* tests: with trace != NULL the planning pass notes every record it would write: read of the pair, index of the region in its
	 * list (-1: the unmapped stand-in), index of the mate's region (-1: unmapped stand-in, -2: none), flag and mapq of the region
	 * at that moment, is_primary */
	int (*trace)[6]; int n_trace, m_trace;
	/* conversion by context (bsconv while aligning; NULL: off): the setting, per region the counts of both strand hypotheses (beside table[],
	 * filled with it), and what the final pass counted over this unit's records: the eight totals, records seen, records filtered */
	const bsx_bsconv_conf_t *bs;
	int bs_filter;
	bsx_glb_ctx_t *zn[2];
	uint32_t bs_tot[10];
	/* BISCUITqc while aligning (0: off): where the unit's reads lie in the chunk's read buffer, and what the final pass wrote */
	int qc;
	uint32_t qc_roff[2];
	bsx_qc_rec_v qc_recs;
	bsx_qc_cig_v qc_cig;
	int qc_meth;              /* also note what the base-averaged conversion table needs (bsx_qc_rec_t.meth ..), quality masks in qc_qm */
	bsx_qc_cig_v qc_qm;
	/* duplicate marking while aligning (md 0: off): the planning pass notes each end's primary record -- index of its region, -1: the unplaced
	 * stand-in, -2: none yet / no such end; md_dup: the template is a duplicate, the final pass writes 0x400 into every record */
	int md, md_dup;
	int md_pri[2];
} samctx_t;
/* is the per-record rule of `biscuit bsconv` on (any member besides annotate off its default)? */
int bsx_bsconv_filters(const bsx_bsconv_conf_t *c);

void bsx_reg2sam_se(const bsx_opt_t *opt, const bsx_index_t *idx, bsx_read_t *s, reg_v *regs, samctx_t *ctx, const char *rg_id);
void bsx_reg2sam_pe(const bsx_opt_t *opt, const bsx_index_t *idx, uint64_t id, bsx_read_t s[2], reg_v regs[2],
                    const bsx_pestat_t *pes, samctx_t *ctx, const char *rg_id);
/* K6 job for one region (band inference of mem_alnreg_setSAM) */
void bsx_setsam_job(const bsx_opt_t *opt, const bsx_index_t *idx, const bsx_read_t *s, uint32_t qoff, const reg_t *reg, bsx_glb_job_t *job);
/* finish a region's SAM record from the device CIGAR: MD/NM/ZC/ZR, D-squeezing, clipping, position */
void bsx_setsam_finish(const bsx_opt_t *opt, const bsx_index_t *idx, const bsx_read_t *s, const reg_t *reg,
                       const uint32_t *cg, int n_cigar, samrec_t *out, const bsx_glb_tag_t *tag, const char *tag_md);
/* the counts by cytosine context of both strand hypotheses over the same CIGAR, walked on the host: for a backend without
 * global_batch_tags_ctx (include/bsx.h has the rule) */
void bsx_setsam_ctx_host(const bsx_index_t *idx, const bsx_read_t *s, const reg_t *reg, const uint32_t *cg, int n_cigar, bsx_glb_ctx_t *out);

extern char bsx_rg_id[256];

#endif
