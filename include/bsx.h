/* bsx.h -- C ABI of the MI355X-native `biscuit align` hot path.
 *
 * The reference (zhou-lab/biscuit, lib/aln) has no plugin/FFI layer; its seams are plain C
 * functions.  Every entry point below replaces one of them (cited file:line under
 * /root/reference) with a batch form: plain pointers + sizes, int status (0 = ok, <0 = BSX_E_*)
 * instead of abort(), no globals.  The kernel-level calls run on the GPU (HIP, gfx950); there is
 * no CPU fallback inside the product library: without a usable HIP device every device call
 * returns BSX_E_NODEVICE.
 */
#ifndef BSX_H
#define BSX_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSX_EXPORT __attribute__((visibility("default")))

#define BSX_OK            0
#define BSX_E_NODEVICE  (-1)   /* no HIP device / HIP runtime error */
#define BSX_E_ARG       (-2)
#define BSX_E_IO        (-3)
#define BSX_E_NOMEM     (-4)
#define BSX_E_FORMAT    (-5)
#define BSX_E_INTERNAL  (-6)

/* ---- flags: identical values to MEM_F_* (lib/aln/bwamem.h:42-52) ---- */
#define BSX_F_PE             0x2
#define BSX_F_NOPAIRING      0x4
#define BSX_F_ALL            0x8
#define BSX_F_NO_MULTI       0x10
#define BSX_F_NO_RESCUE      0x20
#define BSX_F_SELF_OVLP      0x40
#define BSX_F_ALN_REG        0x80
#define BSX_F_REF_HDR        0x100
#define BSX_F_SOFTCLIP       0x200
#define BSX_F_SMARTPE        0x400
#define BSX_F_KEEP_SUPP_MAPQ 0x1000

/* ksw xtra flags (lib/aln/ksw.h:31-35) */
#define BSX_KSW_XBYTE  0x10000
#define BSX_KSW_XSTOP  0x20000
#define BSX_KSW_XSUBO  0x40000
#define BSX_KSW_XSTART 0x80000

/* Alignment options: field-for-field mem_opt_t (lib/aln/bwamem.h:54-124), same defaults
 * (mem_opt_init, lib/aln/bwamem.c:77-128). */
typedef struct bsx_opt {
	int a, b;
	int o_del, e_del;
	int o_ins, e_ins;
	int pen_unpaired;
	int pen_clip5, pen_clip3;
	int w;
	int zdrop;
	uint64_t max_mem_intv;
	int T;
	int flag;
	int min_seed_len;
	int min_chain_weight;
	uint32_t max_chain_extend;
	float split_factor;
	int split_width;
	uint32_t max_occ;
	int max_chain_gap;
	int n_threads;
	int chunk_size;
	float mask_level;
	float drop_ratio;
	float XA_drop_ratio;
	float mask_level_redun;
	float mapQ_coef_len;
	int mapQ_coef_fac;
	int max_ins;
	int max_matesw;
	int max_XA_hits, max_XA_hits_alt;
	int8_t mat[25];
	uint8_t parent;     /* -b */
	uint8_t bsstrand;   /* -f */
	int8_t ctmat[25];
	int8_t gamat[25];
	uint8_t *adaptor1; int l_adaptor1;
	uint8_t *adaptor2; int l_adaptor2;
	int clip5, clip3, min_base_qual;
	uint8_t has_bc;
} bsx_opt_t;

/* insert-size statistics: mem_pestat_t (lib/aln/bwamem.h:126-131) */
typedef struct bsx_pestat {
	int low, high;
	int set;
	int failed;
	double avg, std;
} bsx_pestat_t;

/* one read: the fields of bseq1_t (lib/aln/bwa.h:52-61) that mem_process_seqs reads/writes */
typedef struct bsx_read {
	int l_seq, id;
	char *name, *comment, *barcode, *umi, *qual, *sam;
	uint8_t *seq;        /* nt4 codes; advanced by clip5 after clipping */
	uint8_t *seq0;       /* start of the unclipped sequence (owner of the allocation) */
	int l_seq0;
	int l_adaptor;
	int clip5, clip3;
} bsx_read_t;

/* bi-interval: bwtintv_t (lib/aln/bwt.h:80-82) */
typedef struct bsx_intv {
	uint64_t x[3];
	uint64_t info;       /* beg<<32 | end */
} bsx_intv_t;

/* ------------------------------------------------------------------------------------------
 * Kernel-level batch jobs.  Sequences are never copied into jobs: a job names a *view*
 *   query view : chunk read buffer offset qoff, length qlen, walking direction qdir (+1/-1),
 *                optional complement (3-b for b<4)
 *   target view: reference coordinate tpos in the forward-reverse space [0, 2*l_pac)
 *                (bns_get_seq semantics, lib/aln/bntseq.c:402-422), length tlen, direction tdir
 * element i of a view is buf[qoff + i*qdir] resp. ref(tpos + i*tdir).
 * ------------------------------------------------------------------------------------------ */

/* one strand search: mem_collect_intv (lib/aln/memchain.c:50-106) for read x parent */
typedef struct bsx_seed_task {
	uint32_t qoff;       /* offset of the (clipped) read in the chunk read buffer */
	int32_t  len;
	int32_t  parent;     /* 1: C>T read vs parent index, 0: G>A read vs daughter index */
} bsx_seed_task_t;

/* suffix-array lookup: bwt_sa (lib/aln/bwt.c:87-97) */
typedef struct bsx_sa_job {
	uint64_t k;
	int32_t  parent;     /* which index */
	int32_t  pad;
} bsx_sa_job_t;

/* banded extension: ksw_extend2 (lib/aln/ksw.c:380-479) */
typedef struct bsx_ext_job {
	int64_t  tpos;
	uint32_t qoff;
	int32_t  qlen, tlen;
	int32_t  h0;
	int32_t  w;
	int32_t  end_bonus;
	int8_t   qdir, tdir;
	uint8_t  parent;     /* 1: ctmat, 0: gamat (lib/aln/memchain.c:654,713) */
	uint8_t  pad;
} bsx_ext_job_t;
typedef struct bsx_ext_res {
	int32_t score, qle, tle, gtle, gscore, max_off;
} bsx_ext_res_t;

/* One alignment region as mem_chain2region leaves it (the fields of mem_alnreg_t, lib/aln/mem_alnreg.h:34-66,
 * that lib/aln/memchain.c:822-869 sets; everything else is zero at that point). */
typedef struct bsx_region {
	int64_t rb, re;
	int32_t qb, qe, rid, score, truesc, w, seedcov, seedlen0;
	float   frac_rep;
	uint8_t bss, parent, pad[2];
} bsx_region_t;

/* local SW with 2nd-best + start recovery: ksw_align2 (lib/aln/ksw.c:343-365) */
typedef struct bsx_sw_job {
	int64_t  tpos;
	uint32_t qoff;
	int32_t  qlen, tlen;
	int32_t  xtra;
	int8_t   qdir, tdir;
	uint8_t  qcomp;      /* complement the query view (mate rescue, lib/aln/mem_alnreg.c:411) */
	uint8_t  use_ct;     /* 1: ctmat, 0: gamat */
} bsx_sw_job_t;
typedef struct bsx_sw_res {   /* kswr_t, lib/aln/ksw.h:37-43 */
	int32_t score, te, qe, score2, te2, tb, qb;
} bsx_sw_res_t;

/* banded global alignment + traceback with the band-doubling loop of mem_alnreg_setSAM
 * (lib/aln/mem_alnreg_format.c:63-77) and band set-up of bis_bwa_gen_cigar2
 * (lib/aln/bwa.c:314-340) folded in.  n_try==1 && !want_cigar is the score-only call made by
 * mem_test_reg_concatenation (lib/aln/mem_alnreg.c:92). */
typedef struct bsx_glb_job {
	int64_t  tpos;
	uint32_t qoff;
	int32_t  qlen, tlen;
	int32_t  w0;          /* first band passed as w_ */
	int32_t  w_max;       /* opt->w<<2 cap applied before each try */
	int32_t  truesc;      /* stop when score >= truesc - a */
	int32_t  n_try;       /* 3 for setSAM, 1 for the concatenation test */
	uint32_t cigar_off;   /* where this job's CIGAR goes in the output pool (u32 units) */
	uint32_t cigar_cap;
	int8_t   qdir, tdir;
	uint8_t  use_ct;
	uint8_t  want_cigar;
} bsx_glb_job_t;
typedef struct bsx_glb_res {
	int32_t score;
	int32_t n_cigar;      /* <0: cigar_cap too small, -n_cigar needed */
	int32_t w_used;
	int32_t pad;
} bsx_glb_res_t;

/* ------------------------------------------------------------------------------------------
 * Index (host side): <base>.{par,dau}.{bwt,sa}, <base>.bis.{ann,amb,pac}[, <base>.alt]
 * replaces bwa_idx_load_from_disk (lib/aln/bwa.c:525-554)
 * ------------------------------------------------------------------------------------------ */
typedef struct bsx_index bsx_index_t;
int  bsx_index_load(const char *base, bsx_index_t **out);
void bsx_index_free(bsx_index_t *idx);
/* builds all seven files from a FASTA: main_biscuit_index (lib/aln/bwtindex.c:206-347); host suffix sorter, genomes up
 * to 1.07 Gbp (2 x l_pac < 2^31).  In steps: bsx_index_from_fasta (bis_bns_fasta2bntseq, lib/aln/bntseq.c:542-633: pac +
 * annotation), then the two FM indices on the host (bsx_index_build_host) or, for genomes of any size, on the device
 * (bsx_device_build_index below: what bwt_bwtgen, lib/aln/bwt_gen.c:1595-1607, is for in the reference), then bsx_index_save. */
int  bsx_index_build(const char *fasta, const char *base);
int  bsx_index_from_fasta(const char *fasta, bsx_index_t **out);
int  bsx_index_build_host(bsx_index_t *idx);
int  bsx_index_save(const bsx_index_t *idx, const char *base);
int64_t bsx_index_l_pac(const bsx_index_t *idx);
int  bsx_index_n_seqs(const bsx_index_t *idx);
const uint8_t *bsx_index_pac(const bsx_index_t *idx);    /* 2 bits per base, the .bis.pac layout */
int  bsx_index_contig(const bsx_index_t *idx, int i, const char **name, int64_t *offset, int64_t *len);

/* options: mem_opt_init (lib/aln/bwamem.c:77-128) + the three matrices (lib/aln/bwa.c:146-182) */
void bsx_opt_init(bsx_opt_t *opt);
void bsx_opt_fill_matrices(bsx_opt_t *opt);

/* ------------------------------------------------------------------------------------------
 * Device (HIP) side
 * ------------------------------------------------------------------------------------------ */
typedef struct bsx_device bsx_device_t;
/* open HIP device `ordinal`, create streams; BSX_E_NODEVICE if none */
int  bsx_device_open(int ordinal, bsx_device_t **out);
void bsx_device_close(bsx_device_t *dev);
/* copy both FM indices, SA samples and pac into HBM (resident for the life of dev) */
int  bsx_device_upload_index(bsx_device_t *dev, const bsx_index_t *idx);
/* Build both FM indices (BWT with occurrence blocks + suffix-array samples) of idx's genome on the device, from its pac,
 * and leave them resident exactly as bsx_device_upload_index would: 64-bit suffix sorting in HBM, hg38-sized genomes
 * included (bwt_bwtgen + bwt_bwtupdate_core + bwt_cal_sa, lib/aln/bwtindex.c:258-340).  fill_host != 0 also copies the
 * file-format arrays into idx (for bsx_index_save and for host-side consumers); they are byte-identical to the host
 * builder's and the reference's. */
int  bsx_device_build_index(bsx_device_t *dev, bsx_index_t *idx, int fill_host);
/* copy scoring matrices / penalties used by the DP kernels */
int  bsx_device_set_opt(bsx_device_t *dev, const bsx_opt_t *opt);
/* upload the chunk read buffer (nt4 codes of all clipped reads, concatenated) */
int  bsx_device_set_reads(bsx_device_t *dev, const uint8_t *buf, size_t n);
const char *bsx_device_name(const bsx_device_t *dev);
/* compute units of the device: the grids of the persistent kernels are multiples of it (0 for a null dev) */
int bsx_device_n_cu(const bsx_device_t *dev);

/* K1+K2: all three seeding passes of mem_collect_intv + final ordering by info.
 * out_off has n+1 entries; *out / *out_cap is a caller-owned growable array (realloc'd). */
int bsx_seed_batch(bsx_device_t *dev, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks,
                   bsx_intv_t **out, int64_t *out_cap, int64_t *out_off);
/* K3 */
int bsx_sa_batch(bsx_device_t *dev, int64_t n, const bsx_sa_job_t *jobs, uint64_t *pos);
/* K4 */
int bsx_extend_batch(bsx_device_t *dev, int64_t n, const bsx_ext_job_t *jobs, bsx_ext_res_t *res);
/* K1+K2+K3 and the chaining/extension logic between them in one pass (mem_chain + mem_chain_flt +
 * mem_chain2region, lib/aln/memchain.c:268-488,742-904; called per strand search from lib/aln/bwamem.c:352-372):
 * regions of task i = (*out)[out_off[i] .. out_off[i] + out_n[i]).  out_n[i] < 0 means the device declined the task
 * (a read too long for its on-chip rows, an over-represented interval that has to be walked past max_occ, more
 * occurrences/chains/regions than its tables hold): the caller runs that task through bsx_sa_batch/bsx_extend_batch and its own chaining instead.  For those
 * tasks the sorted SA intervals are handed back so that they need not be seeded again: the j-th declined task with
 * out_n != -1 (in task order) has (*decl_intv)[decl_off[j] .. decl_off[j+1]); out_n == -1 means its interval list
 * overflowed as well and bsx_seed_batch has to redo it.  decl_off must have room for n + 1 entries. */
int bsx_regions_batch(bsx_device_t *dev, const bsx_opt_t *opt, int64_t n, const bsx_seed_task_t *tasks,
                      bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n,
                      bsx_intv_t **decl_intv, int64_t *decl_cap, int64_t *decl_off);
/* out_n[i] == BSX_REGIONS_PENDING: the strand search overflowed the seeding lists (a read inside a tandem repeat) and is
 * being seeded again with much longer lists while the call returns; bsx_regions_finish waits for those, appends their
 * regions to *out and fills out_off/out_n in (-1: seed and chain it on the host).  Same arrays as the batch call. */
#define BSX_REGIONS_PENDING (-100)
int bsx_regions_finish(bsx_device_t *dev, bsx_region_t **out, int64_t *out_cap, int64_t *out_off, int32_t *out_n);
/* C5 for the regions the last bsx_regions_batch left on the device: mem_sort_deduplicate (lib/aln/mem_alnreg.c:112-202) of every
 * read, a read's regions being those of its per_read consecutive strand searches concatenated in call order
 * (lib/aln/bwamem.c:352-372).  out_n[i] >= 0: the read keeps that many regions, out_idx[i * bsx_regions_dedup_cap() + k]
 * naming the k-th by its index in the concatenation; out_n[i] == -1: left to the caller (a strand search of the read was
 * not finished on the device, too many regions, or two regions have to be tested for concatenation, mem_alnreg.c:63-108). */
int bsx_regions_dedup_cap(void);
int bsx_regions_dedup(bsx_device_t *dev, const bsx_opt_t *opt, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx);
/* ... and the reads with MORE regions than that, up to bsx_regions_dedup_long_cap() (a wavefront per read, k_dedup_long): as above, and for
 * such a read long_off[i] >= 0 says where its out_n[i] indices (16 bits each) start in *long_idx (a malloc'd array the call grows:
 * *long_cap entries); long_off[i] == -1: the read's list, if it has one, is in out_idx. */
int bsx_regions_dedup_long_cap(void);
int bsx_regions_dedup2(bsx_device_t *dev, const bsx_opt_t *opt, int64_t n_reads, int per_read, int32_t *out_n, uint8_t *out_idx,
                       int64_t *long_off, uint16_t **long_idx, int64_t *long_cap);
/* K5 */
int bsx_sw_batch(bsx_device_t *dev, int64_t n, const bsx_sw_job_t *jobs, bsx_sw_res_t *res);
/* K6 */
int bsx_global_batch(bsx_device_t *dev, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res,
                     uint32_t *cigar_pool, size_t cigar_pool_len);
/* K6 with the second half of bis_bwa_gen_cigar2 (lib/aln/bwa.c:342-418) done on the device as well: NM, the MD string
 * and BISCUIT's conversion / retention counts of every job that has a CIGAR, walked over the job's own (possibly
 * reversed) sequences.  tags[i].l_md < 0: job i has no CIGAR yet (res[i].n_cigar <= 0).  The MD strings (NUL-terminated)
 * are packed into *md, a buffer the library grows with realloc as bsx_seed_batch grows *out. */
typedef struct bsx_glb_tag {
	int32_t  NM, ZC, ZR;
	int32_t  l_md;        /* strlen of the MD string */
	uint64_t md_off;      /* where it starts in *md */
	uint8_t  bss_u;       /* no conversion seen (bwa.c:415-416) */
	uint8_t  pad[7];
} bsx_glb_tag_t;
int bsx_global_batch_tags(bsx_device_t *dev, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res,
                          uint32_t *cigar_pool, size_t cigar_pool_len, bsx_glb_tag_t *tags, char **md, int64_t *md_cap);
/* ... and, from the same walk, what `biscuit bsconv` (src/bsconv.c:63-109) counts over the alignment: cytosine retention / conversion by
 * the next base, for BOTH bisulfite-strand hypotheses (the strand of a record follows from YD, which depends on the mate: the host picks).
 * Everything is in forward-genome terms whatever the job's view: s[0] = columns whose reference base is C, bucket = the reference base after
 * it, retained = read C, converted = read T; s[1] = columns whose reference base is G, bucket = the complement of the reference base before
 * it, retained = read G, converted = read A.  Bucket 4 ("N"): the neighbour lies outside the contig or in an N hole of the reference
 * (.bis.amb).  A column whose own reference base lies in a hole is counted nowhere (ZC / ZR use the randomised base of pac there).  The
 * counters saturate at 65535.  A job's target window lies on one strand: tpos >= l_pac means a complemented view.  ctx[i] of a job without
 * a CIGAR is all zero. */
typedef struct bsx_glb_ctx {
	uint16_t n[2][5][2];   /* [strand hypothesis][A, C, G, T, N context][retained, converted] */
} bsx_glb_ctx_t;
int bsx_global_batch_tags_ctx(bsx_device_t *dev, int64_t n, const bsx_glb_job_t *jobs, bsx_glb_res_t *res,
                              uint32_t *cigar_pool, size_t cigar_pool_len, bsx_glb_tag_t *tags, char **md, int64_t *md_cap, bsx_glb_ctx_t *ctx);

/* BISCUITqc counts over written records (k_qc.hip): what `biscuit qc` (src/qc.c:112-179) has bsstrand_func, cinread_func (targets CG and CH) and
 * bsconv_func count column by column, one job per mapped record, accumulated in a table that stays on the device.
 * A job is the record as the SAM has it: fpos = forward coordinate (concatenated contigs) of the first aligned column; the read as it lies in the
 * resident read buffer (bsx_device_set_reads), in sequencing orientation: its first stored base at roff, rskip bases of the whole read before the
 * stored ones (bases clipped off before alignment), rlen = the whole read's length; the record's final CIGAR, S and H included, in reference order,
 * n_cigar words (len << 4 | op, op 0..4 = MIDSH) at cig_off of the pool.  A reverse record reads the complement of the read from its far end.
 * Read positions are in whole-read coordinates (S and H both advance them): 0-based from the read's first base on a forward record, rlen - qpos
 * on a reverse one; positions >= 301 are not counted.  Reference columns in an N hole count nowhere; a neighbour in a hole or beyond the contig
 * end is "not G". */
#define BSX_QC_REVERSE  0x1    /* flag 0x10 */
#define BSX_QC_READ2    0x2    /* flag 0x80 */
#define BSX_QC_TAG(f)   (((f) >> 2) & 3)   /* YD: 0 = f, 1 = r, 3 = u */
#define BSX_QC_STRAND   0x10   /* count confusion[tag * 4 + inferred] (bsstrand.c:115-135; inferred: 0 f, 1 r, 2 conflict, 3 unknown) */
#define BSX_QC_CINREAD  0x20   /* count both read-position tables (MAPQ >= 40, not secondary) */
#define BSX_QC_BSCONV   0x40   /* count the eight conversion totals (not secondary, paired, proper, MAPQ >= 40) */
#define BSX_QC_READ_LEN 301
typedef struct bsx_qc_job {
	int64_t fpos;
	uint32_t roff;
	int32_t rskip;
	uint32_t rlen;
	uint32_t cig_off, n_cigar;
	uint32_t flags;
} bsx_qc_job_t;
typedef struct bsx_qc_counts {   /* the device's table, one POD */
	uint64_t readpos[2][2][BSX_QC_READ_LEN][2];   /* [CpG, CpH][read 1, read 2][position][converted, retained] */
	uint64_t conv[8];                             /* CpA retained, CpA converted, CpC .., CpG .., CpT .. (bsconv's retn_conv_counts) */
	uint64_t confusion[16];                       /* [YD tag * 4 + inferred] */
} bsx_qc_counts_t;
/* adds the jobs' counts to the device's table (exact integer sums: the order of jobs and the split into batches do not matter) */
int bsx_qc_batch(bsx_device_t *dev, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len);
/* waits for the batches in flight and copies the table out; reset != 0 zeroes it */
int bsx_qc_read(bsx_device_t *dev, bsx_qc_counts_t *out, int reset);

/* BISCUITqc coverage tables (k_cov.hip): the depth of every reference position under the records written, kept on the device as a difference
 * array over forward concatenated coordinates (l_pac + 1 entries of two signed 32-bit classes: every record, and records with MAPQ >= 40), and
 * the twelve depth distributions scripts/QC.sh:136-421 derives from `bedtools genomecov -bga -split` and a CpG list.  The jobs are
 * bsx_qc_job_t's: a job with BSX_QC_COV adds 1 to every column under an M run of its CIGAR (D, I, S and H cover nothing) in class `all`, and in
 * class `q40` too when it has BSX_QC_COV_Q40; a job without BSX_QC_COV adds nothing.  k_qc ignores both bits.  The state is made (8 bytes per
 * base, zeroed) by the first call that needs it and freed by bsx_cov_reset and bsx_device_close; BSX_E_NOMEM when it cannot be had. */
#define BSX_QC_COV      0x80
#define BSX_QC_COV_Q40  0x100
#define BSX_COV_TILE    4096   /* positions a workgroup scans at a time in the final passes (k_cov.hip) */
#define BSX_COV_N_TABLES 12
#define BSX_COV_MASK_TOPGC 0
#define BSX_COV_MASK_BOTGC 1
/* table (region * 4 + class * 2 + kind): region 0 = the whole genome, 1 = the top-GC mask, 2 = the bottom-GC mask; class 0 = all, 1 = q40;
 * kind 0 = bases, 1 = CpGs -- the order in which QC.sh writes the rows of its uniformity table.  count[d] = positions (CpGs) of depth d,
 * n_bins = the largest `all` depth + 1 for every table there is; without both masks have_gc = 0 and tables 4..11 are empty (n_bins 0, count
 * NULL).  A CpG is a forward C at i and G at i + 1 in one contig, neither in an N hole; its depth is min(depth[i], depth[i + 1]); it lies in
 * a mask when either of its bases does. */
typedef struct bsx_cov_table { uint64_t n_bins; uint64_t *count; } bsx_cov_table_t;
typedef struct bsx_cov_tables { bsx_cov_table_t t[BSX_COV_N_TABLES]; int have_gc; } bsx_cov_tables_t;
/* every job must lie inside the genome and the pool (fpos >= 0, fpos + reference length <= l_pac, cig_off + n_cigar <= cigar_pool_len):
 * BSX_E_ARG otherwise, and nothing is launched.  Exact integer sums: the order of jobs and the split into batches do not matter. */
int bsx_cov_batch(bsx_device_t *dev, int64_t n, const bsx_qc_job_t *jobs, const uint32_t *cigar_pool, size_t cigar_pool_len);
/* mask `which` (BSX_COV_MASK_*) = the union of n_intervals half-open intervals beg_end[2 i], beg_end[2 i + 1] of forward coordinates
 * (0 <= beg <= end <= l_pac; they may overlap); it replaces the mask there was; n_intervals = 0 makes an empty mask */
int bsx_cov_set_mask(bsx_device_t *dev, int which, int64_t n_intervals, const int64_t *beg_end);
/* waits for the batches in flight and makes the tables; the depth state is only read: tables can be read again and more batches can follow.
 * The arrays belong to the caller (bsx_cov_tables_free). */
int bsx_cov_tables(bsx_device_t *dev, bsx_cov_tables_t *out);
void bsx_cov_tables_free(bsx_cov_tables_t *t);
int bsx_cov_reset(bsx_device_t *dev);   /* the depth state and both masks freed: all-zero depth, no masks (it waits for a batch or a tables call in flight) */

/* BISCUITqc base-averaged conversion table (k_meth.hip): what `biscuit pileup`, `biscuit vcf2bed -e -t c` and the awk of scripts/QC.sh:423-450
 * make of a sorted BAM at their defaults, from four counters per forward reference position that stay on the device: ret, conv, opp_ref,
 * opp_alt, 32 bits each, held as two 64-bit words (ret | conv << 32, opp_ref | opp_alt << 32) so that a column is one 64-bit atomic add.
 * A job is a record that counts (the caller has applied the record filters), described as a bsx_qc_job_t describes it -- fpos, the read in the
 * resident read buffer (roff, rskip, rlen), the final CIGAR at cig_off of the pool, flags BSX_QC_REVERSE, BSX_QC_READ2 and the YD tag at
 * BSX_QC_TAG -- plus: qm_off, the word offset in the same pool of the record's quality mask, (rlen + 31) / 32 words, bit (q & 31) of word
 * q >> 5 set when the base at 0-based position q of the whole read in the record's orientation has quality >= 20 (all ones for a read without
 * qualities); and [ov_beg, ov_end), the forward interval whose columns a BSX_QC_READ2 job leaves to its mate (empty otherwise).
 * The strand is 0 for tag 0, 1 for tag 1, else inferred over the M columns with the mask bit set: 0 when ref C / read T columns are at least
 * as many as ref G / read A columns, else 1.  A column counts when its mask bit is set, 3 < q1 and q1 + 3 <= rlen (q1 = q + 1; H advances q
 * like S), its reference base is no N hole and, for BSX_QC_READ2, it lies outside the interval.  At a reference C: strand 0 read C -> ret,
 * read T -> conv, strand 1 read C -> opp_ref, read T -> opp_alt; at a reference G: strand 1 read G -> ret, read A -> conv, strand 0 read G ->
 * opp_ref, read A -> opp_alt.  The state (16 bytes per base, zeroed) is made by the first call that needs it and freed by bsx_meth_reset and
 * bsx_device_close; BSX_E_NOMEM when it cannot be had. */
typedef struct bsx_meth_job {
	int64_t fpos;
	uint32_t roff;
	int32_t rskip;
	uint32_t rlen;
	uint32_t cig_off, n_cigar;
	uint32_t flags;
	uint32_t qm_off;
	uint32_t pad;
	int64_t ov_beg, ov_end;
} bsx_meth_job_t;
#define BSX_METH_N_CTX 5   /* CA, CC, CG, CT, and CN: the neighbour is an N hole or beyond the contig */
/* per context: k = reported sites (a reference C or G outside N holes with ret + conv > 0 that is callable: opp_alt == 0 or 20 * opp_alt <
 * ret + opp_ref), s = the sum over them of the beta in thousandths, the integer printf("%1.3f", (double)ret / (double)(ret + conv)) shows */
typedef struct bsx_meth_tables { uint64_t k[BSX_METH_N_CTX], s[BSX_METH_N_CTX]; } bsx_meth_tables_t;
/* every job must lie inside the genome and the pool (fpos >= 0, fpos + reference length <= l_pac, cig_off + n_cigar <= pool_len, qm_off +
 * (rlen + 31) / 32 <= pool_len): BSX_E_ARG otherwise, and nothing is launched.  The reads are those of bsx_device_set_reads.  Exact integer
 * sums: the order of jobs and the split into batches do not matter. */
int bsx_meth_batch(bsx_device_t *dev, int64_t n, const bsx_meth_job_t *jobs, const uint32_t *pool, size_t pool_len);
/* the four counters of the positions [fpos, fpos + n) into out[4 * i + (0 ret, 1 conv, 2 opp_ref, 3 opp_alt)]; waits for the batches in flight */
int bsx_meth_read(bsx_device_t *dev, int64_t fpos, int64_t n, uint32_t *out);
/* waits for the batches in flight and makes the sums; the state is only read */
int bsx_meth_tables(bsx_device_t *dev, bsx_meth_tables_t *out);
int bsx_meth_reset(bsx_device_t *dev);   /* the state freed: every counter zero */

/* The methylation sites of the same state (k_msite.hip): what `biscuit pileup` -> `biscuit vcf2bed -t TYPE -k K` lists, or with `merge` what
 * `biscuit mergecg` makes of that list, as fixed-size records in ascending forward position.  A site is a site of bsx_meth_tables.  Its class is
 * pileup's CX (bisc_utils.c:33-72) over the five bases f - 2 .. f + 2 read on the cytosine's own strand: CN when one of them is in an N hole or
 * not a base of the site's contig, else CG when the next base is G, else CHG when the one after it is G, else CHH.  type BSX_METH_TYPE_CG keeps
 * class CG, _CH keeps CHG and CHH, _C keeps every class; then a site is kept when ret + conv >= min_cov (>= 1).  Without merge a record is one
 * kept site: fpos its position, the C side filled at a reference C, the G side at a reference G.  With merge (type CG only: BSX_E_ARG otherwise)
 * a kept G at f + 1 is joined to a kept C at f: that record has fpos = f and both sides; a C alone has fpos = f and the C side, a G alone
 * fpos = its own position and the G side.  A record belongs to the position fpos. */
#define BSX_METH_TYPE_CG 0
#define BSX_METH_TYPE_CH 1
#define BSX_METH_TYPE_C  2
#define BSX_METH_CLS_CG  0
#define BSX_METH_CLS_CHG 1
#define BSX_METH_CLS_CHH 2
#define BSX_METH_CLS_CN  3
#define BSX_METH_SITE_C  4u   /* flags: the class in the two low bits (of the C where there is one, else of the G), the sides that are present */
#define BSX_METH_SITE_G  8u
typedef struct bsx_meth_site_opt { int32_t type, merge; uint32_t min_cov, pad; } bsx_meth_site_opt_t;
typedef struct bsx_meth_site {
	int64_t fpos;
	uint32_t ret_c, n_c;   /* retained and ret + conv of the C side, zero when it is absent */
	uint32_t ret_g, n_g;   /* of the G side */
	uint32_t flags;
	uint32_t pad;
} bsx_meth_site_t;
/* the records that belong to [f_lo, f_hi), 0 <= f_lo <= f_hi <= l_pac, taken tile by tile (BSX_COV_TILE positions, tiles start at multiples of
 * it): out gets the records of as many whole tiles from f_lo on as fit cap records, *n their number, *f_next the start of the first tile left
 * out, or f_hi when none is: the caller goes on from there.  cap < BSX_COV_TILE (a tile may hold that many) is BSX_E_ARG and writes nothing.
 * It waits for the batches in flight; the state is only read; without a state there is no record. */
int bsx_meth_sites(bsx_device_t *dev, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n,
                   int64_t *f_next);

/* Duplicate templates (k_markdup.hip): a table of template keys that stays on the device until bsx_markdup_reset or bsx_device_close.
 * A key is the ordered pair of the template's ends, w[0] = read 1 (or the single read), w[1] = read 2; an end that is not placed (its primary
 * record has 0x4) is 0, the second end of a single read is BSX_MD_SINGLE: a single read never equals a pair, not even one whose read 2 is not
 * placed.  A placed end is BSX_MD_END(contig, u5, reverse, yd):
 *   bit 63      placed
 *   bit 62      0x10 of the end's primary record
 *   bit 61      1 when the record's YD tag is r (f and u: 0)
 *   bits 33-60  index of the contig (below 2^28)
 *   bits 0-32   u5 + BSX_MD_U5_BIAS, u5 = the unclipped 5' coordinate, 1-based like POS: POS - (leading S + leading H) on a forward record,
 *               POS + reflen - 1 + (trailing S + trailing H) on a reverse one (reflen: the M, D, N, =, X operations); it may be 0, negative
 *               or beyond the contig's end
 * The key with both words all ones means "no placed end": bsx_markdup_batch skips it and it never enters the table. */
typedef struct bsx_markdup_key { uint64_t w[2]; } bsx_markdup_key_t;
#define BSX_MD_PLACED   (1ull << 63)
#define BSX_MD_REVERSE  (1ull << 62)
#define BSX_MD_YD       (1ull << 61)
#define BSX_MD_U5_BIAS  ((int64_t)1 << 32)
#define BSX_MD_SINGLE   1ull
#define BSX_MD_END(contig, u5, reverse, yd) (BSX_MD_PLACED | ((reverse) ? BSX_MD_REVERSE : 0) | ((yd) ? BSX_MD_YD : 0) | \
	((uint64_t)(contig) & 0xfffffffull) << 33 | ((uint64_t)((int64_t)(u5) + BSX_MD_U5_BIAS) & 0x1ffffffffull))
/* keys[i] is the template with ordinal first_ordinal + i.  dup_out[i] = 1 when an equal key (all 128 bits) with a lower ordinal is in the
 * table or earlier in this batch, else 0 (also for a skipped key); within a batch the lowest ordinal is the one that stays unmarked however
 * the lanes interleave, between batches the order is the caller's: ordinals must not decrease from one batch to the next.  The table grows
 * (twice the slots, every slot moved by k_md_rehash) before a batch would load it beyond one half; BSX_E_NOMEM when the larger table cannot
 * be had, with the size in the message.  The table in use is kept; keys the batch inserted before it failed (in an earlier salt round) stay
 * in it, so the batch is lost and so is the run's marking: reset before marking again.  "markdup_slots" (bsx_tune_set) is the first table's
 * capacity (a power of two; default: 32 slots per key of the first batch, at least 65536).  The claim word of a key is bsx_markdup_hash(key,
 * salt, bits): salt 0 first; a key that meets another key with its claim word tries salt + 1, eight salts at most (BSX_E_INTERNAL beyond);
 * "markdup_hash_bits" (default 64) keeps only the low bits of the claim word, so that tests can make such meetings happen. */
int bsx_markdup_batch(bsx_device_t *dev, int64_t n, const bsx_markdup_key_t *keys, uint64_t first_ordinal, uint8_t *dup_out);
int bsx_markdup_reset(bsx_device_t *dev);   /* an empty table of the initial capacity */
/* For tests and diagnostics, not part of the marking seam: slots of the device's table and how many are taken (0, 0 before the first batch);
 * the claim word of a key (csrc/host/markdup_hash.h). */
int bsx_markdup_table_info(bsx_device_t *dev, uint64_t *n_slots, uint64_t *n_used);
uint64_t bsx_markdup_hash(const bsx_markdup_key_t *key, uint32_t salt, int bits);

/* Coordinate order (k_sort.hip): a stable radix sort of 64-bit keys on the device, and the keys of every sorted run kept there until
 * bsx_sort_reset or bsx_device_close.  A record's key is BSX_SORT_KEY(rank, POS, FLAG & 0x10): rank = the 0-based index of its RNAME among the
 * @SQ lines of the header as written, 0xffffffff for RNAME '*'; POS below 2^31.
 * bsx_sort_run: perm_out[i] = the index, in this call's keys, of the i-th key in stable order (equal keys in input order); the sorted keys stay
 * on the device as the next run (runs number from 0).  n == 0 adds no run; n of 2^31 or more is BSX_E_ARG.
 * bsx_sort_schedule: the stable sort of all retained keys taken as the concatenation of the runs in run order, as the run every output position
 * comes from: (*run_of)[i] for i < *n_total, malloc'd, the caller frees it (NULL when there is no key).  Equal keys come from the lower run
 * first, and within a run in its order: following run_of with one cursor per run merges the runs.  The runs stay as they are.
 * Device memory that cannot be had is BSX_E_NOMEM; nothing is ever sorted on the host by these calls.  BSX_SORT_TILE: the keys of one
 * workgroup; up to that many are sorted by a single workgroup in LDS, more by tiled passes over HBM. */
#define BSX_SORT_TILE 2048
#define BSX_SORT_KEY(rank, pos, rev)  ((uint64_t)(rank) << 32 | (uint64_t)(pos) << 1 | ((rev) != 0))   /* RNAME '*': rank 0xffffffff */
int bsx_sort_run(bsx_device_t *dev, int64_t n, const uint64_t *keys, uint32_t *perm_out);
int bsx_sort_schedule(bsx_device_t *dev, int64_t *n_total, uint32_t **run_of);   /* caller frees */
int bsx_sort_info(bsx_device_t *dev, uint64_t *n_runs, uint64_t *n_keys);
int bsx_sort_reset(bsx_device_t *dev);

/* Coordinate-sorted SAM (--sort; csrc/host/sortout.c).  The sorter takes the SAM body chunk by chunk (whole lines), gets each chunk's order
 * from the device (bsx_sort_run; dev == NULL: the host's own stable merge sort, same result), appends the chunk's lines in that order to one
 * temporary file in tmp_dir (NULL: /tmp; made with mkstemp and unlinked at once) and, at the end, follows bsx_sort_schedule through
 * one pread cursor per run: the host never compares two records.  header: the header text as written (its @SQ lines give the ranks).
 * bsx_sorter_finish hands the sorted body to `sink` in pieces of whole lines (a non-zero return stops it: BSX_E_IO).  "sort_buf_bytes"
 * (bsx_tune_set): the read buffer of every run; a record longer than the buffer still works.  A failed write to the temporary file is
 * BSX_E_IO from bsx_sorter_add and from everything after it.  bsx_sorter_dir_ok: BSX_OK when a temporary file can be made in the directory.
 * bsx_sort_header: the header of a sorted file, malloc'd -- "@HD\tVN:1.6\tSO:coordinate" first when the text has no @HD line, else its @HD line
 * moved to the front with SO:coordinate set (or appended); every other line as it is. */
typedef struct bsx_sorter bsx_sorter_t;
int  bsx_sorter_dir_ok(const char *tmp_dir);
int  bsx_sorter_open(bsx_device_t *dev, const char *header, const char *tmp_dir, bsx_sorter_t **out);
int  bsx_sorter_add(bsx_sorter_t *s, const char *text, size_t len);
int  bsx_sorter_finish(bsx_sorter_t *s, int (*sink)(void *ud, const char *text, size_t len), void *ud);
void bsx_sorter_counts(const bsx_sorter_t *s, uint64_t *n_runs, uint64_t *n_records);
void bsx_sorter_close(bsx_sorter_t *s);
char *bsx_sort_header(const char *header);

/* BAM output (--bam; k_bam.hip, k_bgzf.hip, csrc/host/bam.c).  DESIGN.md section 7 has the rule, tests/bam_model.py is its reference statement.
 * Two batch seams, each a pure function of its input:
 *   bsx_bam_encode    SAM text (whole lines, each ending in '\n') -> the uncompressed BAM records, one per line, in order.  refs: the name table
 *                     of the header the records belong to (bsx_bam_refs_open: one reference per @SQ line of the text, from SN and LN; RNAME is
 *                     the index of the first line with that name).  A line BAM or this encoder cannot hold stops the call: *bad_record = its
 *                     0-based index in the text, *bad_why = BSX_BAM_E_*, the records before it are returned, the return value is BSX_OK
 *                     (*bad_record = -1 when every line was taken).  *n_records: the records returned.
 *   bsx_bgzf_deflate  payload -> BGZF blocks behind each other, one per BSX_BGZF_BLOCK payload bytes (the last one shorter): the gzip member
 *                     header with the BC field, a deflate stream (LZ77 + dynamic Huffman codes on the device; one stored block where that is
 *                     no smaller: n + 31 bytes), CRC32, ISIZE.  The same payload gives the same bytes on every call.  len 0 gives nothing.  The
 *                     compressed bytes are the coder's own: the device's and the host's (zlib level 1) differ, both inflate to the payload.
 * Both write into a caller-owned growable buffer (*out / *out_cap, realloc'd by the call) from its start and set *out_len.  dev == NULL: the
 * host's own statement of the stage (what a backend without the seam runs).
 * The writer: bsx_bam_writer_open takes the header text as written, _add whole lines, _close(finish != 0) the last partial block and the 28-byte
 * EOF block.  The header part ends its block; the record stream is cut every BSX_BGZF_BLOCK bytes counted from the first record across calls
 * (the writer carries the tail), so the file is a function of the header and the record sequence alone.  It works in pieces of at most
 * "bam_piece_bytes" (bsx_tune_set) of text, whole lines.  The sink gets the header's block (is_header = 1) with the first data it is called
 * with -- a run whose first piece is refused has written nothing -- and then runs of whole blocks; a non-zero return from it is BSX_E_IO from
 * the call and from every later one.  A refused line: BSX_E_FORMAT, nothing of its piece or after it reaches the sink, bsx_bam_writer_refused
 * says which record of the whole stream (0-based) and why. */
#define BSX_BGZF_BLOCK   0xff00
#define BSX_BAM_E_LINE   1   /* not a SAM record: fewer than 11 columns, an empty column, a number that is none or out of its field's range */
#define BSX_BAM_E_TAG    2   /* a field after column 11 that is not XX:T:value with T in A i Z f (H and B included) */
#define BSX_BAM_E_INT    3   /* an i value outside -2^31 .. 2^32 - 1 */
#define BSX_BAM_E_NAME   4   /* a read name longer than 254 bytes */
#define BSX_BAM_E_CIGAR  5   /* more than 65535 CIGAR operations */
#define BSX_BAM_E_REF    6   /* an RNAME or RNEXT without an @SQ line */
#define BSX_BAM_E_QUAL   7   /* SEQ and QUAL of different lengths */
typedef struct bsx_bam_refs bsx_bam_refs_t;
typedef struct bsx_bam_writer bsx_bam_writer_t;
typedef int (*bsx_bam_sink_fn)(void *ud, const void *data, size_t len, int is_header);
int  bsx_bam_refs_open(const char *header_text, bsx_bam_refs_t **out);
void bsx_bam_refs_close(bsx_bam_refs_t *refs);
int  bsx_bam_header(const char *header_text, uint8_t **out, size_t *out_len);   /* the header part of the payload, malloc'd */
const char *bsx_bam_strerror(int why);
int  bsx_bam_encode(bsx_device_t *dev, const bsx_bam_refs_t *refs, const char *text, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len,
                    int64_t *n_records, int64_t *bad_record, int *bad_why);
int  bsx_bgzf_deflate(bsx_device_t *dev, const uint8_t *payload, size_t len, uint8_t **out, size_t *out_cap, size_t *out_len);
int  bsx_bam_writer_open(bsx_device_t *dev, const char *header_text, bsx_bam_sink_fn sink, void *ud, bsx_bam_writer_t **out);
int  bsx_bam_writer_add(bsx_bam_writer_t *w, const char *text, size_t len);
int  bsx_bam_writer_close(bsx_bam_writer_t *w, int finish);   /* frees the writer; finish = 0 after an error: nothing more is written */
void bsx_bam_writer_refused(const bsx_bam_writer_t *w, int64_t *record, int *why);
void bsx_bam_writer_counts(const bsx_bam_writer_t *w, uint64_t *n_records, uint64_t *payload_bytes, uint64_t *bytes_written);

/* Settings of the library that never change its output (launch shapes, table sizes, which of two equivalent paths runs: what the tests and
 * the A/B tools switch).  One registry (csrc/host/tune.c has the table of names): bsx_tune_set(name, value) between calls of the library
 * (value NULL: back to the default; BSX_E_ARG for an unknown name), or "$BSX_TUNE=name=value,name=value" for a whole process.  bsx_phases():
 * the diagnostic level ($BSX_PHASES or the setting "phases"). */
int bsx_tune_set(const char *name, const char *value);
const char *bsx_tune_str(const char *name);
long bsx_tune_long(const char *name, long dflt);
int bsx_tune_is_set(const char *name);
int bsx_phases(void);
const char *bsx_tune_name(int i);
const char *bsx_tune_doc(int i);

/* device-side work counters of the last seed/sa batch (algorithmic-bytes model):
 * c[0]=bwt_occ4 calls, c[1]=same-block bwt_2occ4 calls, c[2]=bwt_occ calls (inside bwt_sa, from k_sa and
 * from the region kernels), c[3]=bwt_sa calls */
int bsx_device_counters(bsx_device_t *dev, uint64_t c[4], int reset);
/* the seeding passes of bsx_regions_batch one by one, since the last reset (read it BEFORE bsx_device_counters / bsx_device_seed_table with
 * reset: they zero the same counters): w[0], w[1] = 64-byte FM blocks and table entries read by the chunk-wide first pass (and bsx_seed_batch
 * launches), w[2], w[3] = by the second pass over the strand searches seeded again inside a chunk's launch sequence, w[4] = its launches,
 * w[5] = its strand searches; ms[0], ms[1] = the two passes' summed HIP-event times.  (Each pass's bytes over that pass's time: bench.py) */
int bsx_device_seed_passes(bsx_device_t *dev, uint64_t w[6], double ms[2], int reset);
/* Several GPUs sharing ONE chunk: each process aligns a slice of the chunk's pairs.  Two things tie a read to its chunk:
 * mem_pestat (bwamem.c:464-467), whose result is a function of the chunk's histogram of insert sizes -- bsx_pes_hist_hook, when set, is
 * called with this process's histogram (2 * max_ins + 1 counters) and must return the sum over all processes in place (an all-reduce;
 * bsx_pestat_sync_empty: the call of a process whose slice is empty) -- and the pair's index within the chunk, which seeds the hash that
 * breaks ties between equal hits (bwamem.c:408,413): bsx_chunk_slice_offset(first) says where the NEXT chunk this thread passes to
 * bsx_process_seqs / bsx_stream_push starts within its chunk.  n_processed is the global index of the slice's first read, as always. */
extern void (*bsx_pes_hist_hook)(void *ud, int64_t *hist, int n_bins);
extern void *bsx_pes_hist_ud;
void bsx_pestat_sync_empty(const bsx_opt_t *opt);
void bsx_chunk_slice_offset(int64_t first);
/* what the region kernels (bsx_regions_batch: K3 + C1 + C2 + K4 + C4) were given and made since the last reset, summed over the chunks:
 * w[0] strand searches, w[1] SA intervals read (32 B each), w[2] seed occurrences whose position was looked up (8 B each),
 * w[3] alignment regions written (56 B each), w[4] read bases of the strand searches -- the terms of the family's algorithmic bytes */
int bsx_device_region_work(bsx_device_t *dev, uint64_t w[5], int reset);
/* launches since the last reset whose extension rows were c[0] packed 16-bit (two columns per lane; the scoring options keep every
 * intermediate inside 16 bits) / c[1] 32-bit: a chunk of bsx_regions_batch or a bsx_extend_batch under the setting ext4=4 counts once */
int bsx_ext_forms(uint64_t c[2], int reset);
/* the extensions' stopping rule (the setting ext_stop) since the last reset, five words per launch family -- k_ext4, k_extl, the HBM
 * tiers, chains -> regions, the wavefront-per-job batch form: extensions stopped, evaluations of the rule, rows left at the stops, and with
 * the switch off rows run after the rule would have fired and extensions it would have stopped; c[25] = extensions stopped over all families.
 * Counted by bsx_extend_batch under the setting ext4 and, with phases on, by the region launches */
int bsx_ext_stops(uint64_t c[26], int reset);
/* the seeding kernel's table of k-mer intervals: entries read since the last reset, depth K of the resident table (0: none) */
int bsx_device_seed_table(bsx_device_t *dev, uint64_t *lookups, int *depth, int reset);
/* average GPU time (ms, HIP events on the launch stream) and launch count of each kernel since
 * the last reset: k = 0 seed (the chunk-wide launch of bsx_regions_batch), 1 sa, 2 extend, 3 sw, 4 global, 5 regions (first tier),
 * 6 regions (tiers 1b, 2 and 3), 7 seed outside the chunk-wide launch (the second seeding pass inside a chunk's sequence; bsx_seed_batch launches: the strand searches the host chains) */
int bsx_device_kernel_time(bsx_device_t *dev, int k, double *total_ms, int64_t *launches, int reset);

/* ------------------------------------------------------------------------------------------
 * Several GPUs ("replicas + gather"): one process per GPU, the per-chunk alignment records brought together in input order.
 * The reference has nothing to bind here (it is one process: align.c:100-170 writes its chunks in order from kt_pipeline's third step);
 * what these replace is that ordered write, across processes.  csrc/host/gather.c has the protocol (rounds: sizes to everybody, then either
 * the payload to rank 0 or every rank's own pwrite() into the output file at its offset), over a small communication vtable:
 *   bsx_transport_rccl   RCCL over xGMI (ncclAllGather / ncclSend / ncclRecv / ncclAllReduce; the unique id travels through a file);
 *   bsx_transport_local  the ranks as threads of one process (tests of the protocol).
 * ------------------------------------------------------------------------------------------ */
typedef struct bsx_transport {
	void *ctx;
	int rank, world;
	int (*all_gather)(void *ctx, const int64_t *mine, int n, int64_t *all);   /* n values of every rank, in rank order, to every rank */
	int (*send)(void *ctx, int dst, const void *buf, size_t n_bytes);          /* host memory; returns when buf may be reused */
	int (*recv_many)(void *ctx, int n_src, const int *src, void *const *buf, const size_t *n_bytes);   /* the receives of a round, posted together */
	int (*all_reduce_sum)(void *ctx, int64_t *buf, int n);                     /* in place (the insert-size histograms of ranks sharing a chunk) */
	void (*close)(void *ctx);
} bsx_transport_t;
int bsx_transport_local(int world, bsx_transport_t *out);   /* out[0 .. world): one per thread-rank */
/* rank / world of this process, the HIP device its staging buffers live on, and a path all ranks can read: rank 0 writes the unique ids there
 * (and removes the file when the last communicator is up).  Two communicators: `gather` for the rounds, `reduce` for all_reduce_sum calls
 * made from another thread (either may be NULL).  BSX_E_NODEVICE when librccl cannot be loaded. */
int bsx_transport_rccl(int rank, int world, int device, const char *id_path, bsx_transport_t *gather, bsx_transport_t *reduce);
/* the ranks as processes of one node talking through rank 0 over Unix-domain sockets <path>.0 / <path>.1 (the CPU checker's multi-process
 * runs; a fallback where librccl cannot be loaded) */
int bsx_transport_socket(int rank, int world, const char *path, bsx_transport_t *gather, bsx_transport_t *reduce);
typedef struct bsx_gather bsx_gather_t;
/* direct_path != NULL: every rank writes its own chunks into that file (bsx_gather_direct_ok says whether it may); else rank 0's `sink`
 * is called with every chunk in input order.  max_pending: chunks a rank may hold before bsx_gather_submit blocks. */
int bsx_gather_open(const bsx_transport_t *tr, const char *direct_path, void (*sink)(void *ud, int64_t chunk, const void *buf, size_t n), void *ud,
                    int max_pending, bsx_gather_t **out);
int bsx_gather_set_header(bsx_gather_t *g, const void *hdr, size_t n);       /* rank 0, direct form: what the file starts with */
int bsx_gather_submit(bsx_gather_t *g, int64_t chunk, void *buf, size_t n);  /* buf: malloc'd, the gather's from now on */
int bsx_gather_close_input(bsx_gather_t *g);                                 /* no more chunks from this rank */
int bsx_gather_run(bsx_gather_t *g, int64_t *n_chunks);                      /* the rounds, on the calling thread, until the input has ended everywhere */
void bsx_gather_stats(const bsx_gather_t *g, int64_t out[3]);                /* rounds, payload bytes rank 0 received, bytes this rank wrote itself */
void bsx_gather_free(bsx_gather_t *g);
int bsx_gather_direct_ok(const char *path, int world, int local_world);

/* ------------------------------------------------------------------------------------------
 * The whole path: mem_process_seqs (lib/aln/bwamem.c:432-476, declared bwamem.h:184)
 *   reads[i].{name,comment,seq(nt4),qual,l_seq,barcode,umi} in; reads[i].sam (malloc'd) out;
 *   PE input interleaved, n even.  Returns BSX_OK or an error instead of aborting.
 * ------------------------------------------------------------------------------------------ */
int bsx_process_seqs(bsx_device_t *dev, const bsx_opt_t *opt, const bsx_index_t *idx,
                     int64_t n_processed, int n, bsx_read_t *reads, const bsx_pestat_t *pes0);

/* The same, for a sequence of chunks, as a pipeline: what lib/aln/align.c:100-170 (kt_pipeline over
 * read / mem_process_seqs / write) does for I/O, done here for the two halves of the aligning step itself.  The
 * device-bound front half of a chunk (seeding .. regions) runs on its own device lane and thread while the
 * host-bound back half of an older chunk (merge, pairing, CIGAR, SAM text) runs on the caller's thread; up to
 * depth-1 front halves are in flight ahead of it (depth 3, or 4 against genomes of 1 Gbp and more, unless $BSX_STREAM_DEPTH says otherwise; at most 6).
 *   bsx_stream_push(chunk k) returns once chunk k-(depth-1) is complete (its reads[i].sam are set);
 *   bsx_stream_flush completes the chunks still in flight, in order.  Every chunk is independent, exactly as with
 *   bsx_process_seqs (own insert-size statistics unless pes0 is given): the output does not depend on the depth.
 * opt and idx must outlive the stream; a chunk's reads must stay valid until it is complete. */
typedef struct bsx_stream bsx_stream_t;
int  bsx_stream_open(bsx_device_t *dev, const bsx_opt_t *opt, const bsx_index_t *idx, const bsx_pestat_t *pes0, bsx_stream_t **out);
int  bsx_stream_depth(const bsx_stream_t *s);
int  bsx_stream_push(bsx_stream_t *s, int64_t n_processed, int n, bsx_read_t *reads);
int  bsx_stream_flush(bsx_stream_t *s);
void bsx_stream_close(bsx_stream_t *s);

/* Per-read conversion by context while aligning: what `biscuit bsconv` (src/bsconv.c) does to the aligner's output in a second pass.
 * annotate: every mapped record gains ZN:Z:CA_R<r>C<c>,CC_..,CG_..,CT_.. as its last field, nothing is dropped.  The filters: bsconv's per-record
 * rule on top of that (unmapped and QC-fail records, and YD:u records with filter_u, are filtered; the max_* bounds as in bsconv.c:111-140, -1 and
 * 1.0 meaning none); show_filtered keeps the filtered records instead.  A record is dropped on its own, its mate's fields are not touched.
 * One deliberate difference from the tool: hard-clipped bases are not in SEQ and are not walked (the tool indexes past SEQ there). */
typedef struct bsx_bsconv_conf {
	int annotate;
	int filter_u;
	int show_filtered;
	int max_cph, max_cpa, max_cpc, max_cpt, max_cpy;
	float max_cph_frac, max_cpy_frac;
} bsx_bsconv_conf_t;
void bsx_bsconv_conf_init(bsx_bsconv_conf_t *conf);   /* the tool's defaults: -1 / 1.0, nothing switched on */
/* The per-record rule is on as soon as one of its members differs from the defaults (filter_u, show_filtered, a bound >= 0, a fraction < 1.0),
 * and implies annotate.  conf == NULL, or nothing of it set: off (the default).  The stream keeps a copy.  Call before the first push. */
int  bsx_stream_set_bsconv(bsx_stream_t *s, const bsx_bsconv_conf_t *conf);
/* the tool's retn_conv_counts (CpA retained, CpA converted, CpC .., CpG .., CpT ..) summed over the records written, and its two counters:
 * records seen and records filtered */
int  bsx_stream_bsconv_totals(const bsx_stream_t *s, uint64_t out[8], uint64_t *n, uint64_t *n_filtered);
/* the same for bsx_process_seqs (and for any chunk processed outside a stream that has its own setting): one setting and one set of totals
 * per process; bsx_process_bsconv_totals with reset != 0 zeroes them */
int  bsx_process_set_bsconv(const bsx_bsconv_conf_t *conf);
int  bsx_process_bsconv_totals(uint64_t out[8], uint64_t *n, uint64_t *n_filtered, int reset);

/* The BISCUITqc tables while aligning: what `biscuit qc <ref> <bam> PREFIX` (src/qc.c) would count over the SAM written, a record at a time
 * as it is written (after bsconv's filters: a dropped record is not counted).  Record fields are counted on the host, columns on the device
 * (bsx_qc_batch; a backend without it walks them on the host).  Differences from the tool: hard-clipped bases count towards the read position
 * and are never indexed into SEQ; position 301 is dropped with those beyond it; 64-bit counters. */
#define BSX_QC_N_MAPQ 61
#define BSX_QC_ISIZE  1000
typedef struct bsx_qc_totals {
	bsx_qc_counts_t dev;                    /* the column counts */
	uint64_t mapq[BSX_QC_N_MAPQ + 1];       /* non-secondary records by MAPQ; [61]: unmapped */
	uint64_t isize[BSX_QC_ISIZE + 1];       /* proper pair, MAPQ >= 40, 0 <= TLEN <= 1000, non-secondary */
	uint64_t n_isize;
	uint64_t all_tot, all_dup, q40_tot, q40_dup;   /* the two duplicate counts: records written with 0x400 (only --markdup sets it: 0 without) */
	uint64_t strandcnt[16];                 /* [(no 0x40) * 8 + reverse * 4 + YD tag] over mapped records */
} bsx_qc_totals_t;
/* on != 0: count from the next chunk on, totals from zero.  A stream's own setting takes its chunks out of the process's.  The device's table
 * is one per device: one stream (or the process) at a time counts on a device.  Call before the first push. */
int  bsx_stream_set_qc(bsx_stream_t *s, int on);
int  bsx_stream_qc_totals(bsx_stream_t *s, bsx_qc_totals_t *out);   /* after bsx_stream_flush */
int  bsx_process_set_qc(int on);
int  bsx_process_qc_totals(bsx_qc_totals_t *out, int reset);        /* while the devices the chunks ran on are still open */
/* PREFIX_mapq_table.txt, _dup_report.txt, _strand_table.txt, _totalReadConversionRate.txt, _CpGRetentionByReadPos.txt, _CpHRetentionByReadPos.txt
 * and, with paired != 0, _isize_table.txt: the formatters of src/qc.c:29-110, byte for byte */
int  bsx_qc_write(const char *prefix, const bsx_qc_totals_t *t, int paired);

/* The BISCUITqc coverage tables while aligning (--qc-cov): with set_qc on, every record written without 0x4 -- secondary, supplementary and 0x400
 * records too, as `bedtools genomecov -ibam` counts them; after --bsconv's filters -- goes to the depth state of the device it was aligned on
 * (bsx_cov_batch; a backend without the seam keeps the state on the host, cov.c).  One depth state per device: one stream or one process call
 * at a time.  set_qc_cov(1) needs set_qc(1) before it (BSX_E_ARG otherwise) and starts from all-zero depth; the masks (forward coordinates, as
 * bsx_cov_set_mask; both or neither) are set after it and before the first push.  The tables: after bsx_stream_flush / while the device is open. */
int  bsx_stream_set_qc_cov(bsx_stream_t *s, int on);
int  bsx_stream_set_qc_cov_mask(bsx_stream_t *s, int which, int64_t n_intervals, const int64_t *beg_end);
int  bsx_stream_qc_cov_tables(bsx_stream_t *s, bsx_cov_tables_t *out);
int  bsx_process_set_qc_cov(int on);
int  bsx_process_set_qc_cov_mask(int which, int64_t n_intervals, const int64_t *beg_end);
int  bsx_process_qc_cov_tables(bsx_cov_tables_t *out);
/* PREFIX_covdist_{all,q40}_{base,cpg}[_topgc|_botgc]_table.txt (the GC tables with have_gc) and PREFIX_cv_table.txt, titles and headers as
 * scripts/QC.sh:153-415 prints them: a depth\tcount row per depth with a non-zero count, ascending; a uniformity row per table, in the
 * script's order, where sum(count) > 0 and sum(count * depth) > 0: mu = sum(count * depth) / sum(count) from exact integer sums, sigma =
 * sqrt(sum(count * (depth - mu)^2) / sum(count)) accumulated in double in ascending depth, and sigma / mu, each as %.6g (what awk's default
 * output format prints for every value below 10^6) */
int  bsx_cov_write(const char *prefix, const bsx_cov_tables_t *t);
/* a BED file (plain or gzip; chrom start end, 0-based half-open, further columns ignored, blank lines, lines starting with '#' and lines whose first
 * word is "track" or "browser" skipped) -> forward intervals, *beg_end malloc'd (2 * *n values).  BSX_E_IO: cannot be read; BSX_E_FORMAT: a malformed line, an
 * interval outside its contig, a contig that is not in the index (message on stderr) */
int  bsx_cov_read_bed(const char *path, const bsx_index_t *idx, int64_t *n, int64_t **beg_end);

/* BISCUITqc's base-averaged conversion table while aligning (--qc-meth): with set_qc on, every record written that passes the record filters
 * of `biscuit pileup` at its defaults -- none of 0x4, 0x100, 0x200, 0x400 (after --markdup), MAPQ >= 40, at least 10 bases of SEQ, not paired
 * without 0x2, AS >= 40; after --bsconv's filters -- goes to the counters of the device it was aligned on (bsx_meth_batch; a backend without
 * the seam keeps them on the host, meth.c).  One counter state per device: one stream or one process call at a time.  set_qc_meth(1) needs
 * set_qc(1) before it (BSX_E_ARG otherwise) and starts from zero.  The tables: after bsx_stream_flush / while the device is open. */
int  bsx_stream_set_qc_meth(bsx_stream_t *s, int on);
int  bsx_stream_qc_meth_tables(bsx_stream_t *s, bsx_meth_tables_t *out);
int  bsx_process_set_qc_meth(int on);
int  bsx_process_qc_meth_tables(bsx_meth_tables_t *out);
/* PREFIX_totalBaseConversionRate.txt: the title, CA\tCC\tCG\tCT, and per context -1 when k < 20, else (double)s / (1000.0 * (double)k) as %.6g */
int  bsx_meth_write(const char *prefix, const bsx_meth_tables_t *t);
/* the beta in thousandths: the integer printf("%1.3f", (double)r / (double)n) shows, times 1000 (0 <= r <= n, n > 0), without printf */
uint32_t bsx_meth_milli(uint32_t r, uint32_t n);

/* The per-cytosine methylation BED while aligning (--meth-bed): the sites of the same counters (bsx_meth_sites; meth.c for a backend without
 * the seam), with set_qc_meth on, after bsx_stream_flush / while the device is open.  A state no record has reached yet has no site. */
int  bsx_stream_qc_meth_sites(bsx_stream_t *s, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap,
                              int64_t *n, int64_t *f_next);
int  bsx_process_qc_meth_sites(const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n,
                               int64_t *f_next);
/* the file: contig by contig in `order` (n_seqs indices of the index's contigs; NULL: the index's order; bsx_meth_bed_order makes it from a SAM
 * header: the contigs in the order of its @SQ lines, the first of two equal names counting, those without a line behind the others in the
 * index's order; free() it), every contig window by window through `sites` (a bsx_meth_sites / bsx_*_qc_meth_sites over `ud`) with a buffer of
 * cap records (0: 1 << 20), every record as a line:
 *   without merge  name\tf\tf + 1\tB\tn\n            f the 0-based offset in the contig, n = ret + conv, B = bsx_meth_milli(ret, n) as d.ddd
 *   with merge     name\tbeg\tend\tB\tcov\tC:b:n,G:b:n\n   beg = f and end = f + 2 where there is a C, beg = f - 1 and end = f + 1 for a G alone;
 *                  cov = nC + nG, B = bsx_meth_milli(M, cov) with M = (int)(rintf(bC * nC) + rintf(bG * nG)), b = milli / 1000.0 and the product in
 *                  IEEE double, rintf of it as a float (mergecg.c:116-118), an absent side 0 and printed `C:.:0` / `G:.:0`
 * No printf("%f"): digits from integers.  *n_lines (may be NULL): the lines written. */
typedef int (*bsx_meth_sites_fn)(void *ud, const bsx_meth_site_opt_t *opt, int64_t f_lo, int64_t f_hi, bsx_meth_site_t *out, int64_t cap, int64_t *n,
                                 int64_t *f_next);
int  bsx_meth_bed_write(FILE *f, const bsx_index_t *idx, const int32_t *order, const bsx_meth_site_opt_t *opt, bsx_meth_sites_fn sites, void *ud,
                        int64_t cap, uint64_t *n_lines);
int32_t *bsx_meth_bed_order(const bsx_index_t *idx, const char *sam_header);
/* one record as its line into buf (at least 160 bytes beyond the contig's name); returns the line's length */
size_t bsx_meth_bed_line(char *buf, const char *name, int64_t ctg_off, const bsx_meth_site_opt_t *opt, const bsx_meth_site_t *r);

/* Duplicate marking while aligning (--markdup).  A template is one unit of the input, a pair or a single read; its ordinal is its 0-based index
 * in the input of the stream (or of the process) over all chunks.  Each end's primary record is the one with neither 0x100 nor 0x800; the
 * template's key is bsx_markdup_key_t over them.  A template with no placed end is never a duplicate and never enters the table.  A template
 * is a duplicate when a template with a lower ordinal has an equal key: every record written for it -- primary, secondary, supplementary, an
 * unplaced mate's -- gets 0x400, and nothing else in any record changes.  The decision is made once the CIGARs are final and before bsconv's
 * filters: a template whose records are all dropped still holds its key.  Barcodes, read groups and optical distance are not part of the key,
 * and single-end templates are never compared against pairs, whether both reads of the pair are placed or one (both unlike dupsifter).  Keys are looked up on the device (bsx_markdup_batch),
 * one batch per slice of a chunk, in input order; a backend without markdup_batch uses a table on the host with the same rule.
 * The device's table is one per device: one stream (or the process) at a time marks on a device.  A stream's or the process's first chunk
 * after set_markdup(1) empties the backend's table, so a device kept open over two runs starts the second one with an empty table. */
typedef struct bsx_markdup_totals { uint64_t n_templates, n_keyed, n_dup; } bsx_markdup_totals_t;   /* seen, with a placed end, marked */
int  bsx_stream_set_markdup(bsx_stream_t *s, int on);                  /* before the first push */
int  bsx_stream_markdup_totals(bsx_stream_t *s, bsx_markdup_totals_t *out);   /* after bsx_stream_flush */
int  bsx_process_set_markdup(int on);                                  /* on != 0: from the next chunk on, ordinals and totals from zero */
int  bsx_process_markdup_totals(bsx_markdup_totals_t *out, int reset);

/* `biscuit align` command line: main_align (lib/aln/align.c:319-598).  SAM on `out` (stdout). */
int bsx_align_main(int argc, char **argv);

/* SAM header: bwa_print_sam_hdr (lib/aln/bwa.c:654-684); returns malloc'd text */
char *bsx_sam_header(const bsx_index_t *idx, const char *hdr_line, const char *pg_line);

BSX_EXPORT const char *bsx_version(void);
BSX_EXPORT const char *bsx_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif
