// kernels.h -- launchers of the gfx950 kernels (defined in k_*.hip), used by shim.hip
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "seed_core.hpp"
#include "seed_tab.hpp"
#include "ctr_layout.hpp"

void launch_seed(hipStream_t st, int grid, const DevIndex &ix, const uint8_t *reads, const bsx_seed_task_t *tasks, int n_tasks, const SeedParams &P,
                 DevIntv *scratch, int list_cap, int mem_cap, DevIntv *out, unsigned long long out_cap, unsigned long long *out_cursor,
                 long long *task_off, int *task_n, unsigned int *task_cursor, unsigned long long *counters,
                 int quota, unsigned int *slab_busy, int n_slabs, int trip_budget, int prof = 0, uint32_t *qpack = nullptr, unsigned long long direct_off = ~0ull);   // direct_off (table form only): the lists of strand search t go to out[direct_off + t * mem_cap ...] and stay there (task_off says so; no cursor); scratch holds n_slabs per-wave slabs; slab_busy[n_slabs] zeroed once; qpack: seedt_pack_bytes(n_tasks) of scratch for the table form (the reads as base-3 digits)
// the same over the table of k-mer intervals (k_seedt.hip, seed_tab.hpp): what launch_seed runs when ix.tab.K >= 2 (and $BSX_SEED_FORM is not "classic");
// counters[120] += table entries read
void launch_seedt(hipStream_t st, int grid, const DevIndex &ix, const uint8_t *reads, const bsx_seed_task_t *tasks, int n_tasks, const SeedParams &P,
                  DevIntv *scratch, int list_cap, int mem_cap, DevIntv *out, unsigned long long out_cap, unsigned long long *out_cursor,
                  long long *task_off, int *task_n, unsigned int *task_cursor, unsigned long long *counters,
                  int quota, unsigned int *slab_busy, int n_slabs, int trip_budget, int prof = 0, uint32_t *qpack = nullptr, unsigned long long direct_off = ~0ull);
size_t seedt_pack_bytes(long long n_tasks);
void launch_gather_lists(hipStream_t st, const DevIntv *src, const long long *off, const int *cnt, const long long *which, const long long *dst_off, long long n_list, DevIntv *dst);
// the table of one converted index, K levels (seed_tab_entries(K) entries of 16 bytes at `table`), from the index resident in ix
int seedtab_build(hipStream_t st, const DevIndex &ix, int parent, int K, void *table);
// the symbols of every 64-byte block from the file's 2-bit fields into the device's two bit planes, in place (n_words: the .bwt body)
void launch_bwt_planes(hipStream_t st, uint32_t *bwt, unsigned long long n_words);
void launch_sa(hipStream_t st, int grid, const DevIndex &ix, const bsx_sa_job_t *jobs, long long n, uint64_t *pos, unsigned long long *counters);
// DP kernels: one wavefront per job
void launch_extend(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, const int *order,
                   long long n, bsx_ext_res_t *res, int qcap, int nc, int n_cu);
// the same for queries whose rows outgrow LDS (longer than 16 k bases): rows in `rows`, extend_hbm_row_bytes(qcap) per wave, blocks x 4 waves
size_t extend_hbm_row_bytes(int qcap);
void launch_extend_hbm(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, const int *order,
                       long long n, bsx_ext_res_t *res, int qcap, int blocks, void *rows);
size_t global_hbm_row_bytes(int qcap);
void launch_global_hbm(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_glb_job_t *jobs, const int *order,
                       long long n, bsx_glb_res_t *res, uint32_t *pool, uint8_t *zscratch, size_t zstride, int qcap, int blocks,
                       bsx_glb_tag_t *tags, char *md_pool, unsigned long long md_cap, unsigned long long *md_cursor, void *rows, bsx_glb_ctx_t *ctx = nullptr);   // one wave per workgroup; ctx: the k_global_ctx form
void launch_sw(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_sw_job_t *jobs, const int *order,
               long long n, bsx_sw_res_t *res, unsigned long long *bscratch, int bcap, int blocks, int nc);
void launch_swl(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_sw_job_t *jobs, const int *order,
                long long n, bsx_sw_res_t *res, unsigned long long *bscratch, int bcap, int blocks, int slen_max);   // k_swl.hip: byte-sized jobs, four to a wavefront
void launch_global(hipStream_t st, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_glb_job_t *jobs, const int *order,
                   long long n, bsx_glb_res_t *res, uint32_t *pool, uint8_t *zscratch, size_t zstride, int qcap, int nc, int blocks, int wpb,
                   bsx_glb_tag_t *tags = nullptr, char *md_pool = nullptr, unsigned long long md_cap = 0, unsigned long long *md_cursor = nullptr, int tcap = 0,
                   bsx_glb_ctx_t *ctx = nullptr);   // ctx != nullptr (with tags): k_global_ctx, which also fills ctx[job] (bsx_global_batch_tags_ctx)
// k_qc.hip: the column counts of `biscuit qc` over n records (bsx_qc_job_t), added to the device's table (bsx_qc_counts_t as 64-bit cells)
void launch_qc(hipStream_t st, const DevIndex &ix, const uint8_t *reads, long long reads_len, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool,
               unsigned long long *table, int n_cu);
// k_cov.hip: the BISCUITqc coverage tables.  diff: cov_diff_entries(l_pac) entries of two ints (all, q40), the difference array of the depth, zero
// past entry l_pac; a mask: cov_mask_words(l_pac) words, bit (p & 31) of word p >> 5 for position p.  launch_cov_add: the M runs of the jobs with
// BSX_QC_COV as +1 / -1 events.  The tables, in this order: launch_cov_sums (tsum: cov_n_tiles(l_pac) pairs, afterwards each tile's carry-in),
// launch_cov_max (*gmax, zeroed before: the largest `all` depth), launch_cov_count (bins: BSX_COV_N_TABLES x nb zeroed 64-bit cells, nb > *gmax;
// m_top and m_bot both or neither; lds_bins: a power of two up to COV_LDS_BINS_MAX; a workgroup adds its LDS cells to bins every flush_tiles tiles,
// flush_tiles x BSX_COV_TILE < 2^32).  ix.pac must be readable for 8 bytes past its l_pac / 4 + 1 (bsx_device_upload_index reserves 16): the last
// lanes below l_pac read their 16 bases as one dword and the next base from the byte behind it)
#define COV_LDS_BINS_MAX 512
size_t cov_n_tiles(long long l_pac);
size_t cov_diff_entries(long long l_pac);
size_t cov_mask_words(long long l_pac);
void launch_cov_add(hipStream_t st, int n_cu, void *diff, long long l_pac, const bsx_qc_job_t *jobs, long long n, const uint32_t *pool, long long pool_len);
void launch_cov_paint(hipStream_t st, int n_cu, uint32_t *mask, long long l_pac, const long long *beg_end, long long n);
void launch_cov_sums(hipStream_t st, int n_cu, const void *diff, long long n_tiles, void *tsum);
void launch_cov_max(hipStream_t st, int n_cu, const DevIndex &ix, const void *diff, const void *carry, long long n_tiles, int *gmax);
void launch_cov_count(hipStream_t st, int n_cu, const DevIndex &ix, const void *diff, const void *carry, long long n_tiles, const uint32_t *m_top,
                      const uint32_t *m_bot, int lds_bins, int flush_tiles, unsigned long long *bins, long long nb);
// k_meth.hip: the base-averaged conversion table.  state: meth_state_entries(l_pac) entries of two 64-bit words (ret | conv << 32, opp_ref |
// opp_alt << 32), zero past entry l_pac.  launch_meth_add: the columns of n jobs (bsx_meth_job_t: CIGAR words and quality masks in pool) added
// to it, the reads those of the lane.  launch_meth_tables: out = 2 x BSX_METH_N_CTX zeroed 64-bit cells, the sites per context and then the sums
// of their thousandths; 1 <= flush_tiles <= METH_FLUSH_TILES_MAX; ix.pac readable as launch_cov_count needs it
#define METH_FLUSH_TILES_MAX 1024
size_t meth_n_tiles(long long l_pac);
size_t meth_state_entries(long long l_pac);
void launch_meth_add(hipStream_t st, const DevIndex &ix, const uint8_t *reads, long long reads_len, const bsx_meth_job_t *jobs, long long n,
                     const uint32_t *pool, long long pool_len, void *state, int n_cu);
void launch_meth_tables(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, long long n_tiles, int flush_tiles, unsigned long long *out);
// k_msite.hip: the methylation sites of that state (bsx_meth_sites) over the nt tiles from tile t_lo on.  launch_msite_count: cnt[i] = the records
// that belong to tile t_lo + i and to [f_lo, f_hi).  launch_msite_emit: base = nt + 1 exclusive sums of those counts; the records of tile
// t_lo + i go to out[base[i] .. base[i + 1]), and nothing is written at or beyond out[base[i + 1]]
void launch_msite_count(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, const bsx_meth_site_opt_t &opt, long long f_lo, long long f_hi,
                        long long t_lo, long long nt, uint32_t *cnt);
void launch_msite_emit(hipStream_t st, int n_cu, const DevIndex &ix, const void *state, const bsx_meth_site_opt_t &opt, long long f_lo, long long f_hi,
                       long long t_lo, long long nt, const uint32_t *base, bsx_meth_site_t *out);
// k_bam.hip: SAM lines -> BAM records (bsx_bam_encode; the rule is csrc/host/bam_rec.h).  text: whole lines on a 16-byte boundary, len below 2^31.
// launch_bam_count: cnt[t] = newlines of tile t (bam_n_tiles(len) tiles).  launch_bam_scan: out[i] = in[0] + .. + in[i - 1] for i <= n (n + 1 entries
// out; in place allowed), one workgroup.  launch_bam_starts: base = those sums of cnt; start[0] = 0, start[r + 1] = one past the r-th newline.
// launch_bam_size: size[i] = the record length of line i, 0 for a refused line, errs[i] = 0 or its BSX_BAM_E_*; bad[w] (bam_lines_grid(n_lines)
// words) = the least (line << 4 | code) among lines 256 w .., all ones for none.  launch_bam_emit: record i at out + off[i] for i < n_lines
// (errs: the same n_lines words).  The name table: n_names
// names sorted bytewise, name k = names[noff[k] .. noff[k + 1]), nid[k] its refID
long long bam_n_tiles(long long len);
int bam_lines_grid(long long n_lines);
void launch_bam_count(hipStream_t st, int n_cu, const char *text, long long len, uint32_t *cnt);
void launch_bam_scan(hipStream_t st, const uint32_t *in, uint32_t *out, long long n);
void launch_bam_starts(hipStream_t st, int n_cu, const char *text, long long len, const uint32_t *base, uint32_t *start);
void launch_bam_size(hipStream_t st, const char *text, const uint32_t *start, long long n_lines, const char *names, const uint32_t *noff,
                     const int32_t *nid, int n_names, uint32_t *size, int *errs, unsigned long long *bad);
void launch_bam_emit(hipStream_t st, const char *text, const uint32_t *start, long long n_lines, const char *names, const uint32_t *noff,
                     const int32_t *nid, int n_names, int *errs, const uint32_t *off, uint8_t *out);
// k_bgzf.hip: payload -> BGZF members (bsx_bgzf_deflate), a workgroup per block of 0xff00 bytes: n_launch <= bgzf_grid(blocks left) blocks from
// block b0 on per launch, with bgzf_tok_bytes(n_launch) / bgzf_cand_bytes(n_launch) of workspace; block b's member goes to slots + b * 65536,
// its length to sizes[b].  payload on a 16-byte boundary.  crc_ops: bgzf_crc_ops' 256 words on the device.  launch_bgzf_compact: off = the n_blocks + 1 exclusive sums of sizes; member b moves to out + off[b]
size_t bgzf_lds_bytes(void);
int bgzf_grid(long long n_blocks);
size_t bgzf_tok_bytes(int grid);
size_t bgzf_cand_bytes(int grid);
void bgzf_crc_ops(uint32_t *ops);
void launch_bgzf_deflate(hipStream_t st, const uint8_t *payload, long long len, long long b0, int n_launch, const uint32_t *crc_ops, uint32_t *ws_tok,
                        uint16_t *ws_cand, uint8_t *slots, uint32_t *sizes);
void launch_bgzf_compact(hipStream_t st, int n_cu, const uint8_t *slots, const uint32_t *off, long long n_blocks, uint8_t *out);
// k_markdup.hip: the device's table of template keys (bsx_markdup_batch).  A slot: claim word (0: empty), lowest ordinal, the key (all ones: none yet)
struct MdSlot { unsigned long long claim, ord, k0, k1; };
enum { MD_CTR_TAKEN = 0, MD_CTR_OPEN = 1, MD_CTR_LOST = 2 };   // ctr[] of the two launchers below
enum { MD_RES_FIRST = 0, MD_RES_DUP = 1, MD_RES_OPEN = 2, MD_RES_SKIP = 3, MD_RES_FULL = 4 };   // a key's state in res[] (OPEN: to be looked up in this round)
void launch_md_init(hipStream_t st, MdSlot *T, unsigned long long n_slots);
// one round over the keys still OPEN: k_md_claim, k_md_publish, k_md_decide; ctr[0] += slots taken, ctr[1] += keys left OPEN (another key has their claim word)
void launch_md_round(hipStream_t st, MdSlot *T, unsigned long long n_slots, const bsx_markdup_key_t *keys, long long n, unsigned long long first,
                     unsigned salt, int bits, uint8_t *res, unsigned long long *slot, unsigned long long *ctr);
// every taken slot of `old` into T (initialised, at least twice the slots); ctr[2] += slots that found no room (none)
void launch_md_rehash(hipStream_t st, const MdSlot *old, unsigned long long n_old, MdSlot *T, unsigned long long n_slots, unsigned long long *ctr);
// k_sort.hip: the stable radix sort of bsx_sort_run / bsx_sort_schedule, 8 bits a pass (n below 2^31).  launch_sort_bits: *bits (zeroed before) |=
// key ^ keys[0] over all keys.  launch_sort_pass: one pass on the byte at `shift` from (keys_in, pay_in) to (keys_out, pay_out); pay_in == nullptr:
// the payload is the key's index; counts: 256 x sort_n_tiles(n) words, btot: sort_n_scan_blocks(n) words.  launch_sort_small: n <= BSX_SORT_TILE,
// every pass that moves something, in one workgroup's LDS.
#define SORT_SCAN_BLOCK 2048
size_t sort_n_tiles(long long n);
size_t sort_n_scan_blocks(long long n);
void launch_sort_bits(hipStream_t st, const unsigned long long *keys, long long n, unsigned long long *bits);
void launch_sort_pass(hipStream_t st, const unsigned long long *keys_in, const unsigned int *pay_in, unsigned long long *keys_out, unsigned int *pay_out,
                      long long n, int shift, unsigned int *counts, unsigned int *btot);
void launch_sort_small(hipStream_t st, const unsigned long long *keys_in, const unsigned int *pay_in, unsigned long long *keys_out, unsigned int *pay_out, long long n);
// K4 four to a wavefront (k_ext4.hip): a row of 16 lanes per job, persistent rows taking jobs off *cursor (zero at launch).
// launch_x4: the extensions of the best seed of every chain the tiers exported (records with has_ext), written into the records ahead of
// launch_c2r; jobs = room for job_cap jobs of x4_job_bytes(), ctr32[0..3]: job counts and cursor (zeroed by the call).
// launch_ext4_batch: plain ksw_extend2 jobs through the same rows (tests); jobs it cannot hold (query longer than x4_max_query(16),
// scores of 2^21 or more) are answered with score = X4_DECLINED.
#define X4_DECLINED (-0x7fffffff)
// tests: plain jobs through ext_dp_win (ext_dp.hpp: rows in a register window that follows the band, queries of any length), a wavefront per job
void launch_extwin_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, bsx_ext_res_t *res, long long n);
// tests: plain jobs of up to 255 query bases through ext_dp_pk (ext_pk.hpp: two columns per lane in packed 16-bit) when `packed`, a wavefront per
// job; else through the 32-bit row the region kernels keep for scoring options beyond ext_pk_exact() (ext_pk_bound.h)
void launch_extpk_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, bsx_ext_res_t *res, long long n, bool packed);
int x4_max_query(int ncq);
size_t x4_job_bytes(void);
struct RgXPoolArg; struct RgLaunch;
void launch_x4(hipStream_t st, int n_cu, const RgLaunch &G, const RgXPoolArg &X, void *jobs, unsigned long long job_cap, unsigned int *ctr32, unsigned long long *prof);   // G.n_tasks bounds the number of exported strand searches
// K4 a lane per job (k_extl.hip) for the narrow queue of launch_x4's pool; called by launch_x4
void launch_extl(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const RegParams &P, const uint8_t *reads, void *jobs, unsigned int jcap,
                 unsigned int *ctr32, unsigned char *xbase, long long n_upper, unsigned long long *prof, unsigned int *rows = nullptr);   // rows: RgXPoolArg::rows
void launch_extl_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, bsx_ext_res_t *res,
                       unsigned int n, unsigned int *ctr32);
void launch_ext4_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_ext_job_t *jobs, bsx_ext_res_t *res,
                       unsigned int n, unsigned int *cursor, int max_qlen);
// K3+C1+C2+C4 fused: one wavefront per strand search, from the dense interval lists of launch_seed to alignment regions.
// Tier 1 keeps its tables in LDS; tiers 2 and 3 run what did not fit over per-wave slabs in HBM (grid * 4 slabs of
// regions_slab_bytes(tier)); a tier appends what it declines for table size to the next tier's list.
size_t regions_slab_bytes(int tier);
// where the LDS tiers leave the chains that survive the filter for launch_c2r (chains -> regions): a byte pool with a bump cursor,
// the block of task t at xoff[t], and the list of tasks that have one
struct RgXPoolArg { unsigned char *base; unsigned long long cap; unsigned long long *cursor; long long *xoff; int *xlist; unsigned int *xcount;
                    int ext;      // ext: the records leave room for the extensions launch_x4 makes ahead of launch_c2r
                    unsigned int *rows; };   // $BSX_PHASES only (else null): the rows each job of launch_x4 ran, in the pool's allocation at base + rgx_rows_offset(cap) (rgx.hpp)
// what every launch over one task list is given: the same at every call site of a tier sequence
struct RgLaunch {
	const DevIndex *ix; const DevScoring *sc; const RegParams *P;
	const uint8_t *reads; const bsx_seed_task_t *tasks; int n_tasks;
	const DevIntv *seeds_dense; const long long *task_off; const int *task_n;   // the dense interval lists
	bsx_region_t *out; unsigned long long out_cap; unsigned long long *out_cursor;   // the region pool
	long long *reg_off; int *reg_n;
	unsigned long long *counters;            // the lane's counter block (ctr_layout.hpp)
	long long *pos_off; unsigned long long *pos;   // launch_occ fills them, the region kernels read them
	bool ext_pk = false;                     // extension rows in packed 16-bit (ext_pk.hpp): the scoring options pass ext_pk_exact_reads()
};
void launch_regions(hipStream_t st, int grid, const RgLaunch &G, unsigned int *task_cursor, int *retry_list, unsigned int *retry_count, int quota,
                    const unsigned char *cls, const RgXPoolArg &X, bool long_reads = false);   // cls[t] != 0: not for this tier (launch_occ)
// the tiers in between: larger LDS tables; each consumes the list of the tier before it and appends to the next one's.  The forms: tables, DP
enum RgMidForm { RG_MID,          // RgMid, RgDpLite: four times the first tier's tables, behind it
                 RG_MID_LONGS,    // RgLongS, RgDpLiteL: tables for a kilobase read, one wave per workgroup
                 RG_MID_LONGB,    // RgLongB, RgDpLite: the larger tables for reads of ordinary length
                 RG_MID_LONGB_L,  // RgLongB, RgDpLiteL: kilobase reads, the larger of the two table sizes
                 RG_MID2 };       // RgMid2, RgDpLite: twice RgMid's tables, the tier behind it
void launch_regions_mid(hipStream_t st, int grid, const RgLaunch &G, const int *list, const unsigned int *count, unsigned int *cursor,
                        int *next_list, unsigned int *next_count, const RgXPoolArg &X, int quota, RgMidForm form);   // quota: strand searches per wave
// chains -> regions for everything the launches above exported; what does not fit its tables goes on next_list (may be null: left to the caller)
enum RgC2rForm { RG_C2R,      // RgC2r: ordinary chunks
                 RG_C2R_L,    // RgC2rL: chunks with long reads or the seed filter
                 RG_C2R_B,    // RgC2rB: larger LDS tables, for what RG_C2R declines
                 RG_C2R_H,    // RgC2rH: the large tables in HBM (`slab` = grid x c2r_hbm_slab_bytes(false)), for what RG_C2R_B declines
                 RG_C2R_HL }; // RgC2rHL: the same for what RG_C2R_L declines (`slab` = grid x c2r_hbm_slab_bytes(true))
void launch_c2r(hipStream_t st, int grid, const RgLaunch &G, const RgXPoolArg &X, unsigned int *cursor, int *next_list, unsigned int *next_count,
                int quota, RgC2rForm form = RG_C2R, void *slab = nullptr);
size_t c2r_hbm_slab_bytes(bool long_form);
// C3 between the tiers and launch_c2r: the seed-SW filter of the exported strand searches it applies to (mem_flt_chained_seeds, memchain.c:537-568)
void launch_seedsw(hipStream_t st, int grid, int n_cu, const RgLaunch &G, const RgXPoolArg &XA, unsigned int *cursor, unsigned int *count_cursor,
                   void *jobs, unsigned int job_cap);
size_t seedsw_job_bytes(void);
// tests (setting sw_form): plain score-only jobs of up to 199 x 199 through the seed filter's two alignments.  launch_swl16_batch: the
// k_swl16 launch of launch_seedsw over the jobs in the order given, sixteen consecutive ones to a wavefront (qlen = 0: an empty job); work:
// n * seedsw_job_bytes() + 16 bytes; false, nothing launched: scoring options ssw16_exact (ssw16_bound.h) refuses.  launch_ssw32_batch: a
// wavefront per job through the 32-bit alignment k_seedsw_apply makes for a seed without room in the job list
bool launch_swl16_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_sw_job_t *jobs, bsx_sw_res_t *res,
                        unsigned int n, void *work);
void launch_ssw32_batch(hipStream_t st, int n_cu, const DevIndex &ix, const DevScoring &sc, const uint8_t *reads, const bsx_sw_job_t *jobs, bsx_sw_res_t *res, unsigned int n);
int regions_long_max_query(void);
void launch_regions_slab(hipStream_t st, int tier, int grid, const RgLaunch &G, const int *list, const unsigned int *count, unsigned int *cursor,
                         void *slabs, int *next_list, unsigned int *next_count, const RgXPoolArg *X = nullptr);   // X: export the chains (as the LDS tiers do) instead of making the regions
// a tier's list put in order of decreasing size (occurrences to visit), longest strand search first: what a launch that lasts as long as its longest one wants
void launch_order_list(hipStream_t st, int *list, const unsigned int *count, const DevIntv *seeds_dense, const long long *task_off, const int *task_n, int max_occ);
// K3 ahead of the region kernels: SA ranks of all occurrences of all strand searches listed into desc (pos_off[t] = where task
// t's start, -1 = none listed), then turned into reference positions in place.  pos_off/pos feed launch_regions*.
void launch_occ(hipStream_t st, int n_cu, const RgLaunch &G, int max_occ, unsigned long long desc_cap, unsigned long long *cursor, unsigned char *cls,
                unsigned long long *start = nullptr, int *early_list = nullptr, unsigned int *early_count = nullptr);   // desc = G.pos; early_list: the strand searches only the last HBM tier's tables hold are listed there (cls 3; the first tier then skips them)   // start: an 8-byte device slot; set = only the ranks this call adds to the pool are walked   // cls[t]: the first tier whose interval/occurrence tables hold task t
// out[j] = SA[j * intv] for j < n, from the (sparser) samples ix currently holds: the denser suffix-array sample kept in HBM
void launch_sa_dense(hipStream_t st, int n_cu, const DevIndex &ix, int parent, unsigned int intv, unsigned long long n, unsigned long long *out);
// C5 (k_dedup.hip): mem_sort_deduplicate of every read over the regions of the chunk, a lane per read
int dedup_cap(void);
void launch_dedup(hipStream_t st, const bsx_region_t *regs, const long long *reg_off, const int *reg_n, int n_reads, int per_read,
                  long long l_pac, int max_chain_gap, int opt_w, float mask_level_redun, int *out_n, unsigned char *out_idx,
                  int *long_list = nullptr, unsigned int *long_count = nullptr);   // long_list (2 x n_reads ints) / long_count (2 counters, zeroed): the reads k_dedup_long takes
// ... and a wavefront per read for the reads with more regions than that (up to dedup_long_cap()): 16-bit indices, one list behind the other in pool
int dedup_long_cap(void);
void launch_dedup_long(hipStream_t st, int n_cu, const bsx_region_t *regs, const long long *reg_off, const int *reg_n, int n_reads, int per_read,
                       long long l_pac, int max_chain_gap, int opt_w, float mask_level_redun, const int *long_list, const unsigned int *long_count,
                       int *out_n, long long *out_off, unsigned short *pool, unsigned long long pool_cap, unsigned long long *pool_cursor);

// mate rescue's plan on the device (k_msw.hip): candidates -> jobs (binned for k_swl) + a record per pair
size_t msw_pair_bytes(void);
int msw_hist_bins(void);
void launch_msw_plan(hipStream_t st, int n_cu, const DevIndex &ix, const bsx_region_t *regs, const long long *r_off, const int *r_n,
                     const int *dd_n, const unsigned char *dd_idx, const long long *dd_off, const unsigned short *dd_pool, int dd_cap, int per_read,
                     const unsigned int *roff, int low, int high, int pen_unpaired, int max_matesw, int min_seed_len, int a, int p0, int n_pairs,
                     bsx_sw_job_t *jobs, unsigned int job_cap, unsigned int *job_count, unsigned int *hist, void *table, int *order);
