// Internal interface between the kernels (bgv_kernels.hip) and the host
// orchestration behind the C ABI (the bgv_api*.hip units, bgv_host.h).  Not installed.
#pragma once
#include "pairing.h"
#include "rng.h"
#include "bits_expand.h"
#include "batch_tail.h"

namespace bgv {

// internal per-set codes beyond blst's (see include/bgv.h bgv_set_code)
enum : int32_t {
  C_INDEX_RANGE = 9,
  C_EMPTY_JOB = 10,
};

// A set on the complement path of bgv_verify_bits (bits_expand.h
// bits_complement): its window of the list's resident prefix sums.  The
// aggregate key is *hi - *lo minus the gathered (absent) members.  hi == NULL:
// the set is on the direct path.
struct pk_window {
  const g1j* lo;
  const g1j* hi;
};

// HBM layout of one batch (device pointers).  All arrays are dense and
// indexed by set (or job); see include/bgv.h bgv_batch for their meaning.
struct dev_batch {
  uint32_t n_sets, n_jobs, n_raw, table_n;
  uint32_t span_log2;    // per-job reduction tree covers 2^span_log2 sets
  uint32_t chunk_bound;  // upper bound of pubkey chunks (grid of k_pk_chunk)
  uint32_t miller_coop;     // set pairs: 0 one-lane Miller loop (k_miller), 2 / 4 the two- / four-lane loop
                            // (k_miller_duo / k_miller_quad), else lanes per pair of the cooperative loop (miller_coop.h: 6, 18 or 36)
  uint32_t job_lanes;       // (-G1, S_job) pairs: lanes per pair of the cooperative loop (6, 18 or 36)
  uint32_t pairs_per_item;  // Miller pairs sharing one accumulator (1, or 2 for batches that fill the GPU)
  uint32_t msm;             // sum r_i sigma_i: 0 per-set [r_i] sigma_i + tree (latency mode: cooperative, with the checks),
                            // 1 per-job fused MSM (k_msm_fused), 2 (job, window)-lane MSM (k_msm_bucket), 3 one-lane per-set
                            // scaling + tree with the subgroup checks deferred (latency-mode hash), 4 (job, window,
                            // digit)-lane MSM (k_msm_digit)
  uint32_t split;           // 1: latency mode: hash maps on two lanes per set, subgroup check beside [r_i] sigma_i
  uint32_t clear_lanes;     // latency mode: lanes per point of the cofactor clearing (9, or 3)
  uint32_t miller_kv;       // latency mode: 0, or the slots S of the two-pair Miller loop in views (k_miller_kv, 3 S lanes)
  uint32_t maps_early;      // latency mode: k_hash_map already launched by prepare() (bgv_api.hip early_maps)
  uint32_t prefold_log2;    // >0: two-level job fold, groups of 2^prefold_log2 sets (k_job_prefold); 0: one level
  uint32_t lines;           // one-lane Miller loop over fixed-argument lines: the hash stream stores every set's
                            // 68 unevaluated lines (launch_lines), k_miller evaluates them at P (pairing.h)
  uint32_t defer_from;      // defer_grp: sets below it are checked in ST_SIG as usual, the rest later (multiple of 64)
  uint32_t defer_grp;       // bulk mode: ST_SIG only decodes; the G2 subgroup check runs beside the Miller loops
                            // (launch_sig_check) and its verdicts reach the job codes before the fold (launch_sig_fixup)
  uint32_t steps_slice;     // >0: per-step line products (pairing.h miller_step_lines): the work items are slices of at
                            // most steps_slice sets of a job, k_miller_steps writes f_step and k_job_chain runs the
                            // job recurrence (bgv_cfg.miller_steps); 0: the item loop (k_miller)
  uint32_t steps_dbg;       // bgv_debug_stages on the steps path: k_job_chain also leaves the job's set product at
                            // f_set[first set] and 1 at its other sets
  uint32_t batch_tail;      // steps path: the batch-first tail (bgv_batch_tail): the batch verdict comes from ONE (-G1,
                            // S_batch) pair and ONE recurrence over the step products of all slices; the per-job sums,
                            // pairs and chains run behind k_batch_final and only when it failed
  const uint32_t* job_off;
  const uint32_t* pk_off;
  const uint32_t* pk_idx;
  const g1a* raw_pks;  // Montgomery affine (converted by k_raw_pks)
  const g1a* table;    // index2pubkey, Montgomery affine, 96 B per validator
  const uint8_t* msgs;
  const uint8_t* sigs;
  const uint32_t* sig_len;
  const uint64_t* scalars;
  // bgv_verify_bits on a context with resident sums: per-set windows (NULL for
  // every other entry point and for contexts without sums).  A complement set
  // gets one extra chunk, its first: the window difference; its other chunks
  // hold absent members and are stored negated (k_chunk_count, k_pk_chunk)
  const pk_window* win;
};

// Per-batch intermediates resident in HBM.
struct dev_work {
  g2a* sig_aff;       // decoded signature (affine)
  uint32_t* sig_inf;  // signature is the identity
  int32_t* sig_code;  // parse / subgroup outcome
  g2a* h_aff;         // H(m)
  g2j* q_part;        // [2 n_sets] split mode: the two mapped points of every message
  uint32_t* sig_grp;  // split / defer_grp mode: signature passed the subgroup check
  g2j* msm_bucket;    // [n_jobs * 16 windows * 15 buckets] (msm = 2)
  uint32_t* msm_mask; // [n_jobs * 16] occupied buckets of each (job, window)
  g2j* msm_win;       // [n_jobs * 16] window sums (msm = 2, 4)
  uint32_t* chunk_off;  // [n_sets + 1] scan of per-set pubkey chunk counts
  uint32_t* chunk_set;  // set of every chunk
  g1j* pk_part;         // per-chunk partial sums
  g1a* rpk_aff;       // [r_i] aggregated pubkey, affine
  g1a* pk_agg;        // aggregated pubkey before scaling, affine (bgv_debug_stages only; else NULL)
  int32_t* pk_code;
  g2j* rsig;          // [r_i] sigma_i
  uint32_t* set_job;  // job id of every set
  uint32_t* item_off; // [n_jobs + 1] scan of Miller work items per job (2 sets each)
  uint32_t* item_job; // job of every Miller work item
  g2j* win_tmp;       // batch-first tail: the window sums over the jobs, two regions (launch_batch_sig)
  g2a* s_aff;         // per job: sum [r_i] sigma_i, affine; slot n_jobs: S_batch (batch-first tail)
  uint32_t* s_inf;
  fp2_t* lines;       // [68 steps][3][n_sets] unevaluated Miller lines of H(m_i) (dev_batch.lines)
  fp12_t* f_step;     // [items][68] per (slice, step) line products (dev_batch.steps_slice)
  fp12_t* f_fold;     // batch-first tail: per-step products over groups of slices, two regions (launch_batch_chain)
  fp12_t* f_set;      // per pair Miller value: n_sets set pairs, then n_jobs (-G1, S_job) pairs, then (-G1, S_batch)
  fp12_t* f_job;      // per-job Miller product (incl. the -G1 pair)
  fp12_t* f_batch;    // batch product scratch [n_jobs]; the product ends in f_batch[0]
  fp12_t* f_tmp;      // batch fold ping-pong [ceil(n_jobs / 8)]
  int32_t* job_code;
  int32_t* job_result;
  int32_t* set_code;
  fp12_t* f_part;     // conversion scratch for partials
  uint32_t* flags;    // [0] = whole batch verified; [1] pair classes: an identity class; [FLAG_CODES_KEPT]; [4] bgv_combine_final
};
// batch-first tail under deferred checks: 1 while no check has rejected a job that k_msm_window (job_code16) accepted
constexpr uint32_t FLAG_CODES_KEPT = 2;

enum Stage {
  ST_SIG = 0,
  ST_HASH,
  ST_PK,        // chunked gather + partial sums from the HBM table (k_pk_chunk)
  ST_PK_SCALE,  // per set: fold the chunk sums, [r_i] PK_i, affine (k_pk)
  ST_SIG_SCALE,
  ST_S_TREE,
  ST_MILLER,
  ST_MILLER_JOBS,
  ST_F_TREE,
  ST_BATCH_PROD,
  ST_BATCH_FINAL,
  ST_JOB_FINAL,
  ST_SET_CODES,
  ST_COUNT
};

#ifdef __HIPCC__
BGV_HD bool g1a_is_zero(const g1a& p) { return fp_is_zero(p.x) && fp_is_zero(p.y); }

// row of the pubkey table (or of the raw side table for bit 31); an index
// past either flags range_err and yields the identity
__device__ __forceinline__ void load_pk(g1a& out, const dev_batch& b, uint32_t idx, bool& range_err) {
  if (idx & 0x80000000u) {
    const uint32_t r = idx & 0x7fffffffu;
    if (r >= b.n_raw) { range_err = true; fp_set_zero(out.x); fp_set_zero(out.y); return; }
    out = b.raw_pks[r];
  } else {
    if (idx >= b.table_n) { range_err = true; fp_set_zero(out.x); fp_set_zero(out.y); return; }
    out = b.table[idx];
  }
}
#endif

// keys per chunk of the balanced pubkey gather (k_pk_chunk)
constexpr uint32_t PK_CHUNK = 32;

void launch_pk_gather(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_gather.hip
void launch_raw_pks(hipStream_t st, const uint8_t* raw, g1a* out, uint32_t n);
void launch_table_from_compressed(hipStream_t st, const uint8_t* in, g1a* out, uint32_t n, int32_t* codes);
void launch_table_from_uncompressed(hipStream_t st, const uint8_t* in, g1a* out, uint32_t n, int32_t* codes);
void launch_table_export(hipStream_t st, const g1a* tab, uint8_t* out, uint32_t n);
void launch_pk_validate(hipStream_t st, const uint8_t* in, uint32_t n, int32_t* codes);
void launch_hash_maps(hipStream_t st, const dev_batch& b, const dev_work& w);  // prepare(): before the set-up
void launch_prep(hipStream_t st, const dev_batch& b, const dev_work& w);  // before ST_PK / ST_MILLER
void launch_stage(hipStream_t st, int stage, const dev_batch& b, const dev_work& w);
void launch_miller(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_miller.hip
void launch_lines(hipStream_t st, const dev_batch& b, const dev_work& w);   // bgv_miller.hip
void launch_miller_steps(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_miller.hip
// upper bound of the work items of a batch taken `per` sets at a time: sum ceil(k_j / per) <= n_sets / per + n_jobs
inline uint32_t miller_items_bound(const dev_batch& b, uint32_t per) { return b.n_sets / per + b.n_jobs; }
void launch_miller_duo(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_miller.hip
void launch_miller_quad(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_miller.hip
void launch_sig_check(hipStream_t st, const dev_batch& b, const dev_work& w);   // subgroup checks only (sig_grp)
void launch_sig_fixup(hipStream_t st, const dev_batch& b, const dev_work& w);   // k_sig_fix + k_job_recode
void launch_sig_split_coop(hipStream_t st, const dev_batch& b, const dev_work& w);   // bgv_latency.hip
void launch_hash_clear_coop(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_latency.hip
void launch_hash_clear_trio(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_latency.hip
void launch_s_level_coop(hipStream_t st, const dev_batch& b, const dev_work& w, uint32_t s);  // bgv_latency.hip
void launch_msm_job_coop(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_latency.hip
void launch_pk_coop(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_latency.hip
void launch_miller_kv(hipStream_t st, const dev_batch& b, const dev_work& w);  // bgv_miller.hip
void launch_fp12_tail(hipStream_t st, int stage, const dev_batch& b, const dev_work& w);  // bgv_tail.hip
void launch_batch_sig_redo(hipStream_t st, const dev_batch& b, const dev_work& w);  // batch-first tail, behind launch_sig_fixup
void launch_job_chain_retry(hipStream_t st, const dev_batch& b, const dev_work& w);  // k_job_chain behind flags[0]
void launch_combine_final(hipStream_t st, const fp12_t* parts, uint32_t n, uint32_t* flag);
void launch_final_exp_many(hipStream_t st, const fp12_t* in, fp12_t* out, uint32_t n);  // bgv_debug_stages
void launch_export_g1a(hipStream_t st, const g1a* in, uint8_t* out96, uint32_t n);
void launch_export_g2a(hipStream_t st, const g2a* in, uint8_t* out192, uint32_t n);
void launch_fp12_convert(hipStream_t st, const fp12_t* in, fp12_t* out, uint32_t n, bool to_mont);
void launch_gen_keys(hipStream_t st, g1a* table, uint32_t* sk, uint32_t first, uint32_t n, uint64_t seed);
void launch_gen_sign(hipStream_t st, const dev_batch& b, const uint32_t* sk, uint8_t* out);
void launch_fp_ops(hipStream_t st, const fp_t* ab, fp_t* out, uint32_t n);
void launch_g2_decode_dbg(hipStream_t st, const uint8_t* sigs192, const uint32_t* sig_len, uint8_t* out192, int32_t* codes,
                         uint32_t n);
void launch_bench_fpmul(hipStream_t st, fp_t* io, uint32_t lanes, uint32_t iters);
void launch_gen_scalars(hipStream_t st, const uint32_t key[8], const uint32_t nonce[3], uint64_t* out, uint32_t n);
void launch_bench_mad(hipStream_t st, uint64_t* io, uint32_t lanes, uint32_t iters);

// ---- same-message batches (bgv_verify_same_message, bgv_same_msg.hip) -------
// Single-pubkey sets grouped by message; every group is cut into segments of
// at most SM_SEG sets (msm_g1.h).  A segment is a job of the G2 bucket MSM
// over the real sets and one set = one job of the virtual batch that runs the
// Miller loops, folds and final exponentiations (bgv_api_sm.hip).
enum : int32_t {
  C_SEG_DEAD = 10,   // no set of the segment survived: nothing to pair, nothing to retry
  C_SEG_RETRY = 11,  // sum r_i pk_i is the identity: the sets are decided on their own
};
struct sm_view {
  uint32_t n_sets, n_segs, n_groups, n_raw, table_n;
  const uint32_t* seg_off;    // [n_segs + 1]
  const uint32_t* seg_group;  // [n_segs]
  const uint32_t* pk_idx;     // [n_sets]
  const g1a* raw_pks;
  const g1a* table;
  const uint64_t* scalars;
  const int32_t* sig_code;    // k_sig outcome of every set
  const uint32_t* sig_inf;
  uint32_t* skip;             // [n_sets] 1: the set is left out of its segment's sums
  int32_t* set_code;          // [n_sets] bgv_set_code of a rejected set
  g1j* win;                   // [n_segs * 16] window sums
  g1a* p_seg;                 // [n_segs] sum r_i pk_i, affine (the virtual batch's rpk_aff)
  int32_t* seg_code;          // [n_segs] C_OK, C_SEG_DEAD or C_SEG_RETRY
  const g2a* h_group;         // [n_groups] H(m_g)
  g2a* h_seg;                 // [n_segs] the virtual batch's h_aff
  int32_t* pk_code_v;         // [n_segs] the virtual batch's pk_code
  int32_t* job_code_v;        // [n_segs] the virtual batch's job_code
  const g2a* s_seg;           // [n_segs] sum r_i sigma_i (the per-job MSM over the real sets)
  const uint32_t* s_inf;
  // aggregate sets (bgv_verify_same_message_agg; NULL otherwise)
  const g1j* pk_set;           // [n_sets] PK_i = sum_j pk_ij, Jacobian; the identity for a rejected key
  const int32_t* pk_set_code;  // [n_sets] key code of k_sma_set_sum
};
// per-set retry of failing segments: set list[k] becomes set k = job k of an ordinary batch
struct sm_retry {
  uint32_t n;
  const uint32_t* list;        // [n] set index
  const uint32_t* list_group;  // [n] its group
  const uint32_t* pk_idx;
  const uint8_t* msgs;         // [n_groups][32]
  const uint8_t* sigs;
  const uint32_t* sig_len;
  const uint64_t* scalars;
  uint32_t* o_iota;            // [n + 1] job and pubkey offsets
  uint32_t* o_idx;
  uint8_t* o_msgs;
  uint8_t* o_sigs;
  uint32_t* o_len;
  uint64_t* o_scalars;
};
// split retry (bgv_sm_retry mode 1, sm_split.h), level 1: the surviving sets of
// the retried segments compacted into buffers of their own, set list[t] as set
// t, so that the sum kernels run over them with seg_off = the sub offsets
struct sm_split {
  uint32_t n, n_subs;
  const uint32_t* list;        // [n] set index
  const uint32_t* list_group;  // [n] its group
  const uint32_t* sub_off;     // [n_subs + 1] offsets into list
  const uint32_t* pk_idx;      // one key per set (else NULL)
  const g1j* pk_set;           // aggregate sets: PK_i (else NULL)
  const uint64_t* scalars;
  const g2a* sig_aff;          // the first pass's decoded signatures
  uint32_t* o_idx;             // [n] (one key per set)
  g1j* o_pk;                   // [n] (aggregate sets)
  uint64_t* o_scalars;         // [n]
  g2a* o_sig;                  // [n]
  uint32_t* o_skip;            // [n] zero: every set of the list survived
  uint32_t* o_sub_group;       // [n_subs] the group of every sub
};
// level 2: leaf t (set leaf[t] of group leaf_group[t]) as set t = job t of a
// virtual batch, nothing scaled: (pk_i, H(m_g)) and (-G1, sigma_i)
struct sm_leaves {
  uint32_t n, n_raw, table_n;
  const uint32_t* leaf;        // [n] set index
  const uint32_t* leaf_group;  // [n] its group
  const uint32_t* pk_idx;      // one key per set (else NULL)
  const g1a* raw_pks;
  const g1a* table;
  const g1j* pk_set;           // aggregate sets: PK_i (else NULL)
  const g2a* sig_aff;
  const g2a* h_group;
  g1a* rpk_aff;                // [n] the virtual batch's arrays
  g2a* h_aff;
  g2a* s_aff;
  uint32_t* s_inf;
  int32_t* pk_code;
  int32_t* job_code;
  uint32_t* iota;              // [n + 1] its job offsets
};
void launch_sm_split_gather(hipStream_t st, const sm_split& q);
void launch_sm_split_leaves(hipStream_t st, const sm_leaves& q);
void launch_sm_classify(hipStream_t st, const sm_view& v);
void launch_sm_g1_sum(hipStream_t st, const sm_view& v);
void launch_sm_apply(hipStream_t st, const sm_view& v);
void launch_sm_group_sums(hipStream_t st, const sm_view& v, const uint32_t* group_seg, g1a* p_group, g2a* s_group);
void launch_sm_retry_gather(hipStream_t st, const sm_retry& r);
// aggregate sets: the per-set fold of the gather's chunk sums (b, w: the real
// sets as a dev_batch view, after launch_prep and launch_pk_gather), then the
// stages above over pk_set instead of table rows
void launch_sma_set_sum(hipStream_t st, const dev_batch& b, const dev_work& w, g1j* pk_set, int32_t* pk_set_code);
void launch_sma_classify(hipStream_t st, const sm_view& v);
void launch_sma_g1_sum(hipStream_t st, const sm_view& v);
void launch_sma_pk_aff(hipStream_t st, const g1j* pk_set, g1a* out, uint32_t n);
void launch_sma_retry_gather(hipStream_t st, const sm_retry& r, const g1j* pk_set, g1a* o_pk);
// bgv_verify_same_message_aggregate: the unweighted signature sum of every
// group, compressed (sig_agg.h; k_sm_sig_seg, k_sm_sig_group in bgv_sig_agg.hip)
struct sig_agg_view;
void launch_sm_sig_agg(hipStream_t st, const sig_agg_view& v);

// ---- committee bitfields over resident index lists (bgv_verify_bits, bgv_bits.hip)
struct bits_args {
  uint32_t n_sets;
  const bits_src* src;  // [n_sets]
  bits_view v;
  uint32_t* pk_off;     // [n_sets + 1]: per-set key counts, then their scan
  uint32_t* pk_idx;     // the expansion
  uint32_t cap;         // entries of pk_idx
  // contexts with resident sums (else NULL): the per-set windows k_bits_count
  // writes; pk_off then counts gathered keys.  On-device batches of such a
  // context (else NULL) also get two counters k_bits_count adds to, zeroed by
  // the caller: tally[0] the batch's participating keys (sum of pop and
  // explicit lengths), tally[1] the sets on the complement path; host
  // batches have both from the host check
  pk_window* win;
  uint32_t* tally;
};
void launch_bits_count(hipStream_t st, const bits_args& a);
void launch_bits_expand(hipStream_t st, const bits_args& a);
// resident prefix sums of an index list (bgv_index_list_sums, bgv_sums.hip):
// sums[k] = sum of table[list[j]] for j < k, k = 0 .. n, Jacobian; tmp holds
// sums_tmp_entries(n) entries of scratch
size_t sums_tmp_entries(uint32_t n);
void launch_list_sums(hipStream_t st, const g1a* table, uint32_t table_n, const uint32_t* list, uint32_t n, g1j* sums,
                      g1j* tmp);
void launch_sums_export(hipStream_t st, const g1j* sums, uint8_t* out96, uint32_t n);
// exclusive scan of a[0..n) in place, total at a[n] (bgv_kernels.hip k_scan)
void launch_scan(hipStream_t st, uint32_t* a, uint32_t n);

// ---- message classes of a bulk batch (bgv_cfg.hash_dedup, bgv_dedup.hip) -----
// Sets with equal signing roots form a class; its representative is hashed and
// the other members copy H(m).  Kept out of dev_batch / dev_work: those are
// kernel arguments of every other kernel.
constexpr uint32_t MSG_EMPTY = 0xffffffffu;  // a free slot of the table (hipMemsetAsync 0xff)
struct msg_classes {
  uint32_t n_sets;
  uint32_t mask;        // slots of the table - 1; the table holds a power of two >= 2 n_sets slots
  uint64_t key;         // per-call key of the slot mix (getrandom)
  const uint8_t* msgs;  // [n_sets][32]
  uint32_t* table;      // [mask + 1] MSG_EMPTY, or the set that claimed the slot
  uint32_t* rep;        // [n_sets] representative of every set (rep[rep[i]] == rep[i])
  uint32_t* uniq;       // [n_sets] the representatives, compacted, in no particular order
  uint32_t* n_uniq;     // their count (zeroed per call)
  g2a* h_aff;           // dev_work.h_aff
};
void launch_msg_dedup(hipStream_t st, const msg_classes& c);     // index-only set-up, beside launch_prep
void launch_hash_classes(hipStream_t st, const msg_classes& c);  // ST_HASH of the bulk layout: k_hash_reps, k_hash_spread

// ---- pair classes of a bulk batch (bgv_pair_merge, pair_merge.h, bgv_pair_merge.hip)
// One set-pair Miller loop per (job, signing root).  The caller clears table
// (0xff), head (0xff), class_off, cls_job and *ident (0) on the same stream.
struct pair_classes;
void launch_pair_classes(hipStream_t st, const pair_classes& p);  // index-only set-up, after launch_msg_dedup
void launch_pair_h(hipStream_t st, const pair_classes& p, const g2a* h_aff);  // hash stream, after launch_hash_classes
void launch_pair_lines(hipStream_t st, const pair_classes& p, fp2_t* lines);  // launch_lines, one lane per class
void launch_pair_sum(hipStream_t st, const pair_classes& p, const g1a* rpk_aff, const int32_t* pk_code);  // after ST_PK_SCALE

}  // namespace bgv
