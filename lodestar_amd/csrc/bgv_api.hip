// Host side of the C ABI declared in include/bgv.h: context, HBM-resident
// pubkey table, batch staging and the stage pipeline on one HIP stream.
//
// Reference behaviour re-created (packages/beacon-node/src/chain/bls/):
//   * multithread/worker.ts:30-106  one batch check, per-job fallback
//   * maybeBatch.ts:16-38           job verdict = AND of its sets; parse
//                                    errors reject the job
//   * utils.ts:5-16                 pubkey aggregation (now on the device)
//   * multithread/index.ts:193-214  close()
#include <sys/random.h>
#include <string.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <optional>
#include <vector>
#include <string>

#include "bgv_internal.h"
#include "msm_g1.h"
#include "sig_agg.h"
#include "pair_merge.h"
#include "sm_split.h"
#include "../../include/bgv.h"

using namespace bgv;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) return fail(BGV_E_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <class T>
struct dbuf {
  T* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return 0;
    size_t c = cap ? cap : 64;
    while (c < n) c *= 2;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc((void**)&p, c * sizeof(T)) != hipSuccess) return fail(BGV_E_HIP, "hipMalloc(%zu) failed", c * sizeof(T));
    cap = c;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct bgv_ctx {
  int device = 0;
  bgv_cfg cfg;            // pipeline overrides (bgv_open_cfg; all "auto" from bgv_open)
  bool timed = true;      // the last run_stages recorded per-stage events
  int run_from = 0, run_to = 0;  // stage range of the last run_stages (bgv_last_stats)
  dev_batch last_d = {};         // the last run_stages batch (its pipeline variant for bgv_stats)
  hipStream_t st = nullptr, st_hash = nullptr, st_pk = nullptr;
  bool busy = false;  // prepare(): another batch of this process was in flight on the device
  hipStream_t st_chk = nullptr;  // deferred subgroup checks, low priority (BGV_CHK_STREAM)
  hipEvent_t ev[ST_COUNT + 1] = {};   // ev[s] = start of stage s on its stream
  hipEvent_t ev_end[ST_COUNT] = {};   // end of stage s on its stream
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_prep = nullptr;       // end of launch_prep (latency batches fork the hash leg before it)
  hipEvent_t ev_sigdec = nullptr;     // defer_grp: signatures decoded (the checks may start)
  hipEvent_t ev_grp = nullptr;        // defer_grp: subgroup checks done (the code fix-up may start)
  hipEvent_t ev_maps = nullptr;       // early_maps: the hash maps on st_hash are done
  hipEvent_t ev_chk = nullptr;        // pubkey scaling done: the deferred checks may start on st_chk
  hipEvent_t ev_dep[ST_COUNT] = {};   // untimed cross-stream dependencies (latency batches)
  // index2pubkey table (grown by copy) and synthetic secret keys
  g1a* table = nullptr;
  uint32_t table_n = 0, table_cap = 0;
  dbuf<uint32_t> sk;
  // staging for host batches: every host array of a batch is packed into one
  // pinned buffer and crosses PCIe in ONE copy (pageable copies cost ~30-90 us
  // each on the C2 critical path); results come back through pinned memory too
  dbuf<uint8_t> stage_dev;
  uint8_t* pin_in = nullptr;
  uint8_t* pin_out = nullptr;
  size_t pin_in_cap = 0, pin_out_cap = 0;
  hipEvent_t ev_staged = nullptr;  // the last pin_in -> stage_dev copy
  bool staged_pending = false;
  dbuf<uint8_t> raw_in, gen_out;
  dbuf<g1a> pk_tmp;         // bgv_pubkeys_set: decoded rows before they enter the table
  dbuf<int32_t> pk_codes;   // bgv_pubkeys_set: per-key deserialization codes
  std::vector<int32_t> pk_codes_host;
  // host view of the last prepared batch (offsets from the pinned copy or HBM)
  std::vector<uint32_t> jo_host;
  uint32_t pk_total = 0;
  // bgv_partial -> bgv_partial_finish: the shard's intermediates stay resident
  bool partial_pending = false;
  dev_batch part_d;
  dev_work part_w;
  // bgv_debug_stages
  dbuf<g1a> pk_agg;
  dbuf<fp12_t> dbg_fe, dbg_f;
  dbuf<uint8_t> dbg_out;
  dbuf<uint64_t> scalars;
  dbuf<g1a> raw_conv;
  // per-batch intermediates
  dbuf<g2a> sig_aff, h_aff;
  dbuf<uint32_t> sig_inf, flags;
  dbuf<int32_t> sig_code, pk_code, job_code, job_result, set_code;
  dbuf<g1a> rpk_aff;
  dbuf<uint32_t> chunk_off, chunk_set;
  dbuf<g1j> pk_part;
  dbuf<g2j> rsig, q_part;
  dbuf<uint32_t> sig_grp;
  dbuf<fp2_t> lines;
  uint32_t lines_idle = 0;  // batches in a row that did not use the line buffer
  dbuf<fp12_t> f_step;      // per (slice, step) line products (dev_batch.steps_slice); kept and released with lines
  bgv_miller_path miller_path = {};  // bgv_miller_path_stats (prepare_layout)
  dbuf<fp12_t> f_set, f_job, f_batch, f_tmp, f_part;
  dbuf<uint32_t> set_job, s_inf, item_off, item_job;
  dbuf<g2a> s_aff;
  dbuf<g2j> msm_bucket, msm_win;
  dbuf<uint32_t> msm_mask;
  // bgv_verify_same_message
  dbuf<uint32_t> sm_skip, sm_list;
  dbuf<int32_t> sm_zero, sm_seg_code;
  dbuf<g1j> sm_win;
  dbuf<g2a> sm_hg, sm_sg;
  dbuf<g1a> sm_pg;
  dbuf<uint8_t> sm_retry;
  int32_t sm_mode = 0;              // bgv_sm_retry: 0 per-set retry, 1 split retry (sm_split.h)
  bgv_sm_retry_path sm_path = {};   // bgv_sm_retry_stats
  dbuf<uint8_t> sm_split;           // split retry: the compacted sets of level 1, the lists of both levels
  // bgv_verify_same_message_agg
  dbuf<g1j> sma_pk;           // per set: PK_i, Jacobian
  dbuf<int32_t> sma_pk_code;  // per set: its key code
  dbuf<g1a> sma_aff;          // PK_i affine: the retry's sets, or every set for the debug entry
  // bgv_verify_same_message_aggregate
  dbuf<g2j> sag_seg;          // per segment: the unweighted signature sum
  dbuf<uint32_t> sag_cnt;     // per segment, then per group: sets in the sum
  dbuf<int32_t> sag_code;     // per group: the code of its running aggregate
  dbuf<uint8_t> sag_out;      // per group: 96 compressed bytes
  dbuf<uint8_t> sag_valid;    // second pass: the final verdicts
  dbuf<g2a> sag_sig;          // second pass: the decoded signatures, kept across the per-set retry
  hipEvent_t ev_sag[2] = {};  // around the two kernels of the first pass (bgv_sm_agg_ms)
  bool sag_timed = false;
  // resident index lists (bgv_index_list_set) and the expansion of bgv_verify_bits
  uint32_t* idx_list[BGV_MAX_INDEX_LISTS] = {};
  uint32_t idx_list_n[BGV_MAX_INDEX_LISTS] = {};
  dbuf<uint32_t> bits_off, bits_idx;  // pk_off[n_sets + 1] (+ 2 tally words with sums), pk_idx[gathered keys]
  // resident prefix sums (bgv_index_list_sums): n + 1 Jacobian entries per list
  g1j* idx_sums[BGV_MAX_INDEX_LISTS] = {};
  float sums_build_ms = 0.f;  // device time of the last build (ev_bits around its kernels)
  uint32_t idx_list_max[BGV_MAX_INDEX_LISTS] = {};  // largest entry of the list (range check of the sums)
  dbuf<pk_window> bits_win;           // per-set windows of the last bits batch (contexts with sums)
  bool bits_any_sums = false;         // the last bits batch ran with sums resident
  bool bits_on_device = false;        // ... and was an on-device batch (its path counters live in HBM)
  bgv_bits_path bits_path = {};       // path counters of the last bgv_verify_bits
  uint32_t bits_n = 0;                // sets of the last bits batch
  uint32_t bits_extra_chunks = 0;     // window chunks of the last bits batch (an upper bound for on-device batches)
  hipEvent_t ev_bits[2] = {};         // around the expansion kernels (timed runs)
  bool bits_timed = false;
  // message classes of a bulk batch (bgv_cfg.hash_dedup, bgv_dedup.hip)
  dbuf<uint32_t> msg_rep, msg_uniq, msg_tab, msg_cnt;
  msg_classes mc = {};                // the batch's view of them (work_alloc); n_sets == 0: no class pass
  bgv_hash_path hash_path = {};       // bgv_hash_stats
  bool hash_pending = false;          // hash_path.hashes is still the device's n_uniq: fetched with the results
  // pair classes of a bulk batch (bgv_pair_merge, bgv_pair_merge.hip)
  int32_t pair_merge = 0;             // the switch
  bool pm_entry = false;              // inside bgv_verify / bgv_verify_bits / bgv_partial: run_stages records pair_path
  bool pm_call = false;               // ... and the call may merge (off for the unmerged second pass of a fallback)
  dbuf<uint64_t> pm_tab;
  dbuf<uint32_t> pm_slot, pm_slot_idx, pm_off, pm_cls, pm_head, pm_next, pm_job, pm_rep, pm_item_off, pm_item_job;
  dbuf<g1a> pm_p;
  dbuf<int32_t> pm_code;
  dbuf<g2a> pm_h;
  pair_classes pc = {};               // the batch's view of them (work_alloc); n_sets == 0: no class pass
  bgv_pair_path pair_path = {};       // bgv_pair_stats
  bool pair_pending = false;          // pair_path.pairs and the identity flag are still on the device
  bool pair_redo = false;             // the last merged pass met an identity class: its results are void
  // batch-first tail of the steps path (bgv_batch_tail)
  int32_t batch_tail = -1;            // the switch: -1 auto (on wherever the steps path is), 0 off, 1 on
  dbuf<g2j> win_tmp;                  // dev_work.win_tmp
  dbuf<fp12_t> f_fold;                // dev_work.f_fold
  dev_batch tail_d = {};              // the view ST_F_TREE .. ST_BATCH_FINAL of the last run_stages ran over (the pair
  dev_work tail_w = {};               // classes' when merged): bgv_partial_finish launches the retry kernels over it
  bgv_tail_path tail_path = {};       // bgv_tail_stats
  // microbench scratch
  dbuf<fp_t> mb_fp;
  dbuf<uint64_t> mb_u64;
};

// Definitions below take C linkage from their declarations in bgv.h.

int bgv_abi_version(void) { return BGV_ABI_VERSION; }
#ifndef BGV_SRC_HASH
#define BGV_SRC_HASH "unhashed"
#endif
const char* bgv_build_id(void) { return BGV_SRC_HASH; }
const char* bgv_last_error(void) { return g_err.c_str(); }

const char* bgv_set_code_name(int code) {
  switch (code) {
    case 0: return "BLST_SUCCESS";
    case 1: return "BLST_BAD_ENCODING";
    case 2: return "BLST_POINT_NOT_ON_CURVE";
    case 3: return "BLST_POINT_NOT_IN_GROUP";
    case 4: return "BLST_AGGR_TYPE_MISMATCH";
    case 5: return "BLST_VERIFY_FAIL";
    case 6: return "BLST_PK_IS_INFINITY";
    case 7: return "BLST_BAD_SCALAR";
    case 8: return "BLST_INVALID_SIZE";
    case 9: return "BGV_INDEX_RANGE";
    case 10: return "EMPTY_SIGNATURE_SET";
    default: return "BGV_UNKNOWN";
  }
}

const char* bgv_stage_name(int stage) {
  static const char* names[ST_COUNT] = {"sig_decode_subgroup", "hash_to_g2",       "pk_gather",
                                        "pk_aggregate_scale",  "sig_scale",        "sig_sum_tree",
                                        "miller_loop",         "miller_loop_jobs", "miller_product_tree",
                                        "batch_product",       "batch_final_exp",  "job_final_exp",
                                        "set_codes"};
  return (stage >= 0 && stage < ST_COUNT) ? names[stage] : "unknown";
}

void bgv_cfg_default(bgv_cfg* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->split = cfg->miller = cfg->msm = cfg->prefold = cfg->lines = cfg->defer_pct = cfg->timing = cfg->clear_lanes = -1;
  cfg->miller_kv = cfg->hash_dedup = cfg->miller_steps = -1;
  cfg->job_lanes = cfg->pairs = cfg->cu_split = 0;
}

int bgv_open(int device, bgv_ctx** out) { return bgv_open_cfg(device, nullptr, out); }

int bgv_open_cfg(int device, const bgv_cfg* cfg, bgv_ctx** out) {
  if (!out) return fail(BGV_E_INVALID_ARG, "out is NULL");
  *out = nullptr;
  bgv_cfg k;
  bgv_cfg_default(&k);
  if (cfg) {
    if (cfg->struct_size != sizeof k) return fail(BGV_E_INVALID_ARG, "bgv_cfg.struct_size %u, expected %zu", cfg->struct_size, sizeof k);
    k = *cfg;
    auto lanes_ok = [](int v) { return v == 6 || v == 18 || v == 36; };
    if (k.miller != -1 && k.miller != 1 && k.miller != 2 && k.miller != 4 && !lanes_ok(k.miller)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.miller %d", k.miller);
    if (k.job_lanes != 0 && !lanes_ok(k.job_lanes)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.job_lanes %d", k.job_lanes);
    if (k.pairs < 0 || k.pairs == 3 || k.pairs > 4) return fail(BGV_E_INVALID_ARG, "bgv_cfg.pairs %d", k.pairs);
    if (k.msm < -1 || k.msm > 4) return fail(BGV_E_INVALID_ARG, "bgv_cfg.msm %d", k.msm);
    if (k.clear_lanes != -1 && k.clear_lanes != 1 && k.clear_lanes != 3 && k.clear_lanes != 9)
      return fail(BGV_E_INVALID_ARG, "bgv_cfg.clear_lanes %d", k.clear_lanes);
    if (k.miller_kv != -1 && k.miller_kv != 0 && k.miller_kv != 2 && k.miller_kv != 3 && k.miller_kv != 6 && k.miller_kv != 9)
      return fail(BGV_E_INVALID_ARG, "bgv_cfg.miller_kv %d", k.miller_kv);
    if (k.defer_pct < -1 || k.defer_pct > 100) return fail(BGV_E_INVALID_ARG, "bgv_cfg.defer_pct %d", k.defer_pct);
    auto tri_ok = [](int v) { return v >= -1 && v <= 1; };
    if (!tri_ok(k.split)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.split %d", k.split);
    if (!tri_ok(k.prefold)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.prefold %d", k.prefold);
    if (!tri_ok(k.lines)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.lines %d", k.lines);
    if (!tri_ok(k.timing)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.timing %d", k.timing);
    if (!tri_ok(k.hash_dedup)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.hash_dedup %d", k.hash_dedup);
    if (!tri_ok(k.miller_steps)) return fail(BGV_E_INVALID_ARG, "bgv_cfg.miller_steps %d", k.miller_steps);
    if (k.cu_split < -64 || k.cu_split > 64) return fail(BGV_E_INVALID_ARG, "bgv_cfg.cu_split %d (|N| <= 64 CUs)", k.cu_split);
    // two pairs per item exist only in the one-lane loop
    if (k.pairs >= 2 && k.miller != -1 && k.miller != 1)
      return fail(BGV_E_INVALID_ARG, "bgv_cfg.pairs 2 needs the one-lane Miller loop (miller %d)", k.miller);
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(BGV_E_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(BGV_E_NO_DEVICE, "device %d out of range (%d devices)", device, n);
  HIPCHK(hipSetDevice(device));
  // CU partition between a priority context (the |N| highest CU ids) and the
  // bulk contexts (the rest): a single set's few waves then never queue
  // behind a resident bulk batch (k_hash alone holds two waves on every SIMD
  // for ~16 ms at C4).  Streams with a CU mask take no priority.  Mask bit i
  // is CU i / 8 of XCC i % 8, in shader engine (i / 8) % 4
  // (tools/cu_mask_probe.hip, probed on MI355X: 8 XCCs x 32 CUs), and an XCC
  // left without any bit runs on all of its CUs, so N must be a multiple of
  // the XCC count: the highest 8k ids then take k CUs from every XCC (32: one
  // per SE).  Any other layout is refused rather than half-isolated.
  // Workgroups go round-robin over the SEs, so the bulk side runs at the pace
  // of an SE that lost a CU: C4 +13% for 8, 16 or 32 reserved CUs alike
  // (profiles/r05h_cu_split.txt).
  std::vector<uint32_t> mask;
  if (k.cu_split != 0) {
    int n_cu = 0, n_xcc = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (hipDeviceGetAttribute(&n_xcc, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) n_xcc = 0;
    const int reserve = k.cu_split > 0 ? k.cu_split : -k.cu_split;
    if (n_xcc != 8 || n_cu != 256)
      return fail(BGV_E_INVALID_ARG, "bgv_cfg.cu_split %d: the CU-mask layout is probed for 8 XCCs x 32 CUs (device: %d XCCs, %d CUs)",
                  k.cu_split, n_xcc, n_cu);
    if (reserve % n_xcc != 0)
      return fail(BGV_E_INVALID_ARG, "bgv_cfg.cu_split %d: |N| must be a multiple of the %d XCCs (an XCC without a mask bit runs on all its CUs)",
                  k.cu_split, n_xcc);
    mask.assign((size_t)(n_cu + 31) / 32, 0u);
    for (int cu = 0; cu < n_cu; cu++) {
      const bool reserved = cu >= n_cu - reserve;
      if (reserved == (k.cu_split > 0)) mask[cu / 32] |= 1u << (cu % 32);
    }
  }
  bgv_ctx* c = new bgv_ctx();
  c->device = device;
  c->cfg = k;
  // on a failure below, the streams and events made so far go with the context
  struct guard_t {
    bgv_ctx*& c;
    ~guard_t() { if (c) bgv_close(c); }
  } guard{c};
  // hash -> set-pair Miller is the critical path: its stream (and the pubkey
  // stream feeding it) get the highest priority, signature decode/scaling the
  // lowest (it only feeds the signature tree and the 1 pair per job)
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  if (k.cu_split == 0) {
    HIPCHK(hipStreamCreateWithPriority(&c->st, hipStreamNonBlocking, prio_lo));
    HIPCHK(hipStreamCreateWithPriority(&c->st_hash, hipStreamNonBlocking, prio_hi));
    HIPCHK(hipStreamCreateWithPriority(&c->st_pk, hipStreamNonBlocking, prio_hi));
    HIPCHK(hipStreamCreateWithPriority(&c->st_chk, hipStreamNonBlocking, prio_lo));
  } else {
    hipStream_t* sts[4] = {&c->st, &c->st_hash, &c->st_pk, &c->st_chk};
    for (hipStream_t* p : sts) HIPCHK(hipExtStreamCreateWithCUMask(p, (uint32_t)mask.size(), mask.data()));
  }
  for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
  for (auto& e : c->ev_end) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventCreate(&c->ev_fork));
  HIPCHK(hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming));
  for (auto& e : c->ev_dep) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_sigdec, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_grp, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_maps, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_chk, hipEventDisableTiming));
  for (auto& e : c->ev_bits) HIPCHK(hipEventCreate(&e));
  for (auto& e : c->ev_sag) HIPCHK(hipEventCreate(&e));
  *out = c;
  c = nullptr;  // owned by the caller now
  return BGV_OK;
}

int bgv_close(bgv_ctx* c) {
  if (!c) return BGV_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->st);
  (void)hipStreamSynchronize(c->st_hash);
  (void)hipStreamSynchronize(c->st_pk);
  (void)hipStreamSynchronize(c->st_chk);
  for (auto& e : c->ev) (void)hipEventDestroy(e);
  for (auto& e : c->ev_end) (void)hipEventDestroy(e);
  (void)hipEventDestroy(c->ev_fork);
  (void)hipEventDestroy(c->ev_staged);
  for (auto& e : c->ev_dep) (void)hipEventDestroy(e);
  (void)hipEventDestroy(c->ev_prep);
  (void)hipEventDestroy(c->ev_sigdec);
  (void)hipEventDestroy(c->ev_grp);
  (void)hipEventDestroy(c->ev_maps);
  (void)hipEventDestroy(c->ev_chk);
  for (auto& e : c->ev_bits) (void)hipEventDestroy(e);
  for (auto& e : c->ev_sag) (void)hipEventDestroy(e);
  for (auto& l : c->idx_list)
    if (l) (void)hipFree(l);
  for (auto& l : c->idx_sums)
    if (l) (void)hipFree(l);
  c->bits_off.release(); c->bits_idx.release(); c->bits_win.release();
  c->msg_rep.release(); c->msg_uniq.release(); c->msg_tab.release(); c->msg_cnt.release();
  c->pm_tab.release(); c->pm_slot.release(); c->pm_slot_idx.release(); c->pm_off.release(); c->pm_cls.release();
  c->pm_head.release(); c->pm_next.release(); c->pm_job.release(); c->pm_rep.release(); c->pm_item_off.release();
  c->pm_item_job.release(); c->pm_p.release(); c->pm_code.release(); c->pm_h.release();
  if (c->pin_in) (void)hipHostFree(c->pin_in);
  if (c->pin_out) (void)hipHostFree(c->pin_out);
  if (c->table) (void)hipFree(c->table);
  c->sk.release();
  c->stage_dev.release();
  c->raw_in.release(); c->gen_out.release(); c->pk_tmp.release(); c->pk_codes.release();
  c->pk_agg.release(); c->dbg_fe.release(); c->dbg_f.release(); c->dbg_out.release();
  c->scalars.release(); c->raw_conv.release();
  c->sig_aff.release(); c->h_aff.release(); c->sig_inf.release(); c->flags.release();
  c->sig_code.release(); c->pk_code.release(); c->job_code.release(); c->job_result.release(); c->set_code.release();
  c->rpk_aff.release(); c->chunk_off.release(); c->chunk_set.release(); c->pk_part.release(); c->rsig.release(); c->q_part.release(); c->sig_grp.release(); c->lines.release(); c->f_step.release(); c->f_set.release(); c->f_job.release(); c->f_batch.release(); c->f_tmp.release(); c->f_part.release();
  c->msm_bucket.release(); c->msm_win.release(); c->msm_mask.release();
  c->set_job.release(); c->s_inf.release(); c->item_off.release(); c->item_job.release(); c->s_aff.release();
  c->sm_skip.release(); c->sm_list.release(); c->sm_zero.release(); c->sm_seg_code.release(); c->sm_win.release();
  c->sm_hg.release(); c->sm_sg.release(); c->sm_pg.release(); c->sm_retry.release(); c->sm_split.release();
  c->sma_pk.release(); c->sma_pk_code.release(); c->sma_aff.release();
  c->sag_seg.release(); c->sag_cnt.release(); c->sag_code.release(); c->sag_out.release(); c->sag_valid.release();
  c->sag_sig.release();
  c->win_tmp.release(); c->f_fold.release();
  c->mb_fp.release(); c->mb_u64.release();
  (void)hipStreamDestroy(c->st);
  (void)hipStreamDestroy(c->st_hash);
  (void)hipStreamDestroy(c->st_pk);
  (void)hipStreamDestroy(c->st_chk);
  delete c;
  return BGV_OK;
}

// every stream of the context: a batch still in flight (bgv_partial leaves
// one, a failed call may) can read a list or its sums from any of the four
static int ctx_drain(bgv_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipStreamSynchronize(c->st_hash));
  HIPCHK(hipStreamSynchronize(c->st_pk));
  HIPCHK(hipStreamSynchronize(c->st_chk));
  return 0;
}

// drop the resident sums of one list / of every list, after the streams drained
static int sums_drop(bgv_ctx* c, uint32_t id) {
  if (!c->idx_sums[id]) return 0;
  if (int r = ctx_drain(c)) return r;
  (void)hipFree(c->idx_sums[id]);
  c->idx_sums[id] = nullptr;
  return 0;
}
static int sums_drop_all(bgv_ctx* c) {
  for (uint32_t k = 0; k < BGV_MAX_INDEX_LISTS; k++)
    if (int r = sums_drop(c, k)) return r;
  return 0;
}

static int table_reserve(bgv_ctx* c, uint32_t n) {
  if (n <= c->table_cap) return 0;
  uint32_t cap = c->table_cap ? c->table_cap : 1024;
  while (cap < n) cap = cap * 2u > cap ? cap * 2u : n;
  g1a* t = nullptr;
  HIPCHK(hipMalloc((void**)&t, (size_t)cap * sizeof(g1a)));
  HIPCHK(hipMemsetAsync(t, 0, (size_t)cap * sizeof(g1a), c->st));
  if (c->table) {
    HIPCHK(hipMemcpyAsync(t, c->table, (size_t)c->table_n * sizeof(g1a), hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipFree(c->table));
  }
  c->table = t;
  c->table_cap = cap;
  return 0;
}

// index2pubkey rows are u32 indices with bit 31 reserved for raw_pks
static const uint32_t TABLE_MAX = 0x7fffffffu;

int bgv_pubkeys_set(bgv_ctx* c, uint32_t first, uint32_t n, const uint8_t* data, uint32_t fmt) {
  if (!c || (!data && n)) return fail(BGV_E_INVALID_ARG, "null argument");
  if (fmt != BGV_PK_COMPRESSED_48 && fmt != BGV_PK_UNCOMPRESSED_96) return fail(BGV_E_INVALID_ARG, "bad format %u", fmt);
  c->partial_pending = false;
  if (n == 0) return BGV_OK;
  if ((uint64_t)first + n > TABLE_MAX) return fail(BGV_E_TABLE_RANGE, "rows [%u, %llu) exceed the table limit 2^31 - 1", first, (unsigned long long)first + n);
  if (first > c->table_n)
    return fail(BGV_E_TABLE_RANGE, "row %u would leave a gap after the %u rows of the table (append-only, pubkeyCache.ts:56-77)", first, c->table_n);
  HIPCHK(hipSetDevice(c->device));
  if (int r = table_reserve(c, first + n)) return r;
  const size_t w = fmt == BGV_PK_COMPRESSED_48 ? 48 : 96;
  if (int r = c->raw_in.ensure((size_t)n * w)) return r;
  if (int r = c->pk_tmp.ensure(n)) return r;
  if (int r = c->pk_codes.ensure(n)) return r;
  HIPCHK(hipMemcpyAsync(c->raw_in.p, data, (size_t)n * w, hipMemcpyHostToDevice, c->st));
  if (fmt == BGV_PK_COMPRESSED_48) launch_table_from_compressed(c->st, c->raw_in.p, c->pk_tmp.p, n, c->pk_codes.p);
  else launch_table_from_uncompressed(c->st, c->raw_in.p, c->pk_tmp.p, n, c->pk_codes.p);
  HIPCHK(hipGetLastError());
  c->pk_codes_host.resize(n);
  HIPCHK(hipMemcpyAsync(c->pk_codes_host.data(), c->pk_codes.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (uint32_t i = 0; i < n; i++)
    if (c->pk_codes_host[i] != 0)  // PublicKey.fromBytes throws: nothing is stored
      return fail(BGV_E_BAD_PUBKEY, "pubkey %u: BLST_ERROR: %s", first + i, bgv_set_code_name(c->pk_codes_host[i]));
  if (first < c->table_n)  // a rewrite: no prefix sum may outlive the rows it was built from
    if (int r = sums_drop_all(c)) return r;
  HIPCHK(hipMemcpyAsync(c->table + first, c->pk_tmp.p, (size_t)n * sizeof(g1a), hipMemcpyDeviceToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (first + n > c->table_n) c->table_n = first + n;
  return BGV_OK;
}

int bgv_pubkeys_count(bgv_ctx* c, uint32_t* count) {
  if (!c || !count) return fail(BGV_E_INVALID_ARG, "null argument");
  *count = c->table_n;
  return BGV_OK;
}

int bgv_pubkeys_get(bgv_ctx* c, uint32_t first, uint32_t n, uint8_t* out96) {
  if (!c || (!out96 && n)) return fail(BGV_E_INVALID_ARG, "null argument");
  if ((uint64_t)first + n > c->table_n) return fail(BGV_E_TABLE_RANGE, "range [%u, %u) beyond table size %u", first, first + n, c->table_n);
  if (n == 0) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->gen_out.ensure((size_t)n * 96)) return r;
  launch_table_export(c->st, c->table + first, c->gen_out.p, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out96, c->gen_out.p, (size_t)n * 96, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

int bgv_pubkeys_validate(bgv_ctx* c, const uint8_t* pk48, uint32_t n, int32_t* codes) {
  if (!c || (n && (!pk48 || !codes))) return fail(BGV_E_INVALID_ARG, "null argument");
  if (n == 0) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->raw_in.ensure((size_t)n * 48)) return r;
  if (int r = c->sig_code.ensure(n)) return r;
  HIPCHK(hipMemcpyAsync(c->raw_in.p, pk48, (size_t)n * 48, hipMemcpyHostToDevice, c->st));
  launch_pk_validate(c->st, c->raw_in.p, n, c->sig_code.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(codes, c->sig_code.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

// ---------------------------------------------------------------- batches

static void random_bytes(void* out, size_t n) {
  size_t got = 0;
  uint8_t* p = (uint8_t*)out;
  while (got < n) {
    ssize_t r = getrandom(p + got, n - got, 0);
    if (r > 0) got += (size_t)r;
  }
}

// a device allocation of prepare(): under memory pressure a kept line buffer
// (up to 2.6 GB, see work_alloc) gives way first, then the allocation retries
template <class T>
static int ensure_or_release_lines(bgv_ctx* c, dbuf<T>& b, size_t n) {
  int r = b.ensure(n);
  if (r && c->lines.cap && (const void*)&b != (const void*)&c->lines) {
    c->lines.release();
    if ((const void*)&b != (const void*)&c->f_step) c->f_step.release();
    c->lines_idle = 0;
    r = b.ensure(n);
  }
  return r;
}

static int pinned_reserve(uint8_t*& p, size_t& cap, size_t n) {
  if (n <= cap) return 0;
  size_t c = cap ? cap : 65536;
  while (c < n) c *= 2;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  if (hipHostMalloc((void**)&p, c, hipHostMallocDefault) != hipSuccess) return fail(BGV_E_HIP, "hipHostMalloc(%zu) failed", c);
  cap = c;
  return 0;
}

// one host array of a batch, packed at a 256-byte aligned offset of the staging buffers
struct stage_seg {
  const void* src;
  size_t bytes;
  const void** dst;
  size_t off;  // filled by stage_pack: offset in pin_in / stage_dev
};

// pack the segments into pin_in (host copies only) and point every *dst at
// its future device copy; stage_issue then moves the whole buffer in one transfer
static int stage_pack(bgv_ctx* c, stage_seg* segs, int n_segs, size_t& total) {
  total = 0;
  for (int i = 0; i < n_segs; i++) total += (segs[i].bytes + 255) & ~size_t(255);
  if (c->staged_pending) {  // the previous batch's copy may still read pin_in
    HIPCHK(hipEventSynchronize(c->ev_staged));
    c->staged_pending = false;
  }
  if (int r = pinned_reserve(c->pin_in, c->pin_in_cap, total ? total : 1)) return r;
  if (int r = ensure_or_release_lines(c, c->stage_dev, total ? total : 1)) return r;
  size_t off = 0;
  for (int i = 0; i < n_segs; i++) {
    if (segs[i].bytes) memcpy(c->pin_in + off, segs[i].src, segs[i].bytes);
    segs[i].off = off;
    *segs[i].dst = c->stage_dev.p + off;
    off += (segs[i].bytes + 255) & ~size_t(255);
  }
  return 0;
}

static int stage_issue(bgv_ctx* c, size_t total) {
  if (!total) return 0;
  HIPCHK(hipMemcpyAsync(c->stage_dev.p, c->pin_in, total, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipEventRecord(c->ev_staged, c->st));
  c->staged_pending = true;
  return 0;
}

// latency mode by batch size (prepare(); the r02 sweep: 25,088 sets 24.5 ms
// split against 26.3 ms, 50,176: 35.4 against 29.3; r03: to 65,536)
static const uint32_t SPLIT_MAX = 59000;
// With other batches in flight on the device (this process's bgv_verify /
// bgv_partial calls between entry and results), batches from INFLIGHT_BULK_MIN
// sets take the bulk pipeline (one lane per set, two pairs per Miller item over
// lines), whose kernels do the most work per instruction: with three in flight
// 50,176 sets 19.7-19.8 -> 18.5-18.8 ms per batch, 37,632 sets 15.8-16.4 ->
// 14.8-15.1 (profiles/r06ag_c4_over_2/); alone it loses (23.3-23.8 -> 29.1-29.8).
static const uint32_t INFLIGHT_BULK_MIN = 32000;
static std::atomic<int> g_active[64];
struct active_guard {
  int dev;
  explicit active_guard(int d) : dev(d >= 0 && d < 64 ? d : -1) { if (dev >= 0) g_active[dev]++; }
  ~active_guard() { if (dev >= 0) g_active[dev]--; }
};
static bool layout_split(const bgv_cfg& k, uint32_t n, bool busy) {
  return k.split >= 0 ? k.split != 0 : (n < SPLIT_MAX && !(busy && n >= INFLIGHT_BULK_MIN));
}

// The hash maps of a latency-mode batch read only the messages, and they head
// the critical path (maps -> clearing -> Miller -> fold -> final exp): they are
// launched on the hash stream as soon as the messages are on the device,
// before the host reads back offsets, checks them and sets up the rest
// (on-device batches: ~0.1 ms of idle GPU at 3,136 sets, r04c timeline).
// Timed runs keep the maps inside the hash stage's events.
#ifndef BGV_CHK_STREAM
#define BGV_CHK_STREAM 1
#endif
#ifndef BGV_EARLY_MAPS
#define BGV_EARLY_MAPS 1
#endif
static int early_maps(bgv_ctx* c, dev_batch& d, bool after_staging) {
  const uint32_t n = d.n_sets;
  if (!BGV_EARLY_MAPS) return 0;
  const bool timed = c->cfg.timing >= 0 ? c->cfg.timing != 0 : n >= 65536;
  if (!n || timed || !layout_split(c->cfg, n, c->busy)) return 0;
  if (int r = ensure_or_release_lines(c, c->q_part, 2 * (size_t)n)) return r;
  if (after_staging) HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_staged, 0));
  dev_work w;
  memset(&w, 0, sizeof w);
  w.q_part = c->q_part.p;
  // the batch's start event goes in front of the maps (they head the critical
  // path), so stats total_ms covers them; run_stages then does not re-record it
  HIPCHK(hipEventRecord(c->ev[0], c->st_hash));
  launch_hash_maps(c->st_hash, d, w);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_maps, c->st_hash));
  d.maps_early = 1;
  return 0;
}

static int prepare_layout(bgv_ctx* c, dev_batch& d, const uint64_t* scalars, bool scalars_staged);

// Build the device view of a batch: stage host arrays, convert raw pubkeys.
// Host batches: the arrays are copied into pinned memory FIRST and every
// contract check reads that copy, so the device only ever sees checked
// offsets even if the caller's buffers change during the call.  Index ranges
// are checked per set on the device (BGV_SET_INDEX_RANGE rejects the job).
static int prepare(bgv_ctx* c, const bgv_batch* b, dev_batch& d, bool need_sigs) {
  if (!b) return fail(BGV_E_INVALID_ARG, "batch is NULL");
  if (!b->job_offsets || !b->pk_offsets || !b->pk_indices || !b->msgs || (need_sigs && (!b->sigs || !b->sig_len)))
    return fail(BGV_E_INVALID_ARG, "missing batch array");
  if (b->n_raw && !b->raw_pks) return fail(BGV_E_INVALID_ARG, "n_raw > 0 but raw_pks is NULL");
  const uint32_t n = b->n_sets, J = b->n_jobs;
  memset(&d, 0, sizeof d);
  // another batch of this process in flight on the device (read once per batch)
  c->busy = c->device >= 0 && c->device < 64 && g_active[c->device].load() >= 2;
  d.n_sets = n;
  d.n_jobs = J;
  d.n_raw = b->n_raw;
  d.table_n = c->table_n;
  d.table = c->table;
  d.span_log2 = 7;  // device batches: trees cover jobs of <= 128 sets (multithread/index.ts:39)
  c->jo_host.resize((size_t)J + 1);
  if (!b->on_device) {
    const uint32_t total = b->pk_offsets[n];  // sizes the pk_indices copy; re-checked on the copy
    const uint8_t* raw_dev = nullptr;
    stage_seg segs[8] = {
        {b->job_offsets, ((size_t)J + 1) * 4, (const void**)&d.job_off, 0},
        {b->pk_offsets, ((size_t)n + 1) * 4, (const void**)&d.pk_off, 0},
        {b->pk_indices, (size_t)total * 4, (const void**)&d.pk_idx, 0},
        {b->msgs, (size_t)n * 32, (const void**)&d.msgs, 0},
        {b->raw_pks, (size_t)b->n_raw * 96, (const void**)&raw_dev, 0},
        {b->scalars, b->scalars ? (size_t)n * 8 : 0, (const void**)&d.scalars, 0},
        {b->sigs, need_sigs ? (size_t)n * 192 : 0, (const void**)&d.sigs, 0},
        {b->sig_len, need_sigs ? (size_t)n * 4 : 0, (const void**)&d.sig_len, 0},
    };
    size_t bytes = 0;
    if (int r = stage_pack(c, segs, 8, bytes)) return r;
    const uint32_t* jo = (const uint32_t*)(c->pin_in + segs[0].off);
    const uint32_t* po = (const uint32_t*)(c->pin_in + segs[1].off);
    // host-side contract checks on the pinned copy (the reference rejects these synchronously)
    if (jo[0] != 0 || jo[J] != n) return fail(BGV_E_INVALID_ARG, "job_offsets must span [0, n_sets]");
    uint32_t max_job = 1;
    for (uint32_t j = 0; j < J; j++) {
      if (jo[j + 1] < jo[j]) return fail(BGV_E_INVALID_ARG, "job_offsets not monotone");
      if (jo[j + 1] - jo[j] > max_job) max_job = jo[j + 1] - jo[j];
    }
    d.span_log2 = 0;
    while ((1u << d.span_log2) < max_job && d.span_log2 < 16) d.span_log2++;
    if (po[0] != 0) return fail(BGV_E_INVALID_ARG, "pk_offsets[0] != 0");
    if (po[n] != total) return fail(BGV_E_INVALID_ARG, "pk_offsets changed during the call");
    for (uint32_t i = 0; i < n; i++) {
      if (po[i + 1] < po[i]) return fail(BGV_E_INVALID_ARG, "pk_offsets not monotone");
      if (po[i + 1] == po[i]) return fail(BGV_E_EMPTY_SET, "EMPTY_AGGREGATE_ARRAY (set %u)", i);
    }
    memcpy(c->jo_host.data(), jo, c->jo_host.size() * 4);
    c->pk_total = total;
    if (int r = stage_issue(c, bytes)) return r;
    if (need_sigs)  // verification calls (bgv_gen_sign hashes on its own)
      if (int r = early_maps(c, d, true)) return r;
    if (!b->scalars) d.scalars = nullptr;
    if (!need_sigs) { d.sigs = nullptr; d.sig_len = nullptr; }
    if (int r = ensure_or_release_lines(c, c->raw_conv, b->n_raw ? b->n_raw : 1)) return r;
    launch_raw_pks(c->st, raw_dev, c->raw_conv.p, b->n_raw);
    d.raw_pks = c->raw_conv.p;
  } else {
    d.job_off = b->job_offsets;
    d.pk_off = b->pk_offsets;
    d.pk_idx = b->pk_indices;
    d.msgs = b->msgs;
    d.sigs = b->sigs;
    d.sig_len = b->sig_len;
    if (need_sigs)
      if (int r = early_maps(c, d, false)) return r;
    if (int r = ensure_or_release_lines(c, c->raw_conv, b->n_raw ? b->n_raw : 1)) return r;
    launch_raw_pks(c->st, b->raw_pks, c->raw_conv.p, b->n_raw);
    d.raw_pks = c->raw_conv.p;
    // offsets live in HBM: the host needs the job offsets (stats) and the key total (grid bound)
    HIPCHK(hipMemcpyAsync(c->jo_host.data(), b->job_offsets, c->jo_host.size() * 4, hipMemcpyDeviceToHost, c->st));
    c->pk_total = 0;
    if (n) HIPCHK(hipMemcpyAsync(&c->pk_total, b->pk_offsets + n, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  return prepare_layout(c, d, b->scalars, b->scalars && !b->on_device);
}

// The tail of prepare(), shared with bgv_verify_bits: the pipeline variant of a
// batch whose device view (arrays, n_sets, span_log2) and key total
// (c->pk_total) are set, and its scalars.  scalars_staged: d.scalars already
// points at the staged copy of a host batch.
// sets of a job per lane of k_miller_steps (dev_batch.steps_slice); a
// compile-time knob for A/B builds (DESIGN.md section 3 r07 has the sweep)
#ifndef BGV_STEPS_SLICE
#define BGV_STEPS_SLICE 49
#endif
static const uint32_t STEPS_SLICE = BGV_STEPS_SLICE;

static int prepare_layout(bgv_ctx* c, dev_batch& d, const uint64_t* scalars, bool scalars_staged) {
  const uint32_t n = d.n_sets;
  const uint32_t total = c->pk_total;
  // grid bound of the chunked pubkey gather: sum ceil(k_i/32) <= total/32 + n
  d.chunk_bound = total / 32 + n;
  // Pipeline variant by batch size, from the r02 sweep of on-device C4-shaped
  // batches (tools/sweep_modes.py):
  //  * cooperative Miller loop (36 lanes per pair) below MILLER_COOP_MAX sets;
  //    above it the one-lane loop (36x fewer lanes) wins: 7,840 sets 20.1 ->
  //    18.2 ms, 12,544 sets 28.6 -> 20.0 ms, 50,176 sets 95.6 -> 29.3 ms;
  //  * per-job bucket MSM for sum r_i sigma_i from the same size (its 16
  //    lanes per job lengthen small batches: 98 sets 7.1 -> 17 ms);
  //  * latency mode (two-lane hash maps, cooperative G2) below SPLIT_MAX
  //    (25,088 sets: 24.5 ms split against 26.3 ms; 50,176: 35.4 against 29.3);
  //  * two pairs per Miller work item only when the batch alone fills the chip.
  //  * r03 mid-size sweep (profiles/r03_sweep_mid_sizes.jsonl): the
  //    four-lane Miller loop from 6,000 sets and the two-lane one from
  //    18,000; the three-lane cofactor clearing from 9,000; sum r_i sigma_i
  //    by the (job, window, digit)-lane MSM from 9,000 (bulk batches: the
  //    (job, window) one)
  //    (12,544: 18.4 -> 10.6 ms; 25,088: 24.1 -> 16.9 ms; 6,272: 10.8 -> 9.2 ms);
  //    the latency-mode hash (two-lane maps, one-lane clearing) with the
  //    one-lane Miller loop and the (job, window) MSM up to 65,536 sets
  //    (37,632: 25.1 -> 22.5 ms; 50,176: 26.0 -> 24.9 ms)
  //  * r04 sweeps: the one-lane Miller loop and the (job, window) MSM from
  //    32,000 sets (32,928 / 34,496 sets 25.1 / 25.3 -> 22.0 / 22.1 ms), the
  //    bulk kernels from 59,000 (62,720 sets 32.1 -> 30.3 ms, 59,584 sets
  //    30.5 -> 28.0 ms; 58,016 sets stay split: 27.1 against 28.7 ms;
  //    profiles/r04z_sweep_big.txt, profiles/r04z_sweep_split_edge.txt)
  static const uint32_t MILLER18_MIN = 2000, MILLER4_MIN = 6000, MILLER2_MIN = 15000, MILLER1_MIN = 32000, CLEAR1_MIN = 16500,
                        MSM_MIN = 6000, MSM4_MIN = 9000, MSM2_MIN = 32000, PAIRS2_MIN = 65536,
                        CLEAR3_MIN = 9000, KV6_MIN = 1100, KV3_MIN = 4500, KV_MAX = 11500;
  const bgv_cfg& k = c->cfg;
  d.pairs_per_item = k.pairs ? (uint32_t)k.pairs : (n >= PAIRS2_MIN || (c->busy && n >= INFLIGHT_BULK_MIN) ? 2u : 1u);
  d.split = layout_split(k, n, c->busy) ? 1u : 0u;
  // one lane per point from 16,500 sets (25,088: 16.74 -> 16.5 ms; 17,248:
  // 14.24 -> 13.95 ms; the trio's waves oversubscribe the SIMDs there) and the
  // two-lane Miller loop from 15,000 (r04 sweep, profiles/r04z_sweep_cliff.txt:
  // the four-lane loop's waves oversubscribe from ~15,000 sets: 15,680 sets
  // 12.38 -> 12.10 ms, 17,248 sets 16.61 -> 13.95 ms)
  d.clear_lanes = k.clear_lanes > 0 ? (uint32_t)k.clear_lanes : (n < CLEAR3_MIN ? 9u : n < CLEAR1_MIN ? 3u : 1u);
  // sum r_i sigma_i per job by a bucket MSM (16 x 4-bit windows) when jobs
  // are block-sized (<= 256 sets).  The latency mode takes the fused kernel
  // (one workgroup per job, k_msm_fused: short chain, many idle lanes); bulk
  // batches the (job, window)-lane kernels, which do a third of its SIMD-time
  // (C4: k_msm_fused 49 ms beside the hash, pubkeys and Miller loops,
  // stretching the Miller kernel from 14.5 to 26.4 ms, r03 trace)
  {
    uint32_t auto_msm = 0;
    if (n >= MSM_MIN && d.span_log2 <= 8) {
      if (!d.split || n >= MSM2_MIN) auto_msm = 2;
      else auto_msm = n < MSM4_MIN ? 1 : 4;
    }
    d.msm = k.msm >= 0 ? (uint32_t)k.msm : auto_msm;
  }
  // Deferred subgroup checks: the signature stage only decodes, and the checks
  // of sets [defer_from, n) run beside the Miller loops (bgv_kernels.hip
  // k_job_recode).  Wherever the MSM sums the signatures (the latency mode
  // without it checks beside the per-set scaling, k_sig_split_coop): all of
  // them with one pair per Miller item (C4/2 28.3 -> 26.4 ms); half with two
  // pairs per item: the Miller kernel leaves 240 SIMDs to the MSM tail and
  // the job pairs, and half of the checks fill them without outlasting it
  // (C4, 3 runs each: none 39.75, 50% 39.27, 65% 39.31, all 39.89 ms; r03, with
  // the inlined Fp12 layer: 50% 39.04 / 38.93, 75% 38.54 / 38.79, 25% 39.28 / 38.97).
  // defer_from is a multiple of 64 (wave-uniform).
  const bool deferrable = !d.split || d.msm;
  const int pct = !deferrable ? 0 : (k.defer_pct >= 0 ? k.defer_pct : (!d.split && d.pairs_per_item >= 2 ? 75 : 100));
  d.defer_grp = pct > 0 ? 1u : 0u;
  d.defer_from = pct > 0 ? (uint32_t)(((uint64_t)n * (uint32_t)(100 - pct) / 100u) & ~63ull) : n;
  // two-level per-job fold (bgv_tail.hip) for jobs of >= 64 sets: the fold
  // runs after the Miller kernels with the chip otherwise idle, so groups of
  // ~sqrt(span) sets fold side by side, then the job folds the group values,
  // 2 sqrt(span) sequential Fp12 products instead of span (r05: also for many
  // jobs; C4 product-tree stage 0.36 -> 0.33 ms, profiles/r05l_job_fold.txt)
  {
    const bool few_big = d.span_log2 >= 6 && d.span_log2 <= 8;
    const bool on = k.prefold >= 0 ? (k.prefold && d.span_log2 >= 2 && d.span_log2 <= 8) : few_big;
    d.prefold_log2 = on ? (d.span_log2 + 1) / 2 : 0u;
  }
  // set-pair Miller layout: lanes per pair shrink as the batch grows, so the
  // waves stay near one per SIMD (a pair's loop is a chain of ~1,800 Fp2
  // products on 6 lanes, ~560 product rounds on 36)
  d.miller_coop = k.miller >= 0 ? (k.miller == 1 ? 0u : (uint32_t)k.miller)
                                : (n < MILLER18_MIN ? 36u : n < MILLER4_MIN ? 18u : n < MILLER2_MIN ? 4u
                                   : n < MILLER1_MIN ? 2u : 0u);
  // two-pair Miller loop in Karatsuba views (miller_kv.h) in the latency mode:
  // the squaring of f is shared by two pairs, 3 S lanes per two pairs
  {
    // r04 sweeps (profiles/r04_sweep_kv.txt, r04c_sweep_kv_bounds.txt): 1,960
    // sets 7.57 -> 6.42 ms and 3,136 sets 6.68 -> 6.57 ms with 18 lanes per two
    // pairs (980 sets: 6.02 -> 6.18, 1,176 sets 6.70 -> 6.20: from 1,100); 4,704 sets 7.98 ->
    // 7.87, 6,272 sets 8.88 -> 8.48 ms and 10,976 sets 9.38 -> 9.17 ms with 9;
    // at 12,544 the four-lane one-pair loop stays (9.7 against 10.8 ms: the
    // 9-lane groups' 915 waves leave no SIMD to the checks and the signature chain).
    // 27 lanes per two pairs (miller_kv = 9) ties 18 at 980-1,960 sets and loses
    // from 3,136 (7.05 against 6.52 ms; profiles/r04e_sweep_kv9.txt): A/B only
    const uint32_t auto_kv = n >= KV6_MIN && n < KV3_MIN ? 6u : (n >= KV3_MIN && n < KV_MAX ? 3u : 0u);
    d.miller_kv = k.miller_kv >= 0 ? (uint32_t)k.miller_kv : auto_kv;
    if (!d.split) d.miller_kv = 0;
    if (d.miller_kv) d.pairs_per_item = 2;
    // the cooperative, four- and two-lane loops hold one pair per item (every
    // set has its own Miller value, which the per-job fold relies on)
    else if (d.miller_coop) d.pairs_per_item = 1;
  }
  d.job_lanes = k.job_lanes ? (uint32_t)k.job_lanes : 36u;
  // the scalars are allocated before the line decision below, so a line buffer
  // that ensure_or_release_lines gives up here is seen by that decision
  if (scalars_staged) {
    // staged with the other host arrays by the caller
  } else if (scalars) {
    d.scalars = scalars;
  } else {
    // fresh 64-bit multipliers on the device: ChaCha20 keyed by 32 bytes of
    // getrandom() (+ 12-byte nonce) per call, rng.h
    uint32_t kn[11];
    random_bytes(kn, sizeof kn);
    if (int r = ensure_or_release_lines(c, c->scalars, n ? n : 1)) return r;
    launch_gen_scalars(c->st, kn, kn + 8, c->scalars.p, n);
    HIPCHK(hipGetLastError());
    d.scalars = c->scalars.p;
  }
  // fixed-argument lines (pairing.h miller_lines): the G2 half of the one-lane
  // Miller loop moves to the hash stream, phase 1 (C4 40.4 -> 39.5 ms); with
  // one pair per item it loses (C4/2 26.4 -> 28.5 ms)
  d.lines = (uint32_t)(!d.split && !d.miller_coop && (k.lines >= 0 ? k.lines : d.pairs_per_item >= 2));
  // the lines take 3 x 68 Fp2 = 19.6 KB per set (1.97 GB at C4, 2.6 GB at the
  // Node pool's 2^17-set batch cap): kept only while a quarter of the free HBM
  // covers them, else the loop recomputes them (miller_loop2, same values)
  if (d.lines) {
    const size_t need = (size_t)3 * MILLER_STEPS * n * sizeof(fp2_t);
    size_t free_b = 0, total_b = 0;
    if (need > c->lines.cap * sizeof(fp2_t) &&
        (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b / 4))
      d.lines = 0;
  }
  // four pairs per item exist only over precomputed lines (miller_loop_lines4)
  if (d.pairs_per_item == 4 && !d.lines) d.pairs_per_item = 2;
  // per-step line products (pairing.h miller_step_lines, bgv_tail.hip
  // k_job_chain) in place of the item loop: only over the one-lane layout with
  // lines.  Auto: where the layout itself chose two pairs per item over lines
  // (pairs and lines left at auto); an explicit pairs keeps the item loop.
  // f_step takes 576 B x 68 per slice (39 KB; 120 MB at C4 with 49-set slices):
  // like the lines, only while a quarter of the free HBM covers it.
  {
    const bool can = !d.split && !d.miller_coop && !d.miller_kv && d.lines;
    // (block-sized jobs only, as the MSM: k_job_chain joins a job's slices one after the other)
    const bool want = k.miller_steps >= 0 ? k.miller_steps != 0 : (k.pairs == 0 && d.pairs_per_item >= 2 && d.span_log2 <= 8);
    d.steps_slice = can && want ? STEPS_SLICE : 0u;
    if (d.steps_slice) {
      const size_t need = (size_t)miller_items_bound(d, d.steps_slice) * MILLER_STEPS * sizeof(fp12_t);
      size_t free_b = 0, total_b = 0;
      if (need > c->f_step.cap * sizeof(fp12_t) && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b / 4))
        d.steps_slice = 0;
    }
    // what bgv_miller_path_stats reports: host values only (the job offsets are home since prepare())
    const uint32_t per = d.steps_slice ? d.steps_slice : (d.miller_coop && !d.miller_kv ? 0u : d.pairs_per_item);
    uint32_t items = 0;
    if (per && c->jo_host.size() == (size_t)d.n_jobs + 1)
      for (uint32_t j = 0; j < d.n_jobs; j++) items += miller_item_count(c->jo_host[j + 1] - c->jo_host[j], per);
    c->miller_path = {d.steps_slice ? 1u : 0u, per, items};
  }
  return 0;
}

static int work_alloc_once(bgv_ctx* c, const dev_batch& d, dev_work& w);

// Message classes (bgv_cfg.hash_dedup): the bulk layout only.  A latency-mode
// batch keeps its early two-lane maps and cooperative clearing: its hash heads
// the critical path and is a wave or less per SIMD, where 64 hashes take as
// long as 1,024 (DESIGN.md sections 3c, 3g).  Auto (-1) means OFF, callers opt
// in with 1: on the C4 segment with every root distinct the pass costs nothing
// alone (35.9 against 36.0 ms, inside the spread) but 2.3 ms per batch with
// three batches in flight (35.1 against 32.8 ms, spread 1.0 ms), where its
// set-up kernels queue behind the other batches' waves; with half of the roots
// repeated it gains 1.4 ms alone and 0.75 ms in flight, with three quarters
// 4.5 and 3.4 ms.
// The table's slot count is a uint32_t power of two >= 2 n_sets.
// Pair classes (bgv_pair_merge): the bulk layout's one-lane set-pair loop only,
// and only inside the three entries whose callers can take the fallback.
static bool pair_merge_on(const bgv_ctx* c, const dev_batch& d) {
  return c->pm_call && !d.split && !d.miller_coop && !d.miller_kv && !d.steps_dbg && d.pairs_per_item >= 1 && d.n_jobs > 0 &&
         d.n_sets > 0 && d.n_sets <= (1u << 30);
}
// (merging needs the root representatives, so it implies the class pass)
static bool hash_dedup_on(const bgv_ctx* c, const dev_batch& d) {
  return !d.split && (c->cfg.hash_dedup == 1 || pair_merge_on(c, d)) && d.n_sets > 0 && d.n_sets <= (1u << 30);
}

// a kept line buffer the batch does not use gives way under memory pressure
static int work_alloc(bgv_ctx* c, const dev_batch& d, dev_work& w) {
  int r = work_alloc_once(c, d, w);
  if (r && !d.lines && c->lines.cap) {
    c->lines.release();
    c->f_step.release();
    c->lines_idle = 0;
    r = work_alloc_once(c, d, w);
  }
  return r;
}

static int work_alloc_once(bgv_ctx* c, const dev_batch& d, dev_work& w) {
  const uint32_t n = d.n_sets, J = d.n_jobs;
  const size_t ns = n ? n : 1, nj = J ? J : 1;
  int r = 0;
  if ((r = c->chunk_off.ensure(ns + 1)) || (r = c->chunk_set.ensure((size_t)d.chunk_bound + 1)) ||
      (r = c->pk_part.ensure((size_t)d.chunk_bound + 1)))
    return r;
  w.chunk_off = c->chunk_off.p; w.chunk_set = c->chunk_set.p; w.pk_part = c->pk_part.p;
  if ((r = c->sig_aff.ensure(ns)) || (r = c->h_aff.ensure(ns)) || (r = c->sig_inf.ensure(ns)) ||
      (r = c->sig_code.ensure(ns)) || (r = c->pk_code.ensure(ns)) || (r = c->rpk_aff.ensure(ns)) ||
      (r = c->rsig.ensure(ns)) || (r = c->f_set.ensure(ns + nj + 1)) || (r = c->set_code.ensure(ns)) ||
      (r = c->set_job.ensure(ns)) || (r = c->item_off.ensure(nj + 1)) || (r = c->item_job.ensure(ns + nj + 1)) || (r = c->f_job.ensure(nj)) || (r = c->f_batch.ensure(nj)) || (r = c->f_tmp.ensure(nj / 8 + 1)) ||
      (r = c->s_aff.ensure(nj + 1)) || (r = c->s_inf.ensure(nj + 1)) || (r = c->job_code.ensure(nj)) ||
      (r = c->job_result.ensure(nj)) || (r = c->f_part.ensure(4)) || (r = c->flags.ensure(8)))
    return r;
  w.sig_aff = c->sig_aff.p; w.h_aff = c->h_aff.p; w.sig_inf = c->sig_inf.p; w.sig_code = c->sig_code.p;
  w.pk_code = c->pk_code.p; w.rpk_aff = c->rpk_aff.p; w.rsig = c->rsig.p; w.f_set = c->f_set.p;
  w.set_code = c->set_code.p; w.f_job = c->f_job.p; w.job_code = c->job_code.p; w.job_result = c->job_result.p;
  w.f_part = c->f_part.p; w.flags = c->flags.p;
  w.item_off = c->item_off.p; w.item_job = c->item_job.p;
  w.set_job = c->set_job.p; w.f_batch = c->f_batch.p; w.f_tmp = c->f_tmp.p; w.s_aff = c->s_aff.p; w.s_inf = c->s_inf.p;
  w.q_part = nullptr; w.sig_grp = nullptr; w.pk_agg = nullptr;
  if (d.split) {
    if ((r = c->q_part.ensure(2 * ns)) || (r = c->sig_grp.ensure(ns))) return r;
    w.q_part = c->q_part.p; w.sig_grp = c->sig_grp.p;
  } else if (d.defer_grp) {
    if ((r = c->sig_grp.ensure(ns))) return r;
    w.sig_grp = c->sig_grp.p;
  }
  // the line buffer (19.6 KB per set, 1.3-2.6 GB) stays across batches: a
  // node alternating gossip batches with range-sync segments would otherwise
  // hipFree / hipMalloc gigabytes (each free synchronises the device) on every
  // switch; it goes back after LINES_KEEP batches in a row without lines
  static const uint32_t LINES_KEEP = 64;
  w.lines = nullptr;
  if (d.lines) {
    c->lines_idle = 0;
    if ((r = c->lines.ensure((size_t)3 * MILLER_STEPS * ns))) return r;
    w.lines = c->lines.p;
  } else if ((c->lines.cap || c->f_step.cap) && ++c->lines_idle >= LINES_KEEP) {
    c->lines.release();
    c->f_step.release();
    c->lines_idle = 0;
  }
  // the step products live and die with the lines (steps_slice implies lines)
  w.f_step = nullptr;
  if (d.steps_slice) {
    if ((r = c->f_step.ensure((size_t)miller_items_bound(d, d.steps_slice) * MILLER_STEPS))) return r;
    w.f_step = c->f_step.p;
  }
  // message classes (bgv_dedup.hip): sized with the batch's other buffers, never inside a run
  c->mc = {};
  if (hash_dedup_on(c, d)) {
    size_t slots = 64;
    while (slots < 2 * ns) slots *= 2;
    if ((r = c->msg_rep.ensure(ns)) || (r = c->msg_uniq.ensure(ns)) || (r = c->msg_tab.ensure(slots)) || (r = c->msg_cnt.ensure(1)))
      return r;
    c->mc.n_sets = n;
    c->mc.mask = (uint32_t)(slots - 1);
    c->mc.msgs = d.msgs;
    c->mc.table = c->msg_tab.p; c->mc.rep = c->msg_rep.p; c->mc.uniq = c->msg_uniq.p; c->mc.n_uniq = c->msg_cnt.p;
    c->mc.h_aff = w.h_aff;
  }
  // pair classes (bgv_pair_merge.hip): likewise, and only when merging is on
  c->pc = {};
  if (pair_merge_on(c, d)) {
    size_t slots = 64;
    while (slots < 2 * ns) slots *= 2;
    if ((r = c->pm_tab.ensure(slots)) || (r = c->pm_slot_idx.ensure(slots)) || (r = c->pm_slot.ensure(ns)) ||
        (r = c->pm_off.ensure(nj + 1)) || (r = c->pm_cls.ensure(ns)) || (r = c->pm_head.ensure(ns)) ||
        (r = c->pm_next.ensure(ns)) || (r = c->pm_job.ensure(ns)) || (r = c->pm_rep.ensure(ns)) ||
        (r = c->pm_item_off.ensure(nj + 1)) || (r = c->pm_item_job.ensure(ns + nj + 1)) || (r = c->pm_p.ensure(ns)) ||
        (r = c->pm_code.ensure(ns)) || (r = c->pm_h.ensure(ns)))
      return r;
    pair_classes& p = c->pc;
    p.n_sets = n; p.n_jobs = J;
    p.mask = (uint32_t)(slots - 1);
    p.per = d.steps_slice ? d.steps_slice : d.pairs_per_item;
    p.job_off = d.job_off; p.rep = c->msg_rep.p;
    p.table = c->pm_tab.p; p.slot = c->pm_slot.p; p.slot_idx = c->pm_slot_idx.p; p.class_off = c->pm_off.p;
    p.cls = c->pm_cls.p; p.head = c->pm_head.p; p.next = c->pm_next.p; p.cls_job = c->pm_job.p; p.cls_rep = c->pm_rep.p;
    p.item_off = c->pm_item_off.p; p.item_job = c->pm_item_job.p;
    p.p_cls = c->pm_p.p; p.code_cls = c->pm_code.p; p.h_cls = c->pm_h.p;
    p.ident = c->flags.p + 1;
  }
  // batch-first tail: one extra slot of s_aff / s_inf / f_set above, the window tree and the step folds here
  w.win_tmp = nullptr; w.f_fold = nullptr;
  if (d.batch_tail) {
    if ((r = c->win_tmp.ensure(16 * tail_entries(J, WIN_FAN))) ||
        (r = c->f_fold.ensure(tail_entries(miller_items_bound(d, d.steps_slice), FOLD_FAN) * MILLER_STEPS)))
      return r;
    w.win_tmp = c->win_tmp.p; w.f_fold = c->f_fold.p;
  }
  w.msm_bucket = nullptr; w.msm_mask = nullptr; w.msm_win = nullptr;
  if (d.msm == 2) {
    if ((r = c->msm_bucket.ensure(nj * 16 * 15)) || (r = c->msm_mask.ensure(nj * 16)) || (r = c->msm_win.ensure(nj * 16))) return r;
    w.msm_bucket = c->msm_bucket.p; w.msm_mask = c->msm_mask.p; w.msm_win = c->msm_win.p;
  } else if (d.msm == 4) {
    if ((r = c->msm_win.ensure(nj * 16))) return r;
    w.msm_win = c->msm_win.p;
  }
  return 0;
}

// run stages [from, to) with an event before each
// Stage graph on three streams (the stages read disjoint inputs and write
// disjoint buffers, bgv_kernels.hip):
//   st      : sig -> sig_scale -> [pk] sig_sum_tree -> miller_loop_jobs -> [miller] tail
//   st_hash : hash -> [pk] miller_loop (the set pairs)
//   st_pk   : pk_gather -> pk_aggregate_scale   ([pk] = after pk_aggregate_scale)
// The set-pair Miller loops need only H(m) and the aggregated keys, so they
// start while the signatures are still being scaled: at C4 the Miller kernel
// fills 78% of the SIMDs (one wave each) and sig_scale takes the rest.
// Per-stage timing events (stats->stage_ms) cost ~5 us of queue time each on
// the critical path, so latency batches record only the stream dependencies
// (untimed events) and the total.
static int run_stages(bgv_ctx* c, const dev_batch& d, const dev_work& w, int from, int to) {
  const bool fork = from <= ST_SIG && to > ST_F_TREE;
  const bool timed = c->cfg.timing >= 0 ? c->cfg.timing != 0 : d.n_sets >= 65536;
  c->timed = timed;
  c->last_d = d;
  c->run_from = from;
  c->run_to = to;
  hipEvent_t* dep = timed ? c->ev_end : c->ev_dep;  // what the stream waits below wait on
  if (!timed && !(d.maps_early && from == 0)) HIPCHK(hipEventRecord(c->ev[from], c->st));
  // latency batches fork the hash leg BEFORE the index set-up: hash_to_G2 reads
  // only the messages and heads the critical path (hash -> Miller -> fold ->
  // final exp); large batches keep the set-up alone on the GPU (its
  // one-workgroup scan starves under the bulk kernels).  At C4 the signature
  // decode is dispatched first, on the set-up's own stream: dispatching the
  // hash first ends it at ~12.5 instead of ~16.3 ms, but the signature chain
  // (decode -> MSM buckets -> window sums -> job pairs, ~32 ms of the 37)
  // then runs into the Miller phase, and the step lost 0.2-3.8 ms in every
  // order tried (profiles/r05m_bulk_stage_order.txt)
  const bool early_hash = fork && d.split && from <= ST_HASH && to > ST_HASH;
  const bool hashes = from <= ST_HASH && to > ST_HASH;
  const bool classes = hashes && c->mc.n_sets == d.n_sets && hash_dedup_on(c, d);
  if (hashes) {
    c->hash_path = {d.n_sets, d.n_sets, classes ? 1u : 0u};
    c->hash_pending = classes;  // hashes = n_uniq, home with the results (finish_results, bgv_partial)
  }
  // pair classes: the set-pair kernels and the per-job fold run over a view
  // whose sets are the classes (bgv_pair_merge.hip); n_sets, lines, f_set and
  // f_step stay the real ones, every other stage sees the real batch
  const bool merge = fork && from == 0 && classes && c->pc.n_sets == d.n_sets && pair_merge_on(c, d);
  dev_batch dv = d;
  dev_work wv = w;
  if (merge) {
    dv.job_off = c->pc.class_off;
    wv.rpk_aff = c->pc.p_cls; wv.pk_code = c->pc.code_cls; wv.h_aff = c->pc.h_cls;
    wv.set_job = c->pc.cls_job; wv.item_off = c->pc.item_off; wv.item_job = c->pc.item_job;
  }
  if (c->pm_entry && from <= ST_MILLER && to > ST_MILLER) {
    c->pair_path = {d.n_sets, d.n_sets, merge ? 1u : 0u, 0u};
    c->pair_pending = merge;  // pairs = the class count, home with the results
    c->pair_redo = false;
  }
  c->tail_d = dv;
  c->tail_w = wv;
  auto launch_one = [&](int s) -> int {
    hipStream_t st = c->st;
    // fixed-argument lines: right behind the hash on its stream, before the
    // Miller stage waits for the pubkeys (timed in neither stage)
    if (s == ST_MILLER && d.lines) {
      if (merge) launch_pair_lines(fork ? c->st_hash : c->st, c->pc, w.lines);  // one lane per class
      else launch_lines(fork ? c->st_hash : c->st, d, w);  // bgv_miller.hip
      HIPCHK(hipGetLastError());
    }
    if (fork) {
      if (s == ST_HASH || s == ST_MILLER) st = c->st_hash;
      if (s == ST_PK || s == ST_PK_SCALE) st = c->st_pk;
      if (s == ST_S_TREE || s == ST_MILLER) HIPCHK(hipStreamWaitEvent(st, dep[ST_PK_SCALE], 0));
      if (s == ST_F_TREE) HIPCHK(hipStreamWaitEvent(st, dep[ST_MILLER], 0));
    }

    // maps launched early on st_hash: a hash stage on another stream (a run
    // that does not fork, e.g. bgv_debug_stages' first range) waits for them
    if (s == ST_HASH && d.maps_early && st != c->st_hash) HIPCHK(hipStreamWaitEvent(st, c->ev_maps, 0));
    if (timed) HIPCHK(hipEventRecord(c->ev[s], st));
    // deferred subgroup checks: their verdicts enter the codes before the fold
    if (s == ST_F_TREE && d.defer_grp && !d.batch_tail) {
      if (fork) HIPCHK(hipStreamWaitEvent(st, c->ev_grp, 0));
      launch_sig_fixup(st, d, w);
    }
    if (s == ST_HASH && classes) launch_hash_classes(st, c->mc);  // bgv_dedup.hip: the representatives, then the copies
    else if (merge && (s == ST_MILLER || s == ST_F_TREE || (s == ST_BATCH_FINAL && d.batch_tail))) launch_stage(st, s, dv, wv);
    else launch_stage(st, s, d, w);
    // batch-first tail: the batch sum above ran over the codes k_msm_window left, beside the Miller stage and the
    // checks.  Their verdicts enter the codes here, and the sum runs again only if one of them rejected a job
    // (on the device: FLAG_CODES_KEPT); the main stream carries no Miller work, so the wait costs the fold nothing
    if (s == ST_MILLER_JOBS && d.defer_grp && d.batch_tail) {
      if (fork) HIPCHK(hipStreamWaitEvent(st, c->ev_grp, 0));
      launch_sig_fixup(st, d, w);
      launch_batch_sig_redo(st, d, w);
    }
    if (merge && s == ST_HASH) launch_pair_h(st, c->pc, w.h_aff);  // H(m) per class, for the class lines / the loops
    // P_c per class, in front of whatever waits for the scaled keys
    if (merge && s == ST_PK_SCALE) launch_pair_sum(st, c->pc, w.rpk_aff, w.pk_code);
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(c->ev_end[s], st));
    else if (fork && (s == ST_PK_SCALE || s == ST_HASH || s == ST_MILLER)) HIPCHK(hipEventRecord(c->ev_dep[s], st));
    if (d.defer_grp && s == ST_SIG && fork) HIPCHK(hipEventRecord(c->ev_sigdec, st));
    if (d.defer_grp && s == ST_PK_SCALE) {
      // the checks start once the Miller loops have their keys, beside them;
      // BGV_CHK_STREAM: on a low-priority stream of their own, so the waves of
      // the hash stream (the fixed-argument lines, then the Miller loops) are
      // dispatched first when slots free up
      // (latency-mode batches only: at C4 the checks on the pubkey stream measured
      // 0.3 ms faster, 4 same-box rounds, profiles/r04z_ab_chk_c4.txt)
      hipStream_t cs = st;
      if (fork && BGV_CHK_STREAM && d.split) {
        HIPCHK(hipEventRecord(c->ev_chk, st));
        cs = c->st_chk;
        HIPCHK(hipStreamWaitEvent(cs, c->ev_chk, 0));
      }
      if (fork) HIPCHK(hipStreamWaitEvent(cs, c->ev_sigdec, 0));
      launch_sig_check(cs, d, w);
      HIPCHK(hipGetLastError());
      if (fork) HIPCHK(hipEventRecord(c->ev_grp, cs));
    }
    return 0;
  };
  if (early_hash) {  // enqueued first, so the host's launch latency does not delay it either
    HIPCHK(hipEventRecord(c->ev_fork, c->st));
    HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_fork, 0));
    if (int r = launch_one(ST_HASH)) return r;
  }
  if (from <= ST_PK) {
    launch_prep(c->st, d, w);
    HIPCHK(hipGetLastError());
  }
  // the message classes are index-only set-up too: beside launch_prep, on an
  // otherwise idle GPU and in front of everything the hash stream runs.  The
  // slot key is fresh per call (also when the caller injects the scalars):
  // peers choose roots, and a fixed mix would let them build long probe chains
  if (classes) {
    random_bytes(&c->mc.key, sizeof c->mc.key);
    HIPCHK(hipMemsetAsync(c->mc.table, 0xff, ((size_t)c->mc.mask + 1) * 4, c->st));
    HIPCHK(hipMemsetAsync(c->mc.n_uniq, 0, 4, c->st));
    launch_msg_dedup(c->st, c->mc);
    HIPCHK(hipGetLastError());
  }
  // the pair classes follow the root classes they are built from, in the same place (on the hash stream behind
  // ev_prep they measured the same with three batches in flight)
  if (merge) {
    const pair_classes& p = c->pc;
    random_bytes(&c->pc.key, sizeof c->pc.key);
    HIPCHK(hipMemsetAsync(p.table, 0xff, ((size_t)p.mask + 1) * 8, c->st));
    HIPCHK(hipMemsetAsync(p.head, 0xff, (size_t)p.n_sets * 4, c->st));
    HIPCHK(hipMemsetAsync(p.class_off, 0, ((size_t)p.n_jobs + 1) * 4, c->st));
    HIPCHK(hipMemsetAsync(p.cls_job, 0, (size_t)p.n_sets * 4, c->st));  // the dead tail names job 0 (k_f_level)
    HIPCHK(hipMemsetAsync(p.ident, 0, 4, c->st));
    launch_pair_classes(c->st, c->pc);
    HIPCHK(hipGetLastError());
  }
  if (fork) {
    HIPCHK(hipEventRecord(c->ev_prep, c->st));
    if (!early_hash) HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_prep, 0));
    HIPCHK(hipStreamWaitEvent(c->st_pk, c->ev_prep, 0));
  }
  for (int s = from; s < to; s++)
    if (!(early_hash && s == ST_HASH))
      if (int r = launch_one(s)) return r;
  HIPCHK(hipEventRecord(c->ev[to], c->st));
  return 0;
}

static void stats_layout(bgv_stats* s, const dev_batch& d) {
  s->split = d.split;
  s->miller_lanes = d.miller_coop ? d.miller_coop : 1u;
  s->pairs_per_item = d.pairs_per_item;
  s->msm = d.msm;
  s->lines = d.lines;
  s->defer_from = d.defer_grp ? d.defer_from : d.n_sets;
  s->clear_lanes = d.clear_lanes;
  s->miller_kv = d.miller_kv;
}

// job results, set codes and the batch flag through pinned memory; the
// lodestar_bls_thread_pool_* counters from the host view of the offsets
static int finish_results(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code,
                          bgv_stats* stats) {
  const size_t jr_off = 256, sc_off = jr_off + (((size_t)d.n_jobs * 4 + 255) & ~size_t(255));
  const bool want_sc = set_code && d.n_sets;
  if (int r = pinned_reserve(c->pin_out, c->pin_out_cap, sc_off + (want_sc ? (size_t)d.n_sets * 4 : 0))) return r;
  if (d.n_jobs) HIPCHK(hipMemcpyAsync(c->pin_out + jr_off, w.job_result, (size_t)d.n_jobs * 4, hipMemcpyDeviceToHost, c->st));
  if (want_sc) HIPCHK(hipMemcpyAsync(c->pin_out + sc_off, w.set_code, (size_t)d.n_sets * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out, w.flags, 4, hipMemcpyDeviceToHost, c->st));
  const bool want_uniq = c->hash_pending;  // the class count of this run rides along (written before ev_prep on c->st)
  if (want_uniq) HIPCHK(hipMemcpyAsync(c->pin_out + 64, c->mc.n_uniq, 4, hipMemcpyDeviceToHost, c->st));
  const bool want_pair = c->pair_pending;  // the class count and the identity flag of this run ride along too
  if (want_pair) {
    HIPCHK(hipMemcpyAsync(c->pin_out + 68, c->pc.class_off + c->pc.n_jobs, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(c->pin_out + 72, c->pc.ident, 4, hipMemcpyDeviceToHost, c->st));
  }
  HIPCHK(hipStreamSynchronize(c->st));
  c->staged_pending = false;
  uint32_t flag = 0;
  memcpy(&flag, c->pin_out, 4);
  c->tail_path = {d.batch_tail ? 1u : 0u, d.batch_tail && d.n_jobs && !flag ? 1u : 0u};
  if (want_pair) {
    uint32_t ident = 0;
    memcpy(&c->pair_path.pairs, c->pin_out + 68, 4);
    memcpy(&ident, c->pin_out + 72, 4);
    c->pair_redo = ident != 0;
    c->pair_pending = false;
  }
  if (want_uniq) {
    memcpy(&c->hash_path.hashes, c->pin_out + 64, 4);
    c->hash_pending = false;
  }
  if (d.n_jobs) memcpy(job_result, c->pin_out + jr_off, (size_t)d.n_jobs * 4);
  if (want_sc) memcpy(set_code, c->pin_out + sc_off, (size_t)d.n_sets * 4);
  if (stats) {
    memset(stats, 0, sizeof *stats);
    if (c->timed)
      for (int s = 0; s < ST_COUNT && s < BGV_N_STAGES; s++) HIPCHK(hipEventElapsedTime(&stats->stage_ms[s], c->ev[s], c->ev_end[s]));
    HIPCHK(hipEventElapsedTime(&stats->total_ms, c->ev[0], c->ev[ST_COUNT]));
    stats->n_sets = d.n_sets;
    stats->n_jobs = d.n_jobs;
    stats_layout(stats, d);
    uint32_t valid_jobs = 0, valid_sets = 0;
    const uint32_t* jo = c->jo_host.data();
    for (uint32_t j = 0; j < d.n_jobs; j++)
      if (job_result[j] >= 0) { valid_jobs++; valid_sets += jo[j + 1] - jo[j]; }
    stats->pubkeys_aggregated = c->pk_total;
    stats->batch_retries = (valid_jobs && !flag) ? 1u : 0u;
    stats->batch_sigs_success = flag ? valid_sets : 0u;
  }
  return 0;
}

int bgv_last_stats(bgv_ctx* c, bgv_stats* stats) {
  if (!c || !stats) return fail(BGV_E_INVALID_ARG, "null argument");
  memset(stats, 0, sizeof *stats);
  if (c->run_to <= c->run_from) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->ev[c->run_to]));
  if (c->timed)
    for (int s = c->run_from; s < c->run_to && s < BGV_N_STAGES; s++) HIPCHK(hipEventElapsedTime(&stats->stage_ms[s], c->ev[s], c->ev_end[s]));
  HIPCHK(hipEventElapsedTime(&stats->total_ms, c->ev[c->run_from], c->ev[c->run_to]));
  stats_layout(stats, c->last_d);
  return BGV_OK;
}

// The entries that may merge pairs (bgv_pair_merge): run_stages records
// bgv_pair_stats only inside one of them, and merges only while pm_call is set.
struct pair_entry {
  bgv_ctx* c;
  pair_entry(bgv_ctx* c_, bool may_merge) : c(c_) {
    c->pm_entry = true;
    c->pm_call = may_merge;
    c->pair_path = {};
    c->pair_pending = c->pair_redo = false;
  }
  ~pair_entry() { c->pm_entry = c->pm_call = false; }
};

// the whole pipeline and its results; a merged pass that met an identity class
// is discarded and the batch runs again unmerged (its inputs are still resident)
static int run_and_finish(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code,
                          bgv_stats* stats) {
  if (int r = run_stages(c, d, w, 0, ST_COUNT)) return r;
  if (int r = finish_results(c, d, w, job_result, set_code, stats)) return r;
  if (!c->pair_redo) return 0;
  c->pm_call = false;
  if (int r = run_stages(c, d, w, 0, ST_COUNT)) return r;
  if (int r = finish_results(c, d, w, job_result, set_code, stats)) return r;
  c->pair_path.fallback = 1;
  return 0;
}

// The batch-first tail: the entries whose verdicts come
// from k_batch_final / k_job_final over a batch on the steps path with the
// (job, window) MSM (the window sums it folds).  Called between prepare() and
// work_alloc(); every other entry leaves dev_batch.batch_tail at 0, and with
// it today's tail (the debug entries report per-job values).
static void tail_entry(const bgv_ctx* c, dev_batch& d) {
  d.batch_tail = c->batch_tail != 0 && d.steps_slice && d.msm == 2 && !d.steps_dbg && d.n_jobs ? 1u : 0u;
}

int bgv_verify(bgv_ctx* c, const bgv_batch* b, int32_t* job_result, int32_t* set_code, bgv_stats* stats) {
  if (!c || !b || (!job_result && b->n_jobs)) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  active_guard ag(c->device);
  pair_entry pe(c, c->pair_merge != 0);
  dev_batch d;
  if (int r = prepare(c, b, d, true)) return r;
  tail_entry(c, d);
  dev_work w;
  if (int r = work_alloc(c, d, w)) return r;
  return run_and_finish(c, d, w, job_result, set_code, stats);
}

int bgv_pair_merge(bgv_ctx* c, int32_t mode) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  if (mode != 0 && mode != 1) return fail(BGV_E_INVALID_ARG, "bgv_pair_merge mode %d", mode);
  c->pair_merge = mode;
  return BGV_OK;
}

int bgv_batch_tail(bgv_ctx* c, int32_t mode) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  if (mode < -1 || mode > 1) return fail(BGV_E_INVALID_ARG, "bgv_batch_tail mode %d", mode);
  c->batch_tail = mode;
  return BGV_OK;
}

int bgv_tail_stats(bgv_ctx* c, bgv_tail_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  *out = c->tail_path;
  return BGV_OK;
}

int bgv_pair_stats(bgv_ctx* c, bgv_pair_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  if (c->pair_pending) {  // a call that failed between its launches and its results
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(&c->pair_path.pairs, c->pc.class_off + c->pc.n_jobs, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pair_pending = false;
  }
  *out = c->pair_path;
  return BGV_OK;
}

// ---- committee bitfields over resident index lists ---------------------------
// include/bgv.h bgv_verify_bits.  The expansion (bgv_bits.hip) runs on the main
// stream in front of the ordinary pipeline and leaves an on-device bgv_batch in
// all but name: pk_off / pk_idx in context-owned buffers, everything else the
// staged (or the caller's device) arrays.
static_assert(sizeof(bgv_set_src) == sizeof(bits_src) && BGV_MAX_INDEX_LISTS == BITS_MAX_LISTS &&
                  BGV_SRC_EXPLICIT == BITS_SRC_EXPLICIT,
              "bits_expand.h mirrors include/bgv.h");

int bgv_index_list_set(bgv_ctx* c, uint32_t id, const uint32_t* idx, uint32_t n) {
  if (!c || (!idx && n)) return fail(BGV_E_INVALID_ARG, "null argument");
  if (id >= BGV_MAX_INDEX_LISTS) return fail(BGV_E_INVALID_ARG, "index list %u: ids are below %u", id, (unsigned)BGV_MAX_INDEX_LISTS);
  for (uint32_t i = 0; i < n; i++)
    if (idx[i] & 0x80000000u)
      return fail(BGV_E_INVALID_ARG, "index list %u: entry %u (0x%08x) has bit 31 set (lists hold table rows only)", id, i, idx[i]);
  HIPCHK(hipSetDevice(c->device));
  uint32_t* p = nullptr;
  if (n) {
    if (hipMalloc((void**)&p, (size_t)n * 4) != hipSuccess) return fail(BGV_E_HIP, "hipMalloc(%zu) failed", (size_t)n * 4);
    hipError_t e = hipMemcpyAsync(p, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return fail(BGV_E_HIP, "index list %u upload: %s", id, hipGetErrorString(e));
    }
  }
  if (c->idx_list[id]) {
    // a batch of this context that is still in flight (bgv_partial leaves one,
    // a failed call may) can read the old list from any of the four streams
    if (int r = ctx_drain(c)) { if (p) (void)hipFree(p); return r; }
    (void)hipFree(c->idx_list[id]);
    if (c->idx_sums[id]) (void)hipFree(c->idx_sums[id]);  // sums of the old list: the caller asks again
    c->idx_sums[id] = nullptr;
  }
  c->idx_list[id] = p;
  c->idx_list_n[id] = n;
  uint32_t mx = 0;
  for (uint32_t i = 0; i < n; i++) mx = idx[i] > mx ? idx[i] : mx;
  c->idx_list_max[id] = mx;
  return BGV_OK;
}

int bgv_index_list_sums(bgv_ctx* c, uint32_t id, uint32_t enable) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null argument");
  if (id >= BGV_MAX_INDEX_LISTS) return fail(BGV_E_INVALID_ARG, "index list %u: ids are below %u", id, (unsigned)BGV_MAX_INDEX_LISTS);
  HIPCHK(hipSetDevice(c->device));
  if (!enable) return sums_drop(c, id);
  if (!c->idx_list[id]) return fail(BGV_E_INVALID_ARG, "index list %u is not set", id);
  const uint32_t n = c->idx_list_n[id];
  if (c->idx_list_max[id] >= c->table_n)
    return fail(BGV_E_TABLE_RANGE, "index list %u holds row %u, the table has %u rows: a prefix over a row that does not exist cannot be built",
                id, c->idx_list_max[id], c->table_n);
  if (int r = sums_drop(c, id)) return r;  // rebuilt from the rows as they are now
  g1j *S = nullptr, *tmp = nullptr;
  const size_t entries = (size_t)n + 1, n_tmp = sums_tmp_entries(n);
  if (hipMalloc((void**)&S, entries * sizeof(g1j)) != hipSuccess) return fail(BGV_E_HIP, "hipMalloc(%zu) failed", entries * sizeof(g1j));
  if (hipMalloc((void**)&tmp, n_tmp * sizeof(g1j)) != hipSuccess) {
    (void)hipFree(S);
    return fail(BGV_E_HIP, "hipMalloc(%zu) failed", n_tmp * sizeof(g1j));
  }
  // timed with the expansion's event pair: no batch is in flight on this stream here
  c->bits_timed = false;
  c->sums_build_ms = 0.f;
  (void)hipEventRecord(c->ev_bits[0], c->st);
  launch_list_sums(c->st, c->table, c->table_n, c->idx_list[id], n, S, tmp);
  hipError_t e = hipGetLastError();
  (void)hipEventRecord(c->ev_bits[1], c->st);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);
  if (e == hipSuccess) (void)hipEventElapsedTime(&c->sums_build_ms, c->ev_bits[0], c->ev_bits[1]);
  (void)hipFree(tmp);
  if (e != hipSuccess) {
    (void)hipFree(S);
    return fail(BGV_E_HIP, "index list %u sums: %s", id, hipGetErrorString(e));
  }
  c->idx_sums[id] = S;
  return BGV_OK;
}

int bgv_index_list_sums_ms(bgv_ctx* c, float* ms) {
  if (!c || !ms) return fail(BGV_E_INVALID_ARG, "null argument");
  *ms = c->sums_build_ms;
  return BGV_OK;
}

int bgv_index_list_has_sums(bgv_ctx* c, uint32_t id, uint32_t* has) {
  if (!c || !has) return fail(BGV_E_INVALID_ARG, "null argument");
  if (id >= BGV_MAX_INDEX_LISTS) return fail(BGV_E_INVALID_ARG, "index list %u: ids are below %u", id, (unsigned)BGV_MAX_INDEX_LISTS);
  *has = c->idx_sums[id] ? 1u : 0u;
  return BGV_OK;
}

int bgv_debug_index_list_sums(bgv_ctx* c, uint32_t id, uint32_t first, uint32_t n, uint8_t* out96) {
  if (!c || (!out96 && n)) return fail(BGV_E_INVALID_ARG, "null argument");
  if (id >= BGV_MAX_INDEX_LISTS || !c->idx_sums[id]) return fail(BGV_E_INVALID_ARG, "index list %u has no sums", id);
  if ((uint64_t)first + n > (uint64_t)c->idx_list_n[id] + 1)
    return fail(BGV_E_INVALID_ARG, "entries [%u, %llu) past the %llu sums of list %u", first, (unsigned long long)first + n,
                (unsigned long long)c->idx_list_n[id] + 1, id);
  if (n == 0) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->gen_out.ensure((size_t)n * 96)) return r;
  launch_sums_export(c->st, c->idx_sums[id] + first, c->gen_out.p, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out96, c->gen_out.p, (size_t)n * 96, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

int bgv_index_list_len(bgv_ctx* c, uint32_t id, uint32_t* n) {
  if (!c || !n) return fail(BGV_E_INVALID_ARG, "null argument");
  if (id >= BGV_MAX_INDEX_LISTS) return fail(BGV_E_INVALID_ARG, "index list %u: ids are below %u", id, (unsigned)BGV_MAX_INDEX_LISTS);
  *n = c->idx_list_n[id];
  return BGV_OK;
}

static int bits_check_args(const bgv_bits_batch* b, bool need_sigs) {
  if (!b) return fail(BGV_E_INVALID_ARG, "batch is NULL");
  if (!b->job_offsets || (b->n_sets && (!b->src || (need_sigs && (!b->msgs || !b->sigs || !b->sig_len)))))
    return fail(BGV_E_INVALID_ARG, "missing batch array");
  if (b->bits_len && !b->bits) return fail(BGV_E_INVALID_ARG, "bits_len > 0 but bits is NULL");
  if (b->n_indices && !b->pk_indices) return fail(BGV_E_INVALID_ARG, "n_indices > 0 but pk_indices is NULL");
  if (b->n_raw && !b->raw_pks) return fail(BGV_E_INVALID_ARG, "n_raw > 0 but raw_pks is NULL");
  return BGV_OK;
}

// The contract of a host batch, on the copies the device will see: `v` holds
// host pointers to bits and pk_indices; of the lists only "is set" and the
// length are looked at, and of their sums only "has sums".  Fills the key
// total, the largest job and what the complement rule (bits_expand.h) makes of
// the batch: the sets it sends down the complement path (path, may be NULL)
// and the keys the gather then reads.
struct bits_plan_out {
  uint32_t total = 0, max_job = 1;
  uint32_t gathered = 0, n_complement = 0;
};
// the job-offset half: the bgv_batch rules, and the largest job
static int bits_check_jobs(uint32_t n, uint32_t J, const uint32_t* jo, bits_plan_out* out) {
  if (jo[0] != 0 || jo[J] != n) return fail(BGV_E_INVALID_ARG, "job_offsets must span [0, n_sets]");
  uint32_t max_job = 1;
  for (uint32_t j = 0; j < J; j++) {
    if (jo[j + 1] < jo[j]) return fail(BGV_E_INVALID_ARG, "job_offsets not monotone");
    if (jo[j + 1] - jo[j] > max_job) max_job = jo[j + 1] - jo[j];
  }
  out->max_job = max_job;
  return BGV_OK;
}
// the source half (the host plan): every set's source, its key count and its path
static int bits_check_sources(uint32_t n, const bits_src* src, const bits_view& v, bits_plan_out* out, uint8_t* path) {
  uint64_t total = 0, gathered = 0;
  uint32_t n_complement = 0;
  for (uint32_t i = 0; i < n; i++) {
    const bits_src s = src[i];
    const bool expl = s.list == BITS_SRC_EXPLICIT;
    switch (bits_src_check(s, v)) {
      case BITS_OK: break;
      case BITS_E_LIST: return fail(BGV_E_INVALID_ARG, "set %u: index list %u is not set", i, s.list);
      case BITS_E_SPAN:
        if (expl) return fail(BGV_E_INVALID_ARG, "set %u: off %u + len %u past the %u explicit indices", i, s.off, s.len, v.n_indices);
        return fail(BGV_E_INVALID_ARG, "set %u: off %u + len %u past the %u entries of list %u", i, s.off, s.len,
                    bits_list_len(v, s.list), s.list);
      default:
        return fail(BGV_E_INVALID_ARG, "set %u: bits_off %u + %u bitfield bytes past bits_len %u", i, s.bits_off, bits_bytes(s.len), v.bits_len);
    }
    uint64_t cnt = s.len;
    if (!expl) {
      // aggregationBits.intersectValues throws on a length mismatch: a bit above len is one
      if ((s.len & 7u) && (v.bits[(size_t)s.bits_off + bits_bytes(s.len) - 1] >> (s.len & 7u)))
        return fail(BGV_E_INVALID_ARG, "set %u: padding bits above len %u are not zero", i, s.len);
      cnt = 0;
      const uint32_t words = bits_words(s.len);
      for (uint32_t w = 0; w < words; w++) cnt += bits_popc(bits_src_word(s, v, w));
    }
    if (cnt == 0) return fail(BGV_E_EMPTY_SET, "EMPTY_AGGREGATE_ARRAY (set %u)", i);
    total += cnt;
    const bool cm = bits_src_complement(s, v, (uint32_t)cnt);
    gathered += cm ? s.len - cnt : cnt;
    n_complement += cm ? 1u : 0u;
    if (path) path[i] = cm ? 1 : 0;
  }
  if (total > 0xffffffffull) return fail(BGV_E_INVALID_ARG, "the batch's %llu keys do not fit 32 bits", (unsigned long long)total);
  out->total = (uint32_t)total;
  out->gathered = (uint32_t)gathered;
  out->n_complement = n_complement;
  return BGV_OK;
}
static int bits_check_core(uint32_t n, uint32_t J, const uint32_t* jo, const bits_src* src, const bits_view& v,
                           bits_plan_out* out, uint8_t* path) {
  if (int r = bits_check_jobs(n, J, jo, out)) return r;
  return bits_check_sources(n, src, v, out, path);
}

// a host-only view for the checks: of the lists only "is set", the length and
// "has sums" (list_has_sums may be NULL: none)
static void bits_host_view(bits_view& v, const uint32_t* list_len, const uint8_t* list_has_sums) {
  static const uint32_t present = 0;  // a non-NULL stand-in: the check reads no list entry and no sum
  memset(&v, 0, sizeof v);
  for (uint32_t k = 0; k < BGV_MAX_INDEX_LISTS; k++) {
    v.list[k] = list_len[k] ? &present : nullptr;
    v.list_len[k] = list_len[k];
    v.sums[k] = list_len[k] && list_has_sums && list_has_sums[k] ? &present : nullptr;
  }
}

int bgv_bits_plan(const bgv_bits_batch* b, const uint32_t* list_len, const uint8_t* list_has_sums, uint8_t* path,
                  uint64_t* keys_gathered) {
  if (keys_gathered) *keys_gathered = 0;
  if (int r = bits_check_args(b, true)) return r;
  if (!list_len) return fail(BGV_E_INVALID_ARG, "list_len is NULL");
  if (b->on_device) return BGV_OK;
  bits_view v;
  bits_host_view(v, list_len, list_has_sums);
  v.bits = b->bits; v.bits_len = b->bits_len; v.pk_indices = b->pk_indices; v.n_indices = b->n_indices;
  bits_plan_out po;
  if (int r = bits_check_core(b->n_sets, b->n_jobs, b->job_offsets, (const bits_src*)b->src, v, &po, path)) return r;
  if (keys_gathered) *keys_gathered = po.gathered;
  return BGV_OK;
}

int bgv_bits_check(const bgv_bits_batch* b, const uint32_t* list_len) { return bgv_bits_plan(b, list_len, nullptr, nullptr, nullptr); }

// The set-up every entry that expands bitfields shares: bits_args / bits_view
// over the context's lists (and their sums, unless use_sums is false), the
// offset buffer, the per-set windows when a list has sums, and the context's
// record of the batch (bgv_bits_path_stats).  a.src, a.v.bits and
// a.v.pk_indices are the caller's to fill; the tally of an on-device batch is
// zeroed on `st`, the stream the expansion will run on.
static int bits_setup(bgv_ctx* c, bits_args& a, uint32_t n, uint32_t bits_len, uint32_t n_indices, bool on_device, bool use_sums,
                      hipStream_t st) {
  memset(&a, 0, sizeof a);
  a.n_sets = n;
  bool any_sums = false;
  for (uint32_t k = 0; k < BGV_MAX_INDEX_LISTS; k++) {
    a.v.list[k] = c->idx_list[k]; a.v.list_len[k] = c->idx_list_n[k];
    a.v.sums[k] = use_sums ? c->idx_sums[k] : nullptr;
    any_sums = any_sums || a.v.sums[k];
  }
  a.v.bits_len = bits_len;
  a.v.n_indices = n_indices;
  // with sums resident: two tally words behind the scan's total (bgv_internal.h bits_args)
  if (int r = ensure_or_release_lines(c, c->bits_off, (size_t)n + 3)) return r;
  a.pk_off = c->bits_off.p;
  c->bits_any_sums = any_sums;
  c->bits_on_device = on_device;
  c->bits_path = {};
  c->bits_extra_chunks = 0;
  c->bits_n = n;
  if (any_sums) {
    if (int r = ensure_or_release_lines(c, c->bits_win, n ? n : 1)) return r;
    a.win = c->bits_win.p;
    if (on_device) {
      a.tally = a.pk_off + n + 1;
      HIPCHK(hipMemsetAsync(a.tally, 0, 8, st));
    }
  }
  return 0;
}

// the expansion launches on a given stream, in two halves: an on-device batch
// reads the totals back between them
static void bits_launch_count(hipStream_t st, const bits_args& a) {
  launch_bits_count(st, a);
  if (a.n_sets) launch_scan(st, a.pk_off, a.n_sets);
}
// `gathered`: the keys the expansion holds (the scan's total)
static int bits_launch_expand(bgv_ctx* c, hipStream_t st, bits_args& a, uint32_t gathered) {
  if (int r = ensure_or_release_lines(c, c->bits_idx, gathered ? gathered : 1)) return r;
  a.pk_idx = c->bits_idx.p;
  a.cap = gathered;
  launch_bits_expand(st, a);
  return 0;
}
// the totals of an on-device batch, after bits_launch_count on `st`: the host
// learns the gathered keys (buffer and grid bound) and the participating keys
static int bits_read_totals(bgv_ctx* c, hipStream_t st, const bits_args& a) {
  uint32_t tot[2] = {0, 0};
  if (a.n_sets) HIPCHK(hipMemcpyAsync(tot, a.pk_off + a.n_sets, c->bits_any_sums ? 8 : 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->pk_total = c->bits_any_sums ? tot[1] : tot[0];
  c->bits_path.keys_expanded = c->pk_total;
  c->bits_path.keys_gathered = tot[0];
  c->bits_extra_chunks = c->bits_any_sums ? a.n_sets : 0u;  // the complement sets are counted on the device only
  return 0;
}

// prepare() for a bits batch up to the expanded device view: staging and checks
// (host batches), early hash maps, raw keys, the expansion.  Leaves d.pk_off /
// d.pk_idx, c->jo_host and c->pk_total as prepare() does.
// use_sums = false: the full expansion on the direct path whatever is resident.
static int bits_front(bgv_ctx* c, const bgv_bits_batch* b, dev_batch& d, bool need_sigs, bool use_sums = true) {
  if (int r = bits_check_args(b, need_sigs)) return r;
  const uint32_t n = b->n_sets, J = b->n_jobs;
  memset(&d, 0, sizeof d);
  c->busy = c->device >= 0 && c->device < 64 && g_active[c->device].load() >= 2;
  d.n_sets = n; d.n_jobs = J; d.n_raw = b->n_raw; d.table_n = c->table_n; d.table = c->table;
  d.span_log2 = 7;
  c->jo_host.resize((size_t)J + 1);
  bits_args a;
  if (int r = bits_setup(c, a, n, b->bits_len, b->n_indices, b->on_device != 0, use_sums, c->st)) return r;
  d.win = a.win;
  c->bits_timed = need_sigs && (c->cfg.timing >= 0 ? c->cfg.timing != 0 : n >= 65536);
  if (!b->on_device) {
    const uint8_t* raw_dev = nullptr;
    stage_seg segs[9] = {
        {b->job_offsets, ((size_t)J + 1) * 4, (const void**)&d.job_off, 0},
        {b->src, (size_t)n * sizeof(bits_src), (const void**)&a.src, 0},
        {b->bits, (size_t)b->bits_len, (const void**)&a.v.bits, 0},
        {b->pk_indices, (size_t)b->n_indices * 4, (const void**)&a.v.pk_indices, 0},
        {b->msgs, need_sigs ? (size_t)n * 32 : 0, (const void**)&d.msgs, 0},
        {b->raw_pks, (size_t)b->n_raw * 96, (const void**)&raw_dev, 0},
        {b->scalars, need_sigs && b->scalars ? (size_t)n * 8 : 0, (const void**)&d.scalars, 0},
        {b->sigs, need_sigs ? (size_t)n * 192 : 0, (const void**)&d.sigs, 0},
        {b->sig_len, need_sigs ? (size_t)n * 4 : 0, (const void**)&d.sig_len, 0},
    };
    size_t bytes = 0;
    if (int r = stage_pack(c, segs, 9, bytes)) return r;
    // the checks read the pinned copy; the key total sizes the expansion and
    // the gather's grid without a read-back
    bits_view hv = a.v;
    hv.bits = c->pin_in + segs[2].off;
    hv.pk_indices = (const uint32_t*)(c->pin_in + segs[3].off);
    const uint32_t* jo = (const uint32_t*)(c->pin_in + segs[0].off);
    bits_plan_out po;
    if (int r = bits_check_core(n, J, jo, (const bits_src*)(c->pin_in + segs[1].off), hv, &po, nullptr)) return r;
    const uint32_t total = po.gathered;  // what the expansion holds and the gather reads
    d.span_log2 = 0;
    while ((1u << d.span_log2) < po.max_job && d.span_log2 < 16) d.span_log2++;
    memcpy(c->jo_host.data(), jo, c->jo_host.size() * 4);
    c->pk_total = po.total;
    c->bits_path.sets_complement = po.n_complement;
    c->bits_path.keys_expanded = po.total;
    c->bits_path.keys_gathered = po.gathered;
    c->bits_extra_chunks = po.n_complement;
    if (int r = stage_issue(c, bytes)) return r;
    // the messages sit in the staging buffer whose copy is in flight on the
    // main stream: the hash stream waits for it (early_maps, after_staging)
    if (need_sigs)
      if (int r = early_maps(c, d, true)) return r;
    if (!(need_sigs && b->scalars)) d.scalars = nullptr;
    if (!need_sigs) { d.sigs = nullptr; d.sig_len = nullptr; d.msgs = nullptr; }
    if (int r = ensure_or_release_lines(c, c->raw_conv, b->n_raw ? b->n_raw : 1)) return r;
    launch_raw_pks(c->st, raw_dev, c->raw_conv.p, b->n_raw);
    d.raw_pks = c->raw_conv.p;
    if (c->bits_timed) HIPCHK(hipEventRecord(c->ev_bits[0], c->st));
    bits_launch_count(c->st, a);
    if (int r = bits_launch_expand(c, c->st, a, total)) return r;
    if (c->bits_timed) HIPCHK(hipEventRecord(c->ev_bits[1], c->st));
  } else {
    d.job_off = b->job_offsets;
    a.src = (const bits_src*)b->src;
    a.v.bits = b->bits;
    a.v.pk_indices = b->pk_indices;
    d.msgs = b->msgs; d.sigs = b->sigs; d.sig_len = b->sig_len;
    if (need_sigs)
      if (int r = early_maps(c, d, false)) return r;
    if (int r = ensure_or_release_lines(c, c->raw_conv, b->n_raw ? b->n_raw : 1)) return r;
    launch_raw_pks(c->st, b->raw_pks, c->raw_conv.p, b->n_raw);
    d.raw_pks = c->raw_conv.p;
    if (c->bits_timed) HIPCHK(hipEventRecord(c->ev_bits[0], c->st));
    bits_launch_count(c->st, a);
    HIPCHK(hipGetLastError());
    // the host needs the job offsets (stats) and the key total (buffer and grid bound),
    // with sums resident the gathered total and the participating total together
    HIPCHK(hipMemcpyAsync(c->jo_host.data(), b->job_offsets, c->jo_host.size() * 4, hipMemcpyDeviceToHost, c->st));
    if (int r = bits_read_totals(c, c->st, a)) return r;
    if (int r = bits_launch_expand(c, c->st, a, c->bits_path.keys_gathered)) return r;
    if (c->bits_timed) HIPCHK(hipEventRecord(c->ev_bits[1], c->st));
  }
  HIPCHK(hipGetLastError());
  d.pk_off = c->bits_off.p;
  d.pk_idx = c->bits_idx.p;
  return 0;
}

// prepare_layout() for a bits batch: the pipeline variant goes by the set
// count as ever; the gather's grid bound by the keys it reads, plus one window
// chunk per complement set: sum ceil(k_i / 32) + windows <= gathered / 32 + n + windows
static int bits_layout(bgv_ctx* c, dev_batch& d, const uint64_t* scalars, bool scalars_staged) {
  if (int r = prepare_layout(c, d, scalars, scalars_staged)) return r;
  if (d.win) d.chunk_bound = c->bits_path.keys_gathered / PK_CHUNK + d.n_sets + c->bits_extra_chunks;
  return 0;
}

int bgv_bits_path_stats(bgv_ctx* c, bgv_bits_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  if (c->bits_any_sums && c->bits_on_device) {  // counted by k_bits_count: fetched when asked for
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(&c->bits_path.sets_complement, c->bits_off.p + c->bits_n + 2, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  *out = c->bits_path;
  return BGV_OK;
}

// the same-message entries hash per group on their own (their retries may pass
// through run_stages): bgv_hash_stats reports zeros after them
static void hash_path_clear(bgv_ctx* c) {
  if (!c) return;
  c->hash_path = {};
  c->hash_pending = false;
  c->pair_path = {};  // nor do they merge pairs: bgv_pair_stats reports zeros as well
  c->pair_pending = c->pair_redo = false;
}

int bgv_hash_stats(bgv_ctx* c, bgv_hash_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  if (c->hash_pending) {  // a call that failed between its launches and its results
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(&c->hash_path.hashes, c->mc.n_uniq, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->hash_pending = false;
  }
  *out = c->hash_path;
  return BGV_OK;
}

int bgv_miller_path_stats(bgv_ctx* c, bgv_miller_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  *out = c->miller_path;
  return BGV_OK;
}

int bgv_verify_bits(bgv_ctx* c, const bgv_bits_batch* b, int32_t* job_result, int32_t* set_code, bgv_stats* stats) {
  if (!c || !b || (!job_result && b->n_jobs)) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  active_guard ag(c->device);
  pair_entry pe(c, c->pair_merge != 0);
  dev_batch d;
  if (int r = bits_front(c, b, d, true)) return r;
  if (int r = bits_layout(c, d, b->scalars, b->scalars && !b->on_device)) return r;
  tail_entry(c, d);
  dev_work w;
  if (int r = work_alloc(c, d, w)) return r;
  return run_and_finish(c, d, w, job_result, set_code, stats);
}

int bgv_bits_expand_ms(bgv_ctx* c, float* ms) {
  if (!c || !ms) return fail(BGV_E_INVALID_ARG, "null argument");
  *ms = 0.f;
  if (!c->bits_timed) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->ev_bits[1]));
  HIPCHK(hipEventElapsedTime(ms, c->ev_bits[0], c->ev_bits[1]));
  return BGV_OK;
}

int bgv_debug_bits_expand(bgv_ctx* c, const bgv_bits_batch* b, uint32_t* pk_offsets, uint32_t* pk_indices, uint32_t cap,
                          uint32_t* total) {
  if (!c || !b || !pk_offsets || !total || (!pk_indices && cap)) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  dev_batch d;
  if (int r = bits_front(c, b, d, false, false)) return r;
  HIPCHK(hipMemcpyAsync(pk_offsets, d.pk_off, ((size_t)b->n_sets + 1) * 4, hipMemcpyDeviceToHost, c->st));
  const uint32_t t = c->pk_total;
  if (t && t <= cap) HIPCHK(hipMemcpyAsync(pk_indices, d.pk_idx, (size_t)t * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->staged_pending = false;
  *total = t;
  if (t > cap) return fail(BGV_E_INVALID_ARG, "the expansion holds %u indices, pk_indices has room for %u", t, cap);
  return BGV_OK;
}

int bgv_debug_bits_keys(bgv_ctx* c, const bgv_bits_batch* b, uint8_t* pk_agg96, uint8_t* path, int32_t* pk_code) {
  if (!c || !b) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  dev_batch d;
  if (int r = bits_front(c, b, d, false)) return r;
  if (int r = bits_layout(c, d, nullptr, false)) return r;  // the scaling needs scalars: drawn on the device
  dev_work w;
  if (int r = work_alloc(c, d, w)) return r;
  const uint32_t n = d.n_sets;
  if (int r = c->pk_agg.ensure(n ? n : 1)) return r;
  w.pk_agg = c->pk_agg.p;
  if (int r = run_stages(c, d, w, ST_PK, ST_PK_SCALE + 1)) return r;
  if (int r = c->dbg_out.ensure((size_t)n * 96 + 1)) return r;
  launch_export_g1a(c->st, w.pk_agg, c->dbg_out.p, n);
  HIPCHK(hipGetLastError());
  std::vector<pk_window> win(d.win ? n : 0);
  if (n && pk_agg96) HIPCHK(hipMemcpyAsync(pk_agg96, c->dbg_out.p, (size_t)n * 96, hipMemcpyDeviceToHost, c->st));
  if (n && pk_code) HIPCHK(hipMemcpyAsync(pk_code, w.pk_code, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (n && d.win) HIPCHK(hipMemcpyAsync(win.data(), d.win, (size_t)n * sizeof(pk_window), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->staged_pending = false;
  if (path)
    for (uint32_t i = 0; i < n; i++) path[i] = d.win && win[i].hi ? 1 : 0;
  return BGV_OK;
}

// ---- same-message batches ---------------------------------------------------
// Three entries over one pipeline (include/bgv.h; DESIGN.md section 3c holds
// the table of what differs between them):
//   bgv_verify_same_message      a set has one key
//     (IBlsVerifier.verifySignatureSetsSameMessage)
//   bgv_verify_same_message_agg  a set's key is an aggregate, PK_i = sum_j pk_{i,j}
//   bgv_verify_same_message_bits the aggregate's members given as bgv_verify_bits
//                                gives them
// A front (sm_run, sma_run, smb_run) checks its batch, cuts the segments, stages
// its arrays and fills an sm_dev; sm_back is the device half.  Layout:
//   st      : sig decode + subgroup -> [set sums] classify -> G2 bucket MSM per
//             segment (k_msm_digit / k_msm_job over the real sets, job = segment)
//             -> [pk, hash] apply -> Miller, folds, final exponentiations on
//             the VIRTUAL batch (one set = one job = one segment)
//   st_pk   : aggregate keys: [expansion of bitfield sets ->] chunk set-up ->
//             gather (k_pk_chunk) -> per-set fold (k_sma_set_sum) beside the
//             signature decode; then [classify] the weighted G1 sum per segment
//             (bgv_same_msg.hip)
//   st_hash : one hash per group (the latency-mode hash kernels); aggregate
//             keys: then [apply] the (P_seg, H(m)) pairs beside the
//             (-G1, S_seg) ones
// then, only when the whole-batch check failed, the surviving sets of the
// failing segments as one-set jobs of the ordinary pipeline (an aggregate key
// enters as a raw key); or, on a context in bgv_sm_retry mode 1, as subs of 8
// and then the sets of the failing subs (sm_split_retry).

// the rules every same-message batch shares; what passes has n_sets == 0 (and
// no group: nothing more to check) or 1 <= n_groups <= n_sets
template <class B>
static int sm_check_counts(const B* b) {
  if (!b) return fail(BGV_E_INVALID_ARG, "batch is NULL");
  if (b->n_sets == 0 && b->n_groups == 0) return BGV_OK;
  if (b->n_groups > b->n_sets) return fail(BGV_E_INVALID_ARG, "n_groups %u > n_sets %u (a group is never empty)", b->n_groups, b->n_sets);
  if (b->n_groups == 0) return fail(BGV_E_INVALID_ARG, "n_sets %u without a group", b->n_sets);
  return BGV_OK;
}

// `go`: the copy of the group offsets the segments are cut from
static int sm_check_groups(uint32_t n, uint32_t G, const uint32_t* go) {
  if (go[0] != 0 || go[G] != n) return fail(BGV_E_INVALID_ARG, "group_offsets must span [0, n_sets]");
  for (uint32_t g = 0; g < G; g++) {
    if (go[g + 1] < go[g]) return fail(BGV_E_INVALID_ARG, "group_offsets not monotone");
    if (go[g + 1] == go[g]) return fail(BGV_E_INVALID_ARG, "group %u is empty", g);
  }
  return BGV_OK;
}

// caller-given scalars (NULL: none given, drawn on the device)
static int scalars_nonzero(const uint64_t* sc, uint32_t n) {
  if (sc)
    for (uint32_t i = 0; i < n; i++)
      if (!sc[i]) return fail(BGV_E_INVALID_ARG, "scalars[%u] is zero", i);
  return BGV_OK;
}

static int sm_check_args(const bgv_sm_batch* b) {
  if (int r = sm_check_counts(b)) return r;
  if (b->n_sets == 0) return BGV_OK;
  if (!b->group_offsets || !b->pk_indices || !b->msgs || !b->sigs || !b->sig_len) return fail(BGV_E_INVALID_ARG, "missing batch array");
  if (b->n_raw && !b->raw_pks) return fail(BGV_E_INVALID_ARG, "n_raw > 0 but raw_pks is NULL");
  return BGV_OK;
}

static int sm_check_args(const bgv_sma_batch* b) {
  if (int r = sm_check_counts(b)) return r;
  if (b->n_sets == 0) return BGV_OK;
  if (!b->group_offsets || !b->pk_offsets || !b->pk_indices || !b->msgs || !b->sigs || !b->sig_len)
    return fail(BGV_E_INVALID_ARG, "missing batch array");
  if (b->n_raw && !b->raw_pks) return fail(BGV_E_INVALID_ARG, "n_raw > 0 but raw_pks is NULL");
  return BGV_OK;
}

static int sm_check_args(const bgv_smb_batch* b) {
  if (int r = sm_check_counts(b)) return r;
  if (b->n_sets == 0) return BGV_OK;
  if (!b->group_offsets || !b->src || !b->msgs || !b->sigs || !b->sig_len) return fail(BGV_E_INVALID_ARG, "missing batch array");
  if (b->bits_len && !b->bits) return fail(BGV_E_INVALID_ARG, "bits_len > 0 but bits is NULL");
  if (b->n_indices && !b->pk_indices) return fail(BGV_E_INVALID_ARG, "n_indices > 0 but pk_indices is NULL");
  if (b->n_raw && !b->raw_pks) return fail(BGV_E_INVALID_ARG, "n_raw > 0 but raw_pks is NULL");
  return BGV_OK;
}

// `po`: the copy of the key offsets the device will see; total: the length of pk_indices that is staged
static int sma_check_keys(const bgv_sma_batch* b, const uint32_t* po, uint32_t total) {
  const uint32_t n = b->n_sets;
  if (po[0] != 0 || po[n] != total) return fail(BGV_E_INVALID_ARG, "pk_offsets must span [0, total]");
  for (uint32_t i = 0; i < n; i++)
    if (po[i + 1] < po[i]) return fail(BGV_E_INVALID_ARG, "pk_offsets not monotone");
  for (uint32_t i = 0; i < n; i++)
    if (po[i + 1] == po[i]) return fail(BGV_E_EMPTY_SET, "EMPTY_AGGREGATE_ARRAY (set %u)", i);
  return BGV_OK;
}

int bgv_sm_check(const bgv_sm_batch* b) {
  if (int r = sm_check_args(b)) return r;
  if (b->on_device || b->n_sets == 0) return BGV_OK;
  if (int r = sm_check_groups(b->n_sets, b->n_groups, b->group_offsets)) return r;
  return scalars_nonzero(b->scalars, b->n_sets);
}

int bgv_sma_check(const bgv_sma_batch* b) {
  if (int r = sm_check_args(b)) return r;
  if (b->on_device || b->n_sets == 0) return BGV_OK;
  if (int r = sm_check_groups(b->n_sets, b->n_groups, b->group_offsets)) return r;
  if (int r = sma_check_keys(b, b->pk_offsets, b->pk_offsets[b->n_sets])) return r;
  return scalars_nonzero(b->scalars, b->n_sets);
}

int bgv_smb_check(const bgv_smb_batch* b, const uint32_t* list_len) {
  if (int r = sm_check_args(b)) return r;
  if (!list_len) return fail(BGV_E_INVALID_ARG, "list_len is NULL");
  if (b->on_device || b->n_sets == 0) return BGV_OK;
  if (int r = sm_check_groups(b->n_sets, b->n_groups, b->group_offsets)) return r;
  bits_view v;
  bits_host_view(v, list_len, nullptr);
  v.bits = b->bits; v.bits_len = b->bits_len; v.pk_indices = b->pk_indices; v.n_indices = b->n_indices;
  bits_plan_out po;
  if (int r = bits_check_sources(b->n_sets, (const bits_src*)b->src, v, &po, nullptr)) return r;
  return scalars_nonzero(b->scalars, b->n_sets);
}

// the segments of a same-message batch: every group cut into runs of at most SM_SEG sets
struct sm_segs {
  std::vector<uint32_t> seg_off, seg_group, group_seg, iota;
  uint32_t S = 0;
};
static void sm_cut_segments(const std::vector<uint32_t>& go, uint32_t n, sm_segs& sg) {
  const uint32_t G = (uint32_t)go.size() - 1;
  sg.group_seg.resize((size_t)G + 1);
  sg.seg_off.reserve(n / SM_SEG + G + 1);
  for (uint32_t g = 0; g < G; g++) {
    sg.group_seg[g] = (uint32_t)sg.seg_off.size();
    for (uint32_t i = go[g]; i < go[g + 1]; i += SM_SEG) { sg.seg_off.push_back(i); sg.seg_group.push_back(g); }
  }
  sg.S = (uint32_t)sg.seg_off.size();
  sg.group_seg[G] = sg.S;
  sg.seg_off.push_back(n);
  sg.iota.resize((size_t)sg.S + 1);
  for (uint32_t s = 0; s <= sg.S; s++) sg.iota[s] = s;
}

// A same-message call between its front and sm_back: the segments, and the
// device view of the batch once its arrays are staged (or resident).  sm_open
// fills what every entry has; a front adds the segment tables and its key side.
struct sm_dev {
  uint32_t n = 0, G = 0, n_raw = 0;  // n == 0 after sm_open: an empty batch, the call is done
  std::optional<active_guard> busy;
  std::chrono::steady_clock::time_point t0;
  sm_segs sg;
  const uint32_t *d_seg_off = nullptr, *d_seg_group = nullptr, *d_group_seg = nullptr, *d_iota = nullptr;
  const uint32_t *d_po = nullptr, *d_idx = nullptr, *d_len = nullptr;
  const uint8_t *d_msgs = nullptr, *d_sigs = nullptr, *d_raw = nullptr;
  const uint64_t* d_scalars = nullptr;
  bool draw_scalars = false;  // the caller gave none: drawn on the device (d_scalars is then not read)
  // The key side.  One key per set: d_idx[i] names it, d_po and win stay NULL and
  // chunk_bound n, nothing is gathered.  Aggregates: d_po / d_idx are the lists
  // the gather on the pubkey stream sums into PK_i.
  bool agg = false;
  uint32_t chunk_bound = 0;  // grid bound of the gather
  // bgv_verify_same_message_bits: the per-set windows (contexts with sums, else
  // NULL) and the expansion still to run on the pubkey stream
  const pk_window* win = nullptr;
  bits_args* expand = nullptr;
  bool expand_count = false;  // count and scan too (host batches: their totals come from the host plan)
  uint32_t gathered = 0;      // keys the expansion holds
};

// the opening of every front; k.n stays 0 for an empty batch
template <class B>
static int sm_open(bgv_ctx* c, const B* b, uint8_t* set_valid, bgv_sm_stats* stats, sm_dev& k) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  if (int r = sm_check_args(b)) return r;
  if (stats) memset(stats, 0, sizeof *stats);
  if (b->n_sets == 0) return BGV_OK;
  if (!set_valid) return fail(BGV_E_INVALID_ARG, "set_valid is NULL");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  k.busy.emplace(c->device);
  k.t0 = std::chrono::steady_clock::now();
  k.n = b->n_sets; k.G = b->n_groups; k.n_raw = b->n_raw;
  k.d_len = b->sig_len; k.d_msgs = b->msgs; k.d_sigs = b->sigs; k.d_raw = b->raw_pks; k.d_scalars = b->scalars;
  k.draw_scalars = !b->scalars;
  k.chunk_bound = k.n;
  return BGV_OK;
}

// The group offsets come to the host first: the segments are cut from this
// copy.  An on-device batch may bring one more word (d_word -> *h_word) with
// the same wait.
static int sm_groups(bgv_ctx* c, sm_dev& k, const uint32_t* group_offsets, bool on_device, const uint32_t* d_word = nullptr,
                     uint32_t* h_word = nullptr) {
  std::vector<uint32_t> go((size_t)k.G + 1);
  if (on_device) {
    HIPCHK(hipMemcpyAsync(go.data(), group_offsets, go.size() * 4, hipMemcpyDeviceToHost, c->st));
    if (d_word) HIPCHK(hipMemcpyAsync(h_word, d_word, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  } else {
    memcpy(go.data(), group_offsets, go.size() * 4);
  }
  if (int r = sm_check_groups(k.n, k.G, go.data())) return r;
  sm_cut_segments(go, k.n, k.sg);
  return BGV_OK;
}

// bgv_verify_same_message_aggregate: what sm_back computes on top of the
// verdicts (the three other fronts pass none)
struct sm_agg_req {
  const uint8_t* d_take = nullptr;  // device [n] or NULL
  const uint8_t* d_prev = nullptr;  // device [G][96] or NULL
  uint8_t* agg_sig96 = nullptr;     // host outputs (bgv_sm_agg)
  uint32_t* agg_count = nullptr;
  int32_t* agg_code = nullptr;
};

// A virtual batch of N sets, set t = job t (iota: its job offsets), from the
// Miller loops to the per-job verdicts: the first pass's segments, and the subs
// and leaves of the split retry.  w holds its rpk_aff, h_aff, s_aff, s_inf,
// pk_code and job_code.
static int sm_virtual_batch(bgv_ctx* c, uint32_t N, const uint32_t* d_iota, const dev_work& w, bool agg) {
  dev_batch dB;
  memset(&dB, 0, sizeof dB);
  dB.n_sets = N; dB.n_jobs = N; dB.pairs_per_item = 1; dB.job_lanes = 36;
  dB.miller_coop = N < 2000 ? 36u : (N < 6000 ? 18u : 6u);
  dB.job_off = d_iota;
  int first = ST_MILLER;  // one key per set: every stage of the virtual batch in order on st
  if (agg) {
    // the (P_seg, H(m)) pairs on the hash stream beside the (-G1, S_seg) pairs, as
    // run_stages places them: a few thousand lanes each, one after the other they
    // would both be on the critical path
    HIPCHK(hipEventRecord(c->ev_prep, c->st));
    HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_prep, 0));
    launch_stage(c->st_hash, ST_MILLER, dB, w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_dep[ST_MILLER], c->st_hash));
    launch_stage(c->st, ST_MILLER_JOBS, dB, w);
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_MILLER], 0));
    first = ST_F_TREE;
  }
  for (int s = first; s <= ST_JOB_FINAL; s++) launch_stage(c->st, s, dB, w);
  HIPCHK(hipGetLastError());
  return BGV_OK;
}

// The split retry (bgv_sm_retry mode 1, sm_split.h).
// list / list_group: the surviving sets of the retried segments and their
// groups; sub_off: the subs (offsets into list).  w is the first pass's work
// view: its sig_aff, with sm_hg, sma_pk and sm_skip, is read here and by the
// second pass of bgv_verify_same_message_aggregate, so both levels work in
// c->sm_split and in work buffers no larger than the first pass's set-sized
// ones (work_alloc never moves a buffer that is large enough).  jr1 / jr2:
// pinned room for the sub and leaf verdicts, list.size() words each.
static int sm_split_retry(bgv_ctx* c, const sm_dev& k, const dev_work& w, const uint64_t* d_scalars,
                          const std::vector<uint32_t>& list, const std::vector<uint32_t>& list_group,
                          const std::vector<uint32_t>& sub_off, int32_t* jr1, int32_t* jr2, uint8_t* set_valid,
                          bgv_sm_retry_path& path) {
  const uint32_t nr = (uint32_t)list.size(), T = (uint32_t)sub_off.size() - 1, G = k.G, n_raw = k.n_raw;
  const size_t a = 256;
  auto up = [&](size_t x) { return (x + a - 1) & ~(a - 1); };
  // level 1's inputs, then what the host sends: [list | list_group | sub_off | iota] and level 2's [leaf | leaf_group]
  const size_t o_idx = 0, o_pk = o_idx + up((size_t)nr * 4), o_scal = o_pk + (k.agg ? up((size_t)nr * sizeof(g1j)) : 0),
               o_sig = o_scal + up((size_t)nr * 8), o_skip = o_sig + up((size_t)nr * sizeof(g2a)), o_sg = o_skip + up((size_t)nr * 4),
               o_host = o_sg + up((size_t)T * 4), host_words = 2 * (size_t)nr + 2 * ((size_t)T + 1),
               o_leaf = o_host + up(host_words * 4), o_iota2 = o_leaf + up(2 * (size_t)nr * 4),
               total = o_iota2 + up(((size_t)nr + 1) * 4);
  int r = 0;
  if ((r = c->sm_split.ensure(total)) || (r = c->sm_seg_code.ensure(T)) || (r = c->sm_win.ensure((size_t)T * 16))) return r;
  uint8_t* base = c->sm_split.p;
  uint32_t* d_host = (uint32_t*)(base + o_host);
  const uint32_t *d_list = d_host, *d_list_group = d_host + nr, *d_sub_off = d_host + 2 * (size_t)nr,
                 *d_iota1 = d_host + 2 * (size_t)nr + T + 1;
  std::vector<uint32_t> hv;
  hv.reserve(host_words);
  hv.insert(hv.end(), list.begin(), list.end());
  hv.insert(hv.end(), list_group.begin(), list_group.end());
  hv.insert(hv.end(), sub_off.begin(), sub_off.end());
  for (uint32_t t = 0; t <= T; t++) hv.push_back(t);
  HIPCHK(hipMemcpyAsync(d_host, hv.data(), host_words * 4, hipMemcpyHostToDevice, c->st));

  // ---- level 1: sub t = set t = job t; view A1 (the compacted sets, one job per sub) gives its sums
  dev_batch dA;
  memset(&dA, 0, sizeof dA);
  dA.n_sets = nr; dA.n_jobs = T; dA.n_raw = n_raw; dA.table_n = c->table_n; dA.table = c->table;
  dA.span_log2 = 6; dA.job_lanes = 36; dA.pairs_per_item = 1; dA.msm = 4; dA.clear_lanes = 9;
  dA.chunk_bound = nr; dA.defer_from = nr;
  dA.job_off = d_sub_off; dA.pk_idx = (const uint32_t*)(base + o_idx); dA.raw_pks = c->raw_conv.p;
  dA.scalars = (const uint64_t*)(base + o_scal);
  dev_work w1;
  if ((r = work_alloc(c, dA, w1))) return r;
  sm_split q;
  memset(&q, 0, sizeof q);
  q.n = nr; q.n_subs = T; q.list = d_list; q.list_group = d_list_group; q.sub_off = d_sub_off;
  q.scalars = d_scalars; q.sig_aff = w.sig_aff;
  q.o_scalars = (uint64_t*)(base + o_scal); q.o_sig = (g2a*)(base + o_sig); q.o_skip = (uint32_t*)(base + o_skip);
  q.o_sub_group = (uint32_t*)(base + o_sg);
  if (k.agg) { q.pk_set = c->sma_pk.p; q.o_pk = (g1j*)(base + o_pk); }
  else { q.pk_idx = k.d_idx; q.o_idx = (uint32_t*)(base + o_idx); }
  launch_sm_split_gather(c->st, q);
  HIPCHK(hipGetLastError());
  sm_view v;
  memset(&v, 0, sizeof v);
  v.n_sets = nr; v.n_segs = T; v.n_groups = G; v.n_raw = n_raw; v.table_n = c->table_n;
  v.seg_off = d_sub_off; v.seg_group = q.o_sub_group; v.pk_idx = q.o_idx; v.raw_pks = c->raw_conv.p; v.table = c->table;
  v.scalars = q.o_scalars; v.skip = q.o_skip;
  v.win = c->sm_win.p; v.p_seg = w1.rpk_aff; v.seg_code = c->sm_seg_code.p; v.h_group = c->sm_hg.p; v.h_seg = w1.h_aff;
  v.pk_code_v = w1.pk_code; v.job_code_v = w1.job_code; v.s_seg = w1.s_aff; v.s_inf = w1.s_inf;
  v.pk_set = q.o_pk;
  HIPCHK(hipEventRecord(c->ev_fork, c->st));  // P_sub on the pubkey stream beside S_sub, as in the first pass
  HIPCHK(hipStreamWaitEvent(c->st_pk, c->ev_fork, 0));
  if (k.agg) launch_sma_g1_sum(c->st_pk, v);
  else launch_sm_g1_sum(c->st_pk, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_dep[ST_PK_SCALE], c->st_pk));
  {
    dev_work wz = w1;  // the compacted signatures; every set of the list is live
    wz.sig_aff = q.o_sig;
    wz.sig_code = c->sm_zero.p;
    wz.pk_code = c->sm_zero.p;
    wz.sig_inf = q.o_skip;
    launch_stage(c->st, ST_SIG_SCALE, dA, wz);
    launch_stage(c->st, ST_S_TREE, dA, wz);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_PK_SCALE], 0));
  launch_sm_apply(c->st, v);
  if ((r = sm_virtual_batch(c, T, d_iota1, w1, k.agg))) return r;
  HIPCHK(hipMemcpyAsync(jr1, w1.job_result, (size_t)T * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  sm_split_counts cnt = {0, 0, 0, 0};
  sm_split_tally(cnt, sub_off.data(), jr1, T);
  path.subs = cnt.subs; path.subs_failed = cnt.subs_failed; path.leaves = cnt.leaves; path.pairs = cnt.pairs;
  std::vector<uint32_t> lv;  // [leaf | leaf_group]
  lv.reserve(2 * (size_t)cnt.leaves);
  for (uint32_t t = 0; t < T; t++) {
    const uint32_t beg = sub_off[t], end = sub_off[t + 1];
    if (sm_sub_opens(jr1[t], end - beg)) {
      lv.insert(lv.end(), list.begin() + beg, list.begin() + end);
    } else {
      for (uint32_t j = beg; j < end; j++) set_valid[list[j]] = sm_sub_failed(jr1[t]) ? 0 : 1;
    }
  }
  const uint32_t L = (uint32_t)lv.size();
  if (!L) return BGV_OK;
  for (uint32_t t = 0; t < T; t++)
    if (sm_sub_opens(jr1[t], sub_off[t + 1] - sub_off[t]))
      lv.insert(lv.end(), list_group.begin() + sub_off[t], list_group.begin() + sub_off[t + 1]);

  // ---- level 2: leaf t = set t = job t, nothing scaled
  dev_batch dL;
  memset(&dL, 0, sizeof dL);
  dL.n_sets = L; dL.n_jobs = L; dL.chunk_bound = L;
  dev_work w2;
  if ((r = work_alloc(c, dL, w2))) return r;
  uint32_t* d_leaf = (uint32_t*)(base + o_leaf);
  HIPCHK(hipMemcpyAsync(d_leaf, lv.data(), 2 * (size_t)L * 4, hipMemcpyHostToDevice, c->st));
  sm_leaves ql;
  memset(&ql, 0, sizeof ql);
  ql.n = L; ql.n_raw = n_raw; ql.table_n = c->table_n; ql.leaf = d_leaf; ql.leaf_group = d_leaf + L;
  ql.raw_pks = c->raw_conv.p; ql.table = c->table;
  if (k.agg) ql.pk_set = c->sma_pk.p;
  else ql.pk_idx = k.d_idx;
  ql.sig_aff = w.sig_aff; ql.h_group = c->sm_hg.p;
  ql.rpk_aff = w2.rpk_aff; ql.h_aff = w2.h_aff; ql.s_aff = w2.s_aff; ql.s_inf = w2.s_inf;
  ql.pk_code = w2.pk_code; ql.job_code = w2.job_code; ql.iota = (uint32_t*)(base + o_iota2);
  launch_sm_split_leaves(c->st, ql);
  HIPCHK(hipGetLastError());
  if ((r = sm_virtual_batch(c, L, ql.iota, w2, k.agg))) return r;
  HIPCHK(hipMemcpyAsync(jr2, w2.job_result, (size_t)L * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (uint32_t t = 0; t < L; t++) set_valid[lv[t]] = jr2[t] == 1 ? 1 : 0;
  return BGV_OK;
}

// The device half of a same-message call, from the staged (or resident) arrays
// on.  k.agg picks the key side, where the pairs of the virtual batch run and
// what the retry takes as a set's key; everything else is one path.
// ag (bgv_verify_same_message_aggregate): the unweighted signature sums run
// speculatively on the pubkey stream behind the weighted G1 sum, over the sets
// the classification left in: they need the decode, `skip` and `take`, not the
// pairing.  When the whole-batch check holds that is the answer; when sets went
// to the retry the two kernels run once more with the final verdicts.
static int sm_back(bgv_ctx* c, sm_dev& k, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats, uint8_t* pk_set96,
                   uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192, const sm_agg_req* ag = nullptr) {
  const uint32_t n = k.n, G = k.G, S = k.sg.S, n_raw = k.n_raw;
  const std::vector<uint32_t>&seg_off = k.sg.seg_off, &seg_group = k.sg.seg_group;
  const uint32_t *d_seg_off = k.d_seg_off, *d_seg_group = k.d_seg_group, *d_group_seg = k.d_group_seg, *d_iota = k.d_iota;
  const uint32_t *d_po = k.d_po, *d_idx = k.d_idx, *d_len = k.d_len;
  const uint8_t *d_msgs = k.d_msgs, *d_sigs = k.d_sigs, *d_raw = k.d_raw;
  const uint64_t* d_scalars = k.d_scalars;
  if (k.draw_scalars) {
    uint32_t kn[11];
    random_bytes(kn, sizeof kn);
    if (int r = ensure_or_release_lines(c, c->scalars, n)) return r;
    launch_gen_scalars(c->st, kn, kn + 8, c->scalars.p, n);
    HIPCHK(hipGetLastError());
    d_scalars = c->scalars.p;
  }
  if (int r = ensure_or_release_lines(c, c->raw_conv, n_raw ? n_raw : 1)) return r;
  launch_raw_pks(c->st, d_raw, c->raw_conv.p, n_raw);

  // view A: the real sets, one job per segment ([gather,] signature decode, G2 sums)
  dev_batch dA;
  memset(&dA, 0, sizeof dA);
  dA.n_sets = n; dA.n_jobs = S; dA.n_raw = n_raw; dA.table_n = c->table_n; dA.table = c->table;
  dA.span_log2 = 6; dA.job_lanes = 36; dA.pairs_per_item = 1; dA.msm = 4; dA.clear_lanes = 9;
  dA.chunk_bound = k.chunk_bound;
  dA.win = k.win;
  dA.defer_from = n;
  dA.job_off = d_seg_off; dA.pk_off = d_po; dA.pk_idx = d_idx; dA.raw_pks = c->raw_conv.p;
  dA.sigs = d_sigs; dA.sig_len = d_len; dA.scalars = d_scalars;
  dev_work w;
  if (int r = work_alloc(c, dA, w)) return r;
  int r = 0;
  if ((r = c->sm_skip.ensure(n)) || (r = c->sm_zero.ensure(n)) || (r = c->sm_seg_code.ensure(S)) ||
      (r = c->sm_win.ensure((size_t)S * 16)) || (r = c->sm_hg.ensure(G)) || (r = c->q_part.ensure(2 * (size_t)G)) ||
      (k.agg && ((r = c->sma_pk.ensure(n)) || (r = c->sma_pk_code.ensure(n)))))
    return r;
  c->sag_timed = false;
  if (ag && ((r = c->sag_seg.ensure(S)) || (r = c->sag_cnt.ensure((size_t)S + G)) || (r = c->sag_code.ensure(G)) ||
             (r = c->sag_out.ensure((size_t)G * 96))))
    return r;
  HIPCHK(hipMemsetAsync(c->sm_zero.p, 0, (size_t)n * 4, c->st));
  sm_view v;
  memset(&v, 0, sizeof v);
  v.n_sets = n; v.n_segs = S; v.n_groups = G; v.n_raw = n_raw; v.table_n = c->table_n;
  v.seg_off = d_seg_off; v.seg_group = d_seg_group; v.pk_idx = d_idx; v.raw_pks = c->raw_conv.p; v.table = c->table;
  v.scalars = d_scalars; v.sig_code = w.sig_code; v.sig_inf = w.sig_inf; v.skip = c->sm_skip.p; v.set_code = w.set_code;
  v.win = c->sm_win.p; v.p_seg = w.rpk_aff; v.seg_code = c->sm_seg_code.p; v.h_group = c->sm_hg.p; v.h_seg = w.h_aff;
  v.pk_code_v = w.pk_code; v.job_code_v = w.job_code; v.s_seg = w.s_aff; v.s_inf = w.s_inf;
  if (k.agg) { v.pk_set = c->sma_pk.p; v.pk_set_code = c->sma_pk_code.p; }

  HIPCHK(hipEventRecord(c->ev_fork, c->st));
  HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_fork, 0));
  HIPCHK(hipStreamWaitEvent(c->st_pk, c->ev_fork, 0));
  {  // one hash per group on the hash stream (latency-mode kernels: two lanes per map)
    dev_batch dH;
    memset(&dH, 0, sizeof dH);
    dH.n_sets = G; dH.n_jobs = G; dH.split = 1; dH.msgs = d_msgs;
    dH.clear_lanes = G < 9000 ? 9u : (G < 16500 ? 3u : 1u);
    dev_work wH;
    memset(&wH, 0, sizeof wH);
    wH.q_part = c->q_part.p;
    wH.h_aff = c->sm_hg.p;
    launch_stage(c->st_hash, ST_HASH, dH, wH);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_dep[ST_HASH], c->st_hash));
  }
  // bitfield sets: the decode, which is the critical path, is launched before the key side, whose three
  // expansion launches would otherwise stand in front of it on the host thread
  const bool sig_first = k.expand != nullptr;
  if (sig_first) launch_stage(c->st, ST_SIG, dA, w);
  if (k.agg) {  // the keys of every set on the pubkey stream, beside the signature decode
    dev_batch dP = dA;
    dP.miller_coop = 36;  // launch_prep: the chunk set-up only, no Miller work items
    if (k.expand) {  // bitfield sets: the expansion runs where its reader, the gather, runs
      if (k.expand_count) bits_launch_count(c->st_pk, *k.expand);
      if (int r2 = bits_launch_expand(c, c->st_pk, *k.expand, k.gathered)) return r2;  // into k.d_idx: reserved by the caller
    }
    launch_prep(c->st_pk, dP, w);
    launch_stage(c->st_pk, ST_PK, dP, w);
    launch_sma_set_sum(c->st_pk, dP, w, c->sma_pk.p, c->sma_pk_code.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_dep[ST_PK], c->st_pk));
  }
  if (!sig_first) launch_stage(c->st, ST_SIG, dA, w);
  if (k.agg) {
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_PK], 0));
    launch_sma_classify(c->st, v);
  } else {
    launch_sm_classify(c->st, v);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_sigdec, c->st));
  HIPCHK(hipStreamWaitEvent(c->st_pk, c->ev_sigdec, 0));
  if (k.agg) launch_sma_g1_sum(c->st_pk, v);
  else launch_sm_g1_sum(c->st_pk, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_dep[ST_PK_SCALE], c->st_pk));
  sig_agg_view av;
  memset(&av, 0, sizeof av);
  if (ag) {  // behind the event: nothing of the pairing path waits for these two
    av.n_segs = S; av.n_groups = G; av.seg_off = d_seg_off; av.group_seg = d_group_seg;
    av.sig_aff = w.sig_aff; av.skip = c->sm_skip.p; av.take = ag->d_take; av.prev = ag->d_prev;
    av.seg_sum = c->sag_seg.p; av.seg_cnt = c->sag_cnt.p; av.out96 = c->sag_out.p; av.out_cnt = c->sag_cnt.p + S;
    av.out_code = c->sag_code.p;
    HIPCHK(hipEventRecord(c->ev_sag[0], c->st_pk));
    launch_sm_sig_agg(c->st_pk, av);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_sag[1], c->st_pk));
    c->sag_timed = true;
  }
  {
    // the per-job MSM sums what `skip` leaves in and rejects nothing: a
    // rejected set is left out, its segment goes on
    dev_work wz = w;
    wz.sig_code = c->sm_zero.p;
    wz.pk_code = c->sm_zero.p;
    wz.sig_inf = c->sm_skip.p;
    launch_stage(c->st, ST_SIG_SCALE, dA, wz);
    launch_stage(c->st, ST_S_TREE, dA, wz);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_PK_SCALE], 0));
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_HASH], 0));
  launch_sm_apply(c->st, v);
  if ((r = sm_virtual_batch(c, S, d_iota, w, k.agg))) return r;  // view B: segment s = set s = job s

  // first-pass results
  const size_t o_jr = 256, o_sc = o_jr + (((size_t)S * 4 + 255) & ~size_t(255)), o_sk = o_sc + (((size_t)n * 4 + 255) & ~size_t(255));
  // the aggregate outputs (ag) behind them: 96 bytes, a count and a code per group, then room for the verdicts
  const size_t o_as = o_sk + (((size_t)n * 4 + 255) & ~size_t(255)), o_ac = o_as + (((size_t)G * 96 + 255) & ~size_t(255)),
               o_ad = o_ac + (((size_t)G * 4 + 255) & ~size_t(255)), o_av = o_ad + (((size_t)G * 4 + 255) & ~size_t(255));
  if ((r = pinned_reserve(c->pin_out, c->pin_out_cap, ag ? o_av + n : o_sk + (size_t)n * 4))) return r;
  auto agg_copies = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pin_out + o_as, av.out96, (size_t)G * 96, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(c->pin_out + o_ac, av.out_cnt, (size_t)G * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(c->pin_out + o_ad, av.out_code, (size_t)G * 4, hipMemcpyDeviceToHost, c->st));
    return 0;
  };
  HIPCHK(hipMemcpyAsync(c->pin_out, w.flags, 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + o_jr, w.job_result, (size_t)S * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + o_sc, w.set_code, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + o_sk, c->sm_skip.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (ag) {  // the speculative sums join here: the clean path gains no synchronise
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_sag[1], 0));
    if ((r = agg_copies())) return r;
  }
  if (pk_set96 || p_group96 || s_group192 || h_group192) {  // the debug entries; pk_set96: aggregate keys only
    const size_t o_set = (size_t)G * 480;
    if ((r = c->sm_pg.ensure(G)) || (r = c->sm_sg.ensure(G)) || (k.agg && (r = c->sma_aff.ensure(n))) ||
        (r = c->dbg_out.ensure(o_set + (k.agg ? (size_t)n * 96 : 0))))
      return r;
    launch_sm_group_sums(c->st, v, d_group_seg, c->sm_pg.p, c->sm_sg.p);
    if (k.agg) launch_sma_pk_aff(c->st, c->sma_pk.p, c->sma_aff.p, n);
    uint8_t* o = c->dbg_out.p;
    launch_export_g1a(c->st, c->sm_pg.p, o, G);
    launch_export_g2a(c->st, c->sm_sg.p, o + (size_t)G * 96, G);
    launch_export_g2a(c->st, c->sm_hg.p, o + (size_t)G * 288, G);
    if (k.agg) launch_export_g1a(c->st, c->sma_aff.p, o + o_set, n);
    HIPCHK(hipGetLastError());
    if (p_group96) HIPCHK(hipMemcpyAsync(p_group96, o, (size_t)G * 96, hipMemcpyDeviceToHost, c->st));
    if (s_group192) HIPCHK(hipMemcpyAsync(s_group192, o + (size_t)G * 96, (size_t)G * 192, hipMemcpyDeviceToHost, c->st));
    if (h_group192) HIPCHK(hipMemcpyAsync(h_group192, o + (size_t)G * 288, (size_t)G * 192, hipMemcpyDeviceToHost, c->st));
    if (k.agg && pk_set96) HIPCHK(hipMemcpyAsync(pk_set96, o + o_set, (size_t)n * 96, hipMemcpyDeviceToHost, c->st));
  }
  HIPCHK(hipStreamSynchronize(c->st));
  c->staged_pending = false;
  const int32_t* jr = (const int32_t*)(c->pin_out + o_jr);
  const int32_t* sc = (const int32_t*)(c->pin_out + o_sc);
  const uint32_t* sk = (const uint32_t*)(c->pin_out + o_sk);
  std::vector<uint32_t> list, list_group, sub_off;  // sub_off: the split retry's subs, offsets into list
  uint32_t pairs = 0, groups_retried = 0, last_group = 0xffffffffu;
  const bool split = c->sm_mode == 1;
  bgv_sm_retry_path& path = c->sm_path;
  path = {};
  path.mode = (uint32_t)c->sm_mode;
  for (uint32_t s = 0; s < S; s++) {
    const bool ok = jr[s] == 1, retry = jr[s] == 0 || jr[s] == -C_SEG_RETRY;
    if (jr[s] >= 0) pairs += 2;
    if (retry && seg_group[s] != last_group) { groups_retried++; last_group = seg_group[s]; }
    const uint32_t first = (uint32_t)list.size();
    for (uint32_t i = seg_off[s]; i < seg_off[s + 1]; i++) {
      set_valid[i] = (!sk[i] && ok) ? 1 : 0;
      if (set_code) set_code[i] = sc[i];
      if (retry && !sk[i]) { list.push_back(i); list_group.push_back(seg_group[s]); }
    }
    if (retry) path.segments++;
    if (retry && split) {  // SM_SEG + 1 offsets at the most, the last one the next segment's first
      uint32_t off[SM_SEG + 1];
      const uint32_t T = sm_split_plan((uint32_t)list.size() - first, first, off, SM_SEG + 1);
      sub_off.insert(sub_off.end(), off, off + T);
    }
  }
  const uint32_t nr = (uint32_t)list.size();
  sub_off.push_back(nr);
  if (nr && ag && (r = c->sag_valid.ensure(n))) return r;
  if (nr && split) {
    // the same sets by subset checks: nothing is decoded or hashed again, and the first pass's signatures stay
    // where the second pass below reads them
    if ((r = sm_split_retry(c, k, w, d_scalars, list, list_group, sub_off, (int32_t*)(c->pin_out + o_sc), (int32_t*)(c->pin_out + o_sk),
                            set_valid, path)))
      return r;
  } else if (nr) {
    path.leaves = nr; path.pairs = 2 * nr; path.hashes = nr;
    // the rare path: the surviving sets of the failing segments, each on its
    // own.  An aggregated key enters as row j of a raw-key table (o_pk).
    const size_t a = 256;
    auto up = [&](size_t x) { return (x + a - 1) & ~(a - 1); };
    const size_t o_iota = 0, o_idx = up(((size_t)nr + 1) * 4), o_len = o_idx + up((size_t)nr * 4), o_scal = o_len + up((size_t)nr * 4),
                 o_msg = o_scal + up((size_t)nr * 8), o_sig = o_msg + up((size_t)nr * 32), o_pk = o_sig + up((size_t)nr * 192),
                 total_r = k.agg ? o_pk + up((size_t)nr * 96) : o_pk;
    if ((r = c->sm_retry.ensure(total_r)) || (r = c->sm_list.ensure(2 * (size_t)nr)) || (k.agg && (r = c->sma_aff.ensure(nr)))) return r;
    if (ag) {  // the retry decodes its sets into the same work buffers: keep the batch's signatures for the second pass
      if ((r = c->sag_sig.ensure(n)) || (r = c->sag_valid.ensure(n))) return r;
      HIPCHK(hipMemcpyAsync(c->sag_sig.p, w.sig_aff, (size_t)n * sizeof(g2a), hipMemcpyDeviceToDevice, c->st));
    }
    HIPCHK(hipMemcpyAsync(c->sm_list.p, list.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->sm_list.p + nr, list_group.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->st));
    uint8_t* base = c->sm_retry.p;
    sm_retry q;
    q.n = nr; q.list = c->sm_list.p; q.list_group = c->sm_list.p + nr;
    q.pk_idx = k.agg ? nullptr : d_idx; q.msgs = d_msgs; q.sigs = d_sigs; q.sig_len = d_len; q.scalars = d_scalars;
    q.o_iota = (uint32_t*)(base + o_iota); q.o_idx = (uint32_t*)(base + o_idx); q.o_len = (uint32_t*)(base + o_len);
    q.o_scalars = (uint64_t*)(base + o_scal); q.o_msgs = base + o_msg; q.o_sigs = base + o_sig;
    bgv_batch bb;
    memset(&bb, 0, sizeof bb);
    if (k.agg) {
      launch_sma_retry_gather(c->st, q, c->sma_pk.p, c->sma_aff.p);
      launch_export_g1a(c->st, c->sma_aff.p, base + o_pk, nr);
      bb.raw_pks = base + o_pk; bb.n_raw = nr;
    } else {
      launch_sm_retry_gather(c->st, q);
      bb.raw_pks = d_raw; bb.n_raw = n_raw;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));  // prepare() starts the hash maps on another stream
    bb.n_sets = nr; bb.n_jobs = nr; bb.job_offsets = q.o_iota; bb.pk_offsets = q.o_iota; bb.pk_indices = q.o_idx;
    bb.msgs = q.o_msgs; bb.sigs = q.o_sigs; bb.sig_len = q.o_len;
    bb.scalars = q.o_scalars; bb.on_device = 1;
    dev_batch d2;
    if ((r = prepare(c, &bb, d2, true))) return r;
    dev_work w2;
    if ((r = work_alloc(c, d2, w2))) return r;
    if ((r = run_stages(c, d2, w2, 0, ST_COUNT))) return r;
    std::vector<int32_t> jr2(nr);
    if ((r = finish_results(c, d2, w2, jr2.data(), nullptr, nullptr))) return r;
    for (uint32_t j = 0; j < nr; j++) set_valid[list[j]] = jr2[j] == 1 ? 1 : 0;
  }
  if (nr && ag) {  // second pass: the same two kernels over the sets with set_valid = 1
    memcpy(c->pin_out + o_av, set_valid, n);
    HIPCHK(hipMemcpyAsync(c->sag_valid.p, c->pin_out + o_av, n, hipMemcpyHostToDevice, c->st));
    av.sig_aff = split ? w.sig_aff : c->sag_sig.p;
    av.valid = c->sag_valid.p;
    launch_sm_sig_agg(c->st, av);
    HIPCHK(hipGetLastError());
    if ((r = agg_copies())) return r;
    HIPCHK(hipStreamSynchronize(c->st));
  }
  if (ag) {
    memcpy(ag->agg_sig96, c->pin_out + o_as, (size_t)G * 96);
    if (ag->agg_count) memcpy(ag->agg_count, c->pin_out + o_ac, (size_t)G * 4);
    if (ag->agg_code) memcpy(ag->agg_code, c->pin_out + o_ad, (size_t)G * 4);
  }
  if (stats) {
    stats->n_sets = n; stats->n_groups = G; stats->n_segments = S;
    stats->hashes = G; stats->pairs = pairs;
    stats->groups_retried = groups_retried; stats->sets_retried = nr;
    stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - k.t0).count();
  }
  return BGV_OK;
}

static int sm_run(bgv_ctx* c, const bgv_sm_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                  uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192, const bgv_sm_agg* agg = nullptr) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device)) return r;
  const uint32_t n = k.n, G = k.G, S = k.sg.S;
  const bool host = !b->on_device;
  k.d_idx = b->pk_indices;
  // staging: the segment tables always, the batch arrays of a host batch
  // (bgv_verify_same_message_aggregate: take and prev of a host batch ride behind them in the same copy)
  const uint8_t *d_take = nullptr, *d_prev = nullptr;
  stage_seg segs[12] = {
      {k.sg.seg_off.data(), ((size_t)S + 1) * 4, (const void**)&k.d_seg_off, 0},
      {k.sg.seg_group.data(), (size_t)S * 4, (const void**)&k.d_seg_group, 0},
      {k.sg.group_seg.data(), ((size_t)G + 1) * 4, (const void**)&k.d_group_seg, 0},
      {k.sg.iota.data(), ((size_t)S + 1) * 4, (const void**)&k.d_iota, 0},
      {b->pk_indices, (size_t)n * 4, (const void**)&k.d_idx, 0},
      {b->msgs, (size_t)G * 32, (const void**)&k.d_msgs, 0},
      {b->raw_pks, (size_t)b->n_raw * 96, (const void**)&k.d_raw, 0},
      {b->scalars, b->scalars ? (size_t)n * 8 : 0, (const void**)&k.d_scalars, 0},
      {b->sigs, (size_t)n * 192, (const void**)&k.d_sigs, 0},
      {b->sig_len, (size_t)n * 4, (const void**)&k.d_len, 0},
      {agg ? agg->take : nullptr, agg && agg->take ? (size_t)n : 0, (const void**)&d_take, 0},
      {agg ? agg->prev_sig96 : nullptr, agg && agg->prev_sig96 ? (size_t)G * 96 : 0, (const void**)&d_prev, 0},
  };
  size_t bytes = 0;
  if (int r = stage_pack(c, segs, host ? (agg ? 12 : 10) : 4, bytes)) return r;
  if (host && b->scalars)  // checked on the pinned copy
    if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + segs[7].off), n)) return r;
  if (int r = stage_issue(c, bytes)) return r;
  if (!agg) return sm_back(c, k, set_valid, set_code, stats, nullptr, p_group96, s_group192, h_group192);
  sm_agg_req q;
  q.d_take = !agg->take ? nullptr : (host ? d_take : agg->take);
  q.d_prev = !agg->prev_sig96 ? nullptr : (host ? d_prev : agg->prev_sig96);
  q.agg_sig96 = agg->agg_sig96; q.agg_count = agg->agg_count; q.agg_code = agg->agg_code;
  return sm_back(c, k, set_valid, set_code, stats, nullptr, p_group96, s_group192, h_group192, &q);
}

static int sma_run(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                   uint8_t* pk_set96, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  const uint32_t n = k.n, G = k.G;
  const bool host = !b->on_device;
  // the key total comes with the group offsets: the gather's grid bound is cut from it
  uint32_t total = host ? b->pk_offsets[n] : 0;  // host: sizes the pk_indices copy; re-checked on the pinned copy
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device, b->pk_offsets + n, &total)) return r;
  const uint32_t S = k.sg.S;
  k.agg = true;
  k.d_po = b->pk_offsets; k.d_idx = b->pk_indices;
  // staging: the segment tables always, the batch arrays of a host batch
  stage_seg segs[11] = {
      {k.sg.seg_off.data(), ((size_t)S + 1) * 4, (const void**)&k.d_seg_off, 0},
      {k.sg.seg_group.data(), (size_t)S * 4, (const void**)&k.d_seg_group, 0},
      {k.sg.group_seg.data(), ((size_t)G + 1) * 4, (const void**)&k.d_group_seg, 0},
      {k.sg.iota.data(), ((size_t)S + 1) * 4, (const void**)&k.d_iota, 0},
      {b->pk_offsets, ((size_t)n + 1) * 4, (const void**)&k.d_po, 0},
      {b->pk_indices, (size_t)total * 4, (const void**)&k.d_idx, 0},
      {b->msgs, (size_t)G * 32, (const void**)&k.d_msgs, 0},
      {b->raw_pks, (size_t)b->n_raw * 96, (const void**)&k.d_raw, 0},
      {b->scalars, b->scalars ? (size_t)n * 8 : 0, (const void**)&k.d_scalars, 0},
      {b->sigs, (size_t)n * 192, (const void**)&k.d_sigs, 0},
      {b->sig_len, (size_t)n * 4, (const void**)&k.d_len, 0},
  };
  size_t bytes = 0;
  if (int r = stage_pack(c, segs, host ? 11 : 4, bytes)) return r;
  if (host) {  // the contract, on the pinned copy the device will see
    if (int r = sma_check_keys(b, (const uint32_t*)(c->pin_in + segs[4].off), total)) return r;
    if (b->scalars)
      if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + segs[8].off), n)) return r;
  }
  if (int r = stage_issue(c, bytes)) return r;
  k.chunk_bound = total / PK_CHUNK + n;  // as prepare() sets it: sum ceil(k_i / 32) <= total / 32 + n
  return sm_back(c, k, set_valid, set_code, stats, pk_set96, p_group96, s_group192, h_group192);
}

// The front of bitfield sets is bits_front's (set-up, host plan, expansion), with
// the expansion buffers as d_po / d_idx and the windows of a context with sums.
// The expansion runs on st_pk in front of the gather, its only reader: the
// signature decode on st and the hashes on st_hash start without it.
static int smb_run(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                   uint8_t* pk_set96, uint8_t* path, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device)) return r;
  const uint32_t n = k.n, G = k.G, S = k.sg.S;
  const bool host = !b->on_device;

  bits_args a;
  if (int r = bits_setup(c, a, n, b->bits_len, b->n_indices, !host, true, c->st_pk)) return r;
  c->bits_timed = false;
  a.src = (const bits_src*)b->src; a.v.bits = b->bits; a.v.pk_indices = b->pk_indices;

  // staging: the segment tables always, the batch arrays of a host batch
  stage_seg segs[12] = {
      {k.sg.seg_off.data(), ((size_t)S + 1) * 4, (const void**)&k.d_seg_off, 0},
      {k.sg.seg_group.data(), (size_t)S * 4, (const void**)&k.d_seg_group, 0},
      {k.sg.group_seg.data(), ((size_t)G + 1) * 4, (const void**)&k.d_group_seg, 0},
      {k.sg.iota.data(), ((size_t)S + 1) * 4, (const void**)&k.d_iota, 0},
      {b->src, (size_t)n * sizeof(bits_src), (const void**)&a.src, 0},
      {b->bits, (size_t)b->bits_len, (const void**)&a.v.bits, 0},
      {b->pk_indices, (size_t)b->n_indices * 4, (const void**)&a.v.pk_indices, 0},
      {b->msgs, (size_t)G * 32, (const void**)&k.d_msgs, 0},
      {b->raw_pks, (size_t)b->n_raw * 96, (const void**)&k.d_raw, 0},
      {b->scalars, b->scalars ? (size_t)n * 8 : 0, (const void**)&k.d_scalars, 0},
      {b->sigs, (size_t)n * 192, (const void**)&k.d_sigs, 0},
      {b->sig_len, (size_t)n * 4, (const void**)&k.d_len, 0},
  };
  size_t bytes = 0;
  if (int r = stage_pack(c, segs, host ? 12 : 4, bytes)) return r;
  if (host) {
    // the contract, on the pinned copy the device will see; the plan's totals
    // size the expansion and the gather's grid without a read-back
    bits_view hv = a.v;
    hv.bits = c->pin_in + segs[5].off;
    hv.pk_indices = (const uint32_t*)(c->pin_in + segs[6].off);
    bits_plan_out po;
    if (int r = bits_check_sources(n, (const bits_src*)(c->pin_in + segs[4].off), hv, &po, nullptr)) return r;
    if (b->scalars)
      if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + segs[9].off), n)) return r;
    c->pk_total = po.total;
    c->bits_path.sets_complement = po.n_complement;
    c->bits_path.keys_expanded = po.total;
    c->bits_path.keys_gathered = po.gathered;
    c->bits_extra_chunks = po.n_complement;
    if (int r = stage_issue(c, bytes)) return r;
    k.expand_count = true;
  } else {
    if (int r = stage_issue(c, bytes)) return r;
    // an on-device batch: count and scan now, the 8 bytes of totals come back
    // before the buffers and the gather's grid are sized (as bgv_verify_bits does)
    bits_launch_count(c->st_pk, a);
    HIPCHK(hipGetLastError());
    if (int r = bits_read_totals(c, c->st_pk, a)) return r;
  }
  k.gathered = c->bits_path.keys_gathered;
  if (int r = ensure_or_release_lines(c, c->bits_idx, k.gathered ? k.gathered : 1)) return r;
  k.agg = true;
  k.expand = &a;
  k.d_po = c->bits_off.p;
  k.d_idx = c->bits_idx.p;
  k.win = a.win;
  // as bits_layout: sum ceil(k_i / 32) + windows <= gathered / 32 + n + windows
  k.chunk_bound = k.gathered / PK_CHUNK + n + c->bits_extra_chunks;
  if (int r = sm_back(c, k, set_valid, set_code, stats, pk_set96, p_group96, s_group192, h_group192)) return r;
  if (path) {
    memset(path, 0, n);
    if (a.win) {
      std::vector<pk_window> win(n);
      HIPCHK(hipMemcpyAsync(win.data(), a.win, (size_t)n * sizeof(pk_window), hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
      for (uint32_t i = 0; i < n; i++) path[i] = win[i].hi ? 1 : 0;
    }
  }
  return BGV_OK;
}

// run, then: these entries report bgv_sm_stats.hashes (hash_path_clear)
static int sm_done(bgv_ctx* c, int r) {
  hash_path_clear(c);
  return r;
}

int bgv_verify_same_message(bgv_ctx* c, const bgv_sm_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, nullptr, nullptr, nullptr));
}

static int sm_agg_args(const bgv_sm_agg* agg) {
  if (!agg) return fail(BGV_E_INVALID_ARG, "agg is NULL");
  if (!agg->agg_sig96) return fail(BGV_E_INVALID_ARG, "agg_sig96 is NULL");
  return BGV_OK;
}

int bgv_sm_agg_check(const bgv_sm_batch* b, const bgv_sm_agg* agg) {
  if (int r = bgv_sm_check(b)) return r;
  return sm_agg_args(agg);
}

int bgv_verify_same_message_aggregate(bgv_ctx* c, const bgv_sm_batch* b, const bgv_sm_agg* agg, uint8_t* set_valid,
                                      int32_t* set_code, bgv_sm_stats* stats) {
  if (int r = sm_agg_args(agg)) return r;
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, nullptr, nullptr, nullptr, agg));
}

int bgv_sm_agg_ms(bgv_ctx* c, float* ms) {
  if (!c || !ms) return fail(BGV_E_INVALID_ARG, "null argument");
  *ms = 0.f;
  if (!c->sag_timed) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->ev_sag[1]));
  HIPCHK(hipEventElapsedTime(ms, c->ev_sag[0], c->ev_sag[1]));
  return BGV_OK;
}

int bgv_debug_same_message(bgv_ctx* c, const bgv_sm_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                           uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, p_group96, s_group192, h_group192));
}

int bgv_verify_same_message_agg(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  return sm_done(c, sma_run(c, b, set_valid, set_code, stats, nullptr, nullptr, nullptr, nullptr));
}

int bgv_debug_same_message_agg(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                               uint8_t* pk_set96, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  return sm_done(c, sma_run(c, b, set_valid, set_code, stats, pk_set96, p_group96, s_group192, h_group192));
}

int bgv_verify_same_message_bits(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  return sm_done(c, smb_run(c, b, set_valid, set_code, stats, nullptr, nullptr, nullptr, nullptr, nullptr));
}

int bgv_debug_same_message_bits(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                                uint8_t* pk_set96, uint8_t* path, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  return sm_done(c, smb_run(c, b, set_valid, set_code, stats, pk_set96, path, p_group96, s_group192, h_group192));
}

int bgv_sm_retry(bgv_ctx* c, int32_t mode) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  if (mode != 0 && mode != 1) return fail(BGV_E_INVALID_ARG, "bgv_sm_retry mode %d", mode);
  c->sm_mode = mode;
  return BGV_OK;
}

int bgv_sm_retry_stats(bgv_ctx* c, bgv_sm_retry_path* out) {
  if (!c || !out) return fail(BGV_E_INVALID_ARG, "null argument");
  *out = c->sm_path;
  return BGV_OK;
}

static_assert(SM_SUB == BGV_SM_SUB && SM_SUB <= SM_SEG, "the sub size of sm_split.h is the ABI's");
uint32_t bgv_sm_split_plan(uint32_t m, uint32_t* sub_off, uint32_t cap) { return sm_split_plan(m, 0, sub_off, cap); }

// ---- multi-GPU partials ---------------------------------------------------
// fp12 (plain limbs, already out of Montgomery form on the device) <-> 576 B
static void fp12_plain_to_bytes(uint8_t* out, const fp12_t& f) {
  const fp2_t* cs[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
  for (int k = 0; k < 6; k++) {
    fp_to_be48(out + 96 * k, cs[k]->c0);
    fp_to_be48(out + 96 * k + 48, cs[k]->c1);
  }
}

static void fp12_plain_from_bytes(fp12_t& f, const uint8_t* in) {
  fp2_t* cs[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
  for (int k = 0; k < 6; k++) {
    fp_from_be48(cs[k]->c0, in + 96 * k);
    fp_from_be48(cs[k]->c1, in + 96 * k + 48);
  }
}

int bgv_partial(bgv_ctx* c, const bgv_batch* b, uint8_t* miller576, int32_t* set_code, int32_t* job_result,
                int32_t* ok_out) {
  if (!c || !b || !miller576) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  active_guard ag(c->device);
  dev_batch d;
  if (int r = prepare(c, b, d, true)) return r;
  tail_entry(c, d);
  dev_work w;
  pair_entry pe(c, c->pair_merge != 0);
  if (int r = work_alloc(c, d, w)) return r;
  fp12_t f;
  std::vector<int32_t> jc(d.n_jobs ? d.n_jobs : 1);
  // (a second, unmerged pass only after a merged one met an identity class)
  bool fell_back = false;
  for (int pass = 0; pass < 2; pass++) {
    if (int r = run_stages(c, d, w, ST_SIG, ST_BATCH_FINAL)) return r;
    launch_stage(c->st, ST_SET_CODES, d, w);
    if (d.n_jobs) {
      launch_fp12_convert(c->st, w.f_batch, w.f_part, 1, false);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&f, w.f_part, sizeof f, hipMemcpyDeviceToHost, c->st));
    } else {
      memset(&f, 0, sizeof f);
      f.c0.c0.c0.l[0] = 1;  // plain 1
    }
    if (d.n_jobs) HIPCHK(hipMemcpyAsync(jc.data(), w.job_code, (size_t)d.n_jobs * 4, hipMemcpyDeviceToHost, c->st));
    if (set_code && d.n_sets) HIPCHK(hipMemcpyAsync(set_code, w.set_code, (size_t)d.n_sets * 4, hipMemcpyDeviceToHost, c->st));
    if (c->hash_pending) HIPCHK(hipMemcpyAsync(&c->hash_path.hashes, c->mc.n_uniq, 4, hipMemcpyDeviceToHost, c->st));
    uint32_t ident = 0;
    const bool want_pair = c->pair_pending;
    if (want_pair) {
      HIPCHK(hipMemcpyAsync(&c->pair_path.pairs, c->pc.class_off + c->pc.n_jobs, 4, hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipMemcpyAsync(&ident, c->pc.ident, 4, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(hipStreamSynchronize(c->st));
    c->hash_pending = false;
    c->pair_pending = false;
    c->staged_pending = false;
    if (!(want_pair && ident)) break;
    c->pm_call = false;  // an identity class: the pass is void, once more with one pair per set
    fell_back = true;
  }
  if (fell_back) c->pair_path.fallback = 1;
  fp12_plain_to_bytes(miller576, f);
  int32_t ok = 1;
  for (uint32_t j = 0; j < d.n_jobs; j++) {
    if (jc[j] != 0) ok = 0;
    if (job_result) job_result[j] = jc[j] != 0 ? -jc[j] : 1;
  }
  if (ok_out) *ok_out = ok;
  c->part_d = d;
  c->part_w = w;
  c->tail_path = {d.batch_tail ? 1u : 0u, 0u};
  c->partial_pending = true;
  return BGV_OK;
}

int bgv_partial_finish(bgv_ctx* c, int32_t* job_result, bgv_stats* stats) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  if (!c->partial_pending) return fail(BGV_E_STATE, "bgv_partial_finish needs bgv_partial as the previous call on the context");
  const dev_batch& d = c->part_d;
  const dev_work& w = c->part_w;
  if (!job_result && d.n_jobs) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  c->timed = false;
  c->run_from = 0;
  c->run_to = ST_COUNT;
  HIPCHK(hipEventRecord(c->ev[0], c->st));
  // batch-first tail: k_batch_final, then the guarded per-job kernels over the view the shard's fold ran over
  if (d.batch_tail) launch_stage(c->st, ST_BATCH_FINAL, c->tail_d, c->tail_w);
  else launch_stage(c->st, ST_BATCH_FINAL, d, w);
  launch_stage(c->st, ST_JOB_FINAL, d, w);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev[ST_COUNT], c->st));
  return finish_results(c, d, w, job_result, nullptr, stats);
}

// (keeps a pending bgv_partial state: the dist flow is partial -> combine ->
// partial_finish; the combination touches only f_part and its own flag word)
int bgv_combine_final(bgv_ctx* c, const uint8_t* parts, uint32_t n, int32_t* is_one) {
  if (!c || (!parts && n) || !is_one) return fail(BGV_E_INVALID_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  std::vector<fp12_t> h(n ? n : 1);
  for (uint32_t k = 0; k < n; k++) fp12_plain_from_bytes(h[k], parts + 576u * k);
  if (int r = c->f_part.ensure(2 * (size_t)n + 65)) return r;
  if (int r = c->flags.ensure(8)) return r;
  if (n) HIPCHK(hipMemcpyAsync(c->f_part.p + n, h.data(), (size_t)n * sizeof(fp12_t), hipMemcpyHostToDevice, c->st));
  launch_fp12_convert(c->st, c->f_part.p + n, c->f_part.p, n, true);
  launch_combine_final(c->st, c->f_part.p, n, c->flags.p + 4);
  HIPCHK(hipGetLastError());
  uint32_t flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, c->flags.p + 4, 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  *is_one = flag ? 1 : 0;
  return BGV_OK;
}

// ---- test-only: per-stage intermediates -------------------------------------
int bgv_debug_stages(bgv_ctx* c, const bgv_batch* b, int32_t* job_result, int32_t* set_code, bgv_debug* o) {
  if (!c || !b || !o || (!job_result && b->n_jobs)) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  c->pair_path = {};  // the per-set golden plan: never merged, zeros in bgv_pair_stats
  c->pair_pending = c->pair_redo = false;
  HIPCHK(hipSetDevice(c->device));
  dev_batch d;
  if (int r = prepare(c, b, d, true)) return r;
  dev_work w;
  if (int r = work_alloc(c, d, w)) return r;
  const uint32_t n = d.n_sets, J = d.n_jobs;
  if (int r = c->pk_agg.ensure(n ? n : 1)) return r;
  w.pk_agg = c->pk_agg.p;
  // the steps path has no per-item Miller value: k_job_chain leaves the job's
  // set product at its first set (1 at the others), copied after the tree stage
  d.steps_dbg = d.steps_slice ? 1u : 0u;
  // the Miller values are copied before the product tree, which folds groups
  // of them in place (k_job_prefold, k_f_level); deferred subgroup verdicts
  // are applied first (idempotent: the tree stage applies them again)
  if (int r = run_stages(c, d, w, 0, ST_F_TREE)) return r;
  if (d.defer_grp) launch_sig_fixup(c->st, d, w);
  if (int r = c->dbg_f.ensure((size_t)n + J + 1)) return r;
  if (n + J) HIPCHK(hipMemcpyAsync(c->dbg_f.p, w.f_set, (size_t)(n + J) * sizeof(fp12_t), hipMemcpyDeviceToDevice, c->st));
  if (int r = run_stages(c, d, w, ST_F_TREE, ST_COUNT)) return r;
  if (d.steps_dbg && n) HIPCHK(hipMemcpyAsync(c->dbg_f.p, w.f_set, (size_t)n * sizeof(fp12_t), hipMemcpyDeviceToDevice, c->st));
  // final exponentiations of every Miller value, job product and the batch product
  const uint32_t n_fe = n + 2 * J + 1;
  if (int r = c->dbg_fe.ensure(n_fe)) return r;
  launch_final_exp_many(c->st, c->dbg_f.p, c->dbg_fe.p, n + J);
  launch_final_exp_many(c->st, w.f_job, c->dbg_fe.p + n + J, J);
  if (J) launch_final_exp_many(c->st, w.f_batch, c->dbg_fe.p + n + 2 * J, 1);
  launch_fp12_convert(c->st, c->dbg_fe.p, c->dbg_fe.p, n_fe, false);
  HIPCHK(hipGetLastError());
  struct part { uint8_t* host; size_t bytes; } parts[8];
  int np = 0;
  size_t off = 0;
  auto add = [&](uint8_t* host, size_t bytes) -> uint8_t* {
    const size_t o2 = off;
    off += (bytes + 255) & ~size_t(255);
    parts[np++] = {host, bytes};
    return (uint8_t*)o2;  // offset, rebased below
  };
  uint8_t* o_sig = add(o->sig_aff, (size_t)n * 192);
  uint8_t* o_h = add(o->h_aff, (size_t)n * 192);
  uint8_t* o_pk = add(o->pk_agg, (size_t)n * 96);
  uint8_t* o_rpk = add(o->rpk_aff, (size_t)n * 96);
  uint8_t* o_s = add(o->s_aff, (size_t)J * 192);
  if (int r = c->dbg_out.ensure(off ? off : 1)) return r;
  uint8_t* base = c->dbg_out.p;
  launch_export_g2a(c->st, w.sig_aff, base + (size_t)o_sig, n);
  launch_export_g2a(c->st, w.h_aff, base + (size_t)o_h, n);
  launch_export_g1a(c->st, w.pk_agg, base + (size_t)o_pk, n);
  launch_export_g1a(c->st, w.rpk_aff, base + (size_t)o_rpk, n);
  launch_export_g2a(c->st, w.s_aff, base + (size_t)o_s, J);
  HIPCHK(hipGetLastError());
  size_t pos = 0;
  for (int k = 0; k < np; k++) {
    if (parts[k].host && parts[k].bytes) HIPCHK(hipMemcpyAsync(parts[k].host, base + pos, parts[k].bytes, hipMemcpyDeviceToHost, c->st));
    pos += (parts[k].bytes + 255) & ~size_t(255);
  }
  std::vector<fp12_t> fe(n_fe);
  HIPCHK(hipMemcpyAsync(fe.data(), c->dbg_fe.p, (size_t)n_fe * sizeof(fp12_t), hipMemcpyDeviceToHost, c->st));
  if (int r = finish_results(c, d, w, job_result, set_code, nullptr)) return r;
  if (o->pair_fe)
    for (uint32_t k = 0; k < n + J; k++) fp12_plain_to_bytes(o->pair_fe + 576u * k, fe[k]);
  if (o->job_fe)
    for (uint32_t k = 0; k < J; k++) fp12_plain_to_bytes(o->job_fe + 576u * k, fe[n + J + k]);
  if (o->batch_fe) {
    if (J) fp12_plain_to_bytes(o->batch_fe, fe[n + 2 * J]);
    else memset(o->batch_fe, 0, 576);
  }
  return BGV_OK;
}

// test-only: bgv_verify through the merged path plus the classes (include/bgv.h)
int bgv_debug_pair_classes(bgv_ctx* c, const bgv_batch* b, int32_t* job_result, int32_t* set_code, uint32_t* cls,
                           uint32_t* class_off, uint8_t* p_class96, uint8_t* job_fe, uint8_t* batch_fe) {
  if (!c || !b || (!job_result && b->n_jobs)) return fail(BGV_E_INVALID_ARG, "null argument");
  c->partial_pending = false;
  HIPCHK(hipSetDevice(c->device));
  pair_entry pe(c, true);
  dev_batch d;
  if (int r = prepare(c, b, d, true)) return r;
  if (!pair_merge_on(c, d)) return fail(BGV_E_STATE, "bgv_debug_pair_classes: the batch's layout does not merge pairs");
  dev_work w;
  if (int r = work_alloc(c, d, w)) return r;
  const uint32_t n = d.n_sets, J = d.n_jobs;
  if (int r = run_stages(c, d, w, 0, ST_COUNT)) return r;
  if (int r = finish_results(c, d, w, job_result, set_code, nullptr)) return r;
  // the classes of the merged pass, also when it met an identity class
  const bgv_pair_path path = c->pair_path;
  const uint32_t n_cls = path.pairs <= n ? path.pairs : n;
  if (cls) HIPCHK(hipMemcpyAsync(cls, c->pc.cls, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (class_off) HIPCHK(hipMemcpyAsync(class_off, c->pc.class_off, ((size_t)J + 1) * 4, hipMemcpyDeviceToHost, c->st));
  if (p_class96 && n_cls) {
    if (int r = c->dbg_out.ensure((size_t)n_cls * 96)) return r;
    launch_export_g1a(c->st, c->pc.p_cls, c->dbg_out.p, n_cls);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p_class96, c->dbg_out.p, (size_t)n_cls * 96, hipMemcpyDeviceToHost, c->st));
  }
  HIPCHK(hipStreamSynchronize(c->st));
  if (c->pair_redo) {  // the verdicts and products of the unmerged pass
    c->pm_call = false;
    if (int r = run_stages(c, d, w, 0, ST_COUNT)) return r;
    if (int r = finish_results(c, d, w, job_result, set_code, nullptr)) return r;
    c->pair_path = path;
    c->pair_path.merged = 0;
    c->pair_path.pairs = n;
    c->pair_path.fallback = 1;
  }
  if ((job_fe || batch_fe) && J) {
    if (int r = c->dbg_fe.ensure((size_t)J + 1)) return r;
    launch_final_exp_many(c->st, w.f_job, c->dbg_fe.p, J);
    launch_final_exp_many(c->st, w.f_batch, c->dbg_fe.p + J, 1);
    launch_fp12_convert(c->st, c->dbg_fe.p, c->dbg_fe.p, J + 1, false);
    HIPCHK(hipGetLastError());
    std::vector<fp12_t> fe((size_t)J + 1);
    HIPCHK(hipMemcpyAsync(fe.data(), c->dbg_fe.p, ((size_t)J + 1) * sizeof(fp12_t), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (job_fe)
      for (uint32_t k = 0; k < J; k++) fp12_plain_to_bytes(job_fe + 576u * k, fe[k]);
    if (batch_fe) fp12_plain_to_bytes(batch_fe, fe[J]);
  } else if (batch_fe) {
    memset(batch_fe, 0, 576);
  }
  return BGV_OK;
}

// ---- synthetic data --------------------------------------------------------
int bgv_gen_keys(bgv_ctx* c, uint32_t first, uint32_t n, uint64_t seed) {
  if (!c) return fail(BGV_E_INVALID_ARG, "null ctx");
  c->partial_pending = false;
  if (n == 0) return BGV_OK;
  if ((uint64_t)first + n > TABLE_MAX) return fail(BGV_E_TABLE_RANGE, "rows [%u, %llu) exceed the table limit 2^31 - 1", first, (unsigned long long)first + n);
  if (first > c->table_n) return fail(BGV_E_TABLE_RANGE, "row %u would leave a gap after the %u rows of the table", first, c->table_n);
  HIPCHK(hipSetDevice(c->device));
  if (int r = table_reserve(c, first + n)) return r;
  if (c->sk.cap < (size_t)(first + n) * 8) {
    // keep previously generated keys when growing
    dbuf<uint32_t> nb;
    if (int r = nb.ensure((size_t)(first + n) * 8)) return r;
    HIPCHK(hipMemsetAsync(nb.p, 0, nb.cap * 4, c->st));
    if (c->sk.p) HIPCHK(hipMemcpyAsync(nb.p, c->sk.p, c->sk.cap * 4, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->sk.release();
    c->sk = nb;
  }
  if (first < c->table_n)  // a rewrite: drops every list's sums (bgv_index_list_sums)
    if (int r = sums_drop_all(c)) return r;
  launch_gen_keys(c->st, c->table, c->sk.p, first, n, seed);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
  if (first + n > c->table_n) c->table_n = first + n;
  return BGV_OK;
}

int bgv_gen_sign(bgv_ctx* c, const bgv_batch* b, uint8_t* sigs_out) {
  if (!c || !b || !sigs_out) return fail(BGV_E_INVALID_ARG, "null argument");
  if (!c->sk.p) return fail(BGV_E_INVALID_ARG, "bgv_gen_keys has not run on this context");
  HIPCHK(hipSetDevice(c->device));
  c->partial_pending = false;
  dev_batch d;
  bgv_batch bb = *b;
  bb.scalars = nullptr;
  if (int r = prepare(c, &bb, d, false)) return r;
  uint8_t* out = sigs_out;
  if (!b->on_device) {
    if (int r = c->gen_out.ensure((size_t)d.n_sets * 192 + 1)) return r;
    HIPCHK(hipMemsetAsync(c->gen_out.p, 0, (size_t)d.n_sets * 192, c->st));
    out = c->gen_out.p;
  }
  launch_gen_sign(c->st, d, c->sk.p, out);
  HIPCHK(hipGetLastError());
  if (!b->on_device) HIPCHK(hipMemcpyAsync(sigs_out, out, (size_t)d.n_sets * 192, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

// ---- field self-test ---------------------------------------------------------
int bgv_debug_fp_ops(bgv_ctx* c, const uint32_t* ab_in, uint32_t n, uint32_t* out) {
  if (!c || (n && (!ab_in || !out))) return fail(BGV_E_INVALID_ARG, "null argument");
  if (n > (1u << 20)) return fail(BGV_E_INVALID_ARG, "at most 2^20 operand pairs");
  if (!n) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->mb_fp.ensure((size_t)n * (2 + BGV_FP_OPS_N))) return r;
  fp_t* d_ab = c->mb_fp.p;
  fp_t* d_out = d_ab + (size_t)n * 2;
  HIPCHK(hipMemcpyAsync(d_ab, ab_in, (size_t)n * 2 * sizeof(fp_t), hipMemcpyHostToDevice, c->st));
  launch_fp_ops(c->st, d_ab, d_out, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n * BGV_FP_OPS_N * sizeof(fp_t), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

int bgv_debug_g2_decode(bgv_ctx* c, const uint8_t* sigs192, const uint32_t* sig_len, uint32_t n, uint8_t* out192,
                        int32_t* codes) {
  if (!c || (n && (!sigs192 || !sig_len || !out192 || !codes))) return fail(BGV_E_INVALID_ARG, "null argument");
  if (n > (1u << 20)) return fail(BGV_E_INVALID_ARG, "at most 2^20 encodings");
  if (!n) return BGV_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = (size_t)n * (192 + 4 + 192 + 4);
  if (int r = c->dbg_out.ensure(bytes)) return r;
  uint8_t* d_sig = c->dbg_out.p;
  uint32_t* d_len = (uint32_t*)(d_sig + (size_t)n * 192);
  uint8_t* d_out = (uint8_t*)(d_len + n);
  int32_t* d_code = (int32_t*)(d_out + (size_t)n * 192);
  HIPCHK(hipMemcpyAsync(d_sig, sigs192, (size_t)n * 192, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(d_len, sig_len, (size_t)n * 4, hipMemcpyHostToDevice, c->st));
  launch_g2_decode_dbg(c->st, d_sig, d_len, d_out, d_code, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out192, d_out, (size_t)n * 192, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(codes, d_code, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BGV_OK;
}

// ---- microbenchmarks ---------------------------------------------------------
int bgv_bench_fpmul(bgv_ctx* c, uint32_t lanes, uint32_t iters, float* ms) {
  if (!c || !ms || lanes == 0 || lanes % 256) return fail(BGV_E_INVALID_ARG, "lanes must be a positive multiple of 256");
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->mb_fp.ensure((size_t)lanes * 2)) return r;
  std::vector<fp_t> h((size_t)lanes * 2);
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (auto& e : h) {
    for (int k = 0; k < NL; k++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; e.l[k] = (uint32_t)x; }
    e.l[NL - 1] &= 0x0fffffffu;  // < p
  }
  HIPCHK(hipMemcpyAsync(c->mb_fp.p, h.data(), h.size() * sizeof(fp_t), hipMemcpyHostToDevice, c->st));
  launch_bench_fpmul(c->st, c->mb_fp.p, lanes, 16);  // warm-up
  HIPCHK(hipEventRecord(c->ev[0], c->st));
  launch_bench_fpmul(c->st, c->mb_fp.p, lanes, iters);
  HIPCHK(hipEventRecord(c->ev[1], c->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventSynchronize(c->ev[1]));
  HIPCHK(hipEventElapsedTime(ms, c->ev[0], c->ev[1]));
  return BGV_OK;
}

int bgv_bench_mad(bgv_ctx* c, uint32_t lanes, uint32_t iters, float* ms) {
  if (!c || !ms || lanes == 0 || lanes % 256) return fail(BGV_E_INVALID_ARG, "lanes must be a positive multiple of 256");
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->mb_u64.ensure(lanes)) return r;
  HIPCHK(hipMemsetAsync(c->mb_u64.p, 0x5a, (size_t)lanes * 8, c->st));
  launch_bench_mad(c->st, c->mb_u64.p, lanes, 16);
  HIPCHK(hipEventRecord(c->ev[0], c->st));
  launch_bench_mad(c->st, c->mb_u64.p, lanes, iters);
  HIPCHK(hipEventRecord(c->ev[1], c->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventSynchronize(c->ev[1]));
  HIPCHK(hipEventElapsedTime(ms, c->ev[0], c->ev[1]));
  return BGV_OK;
}

