// What the host units behind the C ABI share: the error string, the device
// buffers, the context and the helpers that cross units.  Not installed.
//   bgv_api.hip        context, pubkey table, staging, the ordinary pipeline
//   bgv_api_bits.hip   index lists, their sums, bitfield sets
//   bgv_api_sm.hip     the same-message entries
//   bgv_api_debug.hip  per-stage intermediates, synthetic data, microbenchmarks
// Included by these four only, which all work inside bgv and bgv::host.
#pragma once
#include <string.h>
#include <atomic>
#include <vector>

#include "bgv_internal.h"
#include "pair_merge.h"
#include "../../include/bgv.h"

namespace bgv {
namespace host {

// the one error string behind bgv_last_error (bgv_api.hip); returns code
int fail(int code, const char* fmt, ...);

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

}  // namespace host
}  // namespace bgv

using namespace bgv;
using namespace bgv::host;

// Every field of every entry family; the comment blocks name the unit that owns
// (writes) the fields below them.  Buffers of the pipeline are read by all.
struct bgv_ctx {
  // ---- bgv_api.hip: context, streams and events
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
  // ---- bgv_api.hip: index2pubkey table (grown by copy)
  g1a* table = nullptr;
  uint32_t table_n = 0, table_cap = 0;
  dbuf<uint8_t> raw_in, gen_out;
  dbuf<g1a> pk_tmp;         // bgv_pubkeys_set: decoded rows before they enter the table
  dbuf<int32_t> pk_codes;   // bgv_pubkeys_set: per-key deserialization codes
  std::vector<int32_t> pk_codes_host;
  // ---- bgv_api.hip: staging for host batches: every host array of a batch is
  // packed into one pinned buffer and crosses PCIe in ONE copy (pageable copies
  // cost ~30-90 us each on the C2 critical path); results come back through
  // pinned memory too
  dbuf<uint8_t> stage_dev;
  uint8_t* pin_in = nullptr;
  uint8_t* pin_out = nullptr;
  size_t pin_in_cap = 0, pin_out_cap = 0;
  hipEvent_t ev_staged = nullptr;  // the last pin_in -> stage_dev copy
  bool staged_pending = false;
  // host view of the last prepared batch (offsets from the pinned copy or HBM)
  std::vector<uint32_t> jo_host;
  uint32_t pk_total = 0;
  dbuf<uint64_t> scalars;
  dbuf<g1a> raw_conv;
  // ---- bgv_api.hip: per-batch intermediates (work_alloc)
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
  // bgv_partial -> bgv_partial_finish: the shard's intermediates stay resident
  bool partial_pending = false;
  dev_batch part_d;
  dev_work part_w;

  // ---- bgv_api_bits.hip: resident index lists (bgv_index_list_set) and the expansion of bgv_verify_bits
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
  dbuf<g1a> pk_agg;                   // bgv_debug_bits_keys (and bgv_debug_stages): dev_work.pk_agg

  // ---- bgv_api_sm.hip: bgv_verify_same_message
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

  // ---- bgv_api_debug.hip: bgv_debug_stages, synthetic secret keys, microbench scratch
  dbuf<fp12_t> dbg_fe, dbg_f;
  dbuf<uint8_t> dbg_out;      // (also the debug exports of the bits and same-message entries)
  dbuf<uint32_t> sk;
  dbuf<fp_t> mb_fp;
  dbuf<uint64_t> mb_u64;
};

namespace bgv {
namespace host {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// ---- bgv_api.hip: context, table, staging ------------------------------------
int ctx_drain(bgv_ctx* c);  // every stream of the context
int table_reserve(bgv_ctx* c, uint32_t n);
// index2pubkey rows are u32 indices with bit 31 reserved for raw_pks
static const uint32_t TABLE_MAX = 0x7fffffffu;

void random_bytes(void* out, size_t n);
int pinned_reserve(uint8_t*& p, size_t& cap, size_t n);

// a device allocation of prepare(): under memory pressure a kept line buffer
// (up to 2.6 GB, see work_alloc) gives way first, then the allocation retries
template <class T>
int ensure_or_release_lines(bgv_ctx* c, dbuf<T>& b, size_t n) {
  int r = b.ensure(n);
  if (r && c->lines.cap && (const void*)&b != (const void*)&c->lines) {
    c->lines.release();
    if ((const void*)&b != (const void*)&c->f_step) c->f_step.release();
    c->lines_idle = 0;
    r = b.ensure(n);
  }
  return r;
}

// one host array of a batch, packed at a 256-byte aligned offset of the staging buffers
struct stage_seg {
  const void* src;
  size_t bytes;
  const void** dst;
  size_t off;  // filled by stage_pack: offset in pin_in / stage_dev
};
int stage_pack(bgv_ctx* c, stage_seg* segs, int n_segs, size_t& total);
int stage_issue(bgv_ctx* c, size_t total);

// batches of this process between entry and results, per device (prepare())
extern std::atomic<int> g_active[64];
struct active_guard {
  int dev;
  explicit active_guard(int d) : dev(d >= 0 && d < 64 ? d : -1) { if (dev >= 0) g_active[dev]++; }
  ~active_guard() { if (dev >= 0) g_active[dev]--; }
};

// ---- bgv_api.hip: the ordinary pipeline ---------------------------------------
int early_maps(bgv_ctx* c, dev_batch& d, bool after_staging);
int prepare(bgv_ctx* c, const bgv_batch* b, dev_batch& d, bool need_sigs);
int prepare_layout(bgv_ctx* c, dev_batch& d, const uint64_t* scalars, bool scalars_staged);
bool pair_merge_on(const bgv_ctx* c, const dev_batch& d);
int work_alloc(bgv_ctx* c, const dev_batch& d, dev_work& w);
int run_stages(bgv_ctx* c, const dev_batch& d, const dev_work& w, int from, int to);
int finish_results(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code, bgv_stats* stats);
int run_and_finish(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code, bgv_stats* stats);
void tail_entry(const bgv_ctx* c, dev_batch& d);
void hash_path_clear(bgv_ctx* c);

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

// A pass (launches and results; it leaves c->pair_redo) that may have merged
// pairs: one that met an identity class is void, and the pass runs once more
// unmerged over the inputs, which are still resident.
template <class F>
int pair_fallback(bgv_ctx* c, F pass) {
  if (int r = pass()) return r;
  if (!c->pair_redo) return 0;
  c->pm_call = false;
  if (int r = pass()) return r;
  c->pair_path.fallback = 1;
  return 0;
}

// fp12 (plain limbs, already out of Montgomery form on the device) <-> 576 B
void fp12_plain_to_bytes(uint8_t* out, const fp12_t& f);
void fp12_plain_from_bytes(fp12_t& f, const uint8_t* in);

// ---- bgv_api_bits.hip ----------------------------------------------------------
int sums_drop_all(bgv_ctx* c);  // a table rewrite: no prefix sum may outlive the rows it was built from
// what the host check makes of a bits batch (bits_check_sources)
struct bits_plan_out {
  uint32_t total = 0, max_job = 1;
  uint32_t gathered = 0, n_complement = 0;
};
int bits_check_sources(uint32_t n, const bits_src* src, const bits_view& v, bits_plan_out* out, uint8_t* path);
void bits_host_view(bits_view& v, const uint32_t* list_len, const uint8_t* list_has_sums);
int bits_setup(bgv_ctx* c, bits_args& a, uint32_t n, uint32_t bits_len, uint32_t n_indices, bool on_device, bool use_sums,
               hipStream_t st);
void bits_launch_count(hipStream_t st, const bits_args& a);
int bits_launch_expand(bgv_ctx* c, hipStream_t st, bits_args& a, uint32_t gathered);
int bits_read_totals(bgv_ctx* c, hipStream_t st, const bits_args& a);

}  // namespace host
}  // namespace bgv
