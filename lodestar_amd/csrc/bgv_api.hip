// Host side of the C ABI declared in include/bgv.h: context, HBM-resident
// pubkey table, batch staging and the stage pipeline on one HIP stream, with
// the entries of the ordinary pipeline (bgv_verify, the bgv_partial family).
// The other entry families have units of their own over the helpers declared
// in bgv_host.h: bgv_api_bits.hip, bgv_api_sm.hip, bgv_api_debug.hip.
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
#include <vector>
#include <string>

#include "bgv_host.h"

static thread_local std::string g_err;

namespace bgv::host {

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace bgv::host

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

namespace bgv::host {

// every stream of the context: a batch still in flight (bgv_partial leaves
// one, a failed call may) can read a list or its sums from any of the four
int ctx_drain(bgv_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipStreamSynchronize(c->st_hash));
  HIPCHK(hipStreamSynchronize(c->st_pk));
  HIPCHK(hipStreamSynchronize(c->st_chk));
  return 0;
}

int table_reserve(bgv_ctx* c, uint32_t n) {
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

}  // namespace bgv::host

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

namespace bgv::host {

void random_bytes(void* out, size_t n) {
  size_t got = 0;
  uint8_t* p = (uint8_t*)out;
  while (got < n) {
    ssize_t r = getrandom(p + got, n - got, 0);
    if (r > 0) got += (size_t)r;
  }
}

int pinned_reserve(uint8_t*& p, size_t& cap, size_t n) {
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

// pack the segments into pin_in (host copies only) and point every *dst at
// its future device copy; stage_issue then moves the whole buffer in one transfer
int stage_pack(bgv_ctx* c, stage_seg* segs, int n_segs, size_t& total) {
  total = 0;
  for (int i = 0; i < n_segs; i++) total += align256(segs[i].bytes);
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
    off += align256(segs[i].bytes);
  }
  return 0;
}

int stage_issue(bgv_ctx* c, size_t total) {
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
std::atomic<int> g_active[64];
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
int early_maps(bgv_ctx* c, dev_batch& d, bool after_staging) {
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

// Build the device view of a batch: stage host arrays, convert raw pubkeys.
// Host batches: the arrays are copied into pinned memory FIRST and every
// contract check reads that copy, so the device only ever sees checked
// offsets even if the caller's buffers change during the call.  Index ranges
// are checked per set on the device (BGV_SET_INDEX_RANGE rejects the job).
int prepare(bgv_ctx* c, const bgv_batch* b, dev_batch& d, bool need_sigs) {
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

int prepare_layout(bgv_ctx* c, dev_batch& d, const uint64_t* scalars, bool scalars_staged) {
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
bool pair_merge_on(const bgv_ctx* c, const dev_batch& d) {
  return c->pm_call && !d.split && !d.miller_coop && !d.miller_kv && !d.steps_dbg && d.pairs_per_item >= 1 && d.n_jobs > 0 &&
         d.n_sets > 0 && d.n_sets <= (1u << 30);
}
// (merging needs the root representatives, so it implies the class pass)
static bool hash_dedup_on(const bgv_ctx* c, const dev_batch& d) {
  return !d.split && (c->cfg.hash_dedup == 1 || pair_merge_on(c, d)) && d.n_sets > 0 && d.n_sets <= (1u << 30);
}

// a kept line buffer the batch does not use gives way under memory pressure
int work_alloc(bgv_ctx* c, const dev_batch& d, dev_work& w) {
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
int run_stages(bgv_ctx* c, const dev_batch& d, const dev_work& w, int from, int to) {
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
int finish_results(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code,
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

}  // namespace bgv::host

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

namespace bgv::host {

// the whole pipeline and its results; a merged pass that met an identity class
// is discarded and the batch runs again unmerged (its inputs are still resident)
int run_and_finish(bgv_ctx* c, const dev_batch& d, const dev_work& w, int32_t* job_result, int32_t* set_code, bgv_stats* stats) {
  return pair_fallback(c, [&]() -> int {
    if (int r = run_stages(c, d, w, 0, ST_COUNT)) return r;
    return finish_results(c, d, w, job_result, set_code, stats);
  });
}

// The batch-first tail: the entries whose verdicts come
// from k_batch_final / k_job_final over a batch on the steps path with the
// (job, window) MSM (the window sums it folds).  Called between prepare() and
// work_alloc(); every other entry leaves dev_batch.batch_tail at 0, and with
// it today's tail (the debug entries report per-job values).
void tail_entry(const bgv_ctx* c, dev_batch& d) {
  d.batch_tail = c->batch_tail != 0 && d.steps_slice && d.msm == 2 && !d.steps_dbg && d.n_jobs ? 1u : 0u;
}

}  // namespace bgv::host

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

namespace bgv::host {

// the same-message entries hash per group on their own (their retries may pass
// through run_stages): bgv_hash_stats reports zeros after them
void hash_path_clear(bgv_ctx* c) {
  if (!c) return;
  c->hash_path = {};
  c->hash_pending = false;
  c->pair_path = {};  // nor do they merge pairs: bgv_pair_stats reports zeros as well
  c->pair_pending = c->pair_redo = false;
}

}  // namespace bgv::host

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

// ---- multi-GPU partials ---------------------------------------------------
namespace bgv::host {

// fp12 (plain limbs, already out of Montgomery form on the device) <-> 576 B
void fp12_plain_to_bytes(uint8_t* out, const fp12_t& f) {
  const fp2_t* cs[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
  for (int k = 0; k < 6; k++) {
    fp_to_be48(out + 96 * k, cs[k]->c0);
    fp_to_be48(out + 96 * k + 48, cs[k]->c1);
  }
}

void fp12_plain_from_bytes(fp12_t& f, const uint8_t* in) {
  fp2_t* cs[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
  for (int k = 0; k < 6; k++) {
    fp_from_be48(cs[k]->c0, in + 96 * k);
    fp_from_be48(cs[k]->c1, in + 96 * k + 48);
  }
}

}  // namespace bgv::host

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
  const int rp = pair_fallback(c, [&]() -> int {
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
    c->pair_redo = want_pair && ident;  // an identity class: the pass is void, once more with one pair per set
    return 0;
  });
  if (rp) return rp;
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
