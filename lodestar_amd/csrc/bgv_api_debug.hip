// Host side of the C ABI (include/bgv.h), the entries no verifier calls: the
// per-stage intermediates and pair classes the tests compare with the oracle,
// synthetic keys and signatures, the field self-tests and the microbenchmarks.
// All of them run the ordinary pipeline's helpers (bgv_api.hip, bgv_host.h).
#include <vector>

#include "bgv_host.h"

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
