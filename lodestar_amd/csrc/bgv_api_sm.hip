// Host side of the C ABI (include/bgv.h), the same-message entries.
//
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
#include <chrono>
#include <optional>
#include <vector>

#include "bgv_host.h"
#include "msm_g1.h"
#include "sig_agg.h"
#include "sm_split.h"

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

// ---- the device half: one synchronise per pass ---------------------------------
//   sm_back:  sm_first_pass -> sm_collect -> (sm_retry_per_set | sm_split_retry) -> sm_agg_second_pass -> stats

// the exports of the debug entries (the verifying entries pass none)
struct sm_debug_out {
  uint8_t *pk_set96 = nullptr, *p_group96 = nullptr, *s_group192 = nullptr, *h_group192 = nullptr;
  bool any() const { return pk_set96 || p_group96 || s_group192 || h_group192; }
};

// where the results land in the pinned output buffer (word 0: the batch flag)
struct sm_out_off {
  size_t jr, sc, sk;      // [S] segment verdicts, [n] set codes, [n] skip flags; the split retry's levels reuse sc and sk
  size_t as, ac, ad, av;  // aggregate entry: 96 bytes, a count and a code per group, then room for the verdicts
  size_t total;
};
static sm_out_off sm_out_layout(uint32_t n, uint32_t S, uint32_t G, bool ag) {
  sm_out_off o;
  o.jr = 256;
  o.sc = o.jr + align256((size_t)S * 4);
  o.sk = o.sc + align256((size_t)n * 4);
  o.as = o.sk + align256((size_t)n * 4);
  o.ac = o.as + align256((size_t)G * 96);
  o.ad = o.ac + align256((size_t)G * 4);
  o.av = o.ad + align256((size_t)G * 4);
  o.total = ag ? o.av + n : o.sk + (size_t)n * 4;
  return o;
}

// What the first pass hands to the retries and the second pass.  w is its work
// view: its sig_aff, with sm_hg, sma_pk and sm_skip, is read by the split retry
// and by the second pass of bgv_verify_same_message_aggregate.
struct sm_pass {
  dev_work w;
  sm_view v;
  sig_agg_view av;            // the aggregate entry's two kernels (zero otherwise)
  const uint64_t* d_scalars;  // the caller's, staged or resident, or the ones drawn on the device
  sm_out_off o;
};

// View A of a level: real (or compacted) sets, one job per segment (or sub), for
// the signature decode and the G2 bucket MSM.  raw_conv holds the raw keys.
static dev_batch sm_sets_view(const bgv_ctx* c, uint32_t n_sets, uint32_t n_jobs, uint32_t n_raw, const uint32_t* job_off,
                              const uint32_t* pk_idx, const uint64_t* scalars, uint32_t chunk_bound) {
  dev_batch d;
  memset(&d, 0, sizeof d);
  d.n_sets = n_sets; d.n_jobs = n_jobs; d.n_raw = n_raw; d.table_n = c->table_n; d.table = c->table;
  d.span_log2 = 6; d.job_lanes = 36; d.pairs_per_item = 1; d.msm = 4; d.clear_lanes = 9;
  d.chunk_bound = chunk_bound; d.defer_from = n_sets;
  d.job_off = job_off; d.pk_idx = pk_idx; d.raw_pks = c->raw_conv.p; d.scalars = scalars;
  return d;
}

// the sum kernels' view of the same level: the segments are dA's jobs, the
// virtual batch's arrays are w's
static sm_view sm_view_over(const bgv_ctx* c, const dev_batch& dA, uint32_t G, const dev_work& w, const uint32_t* seg_group,
                            const uint32_t* pk_idx, const g1j* pk_set, uint32_t* skip) {
  sm_view v;
  memset(&v, 0, sizeof v);
  v.n_sets = dA.n_sets; v.n_segs = dA.n_jobs; v.n_groups = G; v.n_raw = dA.n_raw; v.table_n = dA.table_n;
  v.seg_off = dA.job_off; v.seg_group = seg_group; v.pk_idx = pk_idx; v.raw_pks = dA.raw_pks; v.table = dA.table;
  v.scalars = dA.scalars; v.skip = skip;
  v.win = c->sm_win.p; v.p_seg = w.rpk_aff; v.seg_code = c->sm_seg_code.p; v.h_group = c->sm_hg.p; v.h_seg = w.h_aff;
  v.pk_code_v = w.pk_code; v.job_code_v = w.job_code; v.s_seg = w.s_aff; v.s_inf = w.s_inf;
  v.pk_set = pk_set;
  return v;
}

// One level of checks (the first pass's segments, level 1's subs): P_seg on the
// pubkey stream, released by `fork`, beside S_seg over sig_aff on the main
// stream, then the pairs of the virtual batch (segment s = set s = job s).
// wait_hash: H(m_g) may still be in flight.  spec: the aggregate entry's sums,
// behind the G1 sum on its stream (nothing of the pairing path waits for them).
static int sm_level(bgv_ctx* c, bool agg, const dev_batch& dA, const dev_work& w, const sm_view& v, g2a* sig_aff,
                    const uint32_t* d_iota, hipEvent_t fork, bool wait_hash, const sig_agg_view* spec) {
  HIPCHK(hipEventRecord(fork, c->st));
  HIPCHK(hipStreamWaitEvent(c->st_pk, fork, 0));
  if (agg) launch_sma_g1_sum(c->st_pk, v);
  else launch_sm_g1_sum(c->st_pk, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_dep[ST_PK_SCALE], c->st_pk));
  if (spec) {
    HIPCHK(hipEventRecord(c->ev_sag[0], c->st_pk));
    launch_sm_sig_agg(c->st_pk, *spec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_sag[1], c->st_pk));
    c->sag_timed = true;
  }
  {
    // the per-job MSM sums what `skip` leaves in and rejects nothing: a
    // rejected set is left out, its segment goes on
    dev_work wz = w;
    wz.sig_aff = sig_aff;
    wz.sig_code = c->sm_zero.p;
    wz.pk_code = c->sm_zero.p;
    wz.sig_inf = v.skip;
    launch_stage(c->st, ST_SIG_SCALE, dA, wz);
    launch_stage(c->st, ST_S_TREE, dA, wz);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_PK_SCALE], 0));
  if (wait_hash) HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_HASH], 0));
  launch_sm_apply(c->st, v);
  return sm_virtual_batch(c, v.n_segs, d_iota, w, agg);
}

// one hash per group on the hash stream (latency-mode kernels: two lanes per map)
static int sm_hash_groups(bgv_ctx* c, uint32_t G, const uint8_t* d_msgs) {
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
  return 0;
}

// aggregate sets: the keys of every set on the pubkey stream, beside the signature decode
static int sm_set_keys(bgv_ctx* c, const sm_dev& k, const dev_batch& dA, const dev_work& w) {
  dev_batch dP = dA;
  dP.miller_coop = 36;  // launch_prep: the chunk set-up only, no Miller work items
  if (k.expand) {  // bitfield sets: the expansion runs where its reader, the gather, runs
    if (k.expand_count) bits_launch_count(c->st_pk, *k.expand);
    if (int r = bits_launch_expand(c, c->st_pk, *k.expand, k.gathered)) return r;  // into k.d_idx: reserved by the caller
  }
  launch_prep(c->st_pk, dP, w);
  launch_stage(c->st_pk, ST_PK, dP, w);
  launch_sma_set_sum(c->st_pk, dP, w, c->sma_pk.p, c->sma_pk_code.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_dep[ST_PK], c->st_pk));
  return 0;
}

// the aggregate entry's outputs, queued behind whatever c->st holds
static int sm_agg_copies(bgv_ctx* c, const sm_pass& p, uint32_t G) {
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.as, p.av.out96, (size_t)G * 96, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.ac, p.av.out_cnt, (size_t)G * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.ad, p.av.out_code, (size_t)G * 4, hipMemcpyDeviceToHost, c->st));
  return 0;
}

// the debug entries: per-group sums and hashes; pk_set96: aggregate keys only
static int sm_debug_exports(bgv_ctx* c, const sm_dev& k, const sm_view& v, const sm_debug_out& dbg) {
  const uint32_t n = k.n, G = k.G;
  const size_t o_set = (size_t)G * 480;
  int r = 0;
  if ((r = c->sm_pg.ensure(G)) || (r = c->sm_sg.ensure(G)) || (k.agg && (r = c->sma_aff.ensure(n))) ||
      (r = c->dbg_out.ensure(o_set + (k.agg ? (size_t)n * 96 : 0))))
    return r;
  launch_sm_group_sums(c->st, v, k.d_group_seg, c->sm_pg.p, c->sm_sg.p);
  if (k.agg) launch_sma_pk_aff(c->st, c->sma_pk.p, c->sma_aff.p, n);
  uint8_t* o = c->dbg_out.p;
  launch_export_g1a(c->st, c->sm_pg.p, o, G);
  launch_export_g2a(c->st, c->sm_sg.p, o + (size_t)G * 96, G);
  launch_export_g2a(c->st, c->sm_hg.p, o + (size_t)G * 288, G);
  if (k.agg) launch_export_g1a(c->st, c->sma_aff.p, o + o_set, n);
  HIPCHK(hipGetLastError());
  if (dbg.p_group96) HIPCHK(hipMemcpyAsync(dbg.p_group96, o, (size_t)G * 96, hipMemcpyDeviceToHost, c->st));
  if (dbg.s_group192) HIPCHK(hipMemcpyAsync(dbg.s_group192, o + (size_t)G * 96, (size_t)G * 192, hipMemcpyDeviceToHost, c->st));
  if (dbg.h_group192) HIPCHK(hipMemcpyAsync(dbg.h_group192, o + (size_t)G * 288, (size_t)G * 192, hipMemcpyDeviceToHost, c->st));
  if (k.agg && dbg.pk_set96) HIPCHK(hipMemcpyAsync(dbg.pk_set96, o + o_set, (size_t)n * 96, hipMemcpyDeviceToHost, c->st));
  return 0;
}

// The first pass, from the staged (or resident) arrays to its results in pinned
// memory.  k.agg picks the key side, where the pairs of the virtual batch run
// and what the retry takes as a set's key; everything else is one path.
// ag (bgv_verify_same_message_aggregate): the unweighted signature sums run
// speculatively on the pubkey stream behind the weighted G1 sum, over the sets
// the classification left in: they need the decode, `skip` and `take`, not the
// pairing.  When the whole-batch check holds that is the answer.
static int sm_first_pass(bgv_ctx* c, sm_dev& k, const sm_agg_req* ag, const sm_debug_out& dbg, sm_pass& p) {
  const uint32_t n = k.n, G = k.G, S = k.sg.S, n_raw = k.n_raw;
  p.d_scalars = k.d_scalars;
  if (k.draw_scalars) {
    uint32_t kn[11];
    random_bytes(kn, sizeof kn);
    if (int r = ensure_or_release_lines(c, c->scalars, n)) return r;
    launch_gen_scalars(c->st, kn, kn + 8, c->scalars.p, n);
    HIPCHK(hipGetLastError());
    p.d_scalars = c->scalars.p;
  }
  if (int r = ensure_or_release_lines(c, c->raw_conv, n_raw ? n_raw : 1)) return r;
  launch_raw_pks(c->st, k.d_raw, c->raw_conv.p, n_raw);

  // view A: the real sets, one job per segment ([gather,] signature decode, G2 sums)
  dev_batch dA = sm_sets_view(c, n, S, n_raw, k.d_seg_off, k.d_idx, p.d_scalars, k.chunk_bound);
  dA.win = k.win;
  dA.pk_off = k.d_po; dA.sigs = k.d_sigs; dA.sig_len = k.d_len;
  dev_work& w = p.w;
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
  sm_view& v = p.v;
  v = sm_view_over(c, dA, G, w, k.d_seg_group, k.d_idx, k.agg ? c->sma_pk.p : nullptr, c->sm_skip.p);
  v.sig_code = w.sig_code; v.sig_inf = w.sig_inf; v.set_code = w.set_code;
  if (k.agg) v.pk_set_code = c->sma_pk_code.p;
  sig_agg_view& av = p.av;
  memset(&av, 0, sizeof av);
  if (ag) {
    av.n_segs = S; av.n_groups = G; av.seg_off = k.d_seg_off; av.group_seg = k.d_group_seg;
    av.sig_aff = w.sig_aff; av.skip = c->sm_skip.p; av.take = ag->d_take; av.prev = ag->d_prev;
    av.seg_sum = c->sag_seg.p; av.seg_cnt = c->sag_cnt.p; av.out96 = c->sag_out.p; av.out_cnt = c->sag_cnt.p + S;
    av.out_code = c->sag_code.p;
  }

  HIPCHK(hipEventRecord(c->ev_fork, c->st));
  HIPCHK(hipStreamWaitEvent(c->st_hash, c->ev_fork, 0));
  HIPCHK(hipStreamWaitEvent(c->st_pk, c->ev_fork, 0));
  if ((r = sm_hash_groups(c, G, k.d_msgs))) return r;
  // bitfield sets: the decode, which is the critical path, is launched before the key side, whose three
  // expansion launches would otherwise stand in front of it on the host thread
  const bool sig_first = k.expand != nullptr;
  if (sig_first) launch_stage(c->st, ST_SIG, dA, w);
  if (k.agg && (r = sm_set_keys(c, k, dA, w))) return r;
  if (!sig_first) launch_stage(c->st, ST_SIG, dA, w);
  if (k.agg) {
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_dep[ST_PK], 0));
    launch_sma_classify(c->st, v);
  } else {
    launch_sm_classify(c->st, v);
  }
  HIPCHK(hipGetLastError());
  // view B: segment s = set s = job s
  if ((r = sm_level(c, k.agg, dA, w, v, w.sig_aff, k.d_iota, c->ev_sigdec, true, ag ? &av : nullptr))) return r;

  // first-pass results
  p.o = sm_out_layout(n, S, G, ag != nullptr);
  if ((r = pinned_reserve(c->pin_out, c->pin_out_cap, p.o.total))) return r;
  HIPCHK(hipMemcpyAsync(c->pin_out, w.flags, 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.jr, w.job_result, (size_t)S * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.sc, w.set_code, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->pin_out + p.o.sk, c->sm_skip.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (ag) {  // the speculative sums join here: the clean path gains no synchronise
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_sag[1], 0));
    if ((r = sm_agg_copies(c, p, G))) return r;
  }
  if (dbg.any() && (r = sm_debug_exports(c, k, v, dbg))) return r;
  HIPCHK(hipStreamSynchronize(c->st));
  c->staged_pending = false;
  return BGV_OK;
}

// The per-set retry (bgv_sm_retry mode 0), the rare path: the surviving sets of
// the failing segments, each on its own as a one-set job of the ordinary
// pipeline.  An aggregated key enters as row j of a raw-key table (o_pk).
// keep_sigs: the retry decodes its sets into the first pass's work buffers, so
// the batch's signatures are kept aside for the aggregate entry's second pass.
static int sm_retry_per_set(bgv_ctx* c, const sm_dev& k, const sm_pass& p, bool keep_sigs, const sm_retry_sets& rs,
                            uint8_t* set_valid, bgv_sm_retry_path& path) {
  const uint32_t n = k.n, nr = (uint32_t)rs.list.size();
  path.leaves = nr; path.pairs = 2 * nr; path.hashes = nr;
  const size_t o_iota = 0, o_idx = align256(((size_t)nr + 1) * 4), o_len = o_idx + align256((size_t)nr * 4),
               o_scal = o_len + align256((size_t)nr * 4), o_msg = o_scal + align256((size_t)nr * 8),
               o_sig = o_msg + align256((size_t)nr * 32), o_pk = o_sig + align256((size_t)nr * 192),
               total_r = k.agg ? o_pk + align256((size_t)nr * 96) : o_pk;
  int r = 0;
  if ((r = c->sm_retry.ensure(total_r)) || (r = c->sm_list.ensure(2 * (size_t)nr)) || (k.agg && (r = c->sma_aff.ensure(nr)))) return r;
  if (keep_sigs) {
    if ((r = c->sag_sig.ensure(n)) || (r = c->sag_valid.ensure(n))) return r;
    HIPCHK(hipMemcpyAsync(c->sag_sig.p, p.w.sig_aff, (size_t)n * sizeof(g2a), hipMemcpyDeviceToDevice, c->st));
  }
  HIPCHK(hipMemcpyAsync(c->sm_list.p, rs.list.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->sm_list.p + nr, rs.list_group.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->st));
  uint8_t* base = c->sm_retry.p;
  sm_retry q;
  q.n = nr; q.list = c->sm_list.p; q.list_group = c->sm_list.p + nr;
  q.pk_idx = k.agg ? nullptr : k.d_idx; q.msgs = k.d_msgs; q.sigs = k.d_sigs; q.sig_len = k.d_len; q.scalars = p.d_scalars;
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
    bb.raw_pks = k.d_raw; bb.n_raw = k.n_raw;
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
  for (uint32_t j = 0; j < nr; j++) set_valid[rs.list[j]] = jr2[j] == 1 ? 1 : 0;
  return BGV_OK;
}

// The split retry (bgv_sm_retry mode 1, sm_split.h):
// the same sets by subset checks, nothing is decoded or hashed again.
// rs.list / list_group: the surviving sets of the retried segments and their
// groups; rs.sub_off: the subs (offsets into list).  The first pass's
// signatures stay where the second pass of the aggregate entry reads them, so
// both levels work in c->sm_split and in work buffers no larger than the first
// pass's set-sized ones (work_alloc never moves a buffer that is large enough).
// The sub and leaf verdicts come home where the first pass's set codes and skip
// flags did (read by then): list.size() words each at the most.
static int sm_split_retry(bgv_ctx* c, const sm_dev& k, const sm_pass& p, const sm_retry_sets& rs, uint8_t* set_valid,
                          bgv_sm_retry_path& path) {
  const std::vector<uint32_t>&list = rs.list, &list_group = rs.list_group, &sub_off = rs.sub_off;
  const uint32_t nr = (uint32_t)list.size(), T = (uint32_t)sub_off.size() - 1, n_raw = k.n_raw;
  int32_t *jr1 = (int32_t*)(c->pin_out + p.o.sc), *jr2 = (int32_t*)(c->pin_out + p.o.sk);
  // level 1's inputs, then what the host sends: [list | list_group | sub_off | iota] and level 2's [leaf | leaf_group]
  const size_t o_idx = 0, o_pk = o_idx + align256((size_t)nr * 4), o_scal = o_pk + (k.agg ? align256((size_t)nr * sizeof(g1j)) : 0),
               o_sig = o_scal + align256((size_t)nr * 8), o_skip = o_sig + align256((size_t)nr * sizeof(g2a)),
               o_sg = o_skip + align256((size_t)nr * 4), o_host = o_sg + align256((size_t)T * 4),
               host_words = 2 * (size_t)nr + 2 * ((size_t)T + 1), o_leaf = o_host + align256(host_words * 4),
               o_iota2 = o_leaf + align256(2 * (size_t)nr * 4), total = o_iota2 + align256(((size_t)nr + 1) * 4);
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
  const dev_batch dA = sm_sets_view(c, nr, T, n_raw, d_sub_off, (const uint32_t*)(base + o_idx), (const uint64_t*)(base + o_scal), nr);
  dev_work w1;
  if ((r = work_alloc(c, dA, w1))) return r;
  sm_split q;
  memset(&q, 0, sizeof q);
  q.n = nr; q.n_subs = T; q.list = d_list; q.list_group = d_list_group; q.sub_off = d_sub_off;
  q.scalars = p.d_scalars; q.sig_aff = p.w.sig_aff;
  q.o_scalars = (uint64_t*)(base + o_scal); q.o_sig = (g2a*)(base + o_sig); q.o_skip = (uint32_t*)(base + o_skip);
  q.o_sub_group = (uint32_t*)(base + o_sg);
  if (k.agg) { q.pk_set = c->sma_pk.p; q.o_pk = (g1j*)(base + o_pk); }
  else { q.pk_idx = k.d_idx; q.o_idx = (uint32_t*)(base + o_idx); }
  launch_sm_split_gather(c->st, q);
  HIPCHK(hipGetLastError());
  // the compacted signatures; every set of the list is live.  P_sub on the pubkey stream beside S_sub, as in the first pass
  const sm_view v = sm_view_over(c, dA, k.G, w1, q.o_sub_group, q.o_idx, q.o_pk, q.o_skip);
  if ((r = sm_level(c, k.agg, dA, w1, v, q.o_sig, d_iota1, c->ev_fork, false, nullptr))) return r;
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
  ql.sig_aff = p.w.sig_aff; ql.h_group = c->sm_hg.p;
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

// The aggregate entry's second pass: when sets went to a retry, the same two kernels over the
// sets with set_valid = 1; then the outputs (the speculative ones when nothing was retried).
static int sm_agg_second_pass(bgv_ctx* c, const sm_dev& k, sm_pass& p, const sm_agg_req& ag, bool retried, bool split,
                              const uint8_t* set_valid) {
  const uint32_t n = k.n, G = k.G;
  if (retried) {
    memcpy(c->pin_out + p.o.av, set_valid, n);
    HIPCHK(hipMemcpyAsync(c->sag_valid.p, c->pin_out + p.o.av, n, hipMemcpyHostToDevice, c->st));
    p.av.sig_aff = split ? p.w.sig_aff : c->sag_sig.p;
    p.av.valid = c->sag_valid.p;
    launch_sm_sig_agg(c->st, p.av);
    HIPCHK(hipGetLastError());
    if (int r = sm_agg_copies(c, p, G)) return r;
    HIPCHK(hipStreamSynchronize(c->st));
  }
  memcpy(ag.agg_sig96, c->pin_out + p.o.as, (size_t)G * 96);
  if (ag.agg_count) memcpy(ag.agg_count, c->pin_out + p.o.ac, (size_t)G * 4);
  if (ag.agg_code) memcpy(ag.agg_code, c->pin_out + p.o.ad, (size_t)G * 4);
  return BGV_OK;
}

// The device half of a same-message call: when the first pass's whole-batch check fails, the
// surviving sets of the failing segments go to the retry the context is set to.
static int sm_back(bgv_ctx* c, sm_dev& k, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats, const sm_debug_out& dbg,
                   const sm_agg_req* ag = nullptr) {
  const uint32_t n = k.n, G = k.G, S = k.sg.S;
  sm_pass p;
  if (int r = sm_first_pass(c, k, ag, dbg, p)) return r;
  const bool split = c->sm_mode == 1;
  bgv_sm_retry_path& path = c->sm_path;
  path = {};
  path.mode = (uint32_t)c->sm_mode;
  const sm_retry_sets rs = sm_collect(S, k.sg.seg_off.data(), k.sg.seg_group.data(), (const int32_t*)(c->pin_out + p.o.jr),
                                      (const int32_t*)(c->pin_out + p.o.sc), (const uint32_t*)(c->pin_out + p.o.sk), split,
                                      set_valid, set_code);
  path.segments = rs.segments;
  const uint32_t nr = (uint32_t)rs.list.size();
  if (nr && ag)
    if (int r = c->sag_valid.ensure(n)) return r;
  if (nr)
    if (int r = split ? sm_split_retry(c, k, p, rs, set_valid, path) : sm_retry_per_set(c, k, p, ag != nullptr, rs, set_valid, path))
      return r;
  if (ag)
    if (int r = sm_agg_second_pass(c, k, p, *ag, nr != 0, split, set_valid)) return r;
  if (stats) {
    stats->n_sets = n; stats->n_groups = G; stats->n_segments = S;
    stats->hashes = G; stats->pairs = rs.pairs;
    stats->groups_retried = rs.groups_retried; stats->sets_retried = nr;
    stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - k.t0).count();
  }
  return BGV_OK;
}

// ---- the fronts --------------------------------------------------------------
// The staging table of a front: the segment tables, its key rows, the five arrays every batch
// has.  A front keeps the rows it reads back on the pinned copy by name, not by index.
struct sm_stage {
  stage_seg segs[16];
  int n = 0;
  stage_seg* add(const void* src, size_t bytes, const void** dst) { return &(segs[n++] = {src, bytes, dst, 0}); }
};
static const int SM_STAGE_TABLES = 4;  // staged for every batch; the rows behind them for a host batch only
static void sm_stage_tables(sm_stage& t, sm_dev& k) {
  const size_t S = k.sg.S, G = k.G;
  t.add(k.sg.seg_off.data(), (S + 1) * 4, (const void**)&k.d_seg_off);
  t.add(k.sg.seg_group.data(), S * 4, (const void**)&k.d_seg_group);
  t.add(k.sg.group_seg.data(), (G + 1) * 4, (const void**)&k.d_group_seg);
  t.add(k.sg.iota.data(), (S + 1) * 4, (const void**)&k.d_iota);
}
// msgs, raw_pks, scalars, sigs, sig_len; returns the scalars' row
template <class B>
static stage_seg* sm_stage_arrays(sm_stage& t, sm_dev& k, const B* b) {
  const size_t n = k.n, G = k.G;
  t.add(b->msgs, G * 32, (const void**)&k.d_msgs);
  t.add(b->raw_pks, (size_t)b->n_raw * 96, (const void**)&k.d_raw);
  stage_seg* scalars = t.add(b->scalars, b->scalars ? n * 8 : 0, (const void**)&k.d_scalars);
  t.add(b->sigs, n * 192, (const void**)&k.d_sigs);
  t.add(b->sig_len, n * 4, (const void**)&k.d_len);
  return scalars;
}

static int sm_run(bgv_ctx* c, const bgv_sm_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                  const sm_debug_out& dbg, const bgv_sm_agg* agg = nullptr) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device)) return r;
  const uint32_t n = k.n, G = k.G;
  const bool host = !b->on_device;
  k.d_idx = b->pk_indices;
  // staging: the segment tables always, the batch arrays of a host batch
  // (bgv_verify_same_message_aggregate: take and prev of a host batch ride behind them in the same copy)
  const uint8_t *d_take = nullptr, *d_prev = nullptr;
  sm_stage t;
  sm_stage_tables(t, k);
  t.add(b->pk_indices, (size_t)n * 4, (const void**)&k.d_idx);
  const stage_seg* scalars = sm_stage_arrays(t, k, b);
  if (agg) {
    t.add(agg->take, agg->take ? (size_t)n : 0, (const void**)&d_take);
    t.add(agg->prev_sig96, agg->prev_sig96 ? (size_t)G * 96 : 0, (const void**)&d_prev);
  }
  size_t bytes = 0;
  if (int r = stage_pack(c, t.segs, host ? t.n : SM_STAGE_TABLES, bytes)) return r;
  if (host && b->scalars)  // checked on the pinned copy
    if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + scalars->off), n)) return r;
  if (int r = stage_issue(c, bytes)) return r;
  if (!agg) return sm_back(c, k, set_valid, set_code, stats, dbg);
  sm_agg_req q;
  q.d_take = !agg->take ? nullptr : (host ? d_take : agg->take);
  q.d_prev = !agg->prev_sig96 ? nullptr : (host ? d_prev : agg->prev_sig96);
  q.agg_sig96 = agg->agg_sig96; q.agg_count = agg->agg_count; q.agg_code = agg->agg_code;
  return sm_back(c, k, set_valid, set_code, stats, dbg, &q);
}

static int sma_run(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                   const sm_debug_out& dbg) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  const uint32_t n = k.n;
  const bool host = !b->on_device;
  // the key total comes with the group offsets: the gather's grid bound is cut from it
  uint32_t total = host ? b->pk_offsets[n] : 0;  // host: sizes the pk_indices copy; re-checked on the pinned copy
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device, b->pk_offsets + n, &total)) return r;
  k.agg = true;
  k.d_po = b->pk_offsets; k.d_idx = b->pk_indices;
  // staging: the segment tables always, the batch arrays of a host batch
  sm_stage t;
  sm_stage_tables(t, k);
  const stage_seg* pk_off = t.add(b->pk_offsets, ((size_t)n + 1) * 4, (const void**)&k.d_po);
  t.add(b->pk_indices, (size_t)total * 4, (const void**)&k.d_idx);
  const stage_seg* scalars = sm_stage_arrays(t, k, b);
  size_t bytes = 0;
  if (int r = stage_pack(c, t.segs, host ? t.n : SM_STAGE_TABLES, bytes)) return r;
  if (host) {  // the contract, on the pinned copy the device will see
    if (int r = sma_check_keys(b, (const uint32_t*)(c->pin_in + pk_off->off), total)) return r;
    if (b->scalars)
      if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + scalars->off), n)) return r;
  }
  if (int r = stage_issue(c, bytes)) return r;
  k.chunk_bound = total / PK_CHUNK + n;  // as prepare() sets it: sum ceil(k_i / 32) <= total / 32 + n
  return sm_back(c, k, set_valid, set_code, stats, dbg);
}

// The front of bitfield sets is bits_front's (set-up, host plan, expansion), with
// the expansion buffers as d_po / d_idx and the windows of a context with sums.
// The expansion runs on st_pk in front of the gather, its only reader: the
// signature decode on st and the hashes on st_hash start without it.
static int smb_run(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                   const sm_debug_out& dbg, uint8_t* path) {
  sm_dev k;
  if (int r = sm_open(c, b, set_valid, stats, k)) return r;
  if (!k.n) return BGV_OK;
  if (int r = sm_groups(c, k, b->group_offsets, b->on_device)) return r;
  const uint32_t n = k.n;
  const bool host = !b->on_device;

  bits_args a;
  if (int r = bits_setup(c, a, n, b->bits_len, b->n_indices, !host, true, c->st_pk)) return r;
  c->bits_timed = false;
  a.src = (const bits_src*)b->src; a.v.bits = b->bits; a.v.pk_indices = b->pk_indices;

  // staging: the segment tables always, the batch arrays of a host batch
  sm_stage t;
  sm_stage_tables(t, k);
  const stage_seg* src = t.add(b->src, (size_t)n * sizeof(bits_src), (const void**)&a.src);
  const stage_seg* bits = t.add(b->bits, (size_t)b->bits_len, (const void**)&a.v.bits);
  const stage_seg* indices = t.add(b->pk_indices, (size_t)b->n_indices * 4, (const void**)&a.v.pk_indices);
  const stage_seg* scalars = sm_stage_arrays(t, k, b);
  size_t bytes = 0;
  if (int r = stage_pack(c, t.segs, host ? t.n : SM_STAGE_TABLES, bytes)) return r;
  if (host) {
    // the contract, on the pinned copy the device will see; the plan's totals
    // size the expansion and the gather's grid without a read-back
    bits_view hv = a.v;
    hv.bits = c->pin_in + bits->off;
    hv.pk_indices = (const uint32_t*)(c->pin_in + indices->off);
    bits_plan_out po;
    if (int r = bits_check_sources(n, (const bits_src*)(c->pin_in + src->off), hv, &po, nullptr)) return r;
    if (b->scalars)
      if (int r = scalars_nonzero((const uint64_t*)(c->pin_in + scalars->off), n)) return r;
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
  if (int r = sm_back(c, k, set_valid, set_code, stats, dbg)) return r;
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
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, {}));
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
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, {}, agg));
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
  return sm_done(c, sm_run(c, b, set_valid, set_code, stats, {nullptr, p_group96, s_group192, h_group192}));
}

int bgv_verify_same_message_agg(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  return sm_done(c, sma_run(c, b, set_valid, set_code, stats, {}));
}

int bgv_debug_same_message_agg(bgv_ctx* c, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                               uint8_t* pk_set96, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  return sm_done(c, sma_run(c, b, set_valid, set_code, stats, {pk_set96, p_group96, s_group192, h_group192}));
}

int bgv_verify_same_message_bits(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  return sm_done(c, smb_run(c, b, set_valid, set_code, stats, {}, nullptr));
}

int bgv_debug_same_message_bits(bgv_ctx* c, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats,
                                uint8_t* pk_set96, uint8_t* path, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192) {
  return sm_done(c, smb_run(c, b, set_valid, set_code, stats, {pk_set96, p_group96, s_group192, h_group192}, path));
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
static_assert(SM_JR_IDENTITY == -C_SEG_RETRY, "sm_collect reads the segment verdicts of bgv_same_msg.hip");
uint32_t bgv_sm_split_plan(uint32_t m, uint32_t* sub_off, uint32_t cap) { return sm_split_plan(m, 0, sub_off, cap); }

