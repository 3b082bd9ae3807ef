// Host side of the C ABI (include/bgv.h), the index lists and bitfield sets:
// resident index lists and their prefix sums, the host plan of a bits batch,
// the expansion in front of the ordinary pipeline (bgv_api.hip) and the debug
// entries that export it.  bits_setup and the launch halves are shared with
// the bitfield front of the same-message entries (bgv_api_sm.hip smb_run).
//
// include/bgv.h bgv_verify_bits.  The expansion (bgv_bits.hip) runs on the main
// stream in front of the ordinary pipeline and leaves an on-device bgv_batch in
// all but name: pk_off / pk_idx in context-owned buffers, everything else the
// staged (or the caller's device) arrays.
#include <vector>

#include "bgv_host.h"

static_assert(sizeof(bgv_set_src) == sizeof(bits_src) && BGV_MAX_INDEX_LISTS == BITS_MAX_LISTS &&
                  BGV_SRC_EXPLICIT == BITS_SRC_EXPLICIT,
              "bits_expand.h mirrors include/bgv.h");

namespace bgv::host {

// drop the resident sums of one list / of every list, after the streams drained
static int sums_drop(bgv_ctx* c, uint32_t id) {
  if (!c->idx_sums[id]) return 0;
  if (int r = ctx_drain(c)) return r;
  (void)hipFree(c->idx_sums[id]);
  c->idx_sums[id] = nullptr;
  return 0;
}
int sums_drop_all(bgv_ctx* c) {
  for (uint32_t k = 0; k < BGV_MAX_INDEX_LISTS; k++)
    if (int r = sums_drop(c, k)) return r;
  return 0;
}

}  // namespace bgv::host

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

namespace bgv::host {

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
// (bits_plan_out, bgv_host.h)
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
int bits_check_sources(uint32_t n, const bits_src* src, const bits_view& v, bits_plan_out* out, uint8_t* path) {
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
void bits_host_view(bits_view& v, const uint32_t* list_len, const uint8_t* list_has_sums) {
  static const uint32_t present = 0;  // a non-NULL stand-in: the check reads no list entry and no sum
  memset(&v, 0, sizeof v);
  for (uint32_t k = 0; k < BGV_MAX_INDEX_LISTS; k++) {
    v.list[k] = list_len[k] ? &present : nullptr;
    v.list_len[k] = list_len[k];
    v.sums[k] = list_len[k] && list_has_sums && list_has_sums[k] ? &present : nullptr;
  }
}

}  // namespace bgv::host

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

namespace bgv::host {

// The set-up every entry that expands bitfields shares: bits_args / bits_view
// over the context's lists (and their sums, unless use_sums is false), the
// offset buffer, the per-set windows when a list has sums, and the context's
// record of the batch (bgv_bits_path_stats).  a.src, a.v.bits and
// a.v.pk_indices are the caller's to fill; the tally of an on-device batch is
// zeroed on `st`, the stream the expansion will run on.
int bits_setup(bgv_ctx* c, bits_args& a, uint32_t n, uint32_t bits_len, uint32_t n_indices, bool on_device, bool use_sums,
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
void bits_launch_count(hipStream_t st, const bits_args& a) {
  launch_bits_count(st, a);
  if (a.n_sets) launch_scan(st, a.pk_off, a.n_sets);
}
// `gathered`: the keys the expansion holds (the scan's total)
int bits_launch_expand(bgv_ctx* c, hipStream_t st, bits_args& a, uint32_t gathered) {
  if (int r = ensure_or_release_lines(c, c->bits_idx, gathered ? gathered : 1)) return r;
  a.pk_idx = c->bits_idx.p;
  a.cap = gathered;
  launch_bits_expand(st, a);
  return 0;
}
// the totals of an on-device batch, after bits_launch_count on `st`: the host
// learns the gathered keys (buffer and grid bound) and the participating keys
int bits_read_totals(bgv_ctx* c, hipStream_t st, const bits_args& a) {
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

}  // namespace bgv::host

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
