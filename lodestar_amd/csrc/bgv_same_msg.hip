// Kernels of same-message batch verification (bgv_verify_same_message):
// single-pubkey sets that share their signing root, as gossip attestations of
// one committee do (chain/validation/attestation.ts:271), need
//   prod_i e(pk_i, H(m))^{r_i} = e(sum_i r_i pk_i, H(m))
// so a group of n sets costs one hash and two Miller pairs instead of n of
// each.  This unit holds the pubkey side: the weighted G1 sum over gathered
// table rows (msm_g1.h), and the glue that turns every segment into one set of
// a virtual batch for the existing Miller / fold / final-exponentiation stages.
//
// Compiled like the pubkey gather (bgv_gather.hip): the Fp product inlined, so
// a gathered row's 96 bytes stay in flight across the previous mixed addition.
#define BGV_FPMUL_CALL 0
#ifndef BGV_FP2_INLINE
#define BGV_FP2_INLINE 1
#endif
#ifndef BGV_POINT_INLINE
#define BGV_POINT_INLINE 1
#endif
#include "bgv_internal.h"
#include "msm_g1.h"

namespace bgv {

#define BGV_SM_LB __launch_bounds__(64, 2)

__device__ __forceinline__ static uint32_t sm_gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }

// row of the pubkey table, or of the raw side table for bit 31; false: out of range
__device__ __forceinline__ static bool sm_load_row(g1a& out, const g1a* table, uint32_t table_n, const g1a* raw_pks, uint32_t n_raw,
                                                   uint32_t idx) {
  if (idx & 0x80000000u) {
    const uint32_t r = idx & 0x7fffffffu;
    if (r >= n_raw) return false;
    out = raw_pks[r];
  } else {
    if (idx >= table_n) return false;
    out = table[idx];
  }
  return true;
}
__device__ __forceinline__ static bool sm_load_pk(g1a& out, const sm_view& v, uint32_t idx) {
  return sm_load_row(out, v.table, v.table_n, v.raw_pks, v.n_raw, idx);
}

// per set: which sets enter the sums.  A set is rejected here, with its code
// (signature code first, then the key's, as k_set_codes orders them), when its
// signature did not decode or is outside G2, is the identity, or when its key
// index is out of range or names the identity.
__global__ void BGV_SM_LB k_sm_classify(sm_view v) {
  const uint32_t i = sm_gtid();
  if (i >= v.n_sets) return;
  int32_t code = v.sig_code[i];
  if (code == C_OK) {
    g1a row;
    if (!sm_load_pk(row, v, v.pk_idx[i])) code = C_INDEX_RANGE;
    else if (g1a_is_zero(row)) code = C_PK_IS_INFINITY;
    else if (v.sig_inf[i]) code = C_VERIFY_FAIL;
  }
  v.set_code[i] = code;
  v.skip[i] = code != C_OK ? 1u : 0u;
}

__device__ __forceinline__ static void shfl_down16(g1j& r, const g1j& p, uint32_t st) {
  const uint32_t* src = (const uint32_t*)&p;
  uint32_t* dst = (uint32_t*)&r;
#pragma unroll
  for (int k = 0; k < (int)(sizeof(g1j) / 4); k++) dst[k] = (uint32_t)__shfl_down((int)src[k], st, 16);
}

// lane = (segment, window w, digit d), 256 lanes per segment (four windows per
// wave), the layout of k_msm_digit:
//   1. bucket d of window w in registers: every lane walks its segment's
//      scalars (<= SM_SEG of them) to its next match and gathers that row; the
//      wave runs as many mixed additions as its fullest bucket holds;
//   2. d B_d by double-and-add;
//   3. S_w = sum_d d B_d by a tree over the window's 16 lanes.
// No bucket is indexed at run time: each lane owns exactly one.
// The addend of set i: its table row, added by the mixed addition, or, for
// aggregate sets (AGG), PK_i in Jacobian form from pk_set, added by the full
// one (msm_g1.h msm_g1_bucket_add_jac).
template <bool AGG>
__device__ __forceinline__ static void sm_g1_digit(const sm_view& v) {
  const uint32_t t = sm_gtid();
  const uint32_t s = t >> 8, win = (t >> 4) & 15u, d = t & 15u;
  if (s >= v.n_segs) return;  // whole waves: 256 lanes per segment
  const uint32_t beg = v.seg_off[s], end = v.seg_off[s + 1];
  g1j acc;
  jac_set_inf(acc);
  uint32_t i = beg;
  for (;;) {
    while (i < end) {
      if (d != 0 && !v.skip[i] && msm_g1_digit(v.scalars[i], win) == d) break;
      i++;
    }
    if (!__any(i < end)) break;
    if (i < end) {
      if constexpr (AGG) {
        const g1j pk = v.pk_set[i];  // finite: k_sma_classify skipped the others
        msm_g1_bucket_add_jac(acc, pk);
      } else {
        g1a row;
        if (sm_load_pk(row, v, v.pk_idx[i])) msm_g1_bucket_add(acc, row);  // in range: k_sm_classify skipped the others
      }
      i++;
    }
  }
  msm_g1_scale_digit(acc, d);
  for (uint32_t st = 8; st >= 1; st >>= 1) {
    g1j o;
    shfl_down16(o, acc, st);
    if (d < st) jac_add(acc, acc, o);
  }
  if (d == 0) v.win[16u * s + win] = acc;
}
__global__ void BGV_SM_LB k_sm_g1_digit(sm_view v) { sm_g1_digit<false>(v); }
__global__ void BGV_SM_LB k_sma_g1_digit(sm_view v) { sm_g1_digit<true>(v); }  // k_sm_g1_fold finishes the segment for both

// lane = (segment, window): 16^w S_w, a tree over the segment's 16 lanes, then
// lane 0 converts P_seg to affine and classifies the segment
__global__ void BGV_SM_LB k_sm_g1_fold(sm_view v) {
  const uint32_t t = sm_gtid();
  const uint32_t s = t >> 4, win = t & 15u;
  if (s >= v.n_segs) return;  // whole 16-lane groups
  g1j p = v.win[16u * s + win];
  msm_g1_shift(p, win);
  for (uint32_t st = 8; st >= 1; st >>= 1) {
    g1j o;
    shfl_down16(o, p, st);
    if (win < st) jac_add(p, p, o);
  }
  if (win != 0) return;
  uint32_t live = 0;
  for (uint32_t i = v.seg_off[s]; i < v.seg_off[s + 1]; i++) live += v.skip[i] ? 0u : 1u;
  g1a pa;
  const bool finite = jac_to_aff(pa, p);  // the all-zero point for the identity
  v.p_seg[s] = pa;
  v.seg_code[s] = live == 0 ? C_SEG_DEAD : (finite ? C_OK : C_SEG_RETRY);
}

// per segment, once the hashes and the G2 sums are there: the virtual batch's
// codes and H(m) of the segment's group
__global__ void BGV_SM_LB k_sm_apply(sm_view v) {
  const uint32_t s = sm_gtid();
  if (s >= v.n_segs) return;
  const int32_t code = v.seg_code[s];
  v.pk_code_v[s] = code;
  v.job_code_v[s] = code;
  v.h_seg[s] = v.h_group[v.seg_group[s]];
}

// bgv_debug_same_message: per group, the sums over its segments
__global__ void BGV_SM_LB k_sm_group_sums(sm_view v, const uint32_t* group_seg, g1a* p_group, g2a* s_group) {
  const uint32_t g = sm_gtid();
  if (g >= v.n_groups) return;
  g1j p;
  g2j sg;
  jac_set_inf(p);
  jac_set_inf(sg);
  for (uint32_t s = group_seg[g]; s < group_seg[g + 1]; s++) {
    const g1a a = v.p_seg[s];
    if (!g1a_is_zero(a)) jac_add_aff(p, p, a);
    if (!v.s_inf[s]) {
      const g2a b = v.s_seg[s];
      jac_add_aff(sg, sg, b);
    }
  }
  g1a pa;
  g2a sa;
  jac_to_aff(pa, p);
  jac_to_aff(sa, sg);
  p_group[g] = pa;
  s_group[g] = sa;
}

// the per-set retry's batch: set list[k] as set k = job k with one key, its
// group's message replicated.  Aggregate sets (AGG): the set's aggregated key
// becomes row t of a raw-key table, o_pk[t] = PK_i affine, and the job's single
// index is 0x80000000 | t.
template <bool AGG>
__device__ __forceinline__ static void sm_retry_gather(const sm_retry& r, const g1j* pk_set, g1a* o_pk) {
  const uint32_t t = sm_gtid();
  if (t > r.n) return;
  r.o_iota[t] = t;
  if (t == r.n) return;
  const uint32_t i = r.list[t], g = r.list_group[t];
  if constexpr (AGG) {
    g1a a;
    jac_to_aff(a, pk_set[i]);
    o_pk[t] = a;
    r.o_idx[t] = 0x80000000u | t;
  } else {
    r.o_idx[t] = r.pk_idx[i];
  }
  r.o_len[t] = r.sig_len[i];
  r.o_scalars[t] = r.scalars[i];
  for (uint32_t k = 0; k < 32; k++) r.o_msgs[32u * t + k] = r.msgs[32u * g + k];
  for (uint32_t k = 0; k < 192; k++) r.o_sigs[192u * t + k] = r.sigs[192u * i + k];
}
__global__ void BGV_SM_LB k_sm_retry_gather(sm_retry r) { sm_retry_gather<false>(r, nullptr, nullptr); }
__global__ void BGV_SM_LB k_sma_retry_gather(sm_retry r, const g1j* pk_set, g1a* o_pk) { sm_retry_gather<true>(r, pk_set, o_pk); }

// ---- split retry (bgv_sm_retry mode 1, sm_split.h) ---------------------------
// Level 1 reads what the first pass left on the device: lane t copies set
// list[t]'s scalar, key (its index, or PK_i of an aggregate set) and decoded
// signature to position t of the retry's own buffers, so that the sum kernels
// above and k_msm_digit run over them with a sub as a short segment.  Nothing
// is computed; the first n_subs lanes also write their sub's group.
template <bool AGG>
__device__ __forceinline__ static void sm_split_gather(const sm_split& q) {
  const uint32_t t = sm_gtid();
  if (t >= q.n) return;
  const uint32_t i = q.list[t];
  if constexpr (AGG) {
    const g1j pk = q.pk_set[i];
    q.o_pk[t] = pk;
  } else {
    q.o_idx[t] = q.pk_idx[i];
  }
  q.o_scalars[t] = q.scalars[i];
  const g2a sig = q.sig_aff[i];
  q.o_sig[t] = sig;
  q.o_skip[t] = 0u;
  if (t < q.n_subs) q.o_sub_group[t] = q.list_group[q.sub_off[t]];  // n_subs <= n: a sub is never empty
}
__global__ void BGV_SM_LB k_sm_split_gather(sm_split q) { sm_split_gather<false>(q); }
__global__ void BGV_SM_LB k_sma_split_gather(sm_split q) { sm_split_gather<true>(q); }

// Level 2: leaf t = set t = job t of a virtual batch whose pairs are
// (pk_i, H(m_g)) and (-G1, sigma_i), unscaled, so its verdict is the set's own.
// One jac_to_aff per aggregate key, no other arithmetic.
template <bool AGG>
__device__ __forceinline__ static void sm_split_leaves(const sm_leaves& q) {
  const uint32_t t = sm_gtid();
  if (t > q.n) return;
  q.iota[t] = t;
  if (t == q.n) return;
  const uint32_t i = q.leaf[t];
  g1a pk;
  int32_t code = C_OK;
  if constexpr (AGG) {
    if (!jac_to_aff(pk, q.pk_set[i])) code = C_PK_IS_INFINITY;  // k_sma_classify skipped such a set
  } else {
    if (!sm_load_row(pk, q.table, q.table_n, q.raw_pks, q.n_raw, q.pk_idx[i])) {  // k_sm_classify skipped such a set
      code = C_INDEX_RANGE;
      fp_set_zero(pk.x);
      fp_set_zero(pk.y);
    }
  }
  q.rpk_aff[t] = pk;
  const g2a h = q.h_group[q.leaf_group[t]];
  q.h_aff[t] = h;
  const g2a sig = q.sig_aff[i];
  q.s_aff[t] = sig;
  q.s_inf[t] = 0u;
  q.pk_code[t] = code;
  q.job_code[t] = code;
}
__global__ void BGV_SM_LB k_sm_split_leaves(sm_leaves q) { sm_split_leaves<false>(q); }
__global__ void BGV_SM_LB k_sma_split_leaves(sm_leaves q) { sm_split_leaves<true>(q); }

// ---- aggregate sets (bgv_verify_same_message_agg) ---------------------------
// A set's key is PK_i = sum_j pk_{i,j}.  The balanced gather of the ordinary
// pipeline (k_chunk_count / k_scan / k_chunk_set / k_pk_chunk) leaves one
// partial sum per PK_CHUNK keys; the kernels below fold them per set, and the
// weighted sum (sm_g1_digit<true> above) runs over the folded keys.

// lane = set: the fold of k_pk without its scalar multiplication and without
// its inversion.  PK_i stays Jacobian; the key code is k_pk's: the range marker
// (0, 1, 1) of a chunk (or offsets that run backwards) is C_INDEX_RANGE, the
// identity C_PK_IS_INFINITY.  A rejected set's PK_i is stored as the identity.
__global__ void BGV_SM_LB k_sma_set_sum(dev_batch b, dev_work w, g1j* pk_set, int32_t* pk_set_code) {
  const uint32_t i = sm_gtid();
  if (i >= b.n_sets) return;
  g1j acc;
  jac_set_inf(acc);
  const uint32_t c0 = w.chunk_off[i], c1 = w.chunk_off[i + 1];
  bool range_err = c1 > b.chunk_bound || b.pk_off[i + 1] < b.pk_off[i];
  for (uint32_t c = c0; c < c1 && !range_err; c++) {
    const g1j p = w.pk_part[c];
    if (!jac_is_inf(p) && fp_is_zero(p.x)) range_err = true;
    else jac_add(acc, acc, p);
  }
  int32_t code = C_OK;
  if (range_err) code = C_INDEX_RANGE;
  else if (jac_is_inf(acc)) code = C_PK_IS_INFINITY;
  if (code != C_OK) jac_set_inf(acc);
  pk_set[i] = acc;
  pk_set_code[i] = code;
}

// k_sm_classify for aggregate keys: signature code first, then the key code of
// k_sma_set_sum, then the identity signature
__global__ void BGV_SM_LB k_sma_classify(sm_view v) {
  const uint32_t i = sm_gtid();
  if (i >= v.n_sets) return;
  int32_t code = v.sig_code[i];
  if (code == C_OK) code = v.pk_set_code[i];
  if (code == C_OK && v.sig_inf[i]) code = C_VERIFY_FAIL;
  v.set_code[i] = code;
  v.skip[i] = code != C_OK ? 1u : 0u;
}

// PK_i as an affine point (all-zero for a rejected key): bgv_debug_same_message_agg
__global__ void BGV_SM_LB k_sma_pk_aff(const g1j* pk_set, g1a* out, uint32_t n) {
  const uint32_t i = sm_gtid();
  if (i >= n) return;
  g1a a;
  jac_to_aff(a, pk_set[i]);
  out[i] = a;
}

static inline dim3 sm_grid(uint32_t n) { return dim3((n + 63u) / 64u); }

void launch_sm_classify(hipStream_t st, const sm_view& v) {
  if (v.n_sets) hipLaunchKernelGGL(k_sm_classify, sm_grid(v.n_sets), dim3(64), 0, st, v);
}

void launch_sm_g1_sum(hipStream_t st, const sm_view& v) {
  if (!v.n_segs) return;
  hipLaunchKernelGGL(k_sm_g1_digit, dim3(v.n_segs * 4u), dim3(64), 0, st, v);
  hipLaunchKernelGGL(k_sm_g1_fold, sm_grid(v.n_segs * 16u), dim3(64), 0, st, v);
}

void launch_sm_apply(hipStream_t st, const sm_view& v) {
  if (v.n_segs) hipLaunchKernelGGL(k_sm_apply, sm_grid(v.n_segs), dim3(64), 0, st, v);
}

void launch_sm_group_sums(hipStream_t st, const sm_view& v, const uint32_t* group_seg, g1a* p_group, g2a* s_group) {
  if (v.n_groups) hipLaunchKernelGGL(k_sm_group_sums, sm_grid(v.n_groups), dim3(64), 0, st, v, group_seg, p_group, s_group);
}

void launch_sm_retry_gather(hipStream_t st, const sm_retry& r) {
  hipLaunchKernelGGL(k_sm_retry_gather, sm_grid(r.n + 1u), dim3(64), 0, st, r);
}

void launch_sm_split_gather(hipStream_t st, const sm_split& q) {
  if (!q.n) return;
  if (q.pk_set) hipLaunchKernelGGL(k_sma_split_gather, sm_grid(q.n), dim3(64), 0, st, q);
  else hipLaunchKernelGGL(k_sm_split_gather, sm_grid(q.n), dim3(64), 0, st, q);
}

void launch_sm_split_leaves(hipStream_t st, const sm_leaves& q) {
  if (q.pk_set) hipLaunchKernelGGL(k_sma_split_leaves, sm_grid(q.n + 1u), dim3(64), 0, st, q);
  else hipLaunchKernelGGL(k_sm_split_leaves, sm_grid(q.n + 1u), dim3(64), 0, st, q);
}

void launch_sma_set_sum(hipStream_t st, const dev_batch& b, const dev_work& w, g1j* pk_set, int32_t* pk_set_code) {
  if (b.n_sets) hipLaunchKernelGGL(k_sma_set_sum, sm_grid(b.n_sets), dim3(64), 0, st, b, w, pk_set, pk_set_code);
}

void launch_sma_classify(hipStream_t st, const sm_view& v) {
  if (v.n_sets) hipLaunchKernelGGL(k_sma_classify, sm_grid(v.n_sets), dim3(64), 0, st, v);
}

void launch_sma_g1_sum(hipStream_t st, const sm_view& v) {
  if (!v.n_segs) return;
  hipLaunchKernelGGL(k_sma_g1_digit, dim3(v.n_segs * 4u), dim3(64), 0, st, v);
  hipLaunchKernelGGL(k_sm_g1_fold, sm_grid(v.n_segs * 16u), dim3(64), 0, st, v);
}

void launch_sma_pk_aff(hipStream_t st, const g1j* pk_set, g1a* out, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_sma_pk_aff, sm_grid(n), dim3(64), 0, st, pk_set, out, n);
}

void launch_sma_retry_gather(hipStream_t st, const sm_retry& r, const g1j* pk_set, g1a* o_pk) {
  hipLaunchKernelGGL(k_sma_retry_gather, sm_grid(r.n + 1u), dim3(64), 0, st, r, pk_set, o_pk);
}

}  // namespace bgv
