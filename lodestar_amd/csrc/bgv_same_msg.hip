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
__device__ __forceinline__ static bool sm_load_pk(g1a& out, const sm_view& v, uint32_t idx) {
  if (idx & 0x80000000u) {
    const uint32_t r = idx & 0x7fffffffu;
    if (r >= v.n_raw) return false;
    out = v.raw_pks[r];
  } else {
    if (idx >= v.table_n) return false;
    out = v.table[idx];
  }
  return true;
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
__global__ void BGV_SM_LB k_sm_g1_digit(sm_view v) {
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
      g1a row;
      if (sm_load_pk(row, v, v.pk_idx[i])) msm_g1_bucket_add(acc, row);  // in range: k_sm_classify skipped the others
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
// group's message replicated
__global__ void BGV_SM_LB k_sm_retry_gather(sm_retry r) {
  const uint32_t t = sm_gtid();
  if (t > r.n) return;
  r.o_iota[t] = t;
  if (t == r.n) return;
  const uint32_t i = r.list[t], g = r.list_group[t];
  r.o_idx[t] = r.pk_idx[i];
  r.o_len[t] = r.sig_len[i];
  r.o_scalars[t] = r.scalars[i];
  for (uint32_t k = 0; k < 32; k++) r.o_msgs[32u * t + k] = r.msgs[32u * g + k];
  for (uint32_t k = 0; k < 192; k++) r.o_sigs[192u * t + k] = r.sigs[192u * i + k];
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

}  // namespace bgv
