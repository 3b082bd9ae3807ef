// Kernels of bgv_verify_same_message_aggregate: the unweighted signature sum of
// every group of a same-message batch, compressed (sig_agg.h has the rule and
// the lane order; bgv_api_sm.hip sm_level places the two launches on the pubkey
// stream, beside the Miller, fold and final-exponentiation stages).
//
// A separate unit: two short, latency-bound kernels (at most four mixed
// additions and four tree levels per lane, then one lane per group) that want
// the code generation of bgv_tail.hip, the Fp product inlined into non-inlined
// Fp2 and point routines, so a lane holds two g2j values and one routine's
// temporaries at a time.
#ifndef BGV_FPMUL_CALL
#define BGV_FPMUL_CALL 0
#endif
#include "bgv_internal.h"
#include "sig_agg.h"

namespace bgv {

#define BGV_SM_LB __launch_bounds__(64, 2)

__device__ __forceinline__ static uint32_t sa_gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }

__device__ __forceinline__ static void shfl_down16(g2j& r, const g2j& p, uint32_t st) {
  const uint32_t* src = (const uint32_t*)&p;
  uint32_t* dst = (uint32_t*)&r;
#pragma unroll
  for (int k = 0; k < (int)(sizeof(g2j) / 4); k++) dst[k] = (uint32_t)__shfl_down((int)src[k], st, 16);
}

// lane = (segment, sub-lane q of 16): the walk, then the tree of sig_agg.h
__global__ void BGV_SM_LB k_sm_sig_seg(sig_agg_view v) {
  const uint32_t t = sa_gtid();
  const uint32_t s = t >> 4, q = t & 15u;
  if (s >= v.n_segs) return;  // whole 16-lane groups
  g2j acc;
  uint32_t cnt;
  sig_agg_walk(acc, cnt, v, v.seg_off[s], v.seg_off[s + 1], q);
  for (uint32_t st = SIG_AGG_LANES / 2; st >= 1; st >>= 1) {
    g2j o;
    shfl_down16(o, acc, st);
    const uint32_t oc = (uint32_t)__shfl_down((int)cnt, st, 16);
    if (q < st) {
      jac_add(acc, acc, o);
      cnt += oc;
    }
  }
  if (q == 0) {
    v.seg_sum[s] = acc;
    v.seg_cnt[s] = cnt;
  }
}

// lane = group: segment sums + prev, affine, 96 compressed bytes, count, code
__global__ void BGV_SM_LB k_sm_sig_group(sig_agg_view v) {
  const uint32_t g = sa_gtid();
  if (g >= v.n_groups) return;
  sig_agg_group(v, g);
}

void launch_sm_sig_agg(hipStream_t st, const sig_agg_view& v) {
  if (!v.n_groups) return;
  hipLaunchKernelGGL(k_sm_sig_seg, dim3((v.n_segs * SIG_AGG_LANES + 63u) / 64u), dim3(64), 0, st, v);
  hipLaunchKernelGGL(k_sm_sig_group, dim3((v.n_groups + 63u) / 64u), dim3(64), 0, st, v);
}

}  // namespace bgv
