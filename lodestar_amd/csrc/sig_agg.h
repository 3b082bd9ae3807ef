// Unweighted per-group signature sums of a same-message batch
// (bgv_verify_same_message_aggregate): what the reference's pre-aggregation
// pools compute on the main thread for every attestation that verified,
//   bls.Signature.aggregate([aggregate.signature, signatureFromBytesNoCheck(sig)])
//   (chain/opPools/attestationPool.ts:182-199, syncCommitteeMessagePool.ts:139).
// The batch has every signature decoded, subgroup-checked and affine
// (dev_work.sig_aff) and its sets cut into segments of at most SM_SEG; left is
//   per segment  T_s = sum of sigma_i over the sets the predicate takes
//   per group    A_g = prev_g + sum_s T_s, compressed (ZCash, 96 bytes)
// The weighted sums of the pairing check (sum r_i sigma_i) are other points.
//
// Lane order (bgv_sig_agg.hip gives every (segment, sub-lane) one lane):
//   sub-lane q of 16 walks sets beg + q, beg + q + 16, .. (at most SM_SEG / 16
//   = 4 mixed additions), then four tree levels fold lane q + st into lane q
//   for st = 8, 4, 2, 1.  Additions are curve.h's complete ones: two equal
//   signatures in a segment double, a signature beside its negation cancels.
// Everything here is BGV_HD: sig_agg_segment runs the sixteen sub-lanes and the
// tree in the same order on the host (tests/native/hostcheck_sig_agg.cpp).
#pragma once
#include "msm_g1.h"

namespace bgv {

constexpr uint32_t SIG_AGG_LANES = 16;

struct sig_agg_view {
  uint32_t n_segs, n_groups;
  const uint32_t* seg_off;    // [n_segs + 1]
  const uint32_t* group_seg;  // [n_groups + 1] first segment of every group
  const g2a* sig_aff;         // [n_sets] decoded signatures
  const uint32_t* skip;       // [n_sets] 1: rejected before aggregation (k_sm_classify)
  const uint8_t* take;        // [n_sets] or NULL: 0 keeps a set out of its group's aggregate
  const uint8_t* valid;       // [n_sets] or NULL (first pass): the final verdicts
  const uint8_t* prev;        // [n_groups][96] or NULL: the running aggregates, compressed
  g2j* seg_sum;               // [n_segs] T_s
  uint32_t* seg_cnt;          // [n_segs] sets in T_s
  uint8_t* out96;             // [n_groups][96] compress(A_g)
  uint32_t* out_cnt;          // [n_groups] sets added
  int32_t* out_code;          // [n_groups] 0, or the code with which prev_g did not decode
};

// does set i enter its group's aggregate
BGV_HD bool sig_agg_takes(const sig_agg_view& v, uint32_t i) {
  return !v.skip[i] && (!v.take || v.take[i]) && (!v.valid || v.valid[i]);
}

// sub-lane q of segment [beg, end): its strided share
BGV_HD void sig_agg_walk(g2j& acc, uint32_t& cnt, const sig_agg_view& v, uint32_t beg, uint32_t end, uint32_t q) {
  jac_set_inf(acc);
  cnt = 0;
  for (uint32_t i = beg + q; i < end; i += SIG_AGG_LANES) {
    if (!sig_agg_takes(v, i)) continue;
    const g2a s = v.sig_aff[i];  // finite: an identity signature is skipped by k_sm_classify
    jac_add_aff(acc, acc, s);
    cnt++;
  }
}

// one segment on the host: the sixteen walks, then the tree in lane order
BGV_HD void sig_agg_segment(const sig_agg_view& v, uint32_t s) {
  g2j acc[SIG_AGG_LANES];
  uint32_t cnt[SIG_AGG_LANES];
  for (uint32_t q = 0; q < SIG_AGG_LANES; q++) sig_agg_walk(acc[q], cnt[q], v, v.seg_off[s], v.seg_off[s + 1], q);
  for (uint32_t st = SIG_AGG_LANES / 2; st >= 1; st >>= 1)
    for (uint32_t q = 0; q < st; q++) {
      jac_add(acc[q], acc[q], acc[q + st]);
      cnt[q] += cnt[q + st];
    }
  v.seg_sum[s] = acc[0];
  v.seg_cnt[s] = cnt[0];
}

// group g: the fold of its segment sums, plus its running aggregate when that
// decodes.  prev is trusted as signatureFromBytesNoCheck trusts it: decoded
// (flags, x < p, on the curve), NOT subgroup-checked.
BGV_HD void sig_agg_group(const sig_agg_view& v, uint32_t g) {
  g2j a;
  jac_set_inf(a);
  uint32_t cnt = 0;
  for (uint32_t s = v.group_seg[g]; s < v.group_seg[g + 1]; s++) {
    const g2j t = v.seg_sum[s];
    jac_add(a, a, t);
    cnt += v.seg_cnt[s];
  }
  int32_t code = C_OK;
  if (v.prev) {
    uint8_t pb[96];
    for (int k = 0; k < 96; k++) pb[k] = v.prev[96u * g + k];
    g2a p;
    bool inf = false;
    code = g2_decompress(p, inf, pb);
    if (code == C_OK && !inf) jac_add_aff(a, a, p);
  }
  g2_compress(v.out96 + 96u * g, a);
  v.out_cnt[g] = cnt;
  v.out_code[g] = code;
}

}  // namespace bgv
