// Weighted G1 sum  P = sum_i r_i PK_i  over affine table rows with 64-bit
// weights: the pubkey side of same-message batch verification
// (bgv_verify_same_message; IBlsVerifier.verifySignatureSetsSameMessage).
//
// Bucket method over the sixteen 4-bit windows of the weights, as the G2 side
// does for sum r_i sigma_i (bgv_kernels.hip k_msm_digit / k_msm_job):
//   B_{w,d} = sum of the rows whose digit w is d      (mixed additions)
//   S_w     = sum_d d B_{w,d}                          (d B by double-and-add)
//   P       = sum_w 16^w S_w                           (4 w doublings, a tree)
// The rows are affine, so a bucket addition is madd-2007-bl (11 Fp products);
// per row that is 16 of them, against ~910 products of a per-set 4-bit window
// multiplication.  curve.h jac_add_aff takes the exceptional cases: the same
// validator twice in one bucket (P + P doubles) and a key beside its negation
// (P + (-P) empties the bucket).
//
// Everything here is BGV_HD: the device kernels (bgv_same_msg.hip) give every
// (segment, window, digit) one lane and call these pieces; msm_g1_segment
// runs the same pieces in sequence on the host (tests/native/hostcheck_sm.cpp).
#pragma once
#include "curve.h"

namespace bgv {

// Groups are cut into segments of at most SM_SEG sets: one segment is one
// 256-lane block of the sum kernels and one job of the virtual batch that
// carries the pairing check (its per-job fallback localises to a segment).
constexpr uint32_t SM_SEG = 64;
constexpr uint32_t MSM_G1_WINDOWS = 16;

BGV_HD uint32_t msm_g1_digit(uint64_t k, uint32_t win) { return (uint32_t)(k >> (4u * win)) & 15u; }

// bucket += row (row is not the identity)
BGV_HD void msm_g1_bucket_add(g1j& bucket, const g1a& row) { jac_add_aff(bucket, bucket, row); }

// bucket <- d * bucket, 1 <= d <= 15, MSB first: at most 3 doublings and 3 additions
BGV_HD void msm_g1_scale_digit(g1j& acc, uint32_t d) {
  const g1j base = acc;
  for (int bit = 2; bit >= 0; bit--) {
    if (d >> (bit + 1)) {
      jac_dbl(acc, acc);
      if ((d >> bit) & 1u) jac_add(acc, acc, base);
    }
  }
}

// s <- 16^win * s
BGV_HD void msm_g1_shift(g1j& s, uint32_t win) {
  for (uint32_t k = 0; k < 4u * win; k++) jac_dbl(s, s);
}

// bucket (win, d) of rows[0, n): rows flagged in `skip` (may be NULL) and
// identity rows (all-zero) add nothing
BGV_HD void msm_g1_bucket(g1j& acc, const g1a* rows, const uint64_t* scalars, const uint32_t* skip, uint32_t n,
                          uint32_t win, uint32_t d) {
  jac_set_inf(acc);
  if (d == 0) return;
  for (uint32_t i = 0; i < n; i++) {
    if ((skip && skip[i]) || msm_g1_digit(scalars[i], win) != d) continue;
    if (fp_is_zero(rows[i].x) && fp_is_zero(rows[i].y)) continue;
    msm_g1_bucket_add(acc, rows[i]);
  }
}

// the whole sum of one segment, one (window, digit) after the other; returns
// false (and the all-zero point) when the sum is the identity
BGV_HD bool msm_g1_segment(g1a& out, const g1a* rows, const uint64_t* scalars, const uint32_t* skip, uint32_t n) {
  g1j total;
  jac_set_inf(total);
  for (uint32_t win = 0; win < MSM_G1_WINDOWS; win++) {
    g1j sw;
    jac_set_inf(sw);
    for (uint32_t d = 1; d < 16; d++) {
      g1j b;
      msm_g1_bucket(b, rows, scalars, skip, n, win, d);
      msm_g1_scale_digit(b, d);
      jac_add(sw, sw, b);
    }
    msm_g1_shift(sw, win);
    jac_add(total, total, sw);
  }
  return jac_to_aff(out, total);
}

// ---- aggregate sets (bgv_verify_same_message_agg) ---------------------------
// A set's key is PK_i = sum_j pk_{i,j}, left in Jacobian form by the per-set
// fold of the gather's chunk sums (k_sma_set_sum): no inversion per set.  The
// bucket addition is then add-2007-bl (16 Fp products); curve.h jac_add takes
// the exceptional cases by cross-multiplying, so two representations of one
// point double and a point beside its negation empties the bucket.

// bucket += pk (pk is not the identity)
BGV_HD void msm_g1_bucket_add_jac(g1j& bucket, const g1j& pk) { jac_add(bucket, bucket, pk); }

// bucket (win, d) of pks[0, n): entries flagged in `skip` (may be NULL) and
// identity entries add nothing
BGV_HD void msm_g1_bucket_jac(g1j& acc, const g1j* pks, const uint64_t* scalars, const uint32_t* skip, uint32_t n,
                              uint32_t win, uint32_t d) {
  jac_set_inf(acc);
  if (d == 0) return;
  for (uint32_t i = 0; i < n; i++) {
    if ((skip && skip[i]) || msm_g1_digit(scalars[i], win) != d) continue;
    if (jac_is_inf(pks[i])) continue;
    msm_g1_bucket_add_jac(acc, pks[i]);
  }
}

// msm_g1_segment over Jacobian entries
BGV_HD bool msm_g1_segment_jac(g1a& out, const g1j* pks, const uint64_t* scalars, const uint32_t* skip, uint32_t n) {
  g1j total;
  jac_set_inf(total);
  for (uint32_t win = 0; win < MSM_G1_WINDOWS; win++) {
    g1j sw;
    jac_set_inf(sw);
    for (uint32_t d = 1; d < 16; d++) {
      g1j b;
      msm_g1_bucket_jac(b, pks, scalars, skip, n, win, d);
      msm_g1_scale_digit(b, d);
      jac_add(sw, sw, b);
    }
    msm_g1_shift(sw, win);
    jac_add(total, total, sw);
  }
  return jac_to_aff(out, total);
}

}  // namespace bgv
