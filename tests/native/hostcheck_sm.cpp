// Host-compiled view of the weighted G1 sum of same-message verification
// (lodestar_amd/csrc/msm_g1.h) for CPU tests against the Python oracle.
// TEST ONLY: the product runs these pieces in the kernels of bgv_same_msg.hip.
// I/O convention of hostcheck.cpp: affine G1 = x || y, 48-byte big-endian
// plain integers; the identity is all-zero.
#include <stdint.h>
#include <vector>
#include "../../lodestar_amd/csrc/msm_g1.h"

using namespace bgv;

static void get_fp(fp_t& r, const uint8_t* b) { fp_t t; fp_from_be48(t, b); fp_to_mont(r, t); }
static void put_fp(uint8_t* b, const fp_t& a) { fp_t t; fp_from_mont(t, a); fp_to_be48(b, t); }

extern "C" {

uint32_t hc_sm_seg_max(void) { return SM_SEG; }

// sum_i scalars[i] * rows[i] over one segment; returns 1, or 0 with out96
// all-zero when the sum is the identity
int hc_sm_g1_segment(const uint8_t* rows96, const uint64_t* scalars, const uint32_t* skip, uint32_t n, uint8_t* out96) {
  std::vector<g1a> rows(n ? n : 1);
  for (uint32_t i = 0; i < n; i++) { get_fp(rows[i].x, rows96 + 96 * i); get_fp(rows[i].y, rows96 + 96 * i + 48); }
  g1a out;
  const bool finite = msm_g1_segment(out, rows.data(), scalars, skip, n);
  put_fp(out96, out.x);
  put_fp(out96 + 48, out.y);
  return finite ? 1 : 0;
}

// one bucket addition on its own (the exceptional cases of the mixed addition):
// a + b for affine a, b; returns 0 for the identity
int hc_sm_bucket_pair(const uint8_t* a96, const uint8_t* b96, uint8_t* out96) {
  g1a a, b, o;
  get_fp(a.x, a96); get_fp(a.y, a96 + 48);
  get_fp(b.x, b96); get_fp(b.y, b96 + 48);
  g1j acc;
  jac_set_inf(acc);
  msm_g1_bucket_add(acc, a);
  msm_g1_bucket_add(acc, b);
  const bool finite = jac_to_aff(o, acc);
  put_fp(out96, o.x);
  put_fp(out96 + 48, o.y);
  return finite ? 1 : 0;
}
}
