// Host-compiled view of the weighted G1 sum over aggregated (Jacobian) keys
// (lodestar_amd/csrc/msm_g1.h msm_g1_segment_jac) for CPU tests against the
// Python oracle.  TEST ONLY: the product runs these pieces in the kernels of
// bgv_same_msg.hip (k_sma_g1_digit).
// I/O: a Jacobian G1 point is X || Y || Z, an affine one x || y, every
// coordinate a 48-byte big-endian plain integer; the affine identity is
// all-zero, the Jacobian one has Z = 0.
//
// With HOSTCHECK_SMA_MAIN the file is a stand-alone program (sanitizer builds):
// it reads  n (u32 LE) | n x 144 B points | n x u64 LE scalars | n x u32 LE skip
// from stdin and prints `finite` and the 96 result bytes in hex.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../lodestar_amd/csrc/msm_g1.h"

using namespace bgv;

static void get_fp(fp_t& r, const uint8_t* b) { fp_t t; fp_from_be48(t, b); fp_to_mont(r, t); }
static void put_fp(uint8_t* b, const fp_t& a) { fp_t t; fp_from_mont(t, a); fp_to_be48(b, t); }
static void get_jac(g1j& p, const uint8_t* b) { get_fp(p.x, b); get_fp(p.y, b + 48); get_fp(p.z, b + 96); }
static void put_jac(uint8_t* b, const g1j& p) { put_fp(b, p.x); put_fp(b + 48, p.y); put_fp(b + 96, p.z); }

static int segment_jac(const uint8_t* pks144, const uint64_t* scalars, const uint32_t* skip, uint32_t n, uint8_t* out96) {
  std::vector<g1j> pks(n ? n : 1);
  for (uint32_t i = 0; i < n; i++) get_jac(pks[i], pks144 + 144 * (size_t)i);
  g1a out;
  const bool finite = msm_g1_segment_jac(out, pks.data(), scalars, skip, n);
  put_fp(out96, out.x);
  put_fp(out96 + 48, out.y);
  return finite ? 1 : 0;
}

#ifndef HOSTCHECK_SMA_MAIN
extern "C" {

// sum_i scalars[i] * pks[i] over one segment; returns 1, or 0 with out96
// all-zero when the sum is the identity
int hc_sma_g1_segment(const uint8_t* pks144, const uint64_t* scalars, const uint32_t* skip, uint32_t n, uint8_t* out96) {
  return segment_jac(pks144, scalars, skip, n, out96);
}

// rows[order[0]] + rows[order[1]] + ... by mixed additions, as the gather
// builds a set's key, left in Jacobian form: the representation (its Z)
// depends on the order, the point does not
void hc_sma_sum_rows(const uint8_t* rows96, const uint32_t* order, uint32_t n, uint8_t* out144) {
  g1j acc;
  jac_set_inf(acc);
  for (uint32_t k = 0; k < n; k++) {
    g1a row;
    get_fp(row.x, rows96 + 96 * (size_t)order[k]);
    get_fp(row.y, rows96 + 96 * (size_t)order[k] + 48);
    msm_g1_bucket_add(acc, row);
  }
  put_jac(out144, acc);
}

// one bucket addition on its own: a + b for Jacobian a, b; returns 0 for the identity
int hc_sma_bucket_pair(const uint8_t* a144, const uint8_t* b144, uint8_t* out96) {
  g1j a, b, acc;
  get_jac(a, a144);
  get_jac(b, b144);
  jac_set_inf(acc);
  msm_g1_bucket_add_jac(acc, a);
  msm_g1_bucket_add_jac(acc, b);
  g1a o;
  const bool finite = jac_to_aff(o, acc);
  put_fp(out96, o.x);
  put_fp(out96 + 48, o.y);
  return finite ? 1 : 0;
}
}
#else
int main() {
  uint32_t n = 0;
  if (fread(&n, 4, 1, stdin) != 1 || n > 4096) return 2;
  std::vector<uint8_t> pks((size_t)n * 144);
  std::vector<uint64_t> scalars(n);
  std::vector<uint32_t> skip(n);
  if (n && (fread(pks.data(), 144, n, stdin) != n || fread(scalars.data(), 8, n, stdin) != n || fread(skip.data(), 4, n, stdin) != n))
    return 2;
  uint8_t out[96];
  const int finite = segment_jac(pks.data(), scalars.data(), skip.data(), n, out);
  printf("%d ", finite);
  for (int k = 0; k < 96; k++) printf("%02x", out[k]);
  printf("\n");
  return 0;
}
#endif
