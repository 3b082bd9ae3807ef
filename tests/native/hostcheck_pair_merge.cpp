// Host-compiled view of the pair classes of bgv_pair_merge
// (lodestar_amd/csrc/pair_merge.h) for CPU tests against the Python oracle.
// TEST ONLY: the product runs these pieces in the kernels of
// bgv_pair_merge.hip.  I/O convention of hostcheck.cpp: affine G1 = x || y,
// 48-byte big-endian plain integers, all-zero for the identity.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../lodestar_amd/csrc/pair_merge.h"

using namespace bgv;

static void get_fp(fp_t& r, const uint8_t* b) { fp_t t; fp_from_be48(t, b); fp_to_mont(r, t); }
static void put_fp(uint8_t* b, const fp_t& a) { fp_t t; fp_from_mont(t, a); fp_to_be48(b, t); }

extern "C" {

uint64_t hc_pm_slot_mix(uint32_t job, uint32_t rep, uint64_t key) { return pm_slot_mix(job, rep, key); }
uint32_t hc_pm_job_of(const uint32_t* job_off, uint32_t n_jobs, uint32_t i) { return pm_job_of(job_off, n_jobs, i); }

// One class among n sets: its members are order[0 .. m) (set indices below n),
// linked in that order as k_pm_link leaves them; pts96 / codes are the n sets'
// scaled keys and key codes.  out96: P_c; returns the class code, *ident the
// identity flag.
int32_t hc_pm_class_sum(const uint8_t* pts96, const int32_t* codes, uint32_t n, const uint32_t* order, uint32_t m,
                        uint8_t* out96, uint32_t* ident) {
  std::vector<g1a> rpk(n ? n : 1);
  for (uint32_t i = 0; i < n; i++) {
    get_fp(rpk[i].x, pts96 + 96 * (size_t)i);
    get_fp(rpk[i].y, pts96 + 96 * (size_t)i + 48);
  }
  std::vector<uint32_t> next(n ? n : 1, PM_NONE);
  for (uint32_t k = 0; k + 1 < m; k++) next[order[k]] = order[k + 1];
  g1a out;
  int32_t code;
  bool id;
  pm_class_sum(out, code, id, rpk.data(), codes, next.data(), m ? order[0] : PM_NONE, n);
  put_fp(out96, out.x);
  put_fp(out96 + 48, out.y);
  *ident = id ? 1u : 0u;
  return code;
}
}
