// Host build of the split retry's rule (lodestar_amd/csrc/sm_split.h): the
// same functions bgv_sm_split_plan and sm_back call, compiled with g++ for
// tests/test_sm_retry_host.py.
//
//   g++ -O2 -std=c++17 -shared -fPIC -o libhostcheck_sm_split.so hostcheck_sm_split.cpp
#include <stdint.h>

#include "../../lodestar_amd/csrc/sm_split.h"

using namespace bgv;

extern "C" {

uint32_t hc_sm_sub(void) { return SM_SUB; }
uint32_t hc_sm_sub_count(uint32_t m) { return sm_sub_count(m); }
uint32_t hc_sm_sub_begin(uint32_t m, uint32_t t) { return sm_sub_begin(m, t); }
uint32_t hc_sm_split_plan(uint32_t m, uint32_t base, uint32_t* sub_off, uint32_t cap) { return sm_split_plan(m, base, sub_off, cap); }

// the subs of n_segs retried segments with m[s] surviving sets each, planned one after the
// other as sm_back does (every segment's offsets start where the last one's ended; cap
// entries at sub_off), then the tally of the verdicts jr[]: out[4] = subs, subs_failed,
// leaves, pairs.  Returns the number of subs, or SM_PLAN_FAIL.
uint32_t hc_sm_retry_counts(const uint32_t* m, uint32_t n_segs, const int32_t* jr, uint32_t* sub_off, uint32_t cap, uint32_t* out) {
  uint32_t T = 0, base = 0;
  for (uint32_t s = 0; s < n_segs; s++) {
    if (T > cap) return SM_PLAN_FAIL;
    const uint32_t t = sm_split_plan(m[s], base, sub_off + T, cap - T);
    if (t == SM_PLAN_FAIL) return SM_PLAN_FAIL;
    T += t;
    base += m[s];
  }
  sm_split_counts c = {0, 0, 0, 0};
  sm_split_tally(c, sub_off, jr, T);
  out[0] = c.subs; out[1] = c.subs_failed; out[2] = c.leaves; out[3] = c.pairs;
  return T;
}

}  // extern "C"
