// The split retry of the same-message entries (bgv_sm_retry mode 1, DESIGN.md
// section 3k): how a retried segment is cut into subs, and what the sub
// verdicts cost.  BGV_HD throughout: bgv_sm_split_plan, sm_back (bgv_api.hip)
// and the host check (tests/native/hostcheck_sm_split.cpp) run the same code.
//
// A retried segment has m surviving sets, taken in set order:
//   m <= SM_SUB  m subs of one set each (a sub verdict is then the set's own:
//                the scaled check is the unscaled one raised to r_i != 0)
//   m >  SM_SUB  ceil(m / SM_SUB) subs of SM_SUB sets, the last one shorter
// Level 1 checks every sub like a short segment.  A passing sub makes its sets
// valid, a failing sub of one set makes it invalid, and the sets of a failing
// sub of two or more become leaves, each checked alone at level 2.
#pragma once
#include <stdint.h>

#include "bls_types.h"

namespace bgv {

// sets per sub.  For a segment of 64 with one bad set subs of c cost 64 / c + c
// checks: c = 8 is the minimum
constexpr uint32_t SM_SUB = 8;
constexpr uint32_t SM_PLAN_FAIL = 0xffffffffu;

BGV_HD uint32_t sm_sub_size(uint32_t m) { return m <= SM_SUB ? 1u : SM_SUB; }
BGV_HD uint32_t sm_sub_count(uint32_t m) { return m <= SM_SUB ? m : m / SM_SUB + ((m % SM_SUB) ? 1u : 0u); }
// first surviving set of sub t; t == sm_sub_count(m) gives m
BGV_HD uint32_t sm_sub_begin(uint32_t m, uint32_t t) {
  const uint64_t b = (uint64_t)t * sm_sub_size(m);
  return b < m ? (uint32_t)b : m;
}

// the sub offsets of one segment, count + 1 of them (the last one is m), each
// plus `base`; returns the count, or SM_PLAN_FAIL with nothing written when
// they do not fit cap entries
BGV_HD uint32_t sm_split_plan(uint32_t m, uint32_t base, uint32_t* sub_off, uint32_t cap) {
  const uint32_t T = sm_sub_count(m);
  if (!sub_off || cap <= T) return SM_PLAN_FAIL;
  for (uint32_t t = 0; t <= T; t++) sub_off[t] = base + sm_sub_begin(m, t);
  return T;
}

// what the verdicts of T subs lead to (jr[t]: 1 passed, 0 failed, < 0 P_sub was
// the identity and its pair was skipped): the counters of bgv_sm_retry_path
struct sm_split_counts {
  uint32_t subs, subs_failed, leaves, pairs;
};
BGV_HD bool sm_sub_failed(int32_t jr) { return jr != 1; }
// a failing sub of two or more sets is opened
BGV_HD bool sm_sub_opens(int32_t jr, uint32_t size) { return sm_sub_failed(jr) && size >= 2u; }
BGV_HD void sm_split_tally(sm_split_counts& c, const uint32_t* sub_off, const int32_t* jr, uint32_t T) {
  for (uint32_t t = 0; t < T; t++) {
    const uint32_t size = sub_off[t + 1] - sub_off[t];
    c.subs++;
    if (jr[t] >= 0) c.pairs += 2u;
    if (sm_sub_failed(jr[t])) c.subs_failed++;
    if (sm_sub_opens(jr[t], size)) {
      c.leaves += size;
      c.pairs += 2u * size;
    }
  }
}

}  // namespace bgv
