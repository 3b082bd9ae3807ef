// The split retry of the same-message entries (bgv_sm_retry mode 1, DESIGN.md
// section 3k): how a retried segment is cut into subs, and what the sub
// verdicts cost; and sm_collect, the host fold of the first pass's results that
// feeds it.  bgv_sm_split_plan, sm_back (bgv_api_sm.hip) and the host check
// (tests/native/hostcheck_sm_split.cpp) run the same code.
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
#include <vector>

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

// ---- the host fold between the first pass and a retry (host only) ------------
// A segment's verdict jr: 1 passed, 0 failed, < 0 minus its code.  A failed
// segment and one whose weighted key sum was the identity go to the retry.
constexpr int32_t SM_JR_IDENTITY = -11;  // -C_SEG_RETRY (bgv_internal.h; asserted in bgv_api_sm.hip)

struct sm_retry_sets {
  std::vector<uint32_t> list, list_group;  // the surviving sets of the retried segments, in set order, and their groups
  std::vector<uint32_t> sub_off;           // split: the subs, offsets into list; closed by list.size() either way
  uint32_t pairs = 0, groups_retried = 0, segments = 0;  // pairs of the first pass; groups / segments with a retry
};

// jr[S]: the segment verdicts; sc[n], sk[n]: the code and the skip flag of every
// set.  Writes the first-pass verdict of every set (set_code may be NULL).
inline sm_retry_sets sm_collect(uint32_t S, const uint32_t* seg_off, const uint32_t* seg_group, const int32_t* jr,
                                const int32_t* sc, const uint32_t* sk, bool split, uint8_t* set_valid, int32_t* set_code) {
  sm_retry_sets o;
  uint32_t last_group = 0xffffffffu;
  for (uint32_t s = 0; s < S; s++) {
    const bool ok = jr[s] == 1, retry = jr[s] == 0 || jr[s] == SM_JR_IDENTITY;
    if (jr[s] >= 0) o.pairs += 2;
    if (retry && seg_group[s] != last_group) { o.groups_retried++; last_group = seg_group[s]; }
    const uint32_t first = (uint32_t)o.list.size();
    for (uint32_t i = seg_off[s]; i < seg_off[s + 1]; i++) {
      set_valid[i] = (!sk[i] && ok) ? 1 : 0;
      if (set_code) set_code[i] = sc[i];
      if (retry && !sk[i]) { o.list.push_back(i); o.list_group.push_back(seg_group[s]); }
    }
    if (retry) o.segments++;
    if (retry && split) {  // the segment's subs; the next segment's first offset (or the closing one) ends the last
      const uint32_t m = (uint32_t)o.list.size() - first, T = sm_sub_count(m);
      for (uint32_t t = 0; t < T; t++) o.sub_off.push_back(first + sm_sub_begin(m, t));
    }
  }
  o.sub_off.push_back((uint32_t)o.list.size());
  return o;
}

}  // namespace bgv
