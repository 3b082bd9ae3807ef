// Host build of the split retry's rule and of the host fold in front of it
// (lodestar_amd/csrc/sm_split.h): the same functions bgv_sm_split_plan and
// sm_back call, compiled with g++ for tests/test_sm_retry_host.py.
//
//   g++ -O2 -std=c++17 -shared -fPIC -o libhostcheck_sm_split.so hostcheck_sm_split.cpp
//   g++ -fsanitize=address,undefined -DHOSTCHECK_SM_SPLIT_MAIN ...   (the stand-alone program below)
#include <stddef.h>
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

// sm_collect (the host fold of the first pass's results, as sm_back calls it) over S
// segments, then the tally of the sub verdicts jr1[]: list / list_group / sub_off have room
// for every set (+ 1), counts[8] = pairs, groups_retried, segments, subs planned, then the
// four of sm_split_tally.  Returns the number of retried sets.
uint32_t hc_sm_collect(uint32_t S, const uint32_t* seg_off, const uint32_t* seg_group, const int32_t* jr, const int32_t* sc,
                       const uint32_t* sk, uint32_t split, uint8_t* set_valid, int32_t* set_code, const int32_t* jr1,
                       uint32_t* list, uint32_t* list_group, uint32_t* sub_off, uint32_t* counts) {
  const sm_retry_sets rs = sm_collect(S, seg_off, seg_group, jr, sc, sk, split != 0, set_valid, set_code);
  for (size_t i = 0; i < rs.list.size(); i++) { list[i] = rs.list[i]; list_group[i] = rs.list_group[i]; }
  for (size_t i = 0; i < rs.sub_off.size(); i++) sub_off[i] = rs.sub_off[i];
  const uint32_t T = (uint32_t)rs.sub_off.size() - 1;
  sm_split_counts c = {0, 0, 0, 0};
  if (split) sm_split_tally(c, rs.sub_off.data(), jr1, T);
  const uint32_t out[8] = {rs.pairs, rs.groups_retried, rs.segments, T, c.subs, c.subs_failed, c.leaves, c.pairs};
  for (int i = 0; i < 8; i++) counts[i] = out[i];
  return (uint32_t)rs.list.size();
}

}  // extern "C"

#ifdef HOSTCHECK_SM_SPLIT_MAIN
// Stand-alone (tests/test_sm_retry_host.py builds it with -fsanitize=address,undefined): two
// batches on heap arrays of exactly their size, so a load or store past one is a finding.
//   A  one group of 70 sets = two segments; the first is clean, the second is retried
//   B  one segment of 64 of which 61 sets were skipped: 3 survivors, fewer than one sub
// The subs must be those sm_split_plan gives, the counts those of sm_split_tally over them.
#include <stdio.h>
#include <vector>

static int check(const char* name, const std::vector<uint32_t>& seg_off, const std::vector<int32_t>& jr,
                 const std::vector<uint32_t>& sk, const std::vector<int32_t>& jr1, const std::vector<uint32_t>& want_list,
                 const uint32_t want[4]) {
  const uint32_t S = (uint32_t)jr.size(), n = seg_off[S];
  const std::vector<uint32_t> seg_group(S, 0);
  const std::vector<int32_t> sc(n, 0);
  std::vector<uint8_t> valid(n, 7);
  const sm_retry_sets rs = sm_collect(S, seg_off.data(), seg_group.data(), jr.data(), sc.data(), sk.data(), true, valid.data(), nullptr);
  std::vector<uint32_t> plan(want_list.size() + 1);
  const uint32_t T = sm_split_plan((uint32_t)want_list.size(), 0, plan.data(), (uint32_t)plan.size());
  plan.resize((size_t)T + 1);
  sm_split_counts c = {0, 0, 0, 0};
  if (rs.sub_off.size() == jr1.size() + 1) sm_split_tally(c, rs.sub_off.data(), jr1.data(), (uint32_t)jr1.size());
  const bool ok = rs.list == want_list && rs.list_group == std::vector<uint32_t>(want_list.size(), 0) && rs.sub_off == plan &&
                  rs.groups_retried == 1 && rs.segments == 1 && c.subs == want[0] && c.subs_failed == want[1] &&
                  c.leaves == want[2] && c.pairs == want[3];
  if (!ok) printf("hostcheck sm split: case %s differs\n", name);
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  {  // A: survivors 64 .. 69 (set 66 skipped): five subs of one, the third fails
    std::vector<uint32_t> sk(70, 0);
    sk[66] = 1;
    const uint32_t want[4] = {5, 1, 0, 10};
    bad += check("A", {0, 64, 70}, {1, 0}, sk, {1, 1, 0, 1, 1}, {64, 65, 67, 68, 69}, want);
  }
  {  // B: survivors 3, 30 and 63: three subs of one, two fail; no leaf
    std::vector<uint32_t> sk(64, 1);
    sk[3] = sk[30] = sk[63] = 0;
    const uint32_t want[4] = {3, 2, 0, 6};
    bad += check("B", {0, 64}, {0}, sk, {0, 1, 0}, {3, 30, 63}, want);
  }
  if (!bad) printf("hostcheck sm split OK 2\n");
  return bad;
}
#endif
