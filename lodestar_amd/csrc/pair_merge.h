// One Miller pair per distinct signing root of a job (bgv_pair_merge).
//
// A job's verdict is the AND of its sets and only the job's product is ever
// read (whole-batch check, per-job retry, bgv_partial), so the sets of a job
// that sign the same root m pair once:
//   prod_i e(r_i PK_i, H(m)) = e(sum_i r_i PK_i, H(m))
// The class C(j, m) is the sets of job j with root m; classes never span jobs.
// Everything here is index work plus one G1 sum per class:
//   pm_slot_mix   slot of the key (job, root representative) in the keyed
//                 open-addressing table that elects a leader per class
//   pm_job_of     the job of a set, from the job offsets (empty jobs allowed)
//   pm_class_sum  P_c = sum of the members' scaled keys, walking the class's
//                 member list; affine, with a class code and the identity flag
// BGV_HD throughout: tests/native/hostcheck_pair_merge.cpp runs the same code
// on the host against the oracle; the kernels are in bgv_pair_merge.hip.
#pragma once
#include "curve.h"

namespace bgv {

constexpr uint64_t PM_EMPTY = ~0ull;        // a free slot of the class table (hipMemsetAsync 0xff)
constexpr uint32_t PM_NONE = 0xffffffffu;   // end of a member list / an empty list head
constexpr uint32_t PM_LEAD = 0x80000000u;   // pair_classes.slot: the set claimed the slot (it leads its class)

// What the class pass leaves in HBM (device pointers).  Kept out of dev_batch /
// dev_work like msg_classes: those are kernel arguments of every other kernel.
struct pair_classes {
  uint32_t n_sets, n_jobs;
  uint32_t mask;             // slots of the table - 1; a power of two >= 2 n_sets slots
  uint32_t per;              // sets per Miller work item (pairs_per_item, or steps_slice)
  uint64_t key;              // per-call key of the slot mix
  const uint32_t* job_off;   // [n_jobs + 1] the batch's job offsets
  const uint32_t* rep;       // [n_sets] root representative of every set (msg_classes.rep)
  uint64_t* table;           // [mask + 1] PM_EMPTY, or (job << 32 | rep) of the class that owns the slot
  uint32_t* slot;            // [n_sets] slot of the set's class (| PM_LEAD for the leader)
  uint32_t* slot_idx;        // [mask + 1] index of the slot's class inside its job
  uint32_t* class_off;       // [n_jobs + 1] leaders per job, then their scan: the view's job_off
  uint32_t* cls;             // [n_sets] class of every set
  uint32_t* head;            // [n_sets] per class: its last linked member (PM_NONE past the class count)
  uint32_t* next;            // [n_sets] per set: the next member of its class, or PM_NONE
  uint32_t* cls_job;         // [n_sets] per class: its job (0 past the class count): the view's set_job
  uint32_t* cls_rep;         // [n_sets] per class: the set whose h_aff row holds H(m)
  uint32_t* item_off;        // [n_jobs + 1] the view's Miller work items
  uint32_t* item_job;
  g1a* p_cls;                // [n_sets] per class: P_c affine: the view's rpk_aff
  int32_t* code_cls;         // [n_sets] per class: C_OK or a member's key code: the view's pk_code
  g2a* h_cls;                // [n_sets] per class: H(m): the view's h_aff
  uint32_t* ident;           // one word: a class summed to the identity (the call runs again unmerged)
};

// 64-bit mix of (job, representative) under the per-call key: peers choose the
// roots and so, through k_msg_dedup, which sets represent them
BGV_HD uint64_t pm_slot_mix(uint32_t job, uint32_t rep, uint64_t key) {
  uint64_t h = key ^ (((uint64_t)job << 32) | rep);
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 29;
  return h;
}

// the job j with job_off[j] <= i < job_off[j + 1] (i < job_off[n_jobs]); empty
// jobs repeat an offset and are stepped over
BGV_HD uint32_t pm_job_of(const uint32_t* job_off, uint32_t n_jobs, uint32_t i) {
  uint32_t lo = 0, hi = n_jobs;  // job_off[lo] <= i < job_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (job_off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

BGV_HD bool pm_aff_is_zero(const g1a& p) { return fp_is_zero(p.x) && fp_is_zero(p.y); }

// P_c of the class whose member list starts at `first` (next[] links, PM_NONE
// ends it; at most n_sets members are walked whatever next[] holds).  Members
// are added with curve.h's complete additions: two members with the same key
// and scalar double, a key beside its negation cancels.  A member stored as
// (0, 0) is the identity and adds nothing.  A lone member is copied.
//   code   C_OK, or the largest key code among the members (their job is
//          rejected by the per-set codes; the class only has to stay inert)
//   ident  every member was accepted and the sum is the identity: the pair's
//          value is 1, which the item loop cannot tell from a rejected pair,
//          so the caller falls back to one pair per set
// The affine result does not depend on the order of the list.
BGV_HD void pm_class_sum(g1a& out, int32_t& code, bool& ident, const g1a* rpk, const int32_t* pk_code, const uint32_t* next,
                         uint32_t first, uint32_t n_sets) {
  g1j acc;
  jac_set_inf(acc);
  code = C_OK;
  ident = false;
  uint32_t members = 0, i = first;
  for (uint32_t steps = 0; i < n_sets && steps < n_sets; steps++) {
    const int32_t ci = pk_code[i];
    if (ci != C_OK) {
      if (ci > code) code = ci;
    } else {
      const g1a p = rpk[i];
      if (!pm_aff_is_zero(p)) jac_add_aff(acc, acc, p);
    }
    members++;
    i = next[i];
  }
  fp_set_zero(out.x);
  fp_set_zero(out.y);
  if (code != C_OK) return;
  if (members == 0) {  // no such class: inert
    code = C_PK_IS_INFINITY;
    return;
  }
  if (members == 1) {
    out = rpk[first];
    if (!pm_aff_is_zero(out)) return;
  } else if (jac_to_aff(out, acc)) {
    return;
  }
  fp_set_zero(out.x);
  fp_set_zero(out.y);
  code = C_PK_IS_INFINITY;
  ident = true;
}

}  // namespace bgv
