// Host-compiled view of the unweighted signature sums of
// bgv_verify_same_message_aggregate (lodestar_amd/csrc/sig_agg.h) for CPU tests
// against the Python oracle.  TEST ONLY: the product runs these pieces in the
// kernels of bgv_sig_agg.hip.  I/O convention of hostcheck.cpp: affine G2 =
// x.c0 || x.c1 || y.c0 || y.c1, 48-byte big-endian plain integers.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../lodestar_amd/csrc/sig_agg.h"

using namespace bgv;

static void get_fp(fp_t& r, const uint8_t* b) { fp_t t; fp_from_be48(t, b); fp_to_mont(r, t); }
static void put_fp(uint8_t* b, const fp_t& a) { fp_t t; fp_from_mont(t, a); fp_to_be48(b, t); }

extern "C" {

uint32_t hc_sag_seg_max(void) { return SM_SEG; }
uint32_t hc_sag_lanes(void) { return SIG_AGG_LANES; }

// One group of n sets, cut into segments of at most SM_SEG as the library cuts
// it: every segment by its sixteen sub-lane walks and the tree, then the group
// fold with prev96 (may be NULL), compressed.  skip / take / valid: the
// predicate's inputs (take, valid may be NULL).  seg0_192 (may be NULL): the
// first segment's sum, affine, all-zero for the identity.  Returns the segments.
uint32_t hc_sag_group(const uint8_t* sigs192, uint32_t n, const uint32_t* skip, const uint8_t* take, const uint8_t* valid,
                      const uint8_t* prev96, uint8_t* out96, uint32_t* cnt, int32_t* code, uint8_t* seg0_192) {
  std::vector<g2a> sig(n ? n : 1);
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* b = sigs192 + 192 * (size_t)i;
    get_fp(sig[i].x.c0, b); get_fp(sig[i].x.c1, b + 48); get_fp(sig[i].y.c0, b + 96); get_fp(sig[i].y.c1, b + 144);
  }
  std::vector<uint32_t> seg_off;
  for (uint32_t i = 0; i < n; i += SM_SEG) seg_off.push_back(i);
  const uint32_t S = (uint32_t)seg_off.size();
  seg_off.push_back(n);
  const uint32_t group_seg[2] = {0, S};
  std::vector<g2j> seg_sum(S ? S : 1);
  std::vector<uint32_t> seg_cnt(S ? S : 1);
  sig_agg_view v;
  v.n_segs = S; v.n_groups = 1; v.seg_off = seg_off.data(); v.group_seg = group_seg;
  v.sig_aff = sig.data(); v.skip = skip; v.take = take; v.valid = valid; v.prev = prev96;
  v.seg_sum = seg_sum.data(); v.seg_cnt = seg_cnt.data(); v.out96 = out96; v.out_cnt = cnt; v.out_code = code;
  for (uint32_t s = 0; s < S; s++) sig_agg_segment(v, s);
  if (seg0_192) {
    g2a a;
    if (S) jac_to_aff(a, seg_sum[0]);
    else { a.x = fp2_zero(); a.y = fp2_zero(); }
    put_fp(seg0_192, a.x.c0); put_fp(seg0_192 + 48, a.x.c1); put_fp(seg0_192 + 96, a.y.c0); put_fp(seg0_192 + 144, a.y.c1);
  }
  sig_agg_group(v, 0);
  return S;
}
}
