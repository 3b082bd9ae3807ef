// Host check of the per-step line products (lodestar_amd/csrc/pairing.h
// miller_step_lines, miller_chain, miller_item_count, miller_item_sets): a
// stand-alone program over the same header the kernels k_miller_steps and
// k_job_chain are built from, also built with -fsanitize=address,undefined.
// TEST ONLY.
//
//   hostcheck_steps G [G ...]
// For every slice size G and the job sizes 1, 2, 3, G-1, G, G+1, 2G+1:
//   * the step products (one per slice and step, joined per step) followed by
//     the chain equal the product of the job's miller_loop_lines two-pair
//     items, compared as canonical residues;
//   * a job whose middle set has a rejected pubkey: the slices multiply that
//     set's lines as 1 (the product over the other sets), and the rule of
//     bgv_debug_stages gives 1 at the job's first set;
//   * the slicing arithmetic gives the item counts and offsets of a ragged
//     batch with an empty job.
// Prints "hostcheck steps OK <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../lodestar_amd/csrc/pairing.h"

using namespace bgv;

static unsigned long checks = 0;
static void fail(const char* what, uint32_t G, uint32_t n) {
  printf("FAIL %s (G = %u, job of %u sets)\n", what, G, n);
  exit(1);
}

// equality of the canonical residues of every Fp coefficient
static bool canon_eq(const fp12_t& a, const fp12_t& b) {
  const fp_t* x = (const fp_t*)&a;
  const fp_t* y = (const fp_t*)&b;
  for (int k = 0; k < 12; k++) {
    fp_t u, v;
    fp_from_mont(u, x[k]);
    fp_from_mont(v, y[k]);
    if (memcmp(&u, &v, sizeof u) != 0) return false;
  }
  return true;
}

// the job's value on the steps path: slices of G sets, one product per (slice,
// step) as k_miller_steps writes them (f_step[item][step], allocated exactly:
// a store past the slice count is a sanitizer finding), then k_job_chain's
// join per step and recurrence
static void steps_value(fp12_t& f, const std::vector<fp2_t>& lines, uint32_t n, const std::vector<g1a>& P,
                        const std::vector<int32_t>& pk_code, uint32_t G) {
  const uint32_t items = miller_item_count(n, G);
  std::vector<fp12_t> f_step((size_t)items * MILLER_STEPS);
  for (uint32_t t = 0; t < items; t++) {
    uint32_t i0, cnt;
    miller_item_sets(i0, cnt, 0, n, t, G);
    for (uint32_t s = 0; s < (uint32_t)MILLER_STEPS; s++)
      miller_step_lines(f_step[(size_t)t * MILLER_STEPS + s], lines.data(), n, P.data(), pk_code.data(), i0, cnt, s,
                        miller_step_is_add(s));
  }
  std::vector<fp12_t> L(MILLER_STEPS);
  for (uint32_t s = 0; s < (uint32_t)MILLER_STEPS; s++) {
    L[s] = f_step[s];
    for (uint32_t t = 1; t < items; t++) fp12_mul(L[s], L[s], f_step[(size_t)t * MILLER_STEPS + s]);
  }
  miller_chain(f, L.data());
}

// the product of the two-pair items over the sets with live[i]
static void items_value(fp12_t& f, const std::vector<fp2_t>& lines, uint32_t n, const std::vector<g1a>& P,
                        const std::vector<int32_t>& pk_code) {
  std::vector<uint32_t> idx;
  for (uint32_t i = 0; i < n; i++)
    if (pk_code[i] == C_OK) idx.push_back(i);
  fp12_one(f);
  for (size_t k = 0; k < idx.size(); k += 2) {
    const bool two = k + 1 < idx.size();
    const uint32_t i1 = idx[k], i2 = two ? idx[k + 1] : idx[k];
    fp12_t v;
    miller_loop_lines(v, lines.data(), n, P[i1], i1, P[i2], i2, two);
    fp12_mul(f, f, v);
  }
}

static void check_slicing(uint32_t G) {
  // a ragged batch with an empty job in the middle and at the end
  const uint32_t sizes[] = {1, 2, 0, 3, G - 1 ? G - 1 : 1, G, G + 1, 2 * G + 1, 98, 0};
  const uint32_t J = sizeof sizes / sizeof sizes[0];
  std::vector<uint32_t> job_off(J + 1, 0), item_off(J + 1, 0);
  for (uint32_t j = 0; j < J; j++) job_off[j + 1] = job_off[j] + sizes[j];
  for (uint32_t j = 0; j < J; j++) item_off[j + 1] = item_off[j] + miller_item_count(sizes[j], G);
  const uint32_t n = job_off[J];
  if (item_off[J] > n / G + J) fail("item bound", G, n);
  std::vector<uint32_t> seen(n, 0);
  for (uint32_t j = 0; j < J; j++) {
    const uint32_t want = sizes[j] ? (sizes[j] - 1) / G + 1 : 0;
    if (item_off[j + 1] - item_off[j] != want) fail("item count", G, sizes[j]);
    uint32_t next = job_off[j];
    for (uint32_t k = 0; k < want; k++) {
      uint32_t i0, cnt;
      miller_item_sets(i0, cnt, job_off[j], job_off[j + 1], k, G);
      if (i0 != next || cnt < 1 || cnt > G || i0 + cnt > job_off[j + 1]) fail("slice", G, sizes[j]);
      if (k + 1 < want && cnt != G) fail("inner slice not full", G, sizes[j]);
      for (uint32_t i = i0; i < i0 + cnt; i++) seen[i]++;
      next = i0 + cnt;
      checks++;
    }
    if (next != job_off[j + 1]) fail("slices do not cover the job", G, sizes[j]);
  }
  for (uint32_t i = 0; i < n; i++)
    if (seen[i] != 1) fail("set not in exactly one slice", G, i);
  // the step kinds: 63 doublings and 5 additions, in the loop's order
  uint32_t adds = 0, s = 0;
  for (int b = 62; b >= 0; b--) {
    if (miller_step_is_add(s++)) fail("doubling step reported as addition", G, s);
    if ((BLS_X_ABS >> b) & 1ull) {
      if (!miller_step_is_add(s++)) fail("addition step reported as doubling", G, s);
      adds++;
    }
  }
  if (s != (uint32_t)MILLER_STEPS || adds != 5) fail("step count", G, s);
  checks++;
}

int main(int argc, char** argv) {
  std::vector<uint32_t> Gs;
  for (int k = 1; k < argc; k++) Gs.push_back((uint32_t)strtoul(argv[k], nullptr, 10));
  if (Gs.empty()) Gs.push_back(4);
  uint32_t max_n = 0;
  for (uint32_t G : Gs) {
    if (G < 1 || G > 128) { printf("G out of range\n"); return 2; }
    if (2 * G + 1 > max_n) max_n = 2 * G + 1;
  }
  // distinct Q: H(m) doubled along; distinct P: multiples of the generator
  uint8_t m[32];
  for (int i = 0; i < 32; i++) m[i] = (uint8_t)(i * 11 + 3);
  g2j h;
  hash_to_g2(h, m);
  std::vector<g2a> Q(max_n);
  for (uint32_t i = 0; i < max_n; i++) {
    jac_to_aff(Q[i], h);
    jac_dbl(h, h);
  }
  std::vector<g1a> Pall(max_n);
  {
    g1j g, acc;
    g.x = G1_X_MONT;
    g.y = G1_Y_MONT;
    fe_one(g.z);
    acc = g;
    for (uint32_t i = 0; i < max_n; i++) {
      jac_dbl(acc, acc);
      jac_add(acc, acc, g);
      jac_to_aff(Pall[i], acc);
    }
  }
  for (uint32_t G : Gs) {
    check_slicing(G);
    const uint32_t sizes[] = {1, 2, 3, G - 1, G, G + 1, 2 * G + 1};
    for (uint32_t n : sizes) {
      if (n == 0) continue;  // G = 1: no job of G - 1 sets
      // the lines in the layout k_lines writes, stride n (exactly n sets allocated)
      std::vector<fp2_t> lines((size_t)3 * MILLER_STEPS * n);
      for (uint32_t i = 0; i < n; i++) miller_lines(lines.data(), n, i, Q[i]);
      std::vector<g1a> P(Pall.begin(), Pall.begin() + n);
      std::vector<int32_t> ok(n, C_OK);
      fp12_t want, got;
      items_value(want, lines, n, P, ok);
      steps_value(got, lines, n, P, ok, G);
      if (!canon_eq(got, want)) fail("steps + chain != product of the two-pair items", G, n);
      checks++;
      // a rejected pubkey in the middle set: the slices take its lines as 1 ...
      std::vector<int32_t> bad = ok;
      bad[n / 2] = 6;  // BLST_PK_IS_INFINITY
      items_value(want, lines, n, P, bad);
      steps_value(got, lines, n, P, bad, G);
      if (!canon_eq(got, want)) fail("rejected middle set is not left out", G, n);
      // (a job of one rejected set: every step product is 1, and so is the chain)
      if (n == 1 && !fp12_is_one(got)) fail("a job of one rejected set is not 1", G, n);
      // ... and the debug rule reports 1 at the job's first set (k_job_chain:
      // the chain is skipped when a pubkey of the job was rejected)
      // through the header's scan, whole (one share) and in the kernel's 128 strided shares
      bool any_bad = false, none_ok = false;
      for (uint32_t th = 0; th < 128; th++) {
        any_bad |= miller_job_rejected_pk(bad.data(), 0, n, th, 128);
        none_ok |= miller_job_rejected_pk(ok.data(), 0, n, th, 128);
      }
      if (!any_bad || !miller_job_rejected_pk(bad.data(), 0, n, 0, 1) || none_ok || miller_job_rejected_pk(ok.data(), 0, n, 0, 1))
        fail("rejected-pubkey scan", G, n);
      fp12_t first;
      if (any_bad) fp12_one(first);
      else first = got;
      if (!fp12_is_one(first)) fail("rejected job does not give 1 at its first set", G, n);
      checks += 2;
    }
  }
  printf("hostcheck steps OK %lu\n", checks);
  return 0;
}
