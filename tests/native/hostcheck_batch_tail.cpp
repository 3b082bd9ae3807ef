// Host check of the batch-first tail: a stand-alone
// program over the headers the kernels are built from (pairing.h for the
// recurrence, curve.h for the G2 sums, batch_tail.h for the shapes of the two
// trees), also built with -fsanitize=address,undefined.  It restates the
// launchers' level loops (launch_batch_chain / k_step_fold, launch_batch_sig /
// k_win_fold, k_msm_job's 16-lane Horner) on exactly sized buffers: a store
// past a region is a sanitizer finding.  TEST ONLY.
//
//   hostcheck_batch_tail G
//   * chain identity: the fold of the step values over all slices (fan-in
//     FOLD_FAN, a rejected job's slices read as 1, the grid sized by the item
//     bound) followed by ONE recurrence equals the product over the accepted
//     jobs of the per-job chain, as canonical residues.  1, 2, 8, 9 and 65
//     jobs of 1-3 sets, one job of G + 1 sets (two slices), one rejected job in
//     the middle, one empty job;
//   * S_batch: the window sums over the accepted jobs (fan-in WIN_FAN) and one
//     Horner equal sum_j S_job as affine points, with a rejected job, and for
//     S and -S in two jobs the identity;
//   * pair bilinearity: FE(miller(-G1, S_batch)) = FE(prod_j miller(-G1, S_j)).
// Prints "hostcheck batch_tail OK <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../lodestar_amd/csrc/pairing.h"
#include "../../lodestar_amd/csrc/batch_tail.h"

using namespace bgv;

static unsigned long checks = 0;
static void fail(const char* what, uint32_t a) {
  printf("FAIL %s (%u)\n", what, a);
  exit(1);
}

static bool canon_eq(const fp_t* x, const fp_t* y, int n) {
  for (int k = 0; k < n; k++) {
    fp_t u, v;
    fp_from_mont(u, x[k]);
    fp_from_mont(v, y[k]);
    if (memcmp(&u, &v, sizeof u) != 0) return false;
  }
  return true;
}
static bool canon_eq(const fp12_t& a, const fp12_t& b) { return canon_eq((const fp_t*)&a, (const fp_t*)&b, 12); }
static bool canon_eq(const g2a& a, const g2a& b) { return canon_eq((const fp_t*)&a, (const fp_t*)&b, 4); }

// ------------------------------------------------------------ chain identity
// launch_batch_chain: levels of k_step_fold over [items][68] step values, then k_batch_chain's recurrence
static void batch_chain(fp12_t& f, const std::vector<fp12_t>& f_step, uint32_t items, uint32_t bound,
                        const std::vector<uint32_t>& item_job, const std::vector<int32_t>& job_code) {
  std::vector<fp12_t> fold(tail_entries(bound, FOLD_FAN) * MILLER_STEPS);
  fp12_t* reg[2] = {fold.data(), fold.data() + tail_region1(bound, FOLD_FAN) * MILLER_STEPS};
  const fp12_t* src = f_step.data();
  uint32_t n = bound, lvl = 0;
  do {
    const uint32_t groups = tail_groups(n, FOLD_FAN);
    fp12_t* dst = reg[lvl & 1u];
    const bool level0 = lvl == 0;
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t k = 0; k < (uint32_t)MILLER_STEPS; k++) {
        const uint32_t live = level0 ? (n < items ? n : items) : n;
        const uint32_t beg = g * FOLD_FAN, end = live < beg + FOLD_FAN ? live : beg + FOLD_FAN;
        fp12_t acc;
        bool have = false;
        for (uint32_t t = beg; t < end; t++) {
          if (level0 && job_code[item_job[t]] != C_OK) continue;
          if (!have) acc = src[(size_t)t * MILLER_STEPS + k];
          else fp12_mul(acc, acc, src[(size_t)t * MILLER_STEPS + k]);
          have = true;
        }
        if (!have) fp12_one(acc);
        dst[(size_t)g * MILLER_STEPS + k] = acc;
      }
    src = dst;
    n = groups;
    lvl++;
  } while (n > 1);
  miller_chain(f, src);
}

static void check_chain(uint32_t J, uint32_t G, const fp12_t& seed) {
  // jobs of 1-3 sets; job 0 has G + 1 (two slices); the middle job is rejected, the last one empty
  std::vector<uint32_t> sizes(J);
  std::vector<int32_t> code(J, C_OK);
  for (uint32_t j = 0; j < J; j++) sizes[j] = 1 + j % 3;
  sizes[0] = G + 1;
  if (J >= 3) code[J / 2] = 1;
  if (J >= 2) sizes[J - 1] = 0;
  uint32_t n_sets = 0;
  std::vector<uint32_t> item_off(J + 1, 0), item_job;
  for (uint32_t j = 0; j < J; j++) {
    n_sets += sizes[j];
    item_off[j + 1] = item_off[j] + (sizes[j] ? miller_item_count(sizes[j], G) : 0u);
    for (uint32_t t = item_off[j]; t < item_off[j + 1]; t++) item_job.push_back(j);
    if (sizes[j] == 0) code[j] = 10;  // C_EMPTY_JOB
  }
  const uint32_t items = item_off[J], bound = n_sets / G + J;
  if (items > bound) fail("item bound", J);
  // step values: distinct, non-trivial field elements (the identity is one of field arithmetic); the buffer has
  // the bound's size, its tail past `items` never read
  std::vector<fp12_t> f_step((size_t)bound * MILLER_STEPS);
  fp12_t x = seed;
  for (size_t k = 0; k < (size_t)items * MILLER_STEPS; k++) {
    fp12_sqr(x, x);
    fp12_mul(x, x, seed);
    f_step[k] = x;
  }
  for (size_t k = (size_t)items * MILLER_STEPS; k < f_step.size(); k++) memset(&f_step[k], 0xA5, sizeof(fp12_t));
  fp12_t want;
  fp12_one(want);
  for (uint32_t j = 0; j < J; j++) {  // k_job_chain, one job at a time
    if (code[j] != C_OK || item_off[j + 1] == item_off[j]) continue;
    std::vector<fp12_t> L(MILLER_STEPS);
    for (uint32_t s = 0; s < (uint32_t)MILLER_STEPS; s++) {
      L[s] = f_step[(size_t)item_off[j] * MILLER_STEPS + s];
      for (uint32_t t = item_off[j] + 1; t < item_off[j + 1]; t++) fp12_mul(L[s], L[s], f_step[(size_t)t * MILLER_STEPS + s]);
    }
    fp12_t fj;
    miller_chain(fj, L.data());
    fp12_mul(want, want, fj);
  }
  fp12_t got;
  batch_chain(got, f_step, items, bound, item_job, code);
  if (!canon_eq(got, want)) fail("fold + one recurrence != product of the per-job chains", J);
  checks++;
}

// -------------------------------------------------------------------- S_batch
struct sig_job {
  std::vector<g2a> sig;
  std::vector<uint64_t> r;
  int32_t code;
};

static void window_sums(g2j* win16, const sig_job& job) {  // k_msm_bucket + k_msm_window: W_w = sum_i digit_w(r_i) sigma_i
  for (uint32_t w = 0; w < 16; w++) {
    jac_set_inf(win16[w]);
    for (size_t i = 0; i < job.sig.size(); i++) {
      const uint64_t d = (job.r[i] >> (4u * w)) & 15u;
      if (!d) continue;
      g2j s, t;
      jac_from_aff(s, job.sig[i]);
      jac_mul_u64(t, s, d);
      jac_add(win16[w], win16[w], t);
    }
  }
}

// k_msm_job's 16 lanes: lane w doubles its window sum 4 w times, then the shuffle tree
static void horner16(g2j& out, const g2j* win16) {
  g2j lane[16];
  for (uint32_t w = 0; w < 16; w++) {
    lane[w] = win16[w];
    for (uint32_t k = 0; k < 4u * w; k++) jac_dbl(lane[w], lane[w]);
  }
  for (uint32_t st = 8; st >= 1; st >>= 1)
    for (uint32_t w = 0; w < st; w++) jac_add(lane[w], lane[w], lane[w + st]);
  out = lane[0];
}

// launch_batch_sig: levels of k_win_fold over msm_win, then the Horner of one virtual job
static void batch_sum(g2j& out, const std::vector<g2j>& msm_win, const std::vector<sig_job>& jobs) {
  const uint32_t J = (uint32_t)jobs.size();
  std::vector<g2j> tmp(16 * tail_entries(J, WIN_FAN));
  g2j* reg[2] = {tmp.data(), tmp.data() + 16 * tail_region1(J, WIN_FAN)};
  const g2j* src = msm_win.data();
  uint32_t n = J, lvl = 0;
  do {
    const uint32_t groups = tail_groups(n, WIN_FAN);
    g2j* dst = reg[lvl & 1u];
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t w = 0; w < 16; w++) {
        const uint32_t end = n < WIN_FAN * g + WIN_FAN ? n : WIN_FAN * g + WIN_FAN;
        g2j acc;
        jac_set_inf(acc);
        for (uint32_t j = WIN_FAN * g; j < end; j++) {
          if (lvl == 0 && jobs[j].code != C_OK) continue;
          jac_add(acc, acc, src[16u * j + w]);
        }
        dst[16u * g + w] = acc;
      }
    src = dst;
    n = groups;
    lvl++;
  } while (n > 1);
  horner16(out, src);
}

static void check_sums(const std::vector<sig_job>& jobs, bool want_identity, bool pair) {
  const uint32_t J = (uint32_t)jobs.size();
  std::vector<g2j> msm_win(16 * (size_t)J);
  for (uint32_t j = 0; j < J; j++) window_sums(&msm_win[16 * (size_t)j], jobs[j]);
  g2j sum, sb;
  jac_set_inf(sum);
  std::vector<g2a> s_job(J);
  std::vector<bool> s_live(J, false);
  for (uint32_t j = 0; j < J; j++) {
    if (jobs[j].code != C_OK) continue;
    g2j sj;
    horner16(sj, &msm_win[16 * (size_t)j]);  // the per-job tail's S_job
    s_live[j] = jac_to_aff(s_job[j], sj);
    jac_add(sum, sum, sj);
  }
  batch_sum(sb, msm_win, jobs);
  g2a a, b;
  const bool la = jac_to_aff(a, sum), lb = jac_to_aff(b, sb);
  if (la != lb || la == want_identity) fail("S_batch: identity", J);
  if (la && !canon_eq(a, b)) fail("S_batch != sum of the S_job", J);
  checks++;
  if (!pair) return;
  g1a P;
  P.x = G1_X_MONT;
  P.y = G1_NEG_Y_MONT;
  fp12_t prod, one_pair, fe_a, fe_b;
  fp12_one(prod);
  for (uint32_t j = 0; j < J; j++) {
    if (jobs[j].code != C_OK) continue;
    fp12_t f;
    miller_loop(f, P, false, s_job[j], !s_live[j]);
    fp12_mul(prod, prod, f);
  }
  miller_loop(one_pair, P, false, b, !lb);
  fp12_final_exp(fe_a, prod);
  fp12_final_exp(fe_b, one_pair);
  if (!canon_eq(fe_a, fe_b)) fail("FE(miller(-G1, S_batch)) != FE(prod miller(-G1, S_j))", J);
  if (fp12_is_one(fe_b)) fail("pair value is trivial", J);
  checks++;
}

int main(int argc, char** argv) {
  const uint32_t G = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 4;
  if (G < 1 || G > 128) { printf("G out of range\n"); return 2; }
  uint8_t m[32];
  for (int i = 0; i < 32; i++) m[i] = (uint8_t)(i * 7 + 5);
  g2j h;
  hash_to_g2(h, m);
  std::vector<g2a> Q(12);
  for (auto& q : Q) {
    jac_to_aff(q, h);
    jac_dbl(h, h);
  }
  g1a P;
  P.x = G1_X_MONT;
  P.y = G1_Y_MONT;
  fp12_t seed;
  miller_loop(seed, P, false, Q[0], false);
  const uint32_t Js[] = {1, 2, 8, 9, 65};
  for (uint32_t J : Js) check_chain(J, G, seed);

  // six jobs (two levels of the window tree) of one or two sets, job 2 rejected
  std::vector<sig_job> jobs(6);
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  size_t q = 0;
  for (uint32_t j = 0; j < 6; j++) {
    jobs[j].code = j == 2 ? 3 : C_OK;
    for (uint32_t i = 0; i < 1 + j % 2; i++) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      jobs[j].sig.push_back(Q[q++ % Q.size()]);
      jobs[j].r.push_back(lcg | 1ull);
    }
  }
  check_sums(jobs, false, true);
  // S and -S under the same multiplier in two jobs: the identity, as s_inf reports it
  std::vector<sig_job> two(2);
  g2a neg = Q[3];
  fp2_neg(neg.y, neg.y);
  two[0] = {{Q[3]}, {0xF00DF00D12345679ull}, C_OK};
  two[1] = {{neg}, {0xF00DF00D12345679ull}, C_OK};
  check_sums(two, true, false);
  // one job alone, and every job rejected
  std::vector<sig_job> lone(1);
  lone[0] = {{Q[5]}, {0x8000000000000001ull}, C_OK};
  check_sums(lone, false, false);
  lone[0].code = 1;
  check_sums(lone, true, false);
  printf("hostcheck batch_tail OK %lu\n", checks);
  return 0;
}
