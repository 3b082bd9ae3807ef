// Fp12 tail of the batch verifier: the product trees (ST_F_TREE,
// ST_BATCH_PROD), the final exponentiations (ST_BATCH_FINAL, ST_JOB_FINAL)
// and the multi-GPU combination.
//
// A separate translation unit because it wants the opposite code generation
// to bgv_kernels.hip: these kernels are latency-bound (log2 levels, few lanes
// per level after the first, one wave for the final exponentiation) and run
// fastest with the Fp product inlined into the non-inlined Fp2 routines
// (BGV_FPMUL_CALL=0): k_f_level x7 + k_job_f take 3.2 ms at C4 this way
// against 5.1 ms with the register-ABI leaf.
#ifndef BGV_FPMUL_CALL
#define BGV_FPMUL_CALL 0
#endif
#include "bgv_internal.h"
#include "fp12_coop.h"

namespace bgv {

#ifndef BGV_TREE_WAVES
#define BGV_TREE_WAVES 2
#endif
#define BGV_TREE_LB __launch_bounds__(64, BGV_TREE_WAVES)

__device__ __forceinline__ static uint32_t tree_gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }
#define gtid tree_gtid

// per-job product of the Miller values: segmented pairwise tree over the
// job's sets (level s multiplies f[i] by f[i + s] for i = beg + 2s k), then
// k_job_f folds the span-strided survivors and the job's (-G1, S_job) value
__global__ void BGV_TREE_LB k_f_level(dev_batch b, dev_work w, uint32_t s) {
  const uint32_t i = gtid();
  if (i >= b.n_sets) return;
  const uint32_t j = w.set_job[i];
  const uint32_t beg = b.job_off[j], end = b.job_off[j + 1];
  if (((i - beg) % (2 * s)) != 0 || i + s >= end) return;
  fp12_t a = w.f_set[i];
  fp12_mul(a, a, w.f_set[i + s]);
  w.f_set[i] = a;
}

__global__ void BGV_TREE_LB k_job_f(dev_batch b, dev_work w, uint32_t span) {
  const uint32_t j = gtid();
  if (j >= b.n_jobs) return;
  const uint32_t beg = b.job_off[j], end = b.job_off[j + 1];
  fp12_t f;
  if (w.job_code[j] != C_OK) {
    fp12_one(f);  // rejected jobs take no part in the batch product
  } else {
    f = w.f_set[beg];
    for (uint32_t i = beg + span; i < end; i += span) fp12_mul(f, f, w.f_set[i]);
    fp12_mul(f, f, w.f_set[b.n_sets + j]);
  }
  w.f_job[j] = f;
  w.f_batch[j] = f;
}

// ------------------------------------------- cooperative folds (fp12_coop.h)
#define COOP_LB __launch_bounds__(COOP_THREADS, 2)

// With P pairs per Miller item the item's value sits at offsets P t of the job
// and every other entry is 1 (k_miller, k_miller_kv), so the folds step over
// the items only: at C4 that cuts the per-job chain from 98 to 49 (P = 2) or
// 25 (P = 4) Fp12 products.
__device__ __forceinline__ static uint32_t fold_step(const dev_batch& b) { return b.pairs_per_item ? b.pairs_per_item : 1u; }

// first level of the two-level fold (few large jobs, e.g. one 64-set gossip
// batch, and the C4 segment's 98-set blocks): workgroup (g, j) folds the job's
// values in [beg + G g, beg + G g + G) into f_set[beg + G g] (in place: all
// reads precede the one write, and the groups are disjoint); k_job_fold then
// walks the job with stride G
__global__ void COOP_LB k_job_prefold(dev_batch b, dev_work w) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  const uint32_t j = blockIdx.y, G = 1u << b.prefold_log2;
  const uint32_t beg = b.job_off[j], end = b.job_off[j + 1];
  const uint32_t g0 = beg + blockIdx.x * G;
  if (w.job_code[j] != C_OK || g0 + 1 >= end) return;  // uniform per workgroup
  const uint32_t g1 = min(end, g0 + G);
  c_load(&acc, w.f_set[g0]);
  for (uint32_t i = g0 + fold_step(b); i < g1; i += fold_step(b)) {
    c_load(&x, w.f_set[i]);
    c_mul(&acc, &acc, &x, &s);
  }
  c_store(w.f_set[g0], &acc);
}

// one workgroup per job: f_job = (job pair value) * prod of the job's set
// values (or of its group values after k_job_prefold, stride > 1), folded in
// order at the latency of one Fp product per step
__global__ void COOP_LB k_job_fold(dev_batch b, dev_work w, uint32_t stride) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  const uint32_t j = blockIdx.x;
  const uint32_t beg = b.job_off[j], end = b.job_off[j + 1];
  if (w.job_code[j] != C_OK) {
    c_set_one(&acc);  // rejected jobs take no part in the batch product
  } else {
    c_load(&acc, w.f_set[b.n_sets + j]);
    for (uint32_t i = beg; i < end; i += stride) {
      c_load(&x, w.f_set[i]);
      c_mul(&acc, &acc, &x, &s);
    }
  }
  c_store(w.f_job[j], &acc);
  c_store(w.f_batch[j], &acc);
}

// The steps path (dev_batch.steps_slice, pairing.h): one workgroup per job
// runs the job's Miller recurrence ONCE over the per-step line products that
// k_miller_steps left in f_step: L_k = the product of the job's slice values
// at step k, f <- f^2 L_k on doubling steps, f <- f L_k on addition steps,
// the conjugation (x < 0), then the job's (-G1, S_job) value.  It stands in
// for k_job_prefold / k_job_fold; rejected jobs give 1 as there.
// steps_dbg (bgv_debug_stages): the set product goes to f_set[first set] and 1
// to the job's other sets, 1 to all of them when a pubkey of the job was
// rejected: the item rule of k_miller with the job as the item.
// skip (the batch-first tail's retry launch): non-null and *skip != 0, the
// batch verified and nobody reads f_job: every workgroup returns at once.
__global__ void COOP_LB k_job_chain(dev_batch b, dev_work w, const uint32_t* skip) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x, y;
  __shared__ uint32_t bad_pk;
  if (skip && *skip) return;  // uniform over the grid
  const uint32_t j = blockIdx.x;
  const uint32_t beg = b.job_off[j], end = b.job_off[j + 1];
  const uint32_t t0 = w.item_off[j], t1 = w.item_off[j + 1];
  const bool rejected = w.job_code[j] != C_OK;
  bool run = !rejected && t1 > t0;  // uniform per workgroup, as everything below
  if (b.steps_dbg) {
    if (threadIdx.x == 0) bad_pk = 0u;
    __syncthreads();
    if (miller_job_rejected_pk(w.pk_code, beg, end, threadIdx.x, COOP_THREADS)) bad_pk = 1u;
    __syncthreads();
    run = t1 > t0 && !bad_pk;
  }
  if (!run) {
    c_set_one(&acc);
  } else {
    uint32_t k = 0;
    for (int bit = 62; bit >= 0; bit--) {
      const int sub = ((BLS_X_ABS >> bit) & 1ull) ? 2 : 1;
      for (int a = 0; a < sub; a++, k++) {
        c_load(&x, w.f_step[(size_t)t0 * MILLER_STEPS + k]);
        for (uint32_t t = t0 + 1; t < t1; t++) {
          c_load(&y, w.f_step[(size_t)t * MILLER_STEPS + k]);
          c_mul(&x, &x, &y, &s);
        }
        if (k == 0) {
          c_copy(&acc, &x);
        } else {
          if (a == 0) c_mul(&acc, &acc, &acc, &s);
          c_mul(&acc, &acc, &x, &s);
        }
      }
    }
    c_conj(&acc, &acc);
  }
  if (b.steps_dbg && end > beg) {
    c_store(w.f_set[beg], &acc);
    c_set_one(&y);
    for (uint32_t i = beg + 1; i < end; i++) c_store(w.f_set[i], &y);
  }
  if (rejected) {
    c_set_one(&acc);  // rejected jobs take no part in the batch product
  } else {
    c_load(&x, w.f_set[b.n_sets + j]);
    c_mul(&acc, &acc, &x, &s);
  }
  c_store(w.f_job[j], &acc);
  c_store(w.f_batch[j], &acc);
}

// workgroup g: dst[g] = prod src[F g .. min(n, F g + F)) with fan-in F; with
// one workgroup dst may alias src (every read precedes the write).  A
// fan-in of 8 (FOLD_FAN, batch_tail.h) keeps the chain of sequential Fp12
// products short: 1,024 job values fold in 8 + 8 + 8 + 8 + 2 products instead
// of 32 + 32.
__global__ void COOP_LB k_fold(const fp12_t* src, uint32_t n, fp12_t* dst) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  const uint32_t beg = blockIdx.x * FOLD_FAN, end = min(n, beg + FOLD_FAN);
  c_load(&acc, src[beg]);
  for (uint32_t i = beg + 1; i < end; i++) {
    c_load(&x, src[i]);
    c_mul(&acc, &acc, &x, &s);
  }
  c_store(dst[blockIdx.x], &acc);
}

// The batch-first tail (dev_batch.batch_tail): the recurrence f <- f^2 L_k is
// multiplicative in the L_k, so ONE recurrence over L_k = the product of ALL
// slices' step values equals the product of the per-job chains, as field
// elements.  k_step_fold folds f_step over the slices with fan-in FOLD_FAN,
// one workgroup per (group, step); level 0 reads 1 for a slice past the last
// one (the grid is sized by the host's bound) and for a slice of a rejected
// job.  k_batch_chain then runs the 68 steps once, conjugates, multiplies by
// the (-G1, S_batch) value and leaves the batch product in f_batch[0].
__global__ void COOP_LB k_step_fold(dev_batch b, dev_work w, const fp12_t* src, uint32_t n, fp12_t* dst, uint32_t level0) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  const uint32_t g = blockIdx.x, k = blockIdx.y;
  const uint32_t live = level0 ? min(n, w.item_off[b.n_jobs]) : n;
  const uint32_t beg = g * FOLD_FAN, end = min(live, beg + FOLD_FAN);
  bool have = false;  // uniform per workgroup, as everything here
  for (uint32_t t = beg; t < end; t++) {
    if (level0 && w.job_code[w.item_job[t]] != C_OK) continue;
    if (!have) {
      c_load(&acc, src[(size_t)t * MILLER_STEPS + k]);
      have = true;
    } else {
      c_load(&x, src[(size_t)t * MILLER_STEPS + k]);
      c_mul(&acc, &acc, &x, &s);
    }
  }
  if (!have) c_set_one(&acc);
  c_store(dst[(size_t)g * MILLER_STEPS + k], &acc);
}

__global__ void COOP_LB k_batch_chain(dev_batch b, dev_work w, const fp12_t* steps) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  uint32_t k = 0;
  for (int bit = 62; bit >= 0; bit--) {
    const int sub = ((BLS_X_ABS >> bit) & 1ull) ? 2 : 1;
    for (int a = 0; a < sub; a++, k++) {
      c_load(&x, steps[k]);
      if (k == 0) {
        c_copy(&acc, &x);
      } else {
        if (a == 0) c_mul(&acc, &acc, &acc, &s);
        c_mul(&acc, &acc, &x, &s);
      }
    }
  }
  c_conj(&acc, &acc);
  c_load(&x, w.f_set[b.n_sets + b.n_jobs]);
  c_mul(&acc, &acc, &x, &s);
  c_store(w.f_batch[0], &acc);
}

// the whole-batch check: ONE final exponentiation over 128 lanes
__global__ void COOP_LB k_batch_final(dev_batch b, dev_work w) {
  __shared__ cscratch s;
  if (b.n_jobs == 0) {
    if (threadIdx.x == 0) w.flags[0] = 0u;
    return;
  }
  const bool one = c_final_exp_is_one(w.f_batch[0], &s);
  if (threadIdx.x == 0) w.flags[0] = one ? 1u : 0u;
}

// per-job verdicts; a final exponentiation per job only when the batch check
// failed (the worker's per-job retry, multithread/worker.ts:74-85), one
// workgroup per job
__global__ void COOP_LB k_job_final(dev_batch b, dev_work w) {
  __shared__ cscratch s;
  const uint32_t j = blockIdx.x;
  const int32_t code = w.job_code[j];
  int32_t res;
  if (code != C_OK) {
    res = -code;
  } else if (w.flags[0]) {
    res = 1;  // whole batch verified: every job is valid
  } else {
    res = c_final_exp_is_one(w.f_job[j], &s) ? 1 : 0;
  }
  if (threadIdx.x == 0) w.job_result[j] = res;
}

// ------------------------------------------------- multi-GPU combination
__global__ void COOP_LB k_combine_final(const fp12_t* parts, uint32_t n, uint32_t* flag) {
  __shared__ cscratch s;
  __shared__ wfp12 acc, x;
  __shared__ fp12_t g;
  c_set_one(&acc);
  for (uint32_t k = 0; k < n; k++) {
    c_load(&x, parts[k]);
    c_mul(&acc, &acc, &x, &s);
  }
  c_store(g, &acc);
  const bool one = c_final_exp_is_one(g, &s);
  if (threadIdx.x == 0) flag[0] = one ? 1u : 0u;
}

// bgv_debug_stages: out[i] = FE(in[i]) (the cubed value of c_final_exp), one
// cooperative workgroup per element
__global__ void COOP_LB k_final_exp_many(const fp12_t* in, fp12_t* out) {
  __shared__ cscratch s;
  __shared__ fp12_t r;
  c_final_exp(&r, in[blockIdx.x], &s);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

#undef gtid

// the levels ping-pong between the two regions of f_fold; level 0 always runs
// (it is the one that leaves out the rejected jobs)
static void launch_batch_chain(hipStream_t st, const dev_batch& b, const dev_work& w) {
  const dim3 ct(COOP_THREADS);
  uint32_t n = miller_items_bound(b, b.steps_slice), lvl = 0;
  fp12_t* reg[2] = {w.f_fold, w.f_fold + tail_region1(n, FOLD_FAN) * MILLER_STEPS};
  const fp12_t* src = w.f_step;
  do {
    const uint32_t groups = tail_groups(n, FOLD_FAN);
    fp12_t* dst = reg[lvl & 1u];
    hipLaunchKernelGGL(k_step_fold, dim3(groups, MILLER_STEPS), ct, 0, st, b, w, src, n, dst, lvl == 0 ? 1u : 0u);
    src = dst;
    n = groups;
    lvl++;
  } while (n > 1);
  hipLaunchKernelGGL(k_batch_chain, dim3(1), ct, 0, st, b, w, src);
}

void launch_job_chain_retry(hipStream_t st, const dev_batch& b, const dev_work& w) {
  if (b.n_jobs) hipLaunchKernelGGL(k_job_chain, dim3(b.n_jobs), dim3(COOP_THREADS), 0, st, b, w, (const uint32_t*)w.flags);
}

void launch_fp12_tail(hipStream_t st, int stage, const dev_batch& b, const dev_work& w) {
  const uint32_t span = 1u << b.span_log2;
  auto grid = [](uint32_t n) { return dim3((n + 63u) / 64u); };
  const dim3 ct(COOP_THREADS);
  if (stage == ST_F_TREE) {
    if (!b.n_jobs) return;
    if (b.batch_tail) {  // one recurrence over the step products of all slices
      launch_batch_chain(st, b, w);
      return;
    }
    if (b.steps_slice) {  // per-step line products: the job's recurrence over them
      hipLaunchKernelGGL(k_job_chain, dim3(b.n_jobs), ct, 0, st, b, w, (const uint32_t*)nullptr);
      return;
    }
    if (span <= 256) {  // every job folds in one workgroup
      uint32_t stride = b.pairs_per_item ? b.pairs_per_item : 1u;  // fold_step
      if (b.prefold_log2) {  // few large jobs: fold groups side by side first
        stride = 1u << b.prefold_log2;
        hipLaunchKernelGGL(k_job_prefold, dim3((span + stride - 1) / stride, b.n_jobs), ct, 0, st, b, w);
      }
      hipLaunchKernelGGL(k_job_fold, dim3(b.n_jobs), ct, 0, st, b, w, stride);
      return;
    }
    // larger jobs: segmented pairwise tree first
    if (b.n_sets)
      for (uint32_t s = 1; s < span; s *= 2) hipLaunchKernelGGL(k_f_level, grid(b.n_sets), dim3(64), 0, st, b, w, s);
    hipLaunchKernelGGL(k_job_f, grid(b.n_jobs), dim3(64), 0, st, b, w, span);
  } else if (stage == ST_BATCH_PROD) {
    if (b.batch_tail) return;  // k_batch_chain left the product in f_batch[0]
    // fold by FOLD_FAN, ping-ponging f_batch <-> f_tmp, the product landing in f_batch[0]
    uint32_t n = b.n_jobs;
    fp12_t* src = w.f_batch;
    while (n > FOLD_FAN) {
      fp12_t* dst = src == w.f_batch ? w.f_tmp : w.f_batch;
      const uint32_t groups = (n + FOLD_FAN - 1) / FOLD_FAN;
      hipLaunchKernelGGL(k_fold, dim3(groups), ct, 0, st, src, n, dst);
      src = dst;
      n = groups;
    }
    if (n > 1 || (n == 1 && src != w.f_batch)) hipLaunchKernelGGL(k_fold, dim3(1), ct, 0, st, src, n, w.f_batch);
  } else if (stage == ST_BATCH_FINAL) {
    hipLaunchKernelGGL(k_batch_final, dim3(1), ct, 0, st, b, w);
  } else if (stage == ST_JOB_FINAL) {
    if (b.n_jobs) hipLaunchKernelGGL(k_job_final, dim3(b.n_jobs), ct, 0, st, b, w);
  }
}

void launch_final_exp_many(hipStream_t st, const fp12_t* in, fp12_t* out, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_final_exp_many, dim3(n), dim3(COOP_THREADS), 0, st, in, out);
}

void launch_combine_final(hipStream_t st, const fp12_t* parts, uint32_t n, uint32_t* flag) {
  hipLaunchKernelGGL(k_combine_final, dim3(1), dim3(COOP_THREADS), 0, st, parts, n, flag);
}

}  // namespace bgv
