// Pair classes of a bulk batch: one set-pair Miller loop per distinct signing
// root of a job (bgv_pair_merge, pair_merge.h).
//
// The set-pair kernels (k_miller, k_miller_steps) and the per-job folds reach
// sets only through job_off, item_off / item_job, set_job, rpk_aff, pk_code,
// h_aff and lines, so they run unchanged over a view whose "sets" are the
// classes (bgv_api.hip run_stages).  This unit builds that view:
//
//   k_pm_claim     one lane per set: the class (job, root representative) claims
//                  a slot of a keyed open-addressing table; the first claimant
//                  leads and takes the class's index inside its job from one
//                  returning add per (wave, job)
//   (scan)         leaders per job -> class offsets: the view's job_off
//   k_pm_link      one lane per set: its class index; the members of a class
//                  are linked through an exchange on the class's list head
//   k_pm_items     the view's Miller work items (then a scan, k_pm_item_job)
//   k_pm_h         hash stream, after k_hash_reps: H(m) of every class
//   k_pm_lines     hash stream: the fixed-argument lines, one lane per CLASS
//   k_pm_sum       pubkey stream, after k_pk: P_c = sum of the members' keys
//
// Inside a kernel lanes exchange only what an atomic returns; everything a
// lane stores is read by a later kernel (the per-XCD L2s are not coherent).
// The class count lives on the device only: every grid covers n_sets lanes
// and lanes past class_off[n_jobs] leave at once.  Which set leads a class
// and the order of a job's classes vary from run to run; P_c is affine and
// every fold is a product, so nothing downstream depends on either.
//
// A translation unit of its own, compiled like bgv_kernels.hip: the register
// budgets of the other units' kernels do not move.
#ifndef BGV_FPMUL_CALL
#define BGV_FPMUL_CALL 1
#endif
#ifndef BGV_FP2_INLINE
#define BGV_FP2_INLINE 1
#endif
#ifndef BGV_FP6_INLINE
#define BGV_FP6_INLINE 1
#endif
#ifndef BGV_POINT_INLINE
#define BGV_POINT_INLINE 1
#endif
#ifndef BGV_KERNELS_FP2_LEAF
#define BGV_KERNELS_FP2_LEAF 0
#endif
#ifndef BGV_FP2_LEAF
#define BGV_FP2_LEAF BGV_KERNELS_FP2_LEAF
#endif
#include "bgv_internal.h"
#include "pair_merge.h"

namespace bgv {

#ifndef BGV_WAVES
#define BGV_WAVES 2
#endif
#ifndef BGV_LINES_WAVES
#define BGV_LINES_WAVES 2
#endif

__device__ __forceinline__ static uint32_t pm_gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }

// ------------------------------------------------------------- k_pm_claim
// The table holds >= 2 n_sets slots and at most n_sets distinct keys, so the
// probe loop (bounded by the slot count) ends at the key or at a free slot.
// Slots are masked, jobs come from the offsets, a representative outside the
// batch is replaced by the set itself: no access leaves the buffers.
__global__ void __launch_bounds__(64) k_pm_claim(pair_classes p) {
  const uint32_t i = pm_gtid();
  const uint32_t lane = threadIdx.x & 63u;
  bool lead = false;
  uint32_t j = 0, s = 0;
  if (i < p.n_sets) {
    j = pm_job_of(p.job_off, p.n_jobs, i);
    uint32_t r = p.rep[i];
    if (r >= p.n_sets) r = i;
    const uint64_t mine = ((uint64_t)j << 32) | r;
    s = (uint32_t)pm_slot_mix(j, r, p.key) & p.mask;
    for (uint32_t probes = 0; probes <= p.mask; probes++) {
      const uint64_t prev = atomicCAS((unsigned long long*)&p.table[s], (unsigned long long)PM_EMPTY, (unsigned long long)mine);
      if (prev == PM_EMPTY) { lead = true; break; }
      if (prev == mine) break;
      s = (s + 1u) & p.mask;
    }
  }
  // the leader's index inside its job: one returning add per job present in
  // the wave (a wave's sets are consecutive, so that is one add for most waves;
  // a single word saturates near 88 returning atomics per microsecond)
  uint32_t idx = 0;
  uint64_t todo = __ballot(lead);
  while (todo) {  // wave-uniform
    const int l = __ffsll((unsigned long long)todo) - 1;
    const uint32_t jj = __shfl(j, l, 64);
    const bool in = lead && j == jj;
    const uint64_t same = __ballot(in);
    uint32_t base = 0;
    if (lane == (uint32_t)l) base = atomicAdd(&p.class_off[jj], (uint32_t)__popcll(same));
    base = __shfl(base, l, 64);
    if (in) idx = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  if (i < p.n_sets) {
    p.slot[i] = s | (lead ? PM_LEAD : 0u);
    if (lead) p.slot_idx[s] = idx;
  }
}

// -------------------------------------------------------------- k_pm_link
// after the scan of class_off.  Class indices are below n_sets (a job has at
// most as many classes as sets); an index that is not is clamped.
__global__ void __launch_bounds__(64) k_pm_link(pair_classes p) {
  const uint32_t i = pm_gtid();
  if (i >= p.n_sets) return;
  const uint32_t j = pm_job_of(p.job_off, p.n_jobs, i);
  const uint32_t sl = p.slot[i];
  const uint32_t s = sl & ~PM_LEAD & p.mask;
  uint32_t c = p.class_off[j] + p.slot_idx[s];
  if (c >= p.n_sets) c = p.n_sets - 1u;
  p.cls[i] = c;
  p.next[i] = atomicExch(&p.head[c], i);
  if (sl & PM_LEAD) {
    uint32_t r = p.rep[i];
    if (r >= p.n_sets) r = i;
    p.cls_job[c] = j;
    p.cls_rep[c] = r;
  }
}

// ------------------------------------------------- the view's work items
__global__ void __launch_bounds__(64) k_pm_items(pair_classes p) {
  const uint32_t j = pm_gtid();
  if (j >= p.n_jobs) return;
  const uint32_t lo = p.class_off[j], hi = p.class_off[j + 1];
  p.item_off[j] = hi > lo ? miller_item_count(hi - lo, p.per) : 0u;
}

__global__ void __launch_bounds__(64) k_pm_item_job(pair_classes p) {
  const uint32_t j = pm_gtid();
  if (j >= p.n_jobs) return;
  // items <= classes <= n_sets: inside item_job[n_sets + n_jobs + 1]
  const uint32_t end = min(p.item_off[j + 1], p.n_sets + p.n_jobs);
  for (uint32_t t = p.item_off[j]; t < end; t++) p.item_job[t] = j;
}

// ------------------------------------------------------------------ k_pm_h
// after k_hash_reps on the same stream: 192 bytes per class
static_assert(sizeof(g2a) == 192 && sizeof(g2a) % sizeof(uint4) == 0, "h_aff rows are copied as 12 x 16 bytes");
// (scalar arguments, not the struct: the copy stays in registers)
__global__ void __launch_bounds__(64) k_pm_h(uint32_t n_sets, const uint32_t* n_classes, const uint32_t* cls_rep,
                                             const g2a* __restrict__ h_aff, g2a* __restrict__ h_cls) {
  const uint32_t c = pm_gtid();
  if (c >= n_sets || c >= *n_classes) return;
  const uint32_t r = cls_rep[c];
  if (r >= n_sets) return;
  const uint4* src = reinterpret_cast<const uint4*>(h_aff + r);
  uint4* dst = reinterpret_cast<uint4*>(h_cls + c);
#pragma unroll
  for (int k = 0; k < 12; k++) dst[k] = src[k];  // two buffers: the loads need not all precede the stores
}

// -------------------------------------------------------------- k_pm_lines
// k_lines over the classes: column c of the line buffer (stride n_sets, the
// real one) holds the lines of H(m) of class c
__global__ void __launch_bounds__(64, BGV_LINES_WAVES) k_pm_lines(pair_classes p, fp2_t* lines) {
  const uint32_t c = pm_gtid();
  if (c >= p.n_sets || c >= p.class_off[p.n_jobs]) return;
  miller_lines(lines, p.n_sets, c, p.h_cls[c]);
}

// ---------------------------------------------------------------- k_pm_sum
// after k_pk on the same stream; one lane per class (pair_merge.h pm_class_sum)
__global__ void __launch_bounds__(64, BGV_WAVES) k_pm_sum(pair_classes p, const g1a* rpk_aff, const int32_t* pk_code) {
  const uint32_t c = pm_gtid();
  if (c >= p.n_sets || c >= p.class_off[p.n_jobs]) return;
  g1a out;
  int32_t code;
  bool ident;
  pm_class_sum(out, code, ident, rpk_aff, pk_code, p.next, p.head[c], p.n_sets);
  p.p_cls[c] = out;
  p.code_cls[c] = code;
  if (ident) *p.ident = 1u;  // every writer stores the same value; read by the host after the run
}

static inline dim3 grid64(uint32_t n) { return dim3((n + 63u) / 64u); }

void launch_pair_classes(hipStream_t st, const pair_classes& p) {
  if (!p.n_sets || !p.n_jobs) return;
  hipLaunchKernelGGL(k_pm_claim, grid64(p.n_sets), dim3(64), 0, st, p);
  launch_scan(st, p.class_off, p.n_jobs);
  hipLaunchKernelGGL(k_pm_link, grid64(p.n_sets), dim3(64), 0, st, p);
  hipLaunchKernelGGL(k_pm_items, grid64(p.n_jobs), dim3(64), 0, st, p);
  launch_scan(st, p.item_off, p.n_jobs);
  hipLaunchKernelGGL(k_pm_item_job, grid64(p.n_jobs), dim3(64), 0, st, p);
}

void launch_pair_h(hipStream_t st, const pair_classes& p, const g2a* h_aff) {
  if (p.n_sets)
    hipLaunchKernelGGL(k_pm_h, grid64(p.n_sets), dim3(64), 0, st, p.n_sets, (const uint32_t*)(p.class_off + p.n_jobs),
                       (const uint32_t*)p.cls_rep, h_aff, p.h_cls);
}

void launch_pair_lines(hipStream_t st, const pair_classes& p, fp2_t* lines) {
  if (p.n_sets) hipLaunchKernelGGL(k_pm_lines, grid64(p.n_sets), dim3(64), 0, st, p, lines);
}

void launch_pair_sum(hipStream_t st, const pair_classes& p, const g1a* rpk_aff, const int32_t* pk_code) {
  if (p.n_sets) hipLaunchKernelGGL(k_pm_sum, grid64(p.n_sets), dim3(64), 0, st, p, rpk_aff, pk_code);
}

}  // namespace bgv
