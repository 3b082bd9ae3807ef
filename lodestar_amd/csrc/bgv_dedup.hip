// Message classes of a bulk batch: hash_to_G2 once per distinct signing root.
//
// H(m) depends on m only, and the batches the bulk layout exists for repeat
// their roots (several aggregates of one committee and data in a block, about
// 16 gossip aggregates per committee on one AttestationData root).  Three
// kernels replace k_hash in the bulk layout (bgv_api.hip run_stages):
//
//   k_msg_dedup    one lane per set: the set's class representative (the first
//                  set to claim the root's slot of an open-addressing table)
//                  and the compacted list of representatives
//   k_hash_reps    k_hash over the representatives only
//   k_hash_spread  every other set copies its representative's H(m)
//
// Everything downstream reads the same w.h_aff[] bytes as after k_hash.
//
// A translation unit of its own, compiled like bgv_kernels.hip (same leaf and
// inlining switches, so k_hash_reps is k_hash plus one index load): the
// register budgets of that unit's kernels do not move.
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

namespace bgv {

#ifndef BGV_WAVES
#define BGV_WAVES 2
#endif
#ifndef BGV_HASH_WAVES
#define BGV_HASH_WAVES BGV_WAVES
#endif

__device__ __forceinline__ uint32_t gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }

// the root of set i as four little-endian words; byte loads, as k_hash reads
// them: an on-device batch promises no alignment
__device__ __forceinline__ void load_root(uint64_t r[4], const uint8_t* msgs, uint32_t i) {
  const uint8_t* m = msgs + 32u * (size_t)i;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) v |= (uint64_t)m[8 * k + j] << (8 * j);
    r[k] = v;
  }
}

// 64-bit mix of the whole root under the per-call key (bgv_api.hip): peers
// choose roots, so an unkeyed mix would let crafted roots share a probe chain
__device__ __forceinline__ uint64_t root_mix(const uint64_t r[4], uint64_t key) {
  uint64_t h = key;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    h ^= r[k];
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 29;
  }
  return h;
}

// ------------------------------------------------------------ k_msg_dedup
// Set i claims slot s of the table with a compare-and-swap; the value that
// comes back is the only word lanes exchange (msgs is input, nothing a lane
// stores is read by another inside the kernel).  An occupied slot holds a set
// index below n_sets (the table is cleared to MSG_EMPTY per call and only
// this kernel writes it); equal roots -> that set represents i, else the next
// slot.  The table has at least 2 n_sets slots, so a free slot exists; the
// probe count is bounded all the same, and a set that ran out represents
// itself (it hashes its own root: the same H(m)).  Slots are masked, set
// indices are below n_sets: no access leaves the buffers whatever msgs holds.
//
// The representatives are compacted into uniq[] through ONE returning add per
// wave (ballot, popcount, lane rank): a single counter word saturates near 88
// returning atomics per microsecond, which per lane would be over a
// millisecond at 100,352 sets.  Which equal set wins and the order of uniq[]
// vary from run to run; nothing downstream depends on either.
__global__ void __launch_bounds__(64) k_msg_dedup(msg_classes c) {
  const uint32_t i = gtid();
  bool is_rep = false;
  if (i < c.n_sets) {
    uint64_t mine[4];
    load_root(mine, c.msgs, i);
    uint32_t s = (uint32_t)root_mix(mine, c.key) & c.mask;
    uint32_t r = i;
    for (uint32_t probes = 0; probes <= c.mask; probes++) {
      const uint32_t prev = atomicCAS(&c.table[s], MSG_EMPTY, i);
      if (prev == MSG_EMPTY || prev >= c.n_sets) break;  // the slot is i's
      uint64_t other[4];
      load_root(other, c.msgs, prev);
      if (((mine[0] ^ other[0]) | (mine[1] ^ other[1]) | (mine[2] ^ other[2]) | (mine[3] ^ other[3])) == 0) {
        r = prev;
        break;
      }
      s = (s + 1u) & c.mask;
    }
    c.rep[i] = r;
    is_rep = r == i;
  }
  const uint64_t reps = __ballot(is_rep);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0 && reps) base = atomicAdd(c.n_uniq, (uint32_t)__popcll(reps));
  base = __shfl(base, 0, 64);
  // at most one entry per set: base + rank < n_sets
  if (is_rep) c.uniq[base + (uint32_t)__popcll(reps & ((1ull << lane) - 1ull))] = i;
}

// ------------------------------------------------------------ k_hash_reps
// k_hash with an indirection: lane u hashes the root of representative
// uniq[u] into its own h_aff row.  The grid covers n_sets lanes (the host
// never reads n_uniq to size it); waves past n_uniq leave at once.
__global__ void __launch_bounds__(64, BGV_HASH_WAVES) k_hash_reps(msg_classes c) {
  const uint32_t u = gtid();
  if (u >= c.n_sets || u >= *c.n_uniq) return;
  const uint32_t i = c.uniq[u];
  if (i >= c.n_sets) return;
  uint8_t m[32];
#pragma unroll
  for (int k = 0; k < 32; k++) m[k] = c.msgs[32u * (size_t)i + k];
  g2j h;
  hash_to_g2(h, m);
  g2a ha;
  jac_to_aff(ha, h);  // H(m) is never the identity for a 32-byte root (prob. 2^-255)
  c.h_aff[i] = ha;
}

// ---------------------------------------------------------- k_hash_spread
// after k_hash_reps on the same stream: 192 bytes per repeated set
static_assert(sizeof(g2a) == 192 && sizeof(g2a) % sizeof(uint4) == 0, "h_aff rows are copied as 12 x 16 bytes");
__global__ void __launch_bounds__(64) k_hash_spread(msg_classes c) {
  const uint32_t i = gtid();
  if (i >= c.n_sets) return;
  const uint32_t r = c.rep[i];
  if (r == i || r >= c.n_sets) return;
  const uint4* src = reinterpret_cast<const uint4*>(c.h_aff + r);
  uint4* dst = reinterpret_cast<uint4*>(c.h_aff + i);
  uint4 v[12];
#pragma unroll
  for (int k = 0; k < 12; k++) v[k] = src[k];
#pragma unroll
  for (int k = 0; k < 12; k++) dst[k] = v[k];
}

static inline dim3 grid64(uint32_t n) { return dim3((n + 63u) / 64u); }

void launch_msg_dedup(hipStream_t st, const msg_classes& c) {
  if (c.n_sets) hipLaunchKernelGGL(k_msg_dedup, grid64(c.n_sets), dim3(64), 0, st, c);
}

void launch_hash_classes(hipStream_t st, const msg_classes& c) {
  if (!c.n_sets) return;
  hipLaunchKernelGGL(k_hash_reps, grid64(c.n_sets), dim3(64), 0, st, c);
  hipLaunchKernelGGL(k_hash_spread, grid64(c.n_sets), dim3(64), 0, st, c);
}

}  // namespace bgv
