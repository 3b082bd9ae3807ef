// Committee bitfields over resident index lists (bgv_verify_bits,
// include/bgv.h): the expansion of every set's (list window, participation
// bits) into the pk_offsets / pk_indices arrays the rest of the pipeline reads.
// Three steps on the context's main stream:
//   k_bits_count   per set: its key count (masked popcount, or len); on a
//                  context with resident sums (bgv_index_list_sums) also the
//                  set's path: a complement set counts and expands its ABSENT
//                  members and gets its window of the sums (pk_window)
//   k_scan         counts -> pk_off[n_sets + 1]        (bgv_kernels.hip)
//   k_bits_expand  per set: the list entries of its set bits, in order
//
// Balance.  A batch mixes single-key sets, 128-key attestations, a 512-bit sync
// aggregate and committees of up to 2,048 members.  BITS_LANES = 8 lanes share
// a set and take one 32-bit word each per pass, so a single or a 128-bit
// attestation is one pass and a 2,048-bit committee eight; no lane walks a
// whole committee beside idle neighbours, and a single costs eight lanes for
// one pass, not a wave.  The rank of a word inside its set is the 8-lane prefix
// sum of the popcounts plus a carry from the earlier passes; the group then
// writes the pass's words one after another, eight neighbouring bits per step
// (the rank of a bit inside its word is a popcount below it), so its loads
// and stores touch neighbouring entries.  Explicit sets run through the same
// code as all-ones words over pk_indices (a straight copy).
//
// Bounds.  Host batches are checked before they get here.  On-device batches
// are not: a source that fails bits_src_check counts one key and expands to
// BITS_BAD_INDEX, which the gather rejects (BGV_SET_INDEX_RANGE); bitfield
// bytes come from byte loads inside [bits_off, bits_off + ceil(len / 8)) and
// inside bits_len (bits_fetch_word), padding bits are masked; every store is
// clipped to the set's own [pk_off[i], pk_off[i + 1]) and to the buffer.
#include "bgv_internal.h"
#include "bits_expand.h"

namespace bgv {

constexpr uint32_t BITS_LANES = 8;

// sum over the BITS_LANES lanes of a set (all lanes of the wave take part)
__device__ __forceinline__ uint32_t group_sum(uint32_t x) {
#pragma unroll
  for (uint32_t d = 1; d < BITS_LANES; d <<= 1) x += __shfl_xor(x, d, BITS_LANES);
  return x;
}

__global__ void __launch_bounds__(64) k_bits_count(bits_args a) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = (uint32_t)(g / BITS_LANES), l = (uint32_t)(g % BITS_LANES);
  const bool live = i < a.n_sets;
  uint32_t cnt = 0;
  bool ok = false;
  bits_src s = {0, 0, 0, 0};
  if (live) {
    s = a.src[i];
    ok = bits_src_check(s, a.v) == BITS_OK;
    if (ok && s.list == BITS_SRC_EXPLICIT) {
      cnt = l == 0 ? s.len : 0u;
    } else if (ok) {
      const uint32_t words = bits_words(s.len);
      for (uint32_t w = l; w < words; w += BITS_LANES) cnt += bits_popc(bits_src_word(s, a.v, w));
    }
  }
  cnt = group_sum(cnt);
  const bool lead = live && l == 0;
  uint32_t pop = 0, cmpl = 0;  // this set's share of the two tallies
  if (lead) {
    if (a.win) {  // the context holds sums: the rule of bits_expand.h, per set
      pk_window wd = {nullptr, nullptr};
      pop = ok ? cnt : 1u;
      if (ok && bits_src_complement(s, a.v, cnt)) {
        // s passed the span check: off + len lies inside the list's n + 1 sums
        const g1j* S = (const g1j*)bits_list_sums(a.v, s.list);
        wd.lo = S + s.off;
        wd.hi = S + s.off + s.len;
        cnt = s.len - cnt;  // the absent members are gathered
        cmpl = 1;
      }
      a.win[i] = wd;
    }
    a.pk_off[i] = ok ? cnt : 1u;
  }
  // on-device batches: the host has no bits to count, so the device tallies
  // the participating keys and the complement sets, one atomic pair per wave
  if (a.tally) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      pop += __shfl_xor(pop, d, 64);
      cmpl += __shfl_xor(cmpl, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
      atomicAdd(&a.tally[0], pop);
      atomicAdd(&a.tally[1], cmpl);
    }
  }
}

__global__ void __launch_bounds__(64) k_bits_expand(bits_args a) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = (uint32_t)(g / BITS_LANES), l = (uint32_t)(g % BITS_LANES);
  const bool live = i < a.n_sets;
  bits_src s = {0, 0, 0, 0};
  uint32_t base = 0, end = 0, words = 0;
  bool cmpl = false;  // complement path: the clear bits below len are expanded
  if (live) {
    s = a.src[i];
    base = a.pk_off[i];
    end = min(a.pk_off[i + 1], a.cap);
    if (bits_src_check(s, a.v) == BITS_OK) {
      words = bits_words(s.len);
      cmpl = a.win && a.win[i].hi;
    } else if (l == 0 && base < end) {
      a.pk_idx[base] = BITS_BAD_INDEX;
    }
  }
  // the pass count is made uniform over the wave, so the prefix shuffles below
  // never run under a divergent loop; lanes past their set hold empty words
  uint32_t passes = (words + BITS_LANES - 1) / BITS_LANES;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) passes = max(passes, (uint32_t)__shfl_xor(passes, d, 64));
  uint32_t carry = 0;
  for (uint32_t p = 0; p < passes; p++) {
    const uint32_t w = p * BITS_LANES + l;
    const uint32_t m = w < words ? bits_gather_word(s, a.v, w, cmpl) : 0u;
    const uint32_t c = bits_popc(m);
    uint32_t x = c;  // inclusive prefix over the set's lanes
#pragma unroll
    for (uint32_t d = 1; d < BITS_LANES; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, BITS_LANES);
      if (l >= d) x += y;
    }
    const uint32_t tot = __shfl(x, BITS_LANES - 1, BITS_LANES);
    const uint32_t excl = x - c;
    // The group writes the pass's words one after another, lane l the bits
    // l, 8 + l, 16 + l, 24 + l of each: eight neighbouring list entries are read
    // and (where they participate) eight neighbouring indices written per step,
    // instead of every lane walking its own word 128 bytes from its neighbour's.
#pragma unroll
    for (uint32_t q = 0; q < BITS_LANES; q++) {
      const uint32_t mq = __shfl(m, q, BITS_LANES);     // word p * BITS_LANES + q of the set
      const uint32_t eq = __shfl(excl, q, BITS_LANES);  // keys of the pass's words before it
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t bit = 8u * r + l;
        if ((mq >> bit) & 1u) {
          const uint32_t pos = base + carry + eq + bits_rank(mq, bit);
          if (pos >= base && pos < end) a.pk_idx[pos] = bits_src_entry(s, a.v, 32u * (p * BITS_LANES + q) + bit);
        }
      }
    }
    carry += tot;
  }
}

void launch_bits_count(hipStream_t st, const bits_args& a) {
  if (a.n_sets) hipLaunchKernelGGL(k_bits_count, dim3((uint32_t)(((uint64_t)a.n_sets * BITS_LANES + 63u) / 64u)), dim3(64), 0, st, a);
}

void launch_bits_expand(hipStream_t st, const bits_args& a) {
  if (a.n_sets) hipLaunchKernelGGL(k_bits_expand, dim3((uint32_t)(((uint64_t)a.n_sets * BITS_LANES + 63u) / 64u)), dim3(64), 0, st, a);
}

}  // namespace bgv
