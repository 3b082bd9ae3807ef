// Resident prefix sums of an index list (bgv_index_list_sums, include/bgv.h):
//   S[k] = sum of table[list[j]] over j < k,   k = 0 .. n,
// 144 B Jacobian per entry, so that bgv_verify_bits can take a nearly full
// committee as S[off + len] - S[off] minus its absent members
// (bits_expand.h bits_complement, bgv_gather.hip).  Built once per list and
// epoch, off the verify path: a three-level scan over the group.
//   k_sums_tile    lane t: the sum of tile t (SUMS_TILE entries), the same
//                  pipelined load_pk-style walk as k_pk_chunk
//   k_sums_tile2   lane u: the sum of SUMS_TILE2 tile sums
//   k_sums_top     one lane: exclusive scan of the second-level sums
//   k_sums_carry   lane u: exclusive scan of its tile sums from its carry
//   k_sums_write   lane t: re-walks tile t from its carry and writes S
// A 2^20-entry list is 16,385 tiles, 257 second-level sums; the one-lane top
// scan grows with n / 4096 and is 257 additions there.  Every addition is the
// complete one (curve.h jac_add / jac_add_aff: equal rows double, a row beside
// its negation gives the identity, the identity adds nothing), and a prefix
// that is the identity is stored as such (Z = 0).
//
// Bounds.  The host refuses a list with an entry at or past the table count
// before anything is launched; the kernels still clip: a row past table_n
// reads as the identity, tile t covers [t SUMS_TILE, min((t + 1) SUMS_TILE, n))
// and writes S[..] at those positions only, the last tile also S[n].
//
// Compiled like the gather (product inlined), so a row loaded ahead stays in
// flight across the addition.
#define BGV_FPMUL_CALL 0
#ifndef BGV_FP2_INLINE
#define BGV_FP2_INLINE 1
#endif
#ifndef BGV_POINT_INLINE
#define BGV_POINT_INLINE 1
#endif
#include "bgv_internal.h"

namespace bgv {

constexpr uint32_t SUMS_TILE = 64;   // list entries per first-level tile (one lane each)
constexpr uint32_t SUMS_TILE2 = 64;  // tile sums per second-level tile
static_assert((SUMS_TILE & (SUMS_TILE - 1)) == 0 && (SUMS_TILE2 & (SUMS_TILE2 - 1)) == 0, "tile sizes are powers of two");

// n / SUMS_TILE + 1 tiles: a list that ends on a tile boundary has an empty
// last tile, whose lane writes S[n] alone
static uint32_t sums_tiles(uint32_t n) { return n / SUMS_TILE + 1u; }
static uint32_t sums_tiles2(uint32_t n) { return (sums_tiles(n) + SUMS_TILE2 - 1u) / SUMS_TILE2; }
size_t sums_tmp_entries(uint32_t n) { return (size_t)sums_tiles(n) + sums_tiles2(n); }

struct sums_args {
  const g1a* table;
  uint32_t table_n;
  const uint32_t* list;
  uint32_t n, tiles, tiles2;
  g1j* sums;  // [n + 1]
  g1j* t1;    // [tiles] tile sums, then their exclusive scan
  g1j* t2;    // [tiles2]
};

__device__ __forceinline__ void sums_row(g1a& out, const sums_args& a, uint32_t j) {
  const uint32_t idx = a.list[j];
  if (idx < a.table_n) { out = a.table[idx]; return; }
  fp_set_zero(out.x);
  fp_set_zero(out.y);
}

// Tile t from `acc` on: WRITE stores the running sum in front of every entry
// (the exclusive prefix), and behind the last entry of the list.
template <bool WRITE>
__device__ __forceinline__ void sums_walk(const sums_args& a, uint32_t t, g1j& acc) {
  const uint32_t beg = t * SUMS_TILE;  // t < tiles: beg <= n
  const uint32_t end = beg + min(SUMS_TILE, a.n - beg);
  g1a nxt;
  if (beg < end) sums_row(nxt, a, beg);
  for (uint32_t k = beg; k < end; k++) {
    const g1a p = nxt;
    if (k + 1 < end) sums_row(nxt, a, k + 1);
    if (WRITE) a.sums[k] = acc;
    if (g1a_is_zero(p)) continue;  // an identity row adds nothing
    jac_add_aff(acc, acc, p);
  }
  if (WRITE && t + 1 == a.tiles) a.sums[a.n] = acc;
}

__global__ void __launch_bounds__(64, 2) k_sums_tile(sums_args a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.tiles) return;
  g1j acc;
  jac_set_inf(acc);
  sums_walk<false>(a, t, acc);
  a.t1[t] = acc;
}

__global__ void __launch_bounds__(64, 2) k_sums_tile2(sums_args a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= a.tiles2) return;
  const uint32_t beg = u * SUMS_TILE2, end = beg + min(SUMS_TILE2, a.tiles - beg);
  g1j acc;
  jac_set_inf(acc);
  for (uint32_t k = beg; k < end; k++) {
    const g1j p = a.t1[k];
    jac_add(acc, acc, p);
  }
  a.t2[u] = acc;
}

__global__ void __launch_bounds__(64, 2) k_sums_top(sums_args a) {
  if (blockIdx.x || threadIdx.x) return;
  g1j acc;
  jac_set_inf(acc);
  for (uint32_t u = 0; u < a.tiles2; u++) {
    const g1j p = a.t2[u];
    a.t2[u] = acc;
    jac_add(acc, acc, p);
  }
}

__global__ void __launch_bounds__(64, 2) k_sums_carry(sums_args a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= a.tiles2) return;
  const uint32_t beg = u * SUMS_TILE2, end = beg + min(SUMS_TILE2, a.tiles - beg);
  g1j acc = a.t2[u];
  for (uint32_t k = beg; k < end; k++) {
    const g1j p = a.t1[k];
    a.t1[k] = acc;
    jac_add(acc, acc, p);
  }
}

__global__ void __launch_bounds__(64, 2) k_sums_write(sums_args a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.tiles) return;
  g1j acc = a.t1[t];
  sums_walk<true>(a, t, acc);
}

// entries as affine 96 B big-endian, all-zero for the identity (bgv_debug_index_list_sums)
__global__ void __launch_bounds__(64, 2) k_sums_export(const g1j* sums, uint8_t* out96, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const g1j p = sums[i];
  uint8_t* o = out96 + 96ull * i;
  g1a q;
  if (!jac_to_aff(q, p)) {
    for (int k = 0; k < 96; k++) o[k] = 0;
    return;
  }
  fp_t t;
  fp_from_mont(t, q.x);
  fp_to_be48(o, t);
  fp_from_mont(t, q.y);
  fp_to_be48(o + 48, t);
}

void launch_list_sums(hipStream_t st, const g1a* table, uint32_t table_n, const uint32_t* list, uint32_t n, g1j* sums,
                      g1j* tmp) {
  sums_args a;
  a.table = table; a.table_n = table_n; a.list = list; a.n = n;
  a.tiles = sums_tiles(n); a.tiles2 = sums_tiles2(n);
  a.sums = sums; a.t1 = tmp; a.t2 = tmp + a.tiles;
  const dim3 g1((a.tiles + 63u) / 64u), g2((a.tiles2 + 63u) / 64u), blk(64);
  hipLaunchKernelGGL(k_sums_tile, g1, blk, 0, st, a);
  hipLaunchKernelGGL(k_sums_tile2, g2, blk, 0, st, a);
  hipLaunchKernelGGL(k_sums_top, dim3(1), blk, 0, st, a);
  hipLaunchKernelGGL(k_sums_carry, g2, blk, 0, st, a);
  hipLaunchKernelGGL(k_sums_write, g1, blk, 0, st, a);
}

void launch_sums_export(hipStream_t st, const g1j* sums, uint8_t* out96, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_sums_export, dim3((n + 63u) / 64u), dim3(64), 0, st, sums, out96, n);
}

}  // namespace bgv
