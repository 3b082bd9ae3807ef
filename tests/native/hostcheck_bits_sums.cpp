// Host-compiled check of the complement-path helpers of
// lodestar_amd/csrc/bits_expand.h (bits_complement, bits_src_complement,
// bits_gather_word): the same BGV_HD functions k_bits_count / k_bits_expand and
// the host-side plan run, against a bit-by-bit loop.  TEST ONLY.  A stand-alone
// program (its own main; built once plainly and once with
// -fsanitize=address,undefined by tests/test_bits_sums_host.py): every bitfield
// lives in a heap block that ends on its last byte, so a load past the end is a
// sanitizer finding.  Prints "hostcheck bits sums OK <cases>" and returns 0, or
// names the first mismatch and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../lodestar_amd/csrc/bits_expand.h"

using namespace bgv;

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static int failures = 0;
#define EXPECT(c, ...)                          \
  do {                                          \
    if (!(c)) {                                 \
      if (failures++ < 10) {                    \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                    \
        printf("\n");                           \
      }                                         \
    }                                           \
  } while (0)

// one list set of `len` bits with `pop` of them set, the bitfield at byte `byte_off` of a block that ends with it
static void run_case(uint32_t len, uint32_t pop, uint32_t byte_off, bool dirty_padding) {
  const uint32_t nbytes = bits_bytes(len), bits_len = byte_off + nbytes;
  uint8_t* bits = (uint8_t*)malloc(bits_len);
  memset(bits, 0xff, byte_off);  // a neighbour's bits: never this set's
  memset(bits + byte_off, 0, nbytes);
  std::vector<uint8_t> bit(len, 0);
  for (uint32_t k = 0; k < pop;) {  // pop distinct positions
    const uint32_t j = rnd() % len;
    if (bit[j]) continue;
    bit[j] = 1;
    bits[byte_off + (j >> 3)] |= (uint8_t)(1u << (j & 7u));
    k++;
  }
  if (dirty_padding && (len & 7u)) bits[bits_len - 1] |= (uint8_t)(0xffu << (len & 7u));
  static const uint32_t some = 0;
  bits_view v;
  memset(&v, 0, sizeof v);
  v.list[2] = &some; v.list_len[2] = len + 5;   // with sums
  v.list[6] = &some; v.list_len[6] = len + 5;   // without
  v.sums[2] = &some;
  v.bits = bits; v.bits_len = bits_len;
  const bits_src s = {2, 5, len, byte_off}, t = {6, 5, len, byte_off};
  EXPECT(bits_src_check(s, v) == BITS_OK && bits_src_check(t, v) == BITS_OK, "len %u", len);
  // pop from the masked words, as the kernels and the host check count it
  uint32_t cnt = 0;
  for (uint32_t w = 0; w < bits_words(len); w++) cnt += bits_popc(bits_src_word(s, v, w));
  EXPECT(cnt == pop, "len %u: pop %u, counted %u (padding bits are neither present nor absent)", len, pop, cnt);
  const bool want = (uint64_t)(len - pop) + 2 < pop;
  EXPECT(bits_complement(true, len, pop) == want && !bits_complement(false, len, pop), "len %u pop %u", len, pop);
  EXPECT(bits_src_complement(s, v, pop) == want, "len %u pop %u: list with sums", len, pop);
  EXPECT(!bits_src_complement(t, v, pop), "len %u pop %u: list without sums", len, pop);
  // the words either path gathers, bit by bit
  uint32_t absent = 0;
  for (uint32_t w = 0; w < bits_words(len) + 1; w++) {
    const uint32_t direct = bits_gather_word(s, v, w, false), cmpl = bits_gather_word(s, v, w, true);
    for (uint32_t b = 0; b < 32; b++) {
      const uint32_t j = 32u * w + b;
      const uint32_t want_d = j < len && bit[j] ? 1u : 0u, want_c = j < len && !bit[j] ? 1u : 0u;
      EXPECT(((direct >> b) & 1u) == want_d, "len %u word %u bit %u direct", len, w, b);
      EXPECT(((cmpl >> b) & 1u) == want_c, "len %u word %u bit %u complement", len, w, b);
    }
    absent += bits_popc(cmpl);
  }
  EXPECT(absent == len - pop, "len %u pop %u: %u absent members", len, pop, absent);
  free(bits);
}

int main() {
  const uint32_t lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 512, 2049};
  long cases = 0;
  for (uint32_t len : lens) {
    std::vector<uint32_t> pops = {1, len, len > 1 ? len - 1 : 1, (len + 2) / 2, (len + 2) / 2 + 1, (len + 2) / 2 - 1, len / 2 + 1};
    for (uint32_t pop : pops) {
      if (pop < 1 || pop > len) continue;
      for (uint32_t byte_off = 0; byte_off < 4; byte_off++)
        for (int dirty = 0; dirty < 2; dirty++) {
          run_case(len, pop, byte_off, dirty != 0);
          cases++;
        }
    }
  }
  // the edges of the rule in 64-bit arithmetic, and explicit sets
  EXPECT(!bits_complement(true, 2, 2) && bits_complement(true, 3, 3) && !bits_complement(true, 4, 3) && bits_complement(true, 4, 4),
         "small windows");
  EXPECT(!bits_complement(true, 0xffffffffu, 1) && bits_complement(true, 0xffffffffu, 0xffffffffu), "32-bit edges");
  bits_view v;
  memset(&v, 0, sizeof v);
  static const uint32_t idx[4] = {1, 2, 3, 4};
  v.pk_indices = idx; v.n_indices = 4;
  for (uint32_t k = 0; k < BITS_MAX_LISTS; k++) v.sums[k] = idx;
  const bits_src e = {BITS_SRC_EXPLICIT, 0, 4, 0};
  EXPECT(!bits_src_complement(e, v, 4), "an explicit set never takes the complement path");
  if (failures) {
    printf("hostcheck bits sums FAILED: %d\n", failures);
    return 1;
  }
  printf("hostcheck bits sums OK %ld\n", cases);
  return 0;
}
