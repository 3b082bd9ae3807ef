// Host-compiled check of the bitfield-expansion helpers
// (lodestar_amd/csrc/bits_expand.h): the same BGV_HD functions the kernels of
// bgv_bits.hip and the host-side contract check run, against a bit-by-bit loop.
// TEST ONLY.  A stand-alone program (its own main; built once plainly and once
// with -fsanitize=address,undefined by tests/test_bits_host.py): every bitfield
// and list lives in a heap block of exactly its size, and the last bitfield of
// a case ends on the last byte of `bits`, so a load past an end is a sanitizer
// finding.  Prints "hostcheck bits OK <cases>" and returns 0, or names the
// first mismatch and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../lodestar_amd/csrc/bits_expand.h"

using namespace bgv;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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

enum Pattern { P_FIRST, P_LAST, P_ALL, P_ALT, P_R1, P_R50, P_R99, P_COUNT };

static bool pattern_bit(int pat, uint32_t j, uint32_t len) {
  switch (pat) {
    case P_FIRST: return j == 0;
    case P_LAST: return j == len - 1;
    case P_ALL: return true;
    case P_ALT: return (j & 1u) == 0;
    case P_R1: return rnd() % 100u < 1u;
    case P_R50: return rnd() % 100u < 50u;
    default: return rnd() % 100u < 99u;
  }
}

// one source in exactly-sized heap blocks: the bitfield starts at byte
// `byte_off` of bits and ends on its last byte
static long run_case(uint32_t len, uint32_t byte_off, uint32_t off, int pat, bool dirty_padding) {
  const uint32_t nbytes = bits_bytes(len);
  const uint32_t bits_len = byte_off + nbytes;
  uint8_t* bits = (uint8_t*)malloc(bits_len);
  for (uint32_t k = 0; k < byte_off; k++) bits[k] = 0xff;  // a neighbour's bits: never this set's
  memset(bits + byte_off, 0, nbytes);
  std::vector<uint8_t> want_bit(len);
  for (uint32_t j = 0; j < len; j++) {
    want_bit[j] = pattern_bit(pat, j, len) ? 1 : 0;
    if (want_bit[j]) bits[byte_off + (j >> 3)] |= (uint8_t)(1u << (j & 7u));
  }
  if (dirty_padding && (len & 7u)) bits[bits_len - 1] |= (uint8_t)(0xffu << (len & 7u));
  const uint32_t list_n = off + len;
  uint32_t* list = (uint32_t*)malloc((size_t)list_n * 4);
  for (uint32_t k = 0; k < list_n; k++) list[k] = (k * 2654435761u) & 0x7fffffffu;

  bits_view v;
  memset(&v, 0, sizeof v);
  v.list[3] = list;
  v.list_len[3] = list_n;
  v.bits = bits;
  v.bits_len = bits_len;
  const bits_src s = {3, off, len, byte_off};
  EXPECT(bits_src_check(s, v) == BITS_OK, "check len %u byte_off %u off %u", len, byte_off, off);

  // the bit-by-bit reference, straight from the definition in include/bgv.h
  std::vector<uint32_t> want;
  for (uint32_t j = 0; j < len; j++)
    if ((bits[byte_off + (j >> 3)] >> (j & 7u)) & 1u) {
      if (j < len) want.push_back(list[off + j]);
    }
  if (!dirty_padding)
    for (uint32_t j = 0; j < len; j++) EXPECT(((bits[byte_off + (j >> 3)] >> (j & 7u)) & 1u) == want_bit[j], "pattern bit %u", j);

  // word by word through the helpers, as the kernels go
  const uint32_t words = bits_words(len);
  EXPECT(words == (len + 31u) / 32u, "bits_words(%u) = %u", len, words);
  std::vector<uint32_t> got;
  uint32_t count = 0;
  for (uint32_t w = 0; w < words; w++) {
    const uint32_t m = bits_src_word(s, v, w);
    EXPECT((m & ~bits_len_mask(len, w)) == 0, "padding survives in word %u of len %u", w, len);
    count += bits_popc(m);
    for (uint32_t j = 0; j < 32u; j++)
      if ((m >> j) & 1u) {
        EXPECT(bits_rank(m, j) == (uint32_t)(got.size() - (count - bits_popc(m))), "rank of bit %u in word %u", j, w);
        got.push_back(bits_src_entry(s, v, 32u * w + j));
      }
  }
  EXPECT(bits_src_word(s, v, words) == 0 && bits_src_word(s, v, words + 7u) == 0, "a word past the set is not empty (len %u)", len);
  EXPECT(count == want.size(), "count %u != %zu (len %u byte_off %u pat %d)", count, want.size(), len, byte_off, pat);
  EXPECT(got == want, "expansion differs (len %u byte_off %u off %u pat %d)", len, byte_off, off, pat);

  // bits_src_expand: the same, and it honours its cap
  std::vector<uint32_t> out(want.size() + 1, 0xdeadbeefu);
  const uint32_t k = bits_src_expand(s, v, out.data(), (uint32_t)want.size());
  EXPECT(k == want.size() && out[want.size()] == 0xdeadbeefu, "bits_src_expand count %u", k);
  out.pop_back();
  EXPECT(out == want, "bits_src_expand output (len %u)", len);
  if (!want.empty()) {
    std::vector<uint32_t> small(1, 0xdeadbeefu);
    EXPECT(bits_src_expand(s, v, small.data(), 0) == want.size() && small[0] == 0xdeadbeefu, "bits_src_expand wrote past cap 0");
  }

  // the same bitfield one byte short: the last byte is not read, its bits count as zero
  if (nbytes > 1) {
    uint32_t c2 = 0;
    for (uint32_t w = 0; w < words; w++) c2 += bits_popc(bits_word(bits, bits_len - 1, byte_off, len, w));
    uint32_t want2 = 0;
    for (uint32_t j = 0; j < len && (j >> 3) < nbytes - 1; j++) want2 += (bits[byte_off + (j >> 3)] >> (j & 7u)) & 1u;
    EXPECT(c2 == want2, "clipped at bits_len: %u != %u", c2, want2);
  }
  free(list);
  free(bits);
  return 1;
}

static void explicit_cases() {
  const uint32_t n = 70;
  uint32_t* idx = (uint32_t*)malloc(n * 4);
  for (uint32_t k = 0; k < n; k++) idx[k] = 0x80000000u ^ (k * 7u);
  bits_view v;
  memset(&v, 0, sizeof v);
  v.pk_indices = idx;
  v.n_indices = n;
  const uint32_t lens[] = {1, 32, 33, 64, 70};
  for (uint32_t len : lens) {
    const uint32_t off = n - len;  // ends on the last index
    const bits_src s = {BITS_SRC_EXPLICIT, off, len, 0xfffffff0u /* ignored */};
    EXPECT(bits_src_check(s, v) == BITS_OK, "explicit check len %u", len);
    std::vector<uint32_t> out(len);
    EXPECT(bits_src_expand(s, v, out.data(), len) == len, "explicit count len %u", len);
    EXPECT(memcmp(out.data(), idx + off, (size_t)len * 4) == 0, "explicit copy len %u", len);
  }
  free(idx);
}

static void check_cases() {
  static const uint32_t some = 0;
  bits_view v;
  memset(&v, 0, sizeof v);
  v.list[1] = &some;  // only "is set" and the length are looked at
  v.list_len[1] = 512;
  v.bits_len = 64;
  v.n_indices = 40;
  auto chk = [&](uint32_t list, uint32_t off, uint32_t len, uint32_t bits_off) {
    const bits_src s = {list, off, len, bits_off};
    return bits_src_check(s, v);
  };
  EXPECT(chk(1, 0, 512, 0) == BITS_OK, "exactly the list and the bits");
  EXPECT(chk(1, 511, 1, 63) == BITS_OK, "last entry, last byte");
  EXPECT(chk(1, 0, 513, 0) == BITS_E_SPAN, "one past the list");
  EXPECT(chk(1, 0xfffffff0u, 0x20u, 0) == BITS_E_SPAN, "off + len wraps in 32 bits");
  EXPECT(chk(1, 0, 8, 64) == BITS_E_BITS, "one byte past bits");
  EXPECT(chk(1, 0, 9, 63) == BITS_E_BITS, "ceil(len / 8) past bits");
  EXPECT(chk(1, 0, 8, 0xffffffffu) == BITS_E_BITS, "bits_off + bytes wraps in 32 bits");
  EXPECT(chk(0, 0, 1, 0) == BITS_E_LIST, "list not set");
  EXPECT(chk(8, 0, 1, 0) == BITS_E_LIST, "list id past the lists");
  EXPECT(chk(0xfffffffeu, 0, 1, 0) == BITS_E_LIST, "list id just below explicit");
  EXPECT(chk(BITS_SRC_EXPLICIT, 0, 40, 1000) == BITS_OK, "explicit: all indices, bits_off ignored");
  EXPECT(chk(BITS_SRC_EXPLICIT, 1, 40, 0) == BITS_E_SPAN, "explicit: one past");
  EXPECT(chk(BITS_SRC_EXPLICIT, 0xfffffff0u, 0x20u, 0) == BITS_E_SPAN, "explicit: wraps");
  // masks
  EXPECT(bits_len_mask(32, 0) == 0xffffffffu && bits_len_mask(32, 1) == 0u, "mask at a word boundary");
  EXPECT(bits_len_mask(33, 1) == 1u && bits_len_mask(31, 0) == 0x7fffffffu && bits_len_mask(1, 0) == 1u, "partial masks");
  EXPECT(bits_len_mask(0, 0) == 0u && bits_len_mask(5, 9) == 0u, "empty masks");
  EXPECT(bits_bytes(0) == 0 && bits_bytes(1) == 1 && bits_bytes(8) == 1 && bits_bytes(9) == 2 && bits_bytes(0xffffffffu) == 0x20000000u, "bits_bytes");
  EXPECT(bits_words(0xffffffffu) == 0x08000000u, "bits_words at the top");
}

int main() {
  const uint32_t lens[] = {1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 512, 2047, 2048, 2049, 4100};
  long cases = 0;
  for (uint32_t len : lens)
    for (uint32_t byte_off = 0; byte_off < 4; byte_off++)
      for (uint32_t off : {0u, 1u, 37u})
        for (int pat = 0; pat < P_COUNT; pat++) {
          cases += run_case(len, byte_off, off, pat, false);
          if (len & 7u) cases += run_case(len, byte_off, off, pat, true);  // non-zero padding is masked off
        }
  explicit_cases();
  check_cases();
  if (failures) {
    printf("hostcheck bits FAILED: %d mismatches\n", failures);
    return 1;
  }
  printf("hostcheck bits OK %ld\n", cases);
  return 0;
}
