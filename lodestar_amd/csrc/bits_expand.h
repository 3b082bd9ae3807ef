// Pure helpers of the committee-bitfield expansion (bgv_verify_bits,
// include/bgv.h): a set names a resident index list, a window [off, off + len)
// of it and a byte-packed participation bitfield; its keys are the list
// entries whose bit is set, in ascending position
// (aggregationBits.intersectValues(committeeIndices) of the reference).
// Everything here is BGV_HD: the kernels of bgv_bits.hip, the host-side
// contract check of bgv_api_bits.hip and the stand-alone host test
// (tests/native/hostcheck_bits.cpp) run the same code.
#pragma once
#include "bls_types.h"

namespace bgv {

constexpr uint32_t BITS_MAX_LISTS = 8;            // BGV_MAX_INDEX_LISTS
constexpr uint32_t BITS_SRC_EXPLICIT = 0xffffffffu;  // BGV_SRC_EXPLICIT
constexpr uint32_t BITS_BAD_INDEX = 0x7fffffffu;  // past any table (at most 2^31 - 1 rows)

// bgv_set_src
struct bits_src {
  uint32_t list, off, len, bits_off;
};

// what the sources of one batch point into
struct bits_view {
  const uint32_t* list[BITS_MAX_LISTS];  // resident lists (NULL: not set)
  uint32_t list_len[BITS_MAX_LISTS];
  const uint8_t* bits;
  uint32_t bits_len;
  const uint32_t* pk_indices;  // keys of explicit sets
  uint32_t n_indices;
  // resident prefix sums of a list (bgv_index_list_sums; NULL: none).  Only
  // "has sums" matters here: the entry type belongs to the gather
  const void* sums[BITS_MAX_LISTS];
};

enum : int {
  BITS_OK = 0,
  BITS_E_LIST = 1,   // list id names no list that is set
  BITS_E_SPAN = 2,   // off + len leaves the list (or pk_indices)
  BITS_E_BITS = 3,   // bits_off + ceil(len / 8) leaves bits
};

BGV_HD uint32_t bits_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// 32-bit words (explicit sets: runs of 32 keys) a source of `len` entries spans
BGV_HD uint32_t bits_words(uint32_t len) { return len / 32u + ((len & 31u) ? 1u : 0u); }
BGV_HD uint32_t bits_bytes(uint32_t len) { return len / 8u + ((len & 7u) ? 1u : 0u); }

// the bits of word w that lie below `len`: all of them, the low len % 32 in the
// last word, none past it
BGV_HD uint32_t bits_len_mask(uint32_t len, uint32_t w) {
  const uint32_t full = len / 32u;
  if (w < full) return 0xffffffffu;
  if (w > full) return 0u;
  return (1u << (len & 31u)) - 1u;  // len % 32 == 0: the word is past the set, no bit
}

// Word w of the bitfield that starts at byte bits_off and covers `len` bits, in
// SSZ bit order (bit j of the set is bit j % 8 of byte j / 8, so byte k lands
// in bits 8 (k % 4) .. of word k / 4).  bits_off is a byte offset of any
// alignment, so the word is assembled from byte loads; a byte past the set's
// own ceil(len / 8) bytes or past bits_len is never read and counts as zero.
BGV_HD uint32_t bits_fetch_word(const uint8_t* bits, uint32_t bits_len, uint32_t bits_off, uint32_t len, uint32_t w) {
  const uint32_t nbytes = bits_bytes(len);
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4u; k++) {
    const uint64_t b = (uint64_t)w * 4u + k;
    if (b >= nbytes) break;
    const uint64_t at = (uint64_t)bits_off + b;
    if (at >= bits_len) break;
    v |= (uint32_t)bits[at] << (8u * k);
  }
  return v;
}

// fetch + mask: the participation bits of word w, padding above len cleared
BGV_HD uint32_t bits_word(const uint8_t* bits, uint32_t bits_len, uint32_t bits_off, uint32_t len, uint32_t w) {
  return bits_fetch_word(bits, bits_len, bits_off, len, w) & bits_len_mask(len, w);
}

// rank of bit j inside its word: set bits below it
BGV_HD uint32_t bits_rank(uint32_t word, uint32_t j) { return bits_popc(word & ((1u << (j & 31u)) - 1u)); }

// the list of an id below BITS_MAX_LISTS, picked by compares: on the device
// the view is a kernel argument, which a lane-dependent subscript would spill
BGV_HD const uint32_t* bits_list_ptr(const bits_view& v, uint32_t id) {
  const uint32_t* p = v.list[0];
  for (uint32_t k = 1; k < BITS_MAX_LISTS; k++)
    if (id == k) p = v.list[k];
  return p;
}

BGV_HD uint32_t bits_list_len(const bits_view& v, uint32_t id) {
  uint32_t n = v.list_len[0];
  for (uint32_t k = 1; k < BITS_MAX_LISTS; k++)
    if (id == k) n = v.list_len[k];
  return n;
}

BGV_HD const void* bits_list_sums(const bits_view& v, uint32_t id) {
  const void* p = v.sums[0];
  for (uint32_t k = 1; k < BITS_MAX_LISTS; k++)
    if (id == k) p = v.sums[k];
  return p;
}

// The span checks of one source, in 64-bit arithmetic (off = 0xfffffff0 with
// len = 0x20 must not wrap into the list).
BGV_HD int bits_src_check(const bits_src& s, const bits_view& v) {
  if (s.list == BITS_SRC_EXPLICIT) return (uint64_t)s.off + s.len <= v.n_indices ? BITS_OK : BITS_E_SPAN;
  if (s.list >= BITS_MAX_LISTS || !bits_list_ptr(v, s.list)) return BITS_E_LIST;
  if ((uint64_t)s.off + s.len > bits_list_len(v, s.list)) return BITS_E_SPAN;
  if ((uint64_t)s.bits_off + bits_bytes(s.len) > v.bits_len) return BITS_E_BITS;
  return BITS_OK;
}

// keys of a source that passed bits_src_check: word w holds participation bits
// (list sets) or is a full run of 32 keys (explicit sets)
BGV_HD uint32_t bits_src_word(const bits_src& s, const bits_view& v, uint32_t w) {
  if (s.list == BITS_SRC_EXPLICIT) return bits_len_mask(s.len, w);
  return bits_word(v.bits, v.bits_len, s.bits_off, s.len, w);
}

// The complement rule (bgv_index_list_sums).  A list set with `pop` of its
// `len` bits set has the aggregate key S[off + len] - S[off] - (the sum of
// its len - pop absent members): the window costs two row reads and one
// addition, as much as two gathered keys, so the complement path is taken iff
// the list has sums and absent + 2 < pop.  Padding bits above len are in
// neither count (pop comes from masked words).
BGV_HD bool bits_complement(bool has_sums, uint32_t len, uint32_t pop) {
  return has_sums && (uint64_t)(len - pop) + 2u < pop;
}

// the rule for a source that passed bits_src_check: explicit sets and sets of
// lists without sums stay on the direct path
BGV_HD bool bits_src_complement(const bits_src& s, const bits_view& v, uint32_t pop) {
  return s.list != BITS_SRC_EXPLICIT && bits_complement(bits_list_sums(v, s.list) != nullptr, s.len, pop);
}

// word w of the keys a source gathers: its set bits, or on the complement path
// its clear bits below len
BGV_HD uint32_t bits_gather_word(const bits_src& s, const bits_view& v, uint32_t w, bool complement) {
  const uint32_t m = bits_src_word(s, v, w);
  return complement ? ~m & bits_len_mask(s.len, w) : m;
}

// entry j of a source that passed bits_src_check
BGV_HD uint32_t bits_src_entry(const bits_src& s, const bits_view& v, uint32_t j) {
  return s.list == BITS_SRC_EXPLICIT ? v.pk_indices[s.off + j] : bits_list_ptr(v, s.list)[s.off + j];
}

// Reference expansion of one checked source, one bit at a time through the
// helpers above (host check and tests; the kernels go word by word): appends
// at most cap keys to out and returns the key count.
BGV_HD uint32_t bits_src_expand(const bits_src& s, const bits_view& v, uint32_t* out, uint32_t cap) {
  uint32_t k = 0;
  const uint32_t words = bits_words(s.len);
  for (uint32_t w = 0; w < words; w++) {
    uint32_t m = bits_src_word(s, v, w);
    for (uint32_t j = 0; j < 32u && m; j++, m >>= 1)
      if (m & 1u) {
        if (k < cap) out[k] = bits_src_entry(s, v, 32u * w + j);
        k++;
      }
  }
  return k;
}

}  // namespace bgv
