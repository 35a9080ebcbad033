// engine_feedpack.h — the layout of a packed read-back of lanes' feeds
// (wtfgpu_read_feeds_packed): one definition of
//
//   (lens of the listed lanes) -> each lane's offset, the total, the bytes
//
// compiled by hipcc into k_feed_lens / k_feed_pack (engine_kernels.h) and by
// the host compiler into tests/native/feed_pack_main.cc, as the two mutator
// streams are shared with their twins. tests/test_feed_pack.py restates this
// comment, not the code.
//
// ---- lengths
//   A listed lane without a feed has len ~0u (kNoFeed) and takes no room.
//   whole = 0: the first chunk without its u32 size word, the size clamped to
//     stride - 4 (chunk_len, as k_feed_gather).
//   whole = 1: the region's first byte to feed_end, clamped to stride
//     (whole_len, as k_feed_gather_whole).
//
// ---- layout
//   pad16(len) = len rounded up to a multiple of 16; pad16(kNoFeed) = 0.
//   offs[i] = sum over k < i, in list order, of pad16(lens[k]): 64-bit, since
//     262,144 lanes of 16 KiB are exactly 2^32 bytes.
//   total = offs[n]. Bytes [offs[i], offs[i] + lens[i]) are lane lanes[i]'s;
//   bytes [offs[i] + lens[i], offs[i] + pad16(lens[i])) are zero. A lane listed
//   twice has two places.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FEEDPACK_HD __host__ __device__ inline
#else
#define FEEDPACK_HD inline
#endif

namespace wtffeedpack {

constexpr uint32_t kNoFeed = ~0u;

FEEDPACK_HD uint64_t pad16(uint32_t len) { return len == kNoFeed ? 0 : ((uint64_t)len + 15) & ~15ull; }

FEEDPACK_HD uint32_t chunk_len(bool has, uint32_t size_word, uint64_t stride) {
  if (!has) return kNoFeed;
  return size_word > stride - 4 ? (uint32_t)(stride - 4) : size_word;
}

FEEDPACK_HD uint32_t whole_len(bool has, uint64_t feed_end, uint64_t region, uint64_t stride) {
  if (!has) return kNoFeed;
  const uint64_t len = feed_end - region;
  return (uint32_t)(len > stride ? stride : len);
}

// One 32-bit word of a lane's place: the source word that starts at byte `at`
// of the lane's bytes, with what lies at or after `len` zeroed.
FEEDPACK_HD uint32_t mask_word(uint32_t w, uint32_t at, uint32_t len) {
  if (at >= len) return 0;
  const uint32_t left = len - at;
  return left >= 4 ? w : w & ((1u << (8 * left)) - 1);
}

// offs[0, n) from lens[0, n); returns the total
inline uint64_t offsets(const uint32_t *lens, uint64_t n, uint64_t *offs) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; i++) {
    offs[i] = at;
    at += pad16(lens[i]);
  }
  return at;
}

// The plain host reference of k_feed_pack: src[i] is lane i's first byte
// (unread when lens[i] is 0 or kNoFeed), out has offsets()'s total bytes.
inline uint64_t pack(const uint32_t *lens, const uint8_t *const *src, uint64_t n, uint64_t *offs, uint8_t *out) {
  const uint64_t total = offsets(lens, n, offs);
  for (uint64_t i = 0; i < n; i++) {
    if (lens[i] == kNoFeed) continue;
    uint8_t *o = out + offs[i];
    const uint64_t padded = pad16(lens[i]);
    for (uint64_t k = 0; k < lens[i]; k++) o[k] = src[i][k];
    for (uint64_t k = lens[i]; k < padded; k++) o[k] = 0;
  }
  return total;
}

}  // namespace wtffeedpack
