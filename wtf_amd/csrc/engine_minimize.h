// engine_minimize.h — the minimiser's candidate stream
// (wtfgpu_minimize_feed_lanes, `wtfgpu minimize`): one definition of
//
//   (base, op, index) -> bytes
//
// compiled three times, as engine_mutate.h is: by hipcc into k_minimize_feeds
// (engine_kernels.h), by the host compiler into libwtfhost.a
// (host/minimize.cc: the session re-derives every winner from it, and
// materialises the candidates for executors without the kernel) and into the
// test library tests/native/sim_minimize.cc. Plain C++ when hipcc is not the
// compiler. tests/minimize_model.py restates this comment, not the code.
//
// Nothing here is random and nothing is the reference's (it has no minimiser):
// a round of the session is every candidate of one base, and a candidate is a
// pure function of the base and its index.
//
// ---- units
//   A base has U units. A byte buffer's units are its bytes. A feed's units
//   are its packets, one chunk each (u32 Size, u32 Command, u16 Id, u16
//   BodySize, Body; 4 + Size bytes, nothing between chunks: the feed
//   engine_mutate_packets.h describes and wtfgpu_corpus_add_feed validates).
//
// ---- levels and candidates
//   Levels run k = floor(log2 U) down to 0. Level k has chunk length
//   C = 2^k units and n_k = ceil(U / C) candidates; candidate j (0 <= j < n_k)
//   of level k covers the units [j * C, min(U, (j + 1) * C)).
//   U <= 16384 (a lane's feed region), so there are at most 15 levels.
//
// ---- indices
//   T(U) = sum of n_k over the levels; T(0) = 0 (no level, no candidate).
//   Indices 0 .. T(U) - 1 run through the levels from the largest chunk
//   (k = floor(log2 U), index 0) to the smallest (k = 0, the last U indices),
//   ascending j within a level. Index -> (k, j) is a walk over the levels:
//   while index >= n_k, index -= n_k and k -= 1; then j = index. It depends on
//   (U, index) alone: no lane number, launch shape, queue or call boundary
//   enters.
//
// ---- the two ops on the candidate's range [lo, hi) of units
//   0 REMOVE  the base without the range. Bytes: base[0, lo) then base[hi, U),
//             U - (hi - lo) bytes. Feed: the chunks of packets [0, lo) then
//             those of packets [hi, U), each copied whole, so they still tile
//             the result exactly; a result of zero packets is a feed of zero
//             bytes.
//   1 ZERO    byte buffers only: the base with bytes [lo, hi) set to 0, U
//             bytes. (Not defined for feeds.)
//
// Every result is a gather of at most two runs of the base and, for ZERO, a
// constant run in between, in the Plan shape of engine_mutate.h: a head
// base[j] for j < a, a middle of n zero bytes, a tail base[j + shift].
// k_minimize_feeds computes the plan wave-uniformly.
//
// ---- the base as this header reads it
// Entry e of a device corpus arena (engine_mutate.h's Corpus): a byte buffer
// is bytes[off[e], off[e + 1]), at any alignment; a feed is the 4-aligned
// indexed entry of engine_mutate_packets.h (u32 P, u32 coff[P + 1], the
// chunks). Nothing here validates an entry or an index: the caller checks
// index < T(U) (wtfgpu_minimize_feed_lanes does, from the unit counts the
// engine keeps on the host).
#pragma once
#include "engine_mutate_packets.h"

namespace wtfmin {

using wtfmut::Corpus;

enum Op : uint32_t { kRemove, kZero, kNumOps };

MUT_HD uint32_t top_level(uint32_t U) {  // floor(log2 U), U >= 1
  uint32_t k = 0;
  while ((U >> k) > 1) k++;
  return k;
}

// n_k = ceil(U / 2^k)
MUT_HD uint32_t level_count(uint32_t U, uint32_t k) { return (uint32_t)(((uint64_t)U + (1ull << k) - 1) >> k); }

MUT_HD uint64_t total(uint32_t U) {
  if (U == 0) return 0;
  uint64_t t = 0;
  for (uint32_t k = top_level(U) + 1; k-- > 0;) t += level_count(U, k);
  return t;
}

struct Where {
  uint32_t k, j;    // level, candidate of the level
  uint32_t lo, hi;  // the units it covers
};

// index < total(U)
MUT_HD Where locate(uint32_t U, uint64_t index) {
  uint32_t k = top_level(U);
  for (;;) {
    const uint32_t n = level_count(U, k);
    if (index < n || k == 0) break;
    index -= n;
    k--;
  }
  Where w;
  w.k = k;
  w.j = (uint32_t)index;
  const uint64_t lo = (uint64_t)w.j << k, hi = lo + (1ull << k);
  w.lo = (uint32_t)lo;
  w.hi = hi < U ? (uint32_t)hi : U;
  return w;
}

// out[j] = base[j] for j < a; 0 for j - a < n; base[j + shift] after that
struct Plan {
  const uint8_t *base;
  uint32_t size;  // of the result
  uint32_t a, n, shift;
};

// Units of entry e: a byte buffer's length, a feed's packets
MUT_HD uint32_t entry_units(const Corpus &c, uint32_t e, bool feeds) {
  if (feeds) return wtfpkt::ld32(c.bytes + c.off[e]);
  return (uint32_t)(c.off[e + 1] - c.off[e]);
}

// Candidate `index` (< T(U)) of `op` over a byte-buffer base of U bytes
MUT_HD void plan_bytes(Plan &p, const uint8_t *base, uint32_t U, uint32_t op, uint64_t index) {
  const Where w = locate(U, index);
  p.base = base;
  p.a = w.lo;
  if (op == kZero) {
    p.n = w.hi - w.lo;
    p.shift = 0;
    p.size = U;
  } else {
    p.n = 0;
    p.shift = w.hi - w.lo;
    p.size = U - p.shift;
  }
}

// REMOVE candidate `index` (< T(P)) over an indexed feed entry
MUT_HD void plan_feed(Plan &p, const uint8_t *entry, uint64_t index) {
  const uint32_t P = wtfpkt::ld32(entry);
  const uint8_t *coff = entry + 4;
  const Where w = locate(P, index);
  const uint32_t lo = wtfpkt::ld32(coff + 4 * (uint64_t)w.lo), hi = wtfpkt::ld32(coff + 4 * (uint64_t)w.hi);
  p.base = entry + 8 + 4 * (uint64_t)P;
  p.a = lo;
  p.n = 0;
  p.shift = hi - lo;
  p.size = wtfpkt::ld32(coff + 4 * (uint64_t)P) - p.shift;
}

// The plan of candidate `index` of `op` over arena entry e
MUT_HD void make_plan(Plan &p, const Corpus &c, uint32_t e, bool feeds, uint32_t op, uint64_t index) {
  if (feeds) plan_feed(p, c.bytes + c.off[e], index);
  else plan_bytes(p, c.bytes + c.off[e], (uint32_t)(c.off[e + 1] - c.off[e]), op, index);
}

// Byte j (< p.size) of the result.
MUT_HD uint8_t plan_byte(const Plan &p, uint32_t j) {
  if (j < p.a) return p.base[j];
  if (j - p.a < p.n) return 0;
  return p.base[j + p.shift];
}

// ---- for the host: whole candidates (out has room for the base's bytes)

inline uint32_t candidate_bytes(const uint8_t *base, uint32_t U, uint32_t op, uint64_t index, uint8_t *out) {
  Plan p;
  plan_bytes(p, base, U, op, index);
  for (uint32_t j = 0; j < p.size; j++) out[j] = plan_byte(p, j);
  return p.size;
}

// `entry` is what wtfpkt::entry_write made of a feed
inline uint32_t candidate_feed(const uint8_t *entry, uint64_t index, uint8_t *out) {
  Plan p;
  plan_feed(p, entry, index);
  for (uint32_t j = 0; j < p.size; j++) out[j] = plan_byte(p, j);
  return p.size;
}

}  // namespace wtfmin
