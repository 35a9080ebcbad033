// engine_analyze.h — the analyzer's rule (`wtfgpu analyze`,
// wtfgpu_analyze_feed_lanes, wtfgpu_coverage_signature): one definition of
//
//   (base, index) -> bytes            the candidate stream
//   a set of 64-bit values -> (sig, size)   the signature of a coverage set
//   five outcomes -> the class of a byte position
//
// compiled three times, as engine_minimize.h is: by hipcc into k_analyze_feeds
// and k_cov_signature (engine_kernels.h), by the host compiler into
// libwtfhost.a (host/analyze.cc: the session classifies with it, and
// materialises candidates and signatures for executors without the kernels)
// and into the test library tests/native/sim_analyze.cc. Plain C++ when hipcc
// is not the compiler. tests/analyze_model.py restates this comment, not the
// code.
//
// Nothing here is random and nothing is the reference's (it has no analyzer).
//
// ---- positions
//   A byte-buffer base has U bytes; every byte is a position, 0 <= p < U.
//   A feed base is its chunk bytes (u32 Size, u32 Command, u16 Id, u16
//   BodySize, Body; 4 + Size bytes a chunk, nothing between chunks), of length
//   U = coff[P] for its P packets, where chunk k is bytes [coff[k], coff[k+1]).
//   Every byte of a feed is a position except the four bytes of each chunk's
//   u32 Size, [coff[k], coff[k] + 4): those are framing, and no candidate ever
//   changes one (the chunks of every candidate tile it as the base's do).
//   Command, Id and BodySize are positions like the body's bytes.
//
// ---- variants: what position p's byte b becomes
//   0: b ^ 0xFF     1: b ^ 0x01     2: b + 0x10     3: b - 0x10    (mod 256)
//   All four differ from b and from each other, for every b.
//
// ---- indices
//   index = 4 * p + v, index < 4 * U. Candidate `index` is the base with byte
//   p replaced by variant v of it; its size is the base's. It depends on
//   (base, index) alone: no lane number, launch shape, queue or call boundary
//   enters.
//
// ---- the signature of a set S of 64-bit values
//   sig(S) = the sum over S of mix64(v), 64-bit wrap-around, paired with |S|.
//   mix64 is engine_covkeep.h's. The empty set is (0, 0). The sum does not
//   depend on the order of the values. Two host forms: over a list of unique
//   values, and over a lane's table (rip[H], gen[H], g), where the values are
//   those of the live slots as engine_covkeep.h states it: slot s is live iff
//   gen[s] == g, whatever any other slot holds.
//
// ---- the outcome of a run
//   (kind, name, sig, size, overflow): kind is one of Ok, Crash, Timedout,
//   Cr3Change, engine error; name is the crash name where the kind is Crash
//   and empty otherwise; (sig, size) is the signature of the run's whole
//   coverage set; overflow says the set filled up and dropped a value.
//   Two outcomes are the same iff neither overflowed and kind, name, sig and
//   size are equal. An overflowed outcome is different from every outcome,
//   itself included.
//
// ---- the class of a position, from the base's outcome B and its four
//      variants' outcomes V0..V3
//   d = how many of V0..V3 are not the same as B.
//   '.' NONE      d == 0
//   'm' MINOR     1 <= d <= 3
//   'F' FIXED     d == 4 and V0, V1, V2, V3 are the same as each other (every
//                 pair): a magic value or a checksum, any change takes one
//                 failing path
//   'V' VARIABLE  d == 4 otherwise: a length, an opcode, data that steers
//   '#' FRAMING   a feed's Size bytes: not tested
//
// ---- the base as this header reads it
// Entry e of a device corpus arena, as engine_minimize.h reads it: a byte
// buffer is bytes[off[e], off[e + 1]), at any alignment; a feed is the
// 4-aligned indexed entry of engine_mutate_packets.h (u32 P, u32 coff[P + 1],
// the chunks). Nothing here validates an entry or an index: the caller checks
// index < 4 * U and, for a feed, that the position is not framing
// (wtfgpu_analyze_feed_lanes does, with is_framing over the offsets the engine
// keeps on the host for each feed entry).
#pragma once
#include "engine_covkeep.h"
#include "engine_mutate_packets.h"

namespace wtfana {

using wtfmut::Corpus;

constexpr uint32_t kVariants = 4;

MUT_HD uint8_t variant(uint8_t b, uint32_t v) {
  switch (v & 3) {
    case 0: return (uint8_t)(b ^ 0xFF);
    case 1: return (uint8_t)(b ^ 0x01);
    case 2: return (uint8_t)(b + 0x10);
    default: return (uint8_t)(b - 0x10);
  }
}

// 4 * U
MUT_HD uint64_t total(uint32_t U) { return (uint64_t)kVariants * U; }

// A candidate: the base with byte p replaced by nb
struct Plan {
  const uint8_t *base;  // the base's bytes (a feed's chunk bytes)
  uint32_t size;        // of the base and of the result
  uint32_t p;           // the position
  uint32_t v;           // the variant
};

MUT_HD void plan_bytes(Plan &q, const uint8_t *base, uint32_t U, uint64_t index) {
  q.base = base;
  q.size = U;
  q.p = (uint32_t)(index >> 2);
  q.v = (uint32_t)(index & 3);
}

// over an indexed feed entry
MUT_HD void plan_feed(Plan &q, const uint8_t *entry, uint64_t index) {
  const uint32_t P = wtfpkt::ld32(entry);
  plan_bytes(q, entry + 8 + 4 * (uint64_t)P, wtfpkt::ld32(entry + 4 + 4 * (uint64_t)P), index);
}

MUT_HD void make_plan(Plan &q, const Corpus &c, uint32_t e, bool feeds, uint64_t index) {
  if (feeds) plan_feed(q, c.bytes + c.off[e], index);
  else plan_bytes(q, c.bytes + c.off[e], (uint32_t)(c.off[e + 1] - c.off[e]), index);
}

// Byte j (< q.size) of the result
MUT_HD uint8_t plan_byte(const Plan &q, uint32_t j) {
  const uint8_t b = q.base[j];
  return j == q.p ? variant(b, q.v) : b;
}

// Is position p (< coff[P]) of a feed framing? coff[0 .. P] are the chunks'
// offsets, ascending, coff[P] the feed's length.
inline bool is_framing(const uint32_t *coff, uint32_t P, uint32_t p) {
  uint32_t lo = 0, hi = P;  // the last chunk k with coff[k] <= p
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (coff[mid] <= p) lo = mid;
    else hi = mid;
  }
  return P == 0 || p - coff[lo] < 4;
}

// ---- the signature

struct Sig {
  uint64_t sum;
  uint32_t size;
};

// over a list of unique values
inline Sig sig_list(const uint64_t *v, size_t n) {
  Sig s{0, (uint32_t)n};
  for (size_t i = 0; i < n; i++) s.sum += wtfkeep::mix64(v[i]);
  return s;
}

// over a lane's table
inline Sig sig_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g) {
  Sig s{0, 0};
  for (uint32_t h = 0; h < H; h++)
    if (gen[h] == g) {
      s.sum += wtfkeep::mix64(rip[h]);
      s.size++;
    }
  return s;
}

// ---- outcomes and classes

enum Kind : uint32_t { kOk, kCrash, kTimedout, kCr3Change, kError, kNumKinds };

// `name` is an id of the crash name (equal ids iff equal names; 0 where the
// kind is not kCrash)
struct Outcome {
  uint32_t kind, name;
  uint64_t sig;
  uint32_t size;
  bool overflow;
};

MUT_HD bool same(const Outcome &a, const Outcome &b) {
  return !a.overflow && !b.overflow && a.kind == b.kind && a.name == b.name && a.sig == b.sig && a.size == b.size;
}

enum Class : char { kNone = '.', kMinor = 'm', kFixed = 'F', kVariable = 'V', kFraming = '#' };

MUT_HD char classify(const Outcome &base, const Outcome *v) {
  uint32_t d = 0;
  for (uint32_t k = 0; k < kVariants; k++) d += !same(base, v[k]);
  if (d == 0) return kNone;
  if (d < kVariants) return kMinor;
  for (uint32_t a = 0; a < kVariants; a++)
    for (uint32_t b = a + 1; b < kVariants; b++)
      if (!same(v[a], v[b])) return kVariable;
  return kFixed;
}

// ---- for the host: whole candidates (out has room for the base's bytes)

inline uint32_t candidate_bytes(const uint8_t *base, uint32_t U, uint64_t index, uint8_t *out) {
  Plan q;
  plan_bytes(q, base, U, index);
  for (uint32_t j = 0; j < q.size; j++) out[j] = plan_byte(q, j);
  return q.size;
}

// `entry` is what wtfpkt::entry_write made of a feed
inline uint32_t candidate_feed(const uint8_t *entry, uint64_t index, uint8_t *out) {
  Plan q;
  plan_feed(q, entry, index);
  for (uint32_t j = 0; j < q.size; j++) out[j] = plan_byte(q, j);
  return q.size;
}

}  // namespace wtfana
