// engine_mutate_packets.h — the device packet mutator
// (wtfgpu_mutate_packets_lanes, `wtfgpu fuzz --device-packets`): one
// definition of
//
//   (seed, index, corpus of feeds, ncorpus, params) -> feed bytes
//
// compiled three times, as engine_mutate.h is: by hipcc into k_mutate_packets
// (engine_kernels.h), by the host compiler into libwtfhost.a
// (host/device_mutator.cc) and into the test library
// tests/native/sim_packets.cc. tests/packet_mutate_model.py restates this
// comment, not the code.
//
// A feed is a list of packets as the lanes consume it, per packet a chunk
//   u32 Size (= 8 + body bytes), u32 Command, u16 Id, u16 BodySize, Body
// little-endian, 12 + body bytes long, nothing between chunks. A feed of zero
// bytes (no packet) is a feed.
//
// THIS IS A NEW STREAM, not the reference's. The operators are the tlv
// module's CustomMutator_t (fuzzer_tlv_server.cc:204-365, restated in
// host/modules/fuzzer_tlv_server.cc) read as pure functions of one corpus
// entry; the generator is engine_mutate.h's, not std::mt19937_64 with
// uniform_int_distribution. A campaign with --device-packets is compared with
// the twin running this header, never with the reference's mutator.
//
// ---- randomness: engine_mutate.h's mix, s0, next() and R(n), unchanged
//   s0 = mix(mix(seed + G) + index); the k-th draw is mix(s0 + k * G);
//   R(n) = ((draw >> 32) * n) >> 32 for 1 <= n <= 2^32; R(0) = 0, no draw.
//   Every n below is >= 1 (Params are checked, and P >= 1 where R(P) is drawn),
//   so the draws are numbered as written.
//
// ---- params, declared by the target (tlv's values)
//   GenMaxPackets 10, GenCommands 11, GenMaxBody 100, FlipOneIn 3,
//   InsertMaxPackets 10, MaxFeed 16384 (WTFGPU_FEED_STRIDE: a lane's region).
//   Valid: 1 <= GenMaxPackets <= 64, GenCommands >= 1, FlipOneIn >= 1,
//   GenMaxBody <= 65535 and GenMaxPackets * (12 + GenMaxBody) <= MaxFeed.
//
// ---- one testcase
//   draw 1: g = R(5)
//   g == 4, Generate:
//     draw 2: N = R(GenMaxPackets) + 1
//     packet p (0-based) ALWAYS uses draws 3 + 4p .. 6 + 4p, in this order:
//       Command = R(GenCommands), Len = R(GenMaxBody + 1), f = R(FlipOneIn),
//       b = R(16)   (b is drawn whether or not f == 0: any lane can compute
//       any packet from its number alone)
//     BodySize = (u16)Len ^ (f == 0 ? 1 << b : 0); Id = p; Body = Len zero bytes
//   otherwise, mutate:
//     draw 2: base = corpus[R(ncorpus)]; draw 3: op = R(3); P = base's packets
//     op 0, insert-copy: P == 0 or P > InsertMaxPackets: the base. Otherwise
//       From = R(P), To = R(P + 1); a copy of packet From inserted before
//       position To (To == P: appended).
//     op 1, copy-field: P == 0: the base. Otherwise Src = R(P), Dst = R(P),
//       f = R(4); packet Dst takes Src's 0 Id, 1 Command, 2 BodySize, 3 Body
//       (and with the Body, the chunk's Size).
//     op 2, erase: P == 0: the base. Otherwise packet R(P) erased.
//     A result longer than MaxFeed is replaced by the base, unchanged (only
//     op 0 and op 1 with f == 3 grow). A base always fits: the arena refuses
//     longer entries.
//
// Every mutate result is one gather over the base's chunk bytes, in the Plan
// shape of engine_mutate.h: a head base[j], a middle of n bytes from another
// offset of the base, a tail base[j + shift], and a patched window of at most
// 4 bytes (the changed header field, or the Size of the chunk whose body was
// replaced). k_mutate_packets computes the plan wave-uniformly.
//
// ---- the corpus as this header reads it (wtfgpu_corpus_add_feed writes it)
// Entry i is bytes[off[i], off[i + 1]), 4-aligned, in the indexed layout
//   u32 P, u32 coff[P + 1], the chunks, zero padding to a multiple of 4
// where chunk k is chunk bytes [coff[k], coff[k + 1]) and coff[P] the feed's
// length: packet k is found with two loads and no walk over the chunks.
// Nothing here validates a feed: entry_packets() below is the only gate.
#pragma once
#include "engine_mutate.h"

namespace wtfpkt {

using wtfmut::Corpus;
using wtfmut::Rng;

// engine_mutate.h's Plan with what this stream needs of it: the middle is
// always a run of the base, and the window is one little-endian word instead
// of 20 bytes indexed at run time, so on the device the plan stays in
// registers (no scratch, no LDS).
struct Plan {
  const uint8_t *base;  // the base's chunk bytes
  uint32_t size;        // of the result
  uint32_t a, n;        // the middle is [a, a + n), from base[mid_off ...]
  uint32_t mid_off;
  int32_t shift;        // the tail: out[j] = base[j + shift], j >= a + n
  uint32_t w_at, w_n, w;  // the window: bytes [w_at, w_at + w_n) are w's low bytes
  uint32_t what;        // What
};

struct Params {
  uint32_t GenMaxPackets, GenCommands, GenMaxBody, FlipOneIn, InsertMaxPackets, MaxFeed;
};

// what a testcase was (Plan::what, Info::what): the tests count these
enum What : uint32_t {
  kGenerate,
  kInsert, kInsertEmpty, kInsertTooMany, kInsertTooLong,
  kCopyId, kCopyCommand, kCopyBodySize, kCopyBody, kCopyEmpty, kCopyBodyTooLong,
  kErase, kEraseEmpty,
  kNumWhat
};

MUT_HD bool params_valid(const Params &q) {
  return q.GenMaxPackets >= 1 && q.GenMaxPackets <= 64 && q.GenCommands >= 1 && q.FlipOneIn >= 1 &&
         q.GenMaxBody <= 0xffff && (uint64_t)q.GenMaxPackets * (12 + (uint64_t)q.GenMaxBody) <= q.MaxFeed;
}

// ---- the indexed entry

// Packets of a valid feed; -1 when the chunks do not tile [0, len) exactly,
// a Size is below 8, or len is above max_feed.
inline int64_t entry_packets(const uint8_t *feed, uint64_t len, uint32_t max_feed) {
  if (len > max_feed) return -1;
  uint64_t at = 0;
  int64_t P = 0;
  while (at < len) {
    if (len - at < 4) return -1;
    const uint32_t size = (uint32_t)feed[at] | ((uint32_t)feed[at + 1] << 8) | ((uint32_t)feed[at + 2] << 16) |
                          ((uint32_t)feed[at + 3] << 24);
    if (size < 8 || size > len - at - 4) return -1;
    at += 4 + (uint64_t)size;
    P++;
  }
  return P;
}
inline uint64_t entry_bytes(uint64_t P, uint64_t len) { return (8 + 4 * P + len + 3) & ~3ull; }
// The entry of a feed entry_packets() accepted, into out (entry_bytes(P, len) bytes)
inline void entry_write(const uint8_t *feed, uint64_t len, uint64_t P, uint8_t *out) {
  const auto put = [out](uint64_t word, uint32_t v) {
    for (uint32_t k = 0; k < 4; k++) out[4 * word + k] = (uint8_t)(v >> (8 * k));
  };
  put(0, (uint32_t)P);
  uint64_t at = 0;
  for (uint64_t k = 0; k < P; k++) {
    put(1 + k, (uint32_t)at);
    at += 4 + ((uint64_t)feed[at] | ((uint64_t)feed[at + 1] << 8) | ((uint64_t)feed[at + 2] << 16) |
               ((uint64_t)feed[at + 3] << 24));
  }
  put(1 + P, (uint32_t)len);
  uint8_t *c = out + 8 + 4 * P;
  for (uint64_t k = 0; k < len; k++) c[k] = feed[k];
  for (uint64_t k = 8 + 4 * P + len; k < entry_bytes(P, len); k++) out[k] = 0;
}

// ---- Generate

// The k-th draw of the stream s0, mapped as R(n) maps it (n >= 1)
MUT_HD uint32_t draw(uint64_t s0, uint64_t k, uint32_t n) {
  return (uint32_t)(((wtfmut::mix(s0 + k * 0x9E3779B97F4A7C15ull) >> 32) * (uint64_t)n) >> 32);
}

// Packet p of a generated testcase: its chunk's three header words (Size;
// Command; Id | BodySize << 16). The body is Size - 8 zero bytes.
struct GenPacket {
  uint32_t w[3];
};
MUT_HD GenPacket gen_packet(uint64_t s0, uint32_t p, const Params &q) {
  const uint64_t k = 3 + 4 * (uint64_t)p;
  const uint32_t cmd = draw(s0, k, q.GenCommands), len = draw(s0, k + 1, q.GenMaxBody + 1);
  const uint32_t f = draw(s0, k + 2, q.FlipOneIn), b = draw(s0, k + 3, 16);
  const uint32_t bs = (len ^ (f == 0 ? 1u << b : 0u)) & 0xffff;
  return GenPacket{{8 + len, cmd, p | (bs << 16)}};
}

// ---- mutate

MUT_HD uint32_t ld32(const uint8_t *p) {  // entries are 4-aligned: one load
  uint32_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

// The plan of a testcase that is not generated; g has given draw 1.
MUT_HD void make_plan(Plan &p, Rng &g, const Corpus &c, uint32_t ncorpus, const Params &q) {
  const uint8_t *e = c.bytes + c.off[g.R(ncorpus)];
  const uint32_t op = (uint32_t)g.R(3);
  const uint32_t P = ld32(e);
  const uint8_t *coff = e + 4, *base = e + 8 + 4 * (uint64_t)P;
  const uint32_t L = ld32(coff + 4 * (uint64_t)P);
  p.base = base;
  p.size = L;
  p.a = L;  // all head
  p.n = p.mid_off = p.w_at = p.w_n = p.w = 0;
  p.shift = 0;
  if (P == 0) {
    p.what = op == 0 ? kInsertEmpty : op == 1 ? kCopyEmpty : kEraseEmpty;
    return;
  }
  if (op == 0) {
    if (P > q.InsertMaxPackets) {
      p.what = kInsertTooMany;
      return;
    }
    const uint32_t from = (uint32_t)g.R(P), to = (uint32_t)g.R((uint64_t)P + 1);
    const uint32_t fo = ld32(coff + 4 * (uint64_t)from), n = ld32(coff + 4 * (uint64_t)from + 4) - fo;
    if (L + n > q.MaxFeed) {
      p.what = kInsertTooLong;
      return;
    }
    p.what = kInsert;
    p.a = ld32(coff + 4 * (uint64_t)to);
    p.n = n;
    p.mid_off = fo;
    p.shift = -(int32_t)n;
    p.size = L + n;
    return;
  }
  if (op == 1) {
    const uint32_t src = (uint32_t)g.R(P), dst = (uint32_t)g.R(P), f = (uint32_t)g.R(4);
    const uint32_t so = ld32(coff + 4 * (uint64_t)src), se = ld32(coff + 4 * (uint64_t)src + 4);
    const uint32_t d_o = ld32(coff + 4 * (uint64_t)dst), de = ld32(coff + 4 * (uint64_t)dst + 4);
    if (f == 3) {
      const uint32_t sb = se - so - 12, db = de - d_o - 12;
      if (L - db + sb > q.MaxFeed) {
        p.what = kCopyBodyTooLong;
        return;
      }
      p.what = kCopyBody;
      p.a = d_o + 12;
      p.n = sb;
        p.mid_off = so + 12;
      p.shift = (int32_t)db - (int32_t)sb;
      p.size = L - db + sb;
      p.w_at = d_o;
      p.w_n = 4;
      p.w = 8 + sb;
      return;
    }
    // Id at +8 (2 bytes), Command at +4 (4 bytes), BodySize at +10 (2 bytes)
    const uint32_t at = f == 0 ? 8 : f == 1 ? 4 : 10, wn = f == 1 ? 4 : 2;
    p.what = kCopyId + f;
    p.w_at = d_o + at;
    p.w_n = wn;
    p.w = (uint32_t)base[so + at] | ((uint32_t)base[so + at + 1] << 8);
    if (f == 1) p.w |= ((uint32_t)base[so + at + 2] << 16) | ((uint32_t)base[so + at + 3] << 24);
    return;
  }
  const uint32_t k = (uint32_t)g.R(P);
  const uint32_t ko = ld32(coff + 4 * (uint64_t)k), n = ld32(coff + 4 * (uint64_t)k + 4) - ko;
  p.what = kErase;
  p.a = ko;
  p.shift = (int32_t)n;
  p.size = L - n;
}

// Byte j (< p.size) of the result.
MUT_HD uint8_t plan_byte(const Plan &p, uint32_t j) {
  if (j - p.w_at < p.w_n) return (uint8_t)(p.w >> (8 * (j - p.w_at)));
  if (j < p.a) return p.base[j];
  if (j - p.a < p.n) return p.base[p.mid_off + (j - p.a)];
  return p.base[(uint32_t)((int32_t)j + p.shift)];
}

struct Info {
  uint32_t what, packets;  // What; packets generated (kGenerate)
};

// The whole testcase into out (room for q.MaxFeed bytes); its size.
inline uint32_t materialise(uint64_t seed, uint64_t index, const Corpus &c, uint32_t ncorpus, const Params &q,
                            uint8_t *out, Info *info = nullptr) {
  Rng g(seed, index);
  const uint64_t s0 = g.s;
  if (g.R(5) == 4) {
    const uint32_t N = (uint32_t)g.R(q.GenMaxPackets) + 1;
    uint32_t at = 0;
    for (uint32_t p = 0; p < N; p++) {
      const GenPacket k = gen_packet(s0, p, q);
      for (uint32_t j = 0; j < 12; j++) out[at + j] = (uint8_t)(k.w[j / 4] >> (8 * (j % 4)));
      for (uint32_t j = 12; j < 4 + k.w[0]; j++) out[at + j] = 0;
      at += 4 + k.w[0];
    }
    if (info) *info = Info{kGenerate, N};
    return at;
  }
  Plan p;
  make_plan(p, g, c, ncorpus, q);
  for (uint32_t j = 0; j < p.size; j++) out[j] = plan_byte(p, j);
  if (info) *info = Info{p.what, 0};
  return p.size;
}

}  // namespace wtfpkt
