// engine_mutate.h — the device mutator (wtfgpu_mutate_feed_lanes,
// `wtfgpu fuzz --device-mutate`): one definition of
//
//   (seed, index, corpus view, ncorpus, max_len) -> bytes
//
// compiled three times: by hipcc into k_mutate_feeds (engine_kernels.h), by
// the host compiler into libwtfhost.a (host/device_mutator.cc: the executors
// that do not mutate on the device materialise the same orders), and into the
// test library tests/native/sim_mutate.cc. Plain C++ when hipcc is not the
// compiler. tests/mutate_model.py restates this comment, not the code.
//
// THIS IS A NEW STREAM, not the reference's. The operators are libFuzzer's
// (FuzzerMutate.cpp:212-575, as LibfuzzerMutator_t::Apply restates them in
// host/mutator_lite.cc) read as pure functions of the base testcase; what the
// host mutator carries from one testcase to the next (its scratch buffer's
// stale tail, MutateInPlaceHere) does not exist here, CrossOver's
// interleaving mode and the two dictionary operators are left out, and the
// generator is counter-based instead of std::minstd_rand. A campaign with
// --device-mutate is therefore compared with the twin running this header,
// never with the reference's mutator.
//
// ---- randomness: splitmix64, keyed by (seed, index) and nothing else
//   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
//            z ^= z >> 27; z *= 0x94D049BB133111EB;  z ^= z >> 31   (mod 2^64)
//   s0 = mix(mix(seed + G) + index),  G = 0x9E3779B97F4A7C15
//   k-th draw (k = 1, 2, ...):  next() = mix(s0 + k * G)
//   R(n), n a u64:  n == 0       -> 0, and NO draw is consumed
//                   n <= 2^32    -> ((next() >> 32) * n) >> 32
//                   otherwise    -> next() % n
//   RandCh():  R(2) != 0 ? R(256) : kSpecial[R(30)]
// No lane number, wave, launch shape, queue or call boundary enters.
//
// ---- one testcase
//   base    = corpus[R(ncorpus)]      (drawn first)
//   partner = corpus[R(ncorpus)]      (drawn second, always)
//   S = min(len(base), max_len): a longer base is clipped; PS = len(partner).
//   up to 100 times: op = R(10); apply it; a result size != 0 ends the loop.
//   After 100 failures the (clipped) base is the result, unchanged.
//   No result is longer than max_len (Max below).
//
// ---- the ten operators, draws in the order written ("fail" = size 0)
//  0 EraseBytes           S <= 1 fails. N = R(S / 2) + 1; At = R(S - N + 1);
//                         bytes [At, At + N) removed.
//  1 InsertByte           S >= Max fails. At = R(S + 1); c = RandCh(); c
//                         inserted before position At.
//  2 InsertRepeatedBytes  S + 3 >= Max fails. N = R(min(Max - S, 128) - 2) + 3;
//                         At = R(S + 1); c = R(2) ? R(256) : (R(2) ? 0 : 255);
//                         N copies of c inserted before At.
//  3 ChangeByte           S == 0 fails. At = R(S); byte At becomes RandCh().
//  4 ChangeBit            S == 0 fails. At = R(S); byte At ^= 1 << R(8).
//  5 ShuffleBytes         S == 0 fails. N = R(min(S, 8)) + 1; At = R(S - N);
//                         w = bytes [At, At + N); for i = N - 1 down to 1:
//                         j = R(i + 1), swap(w[i], w[j]); w written back.
//  6 ChangeASCIIInteger   S == 0 fails. B = R(S), advanced to the first
//                         '0'..'9' at or after it; none fails. E = end of that
//                         digit run; V = its value mod 2^64. c = R(5): 0 V + 1,
//                         1 V - 1, 2 V / 2, 3 V * 2, 4 R(V * V) (all mod 2^64).
//                         [B, E) becomes V in decimal, same width, rightmost
//                         digit first, zero-filled on the left (digits that do
//                         not fit are dropped).
//  7 ChangeBinaryInteger  W = 1 << R(4) bytes. S < W fails. Off = R(S - W + 1).
//                         If Off < 64 and R(4) == 0: V = S truncated to W
//                         bytes, byte-swapped when R(2). Otherwise V = the
//                         little-endian W bytes at Off; A = R(21) - 10;
//                         R(2) ? V = bswap(bswap(V) + A) : V = V + A; then,
//                         when A == 0 (no draw) or else when R(2), V = ~V.
//                         V stored little-endian at Off. (R(4) after Off is
//                         drawn only when Off < 64.)
//  8 CopyPart             S == 0 fails. S == Max (no draw) or else R(2):
//                         CopyPartOf(base -> base), otherwise
//                         InsertPartOf(base -> base).
//  9 CrossOver            S == 0 or PS == 0 fails. R(2) == 0:
//                         CopyPartOf(partner -> base), otherwise
//                         InsertPartOf(partner -> base).
//  CopyPartOf(From, FS):  ToBeg = R(S); N = min(R(S - ToBeg) + 1, FS);
//                         FromBeg = R(FS - N + 1); result[ToBeg + i] =
//                         From[FromBeg + i], i < N; size S.
//  InsertPartOf(From, FS): S >= Max fails. N = R(min(Max - S, FS)) + 1;
//                         FromBeg = R(FS - N + 1); At = R(S + 1);
//                         From[FromBeg, FromBeg + N) inserted before At.
//  From is always read as it was before the operator (a pure function).
//
// Every result is a gather: Plan says, for each output position j, whether
// the byte is base[j] (the head), a middle of n bytes from position a (a
// constant, or a run of the base or the partner), base[j + shift] (the tail),
// or one of at most 20 bytes of a patched window (ShuffleBytes and the
// integer operators). k_mutate_feeds computes the plan wave-uniformly and its
// 64 lanes then write out[j] for j = lane, lane + 64, ...
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MUT_HD __host__ __device__ inline
#else
#define MUT_HD inline
#endif

namespace wtfmut {

constexpr uint32_t kMaxTries = 100;
constexpr uint32_t kNumOps = 10;
constexpr uint32_t kWindow = 20;  // a u64 has at most 20 decimal digits
enum Op : uint32_t {
  kEraseBytes, kInsertByte, kInsertRepeatedBytes, kChangeByte, kChangeBit, kShuffleBytes,
  kChangeASCIIInteger, kChangeBinaryInteger, kCopyPart, kCrossOver
};

// Entry i of the corpus is bytes[off[i], off[i + 1]).
struct Corpus {
  const uint8_t *bytes;
  const uint64_t *off;
};

enum Mid : uint32_t { kMidNone, kMidConst, kMidBase, kMidPartner };

struct Plan {
  const uint8_t *base, *partner;
  uint32_t size;     // of the result
  uint32_t a, n;     // the middle is [a, a + n)
  uint32_t mid;      // Mid
  uint32_t mid_off;  // kMidConst: the byte; else the source position of the middle's first byte
  int32_t shift;     // the tail: out[j] = base[j + shift], j >= a + n
  uint32_t w_at, w_n;
  uint8_t w[kWindow];
  // what the tests read: the operator that succeeded (kNumOps: none), and how
  // many attempts failed, per operator, as a bit each
  uint32_t op, tries, failed_ops;
};

MUT_HD uint64_t mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

struct Rng {
  uint64_t s;
  MUT_HD Rng(uint64_t seed, uint64_t index) : s(mix(mix(seed + 0x9E3779B97F4A7C15ull) + index)) {}
  MUT_HD uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    return mix(s);
  }
  MUT_HD uint64_t R(uint64_t n) {
    if (n == 0) return 0;
    if (n <= (1ull << 32)) return ((next() >> 32) * n) >> 32;
    return next() % n;
  }
  MUT_HD uint8_t ch() {
    const uint8_t special[30] = {'!', '*', '\'', '(', ')', ';', ':', '@', '&', '=', '+', '$', ',', '/', '?',
                                 '%', '#', '[', ']', '0', '1', '2', 'A', 'z', '-', '`', '~', '.', 0xff, 0};
    if (R(2)) return (uint8_t)R(256);
    return special[R(30)];
  }
};

MUT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// The first position in [from, size) whose byte is (digit == want) a decimal
// digit; size when there is none. On the device the 64 lanes of the wave (all
// active: every decision is wave-uniform) look at 64 bytes a round.
MUT_HD uint32_t find_digit(const uint8_t *b, uint32_t from, uint32_t size, bool want) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t l = threadIdx.x & 63;
  for (uint32_t at = from; at < size; at += 64) {
    const bool hit = at + l < size && is_digit(b[at + l]) == want;
    const unsigned long long m = __ballot(hit);
    if (m) return at + (uint32_t)__ffsll((long long)m) - 1;
  }
  return size;
#else
  while (from < size && is_digit(b[from]) != want) from++;
  return from;
#endif
}

MUT_HD uint64_t bswap_w(uint64_t v, uint32_t w) {  // the low w bytes reversed
  uint64_t r = 0;
  for (uint32_t i = 0; i < w; i++) r |= ((v >> (8 * i)) & 0xff) << (8 * (w - 1 - i));
  return r;
}

MUT_HD void copy_part_of(Plan &p, Rng &g, uint32_t S, uint32_t from, uint32_t FS) {
  const uint32_t to_beg = (uint32_t)g.R(S);
  uint32_t n = (uint32_t)g.R(S - to_beg) + 1;
  if (n > FS) n = FS;
  p.mid_off = (uint32_t)g.R(FS - n + 1);
  p.a = to_beg;
  p.n = n;
  p.mid = from;
  p.size = S;
}

MUT_HD void insert_part_of(Plan &p, Rng &g, uint32_t S, uint32_t Max, uint32_t from, uint32_t FS) {
  if (S >= Max) return;
  const uint32_t room = Max - S;
  const uint32_t n = (uint32_t)g.R(room < FS ? room : FS) + 1;
  p.mid_off = (uint32_t)g.R(FS - n + 1);
  p.a = (uint32_t)g.R(S + 1);
  p.n = n;
  p.mid = from;
  p.shift = -(int32_t)n;
  p.size = S + n;
}

// One operator on base[0, S); p.size stays 0 when it does not apply.
MUT_HD void apply(Plan &p, Rng &g, uint32_t op, uint32_t S, uint32_t PS, uint32_t Max) {
  const uint8_t *b = p.base;
  switch (op) {
    case kEraseBytes: {
      if (S <= 1) return;
      const uint32_t n = (uint32_t)g.R(S / 2) + 1;
      p.a = (uint32_t)g.R(S - n + 1);
      p.shift = (int32_t)n;
      p.size = S - n;
      return;
    }
    case kInsertByte: {
      if (S >= Max) return;
      p.a = (uint32_t)g.R(S + 1);
      p.n = 1;
      p.mid = kMidConst;
      p.mid_off = g.ch();
      p.shift = -1;
      p.size = S + 1;
      return;
    }
    case kInsertRepeatedBytes: {
      if (S + 3 >= Max) return;
      const uint32_t room = Max - S < 128 ? Max - S : 128;
      const uint32_t n = (uint32_t)g.R(room - 2) + 3;
      p.a = (uint32_t)g.R(S + 1);
      p.n = n;
      p.mid = kMidConst;
      p.mid_off = g.R(2) ? (uint32_t)g.R(256) : (g.R(2) ? 0u : 255u);
      p.shift = -(int32_t)n;
      p.size = S + n;
      return;
    }
    case kChangeByte: {
      if (S == 0) return;
      p.w_at = (uint32_t)g.R(S);
      p.w_n = 1;
      p.w[0] = g.ch();
      p.size = S;
      return;
    }
    case kChangeBit: {
      if (S == 0) return;
      p.w_at = (uint32_t)g.R(S);
      p.w_n = 1;
      p.w[0] = (uint8_t)(b[p.w_at] ^ (1u << g.R(8)));
      p.size = S;
      return;
    }
    case kShuffleBytes: {
      if (S == 0) return;
      const uint32_t n = (uint32_t)g.R(S < 8 ? S : 8) + 1;
      const uint32_t at = (uint32_t)g.R(S - n);
      for (uint32_t i = 0; i < n; i++) p.w[i] = b[at + i];
      for (uint32_t i = n - 1; i >= 1; i--) {
        const uint32_t j = (uint32_t)g.R(i + 1);
        const uint8_t t = p.w[i];
        p.w[i] = p.w[j];
        p.w[j] = t;
      }
      p.w_at = at;
      p.w_n = n;
      p.size = S;
      return;
    }
    case kChangeASCIIInteger: {
      if (S == 0) return;
      const uint32_t B = find_digit(b, (uint32_t)g.R(S), S, true);
      if (B == S) return;
      const uint32_t E = find_digit(b, B, S, false);
      // the value mod 2^64: 2^64 divides 10^64, so a digit 64 or more places
      // left of the last one adds nothing
      uint64_t v = 0;
      for (uint32_t i = E - B > 64 ? E - 64 : B; i < E; i++) v = v * 10 + (uint64_t)(b[i] - '0');
      switch (g.R(5)) {
        case 0: v++; break;
        case 1: v--; break;
        case 2: v /= 2; break;
        case 3: v *= 2; break;
        default: v = g.R(v * v); break;
      }
      const uint32_t wn = E - B < kWindow ? E - B : kWindow;
      for (uint32_t i = wn; i-- > 0;) {
        p.w[i] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
      p.a = B;  // zero fill under the window
      p.n = E - B;
      p.mid = kMidConst;
      p.mid_off = '0';
      p.w_at = E - wn;
      p.w_n = wn;
      p.size = S;
      return;
    }
    case kChangeBinaryInteger: {
      const uint32_t W = 1u << g.R(4);
      if (S < W) return;
      const uint32_t off = (uint32_t)g.R(S - W + 1);
      const uint64_t mask = W == 8 ? ~0ull : (1ull << (8 * W)) - 1;
      uint64_t v;
      if (off < 64 && g.R(4) == 0) {
        v = (uint64_t)S & mask;
        if (g.R(2)) v = bswap_w(v, W);
      } else {
        v = 0;
        for (uint32_t i = 0; i < W; i++) v |= (uint64_t)b[off + i] << (8 * i);
        const uint64_t add = g.R(21) - 10;  // mod 2^64, cut to W bytes below
        if (g.R(2)) v = bswap_w((bswap_w(v, W) + add) & mask, W);
        else v = (v + add) & mask;
        if (add == 0 || g.R(2)) v = ~v & mask;
      }
      for (uint32_t i = 0; i < W; i++) p.w[i] = (uint8_t)(v >> (8 * i));
      p.w_at = off;
      p.w_n = W;
      p.size = S;
      return;
    }
    case kCopyPart: {
      if (S == 0) return;
      if (S == Max || g.R(2)) copy_part_of(p, g, S, kMidBase, S);
      else insert_part_of(p, g, S, Max, kMidBase, S);
      return;
    }
    default: {  // kCrossOver
      if (S == 0 || PS == 0) return;
      if (g.R(2) == 0) copy_part_of(p, g, S, kMidPartner, PS);
      else insert_part_of(p, g, S, Max, kMidPartner, PS);
      return;
    }
  }
}

MUT_HD void plan_clear(Plan &p) {
  p.size = p.a = p.n = p.mid_off = p.w_at = p.w_n = 0;
  p.mid = kMidNone;
  p.shift = 0;
}

// The testcase `index` of the stream `seed`, over the first `ncorpus` (>= 1)
// entries of the corpus.
MUT_HD void make_plan(Plan &p, uint64_t seed, uint64_t index, const Corpus &c, uint32_t ncorpus, uint32_t max_len) {
  Rng g(seed, index);
  const uint64_t bi = g.R(ncorpus), pi = g.R(ncorpus);
  const uint64_t blen = c.off[bi + 1] - c.off[bi], plen = c.off[pi + 1] - c.off[pi];
  const uint32_t S = blen < max_len ? (uint32_t)blen : max_len;
  const uint32_t PS = (uint32_t)plen;
  p.base = c.bytes + c.off[bi];
  p.partner = c.bytes + c.off[pi];
  p.failed_ops = 0;
  for (p.tries = 0; p.tries < kMaxTries; p.tries++) {
    plan_clear(p);
    p.op = (uint32_t)g.R(kNumOps);
    apply(p, g, p.op, S, PS, max_len);
    if (p.size) return;
    p.failed_ops |= 1u << p.op;
  }
  plan_clear(p);
  p.op = kNumOps;
  p.size = S;
}

// Byte j (< p.size) of the result.
MUT_HD uint8_t plan_byte(const Plan &p, uint32_t j) {
  if (j - p.w_at < p.w_n) return p.w[j - p.w_at];
  if (j < p.a) return p.base[j];
  if (j - p.a < p.n) {
    if (p.mid == kMidConst) return (uint8_t)p.mid_off;
    return (p.mid == kMidBase ? p.base : p.partner)[p.mid_off + (j - p.a)];
  }
  return p.base[(uint32_t)((int32_t)j + p.shift)];
}

// The whole testcase into out (room for max_len bytes); its size.
inline uint32_t materialise(uint64_t seed, uint64_t index, const Corpus &c, uint32_t ncorpus, uint32_t max_len,
                            uint8_t *out, Plan *plan_out = nullptr) {
  Plan p;
  make_plan(p, seed, index, c, ncorpus, max_len);
  for (uint32_t j = 0; j < p.size; j++) out[j] = plan_byte(p, j);
  if (plan_out) *plan_out = p;
  return p.size;
}

}  // namespace wtfmut
