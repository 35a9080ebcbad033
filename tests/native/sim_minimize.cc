// sim_minimize.cc — TEST INFRASTRUCTURE ONLY: the minimiser's candidate stream
// (wtf_amd/csrc/engine_minimize.h) built for the host, behind a C interface
// for tests/test_minimize.py and tests/native/sim_minimize_main.cc.
#include <cstdlib>
#include <cstring>

#include "../../wtf_amd/csrc/engine_minimize.h"

extern "C" {

uint64_t sim_min_total(uint32_t U) { return wtfmin::total(U); }

// out4: k, j, lo, hi
void sim_min_locate(uint32_t U, uint64_t index, uint32_t *out4) {
  const wtfmin::Where w = wtfmin::locate(U, index);
  out4[0] = w.k, out4[1] = w.j, out4[2] = w.lo, out4[3] = w.hi;
}

// Candidates indices[i] of `op` over the byte buffer base[0, U), i < n, into
// out + i * stride (stride >= U); lens[i] its size. Each is made in a buffer
// of exactly its size, from a copy of the base of exactly U bytes.
void sim_min_bytes(const uint8_t *base, uint32_t U, uint32_t op, const uint64_t *indices, uint32_t n, uint8_t *out,
                   uint64_t stride, uint32_t *lens) {
  uint8_t *b = (uint8_t *)malloc(U ? U : 1);
  memcpy(b, base, U);
  for (uint32_t i = 0; i < n; i++) {
    wtfmin::Plan p;
    wtfmin::plan_bytes(p, b, U, op, indices[i]);
    uint8_t *o = (uint8_t *)malloc(p.size ? p.size : 1);
    lens[i] = wtfmin::candidate_bytes(b, U, op, indices[i], o);
    memcpy(out + i * stride, o, p.size);
    free(o);
  }
  free(b);
}

// The same over a feed of `len` bytes (valid: its chunks tile it), through the
// indexed entry wtfgpu_corpus_add_feed makes of it. -1: not a valid feed.
int sim_min_feed(const uint8_t *feed, uint32_t len, const uint64_t *indices, uint32_t n, uint8_t *out,
                 uint64_t stride, uint32_t *lens) {
  const int64_t P = wtfpkt::entry_packets(feed, len, 16384);
  if (P < 0) return -1;
  const uint64_t eb = wtfpkt::entry_bytes((uint64_t)P, len);
  uint8_t *e = (uint8_t *)malloc(eb);  // 4-aligned, as the arena's entries are
  wtfpkt::entry_write(feed, len, (uint64_t)P, e);
  for (uint32_t i = 0; i < n; i++) {
    wtfmin::Plan p;
    wtfmin::plan_feed(p, e, indices[i]);
    uint8_t *o = (uint8_t *)malloc(p.size ? p.size : 1);
    lens[i] = wtfmin::candidate_feed(e, indices[i], o);
    memcpy(out + i * stride, o, p.size);
    free(o);
  }
  free(e);
  return (int)P;
}
}
