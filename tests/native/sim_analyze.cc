// sim_analyze.cc — TEST INFRASTRUCTURE ONLY: the analyzer's rule
// (wtf_amd/csrc/engine_analyze.h) built for the host, behind a C interface for
// tests/test_analyze.py and tests/native/sim_analyze_main.cc.
#include <cstdlib>
#include <cstring>

#include "../../wtf_amd/csrc/engine_analyze.h"

extern "C" {

uint64_t sim_ana_total(uint32_t U) { return wtfana::total(U); }
uint32_t sim_ana_variant(uint32_t b, uint32_t v) { return wtfana::variant((uint8_t)b, v); }

// Candidates indices[i] over the byte buffer base[0, U), i < n, into
// out + i * stride (stride >= U). Each is made in a buffer of exactly U bytes,
// from a copy of the base of exactly U bytes.
void sim_ana_bytes(const uint8_t *base, uint32_t U, const uint64_t *indices, uint32_t n, uint8_t *out,
                   uint64_t stride) {
  uint8_t *b = (uint8_t *)malloc(U ? U : 1);
  memcpy(b, base, U);
  for (uint32_t i = 0; i < n; i++) {
    uint8_t *o = (uint8_t *)malloc(U ? U : 1);
    wtfana::candidate_bytes(b, U, indices[i], o);
    memcpy(out + i * stride, o, U);
    free(o);
  }
  free(b);
}

// The same over a feed of `len` bytes (valid: its chunks tile it), through the
// indexed entry wtfgpu_corpus_add_feed makes of it. Returns its packets; -1:
// not a valid feed. framing (len bytes, may be null): 1 where the helper the
// engine uses (is_framing over the entry's offsets) calls the position framing.
int sim_ana_feed(const uint8_t *feed, uint32_t len, const uint64_t *indices, uint32_t n, uint8_t *out,
                 uint64_t stride, uint8_t *framing) {
  const int64_t P = wtfpkt::entry_packets(feed, len, 16384);
  if (P < 0) return -1;
  const uint64_t eb = wtfpkt::entry_bytes((uint64_t)P, len);
  uint8_t *e = (uint8_t *)malloc(eb);  // 4-aligned, as the arena's entries are
  wtfpkt::entry_write(feed, len, (uint64_t)P, e);
  for (uint32_t i = 0; i < n; i++) {
    uint8_t *o = (uint8_t *)malloc(len ? len : 1);
    wtfana::candidate_feed(e, indices[i], o);
    memcpy(out + i * stride, o, len);
    free(o);
  }
  if (framing) {
    uint32_t *coff = (uint32_t *)malloc(4 * ((size_t)P + 1));  // as the engine keeps them: exactly P + 1 words
    memcpy(coff, e + 4, 4 * ((size_t)P + 1));
    for (uint32_t p = 0; p < len; p++) framing[p] = wtfana::is_framing(coff, (uint32_t)P, p);
    free(coff);
  }
  free(e);
  return (int)P;
}

uint32_t sim_ana_sig_list(const uint64_t *v, uint64_t n, uint64_t *sum) {
  const wtfana::Sig s = wtfana::sig_list(v, (size_t)n);
  *sum = s.sum;
  return s.size;
}

uint32_t sim_ana_sig_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g, uint64_t *sum) {
  const wtfana::Sig s = wtfana::sig_table(rip, gen, H, g);
  *sum = s.sum;
  return s.size;
}

// Five outcomes (the base, then variants 0..3) as parallel arrays
static void outcomes(wtfana::Outcome *o, const uint32_t *kind, const uint32_t *name, const uint64_t *sig,
                     const uint32_t *size, const uint32_t *ovf) {
  for (int k = 0; k < 5; k++) o[k] = wtfana::Outcome{kind[k], name[k], sig[k], size[k], ovf[k] != 0};
}

int sim_ana_classify(const uint32_t *kind, const uint32_t *name, const uint64_t *sig, const uint32_t *size,
                     const uint32_t *ovf) {
  wtfana::Outcome o[5];
  outcomes(o, kind, name, sig, size, ovf);
  return wtfana::classify(o[0], o + 1);
}

// same(outcome a, outcome b) of the five
int sim_ana_same(const uint32_t *kind, const uint32_t *name, const uint64_t *sig, const uint32_t *size,
                 const uint32_t *ovf, uint32_t a, uint32_t b) {
  wtfana::Outcome o[5];
  outcomes(o, kind, name, sig, size, ovf);
  return wtfana::same(o[a], o[b]);
}
}
