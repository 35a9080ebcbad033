// sim_mutate.cc — TEST INFRASTRUCTURE ONLY: the device mutator's definition
// (wtf_amd/csrc/engine_mutate.h) built for the host, behind a C interface for
// tests/test_device_mutate.py.
#include <cstring>

#include "../../wtf_amd/csrc/engine_mutate.h"

extern "C" {

// Testcase indices[i] of the stream, i < n, into out + i * stride (stride >=
// max_len); lens[i] its size; info[3 * i ..] the operator that succeeded (10:
// none), the failed attempts before it, and the failed operators as bits.
void sim_mutate_many(uint64_t seed, const uint64_t *indices, uint32_t n, const uint8_t *bytes, const uint64_t *off,
                     uint32_t ncorpus, uint32_t max_len, uint8_t *out, uint64_t stride, uint32_t *lens,
                     uint32_t *info) {
  const wtfmut::Corpus c{bytes, off};
  for (uint32_t i = 0; i < n; i++) {
    wtfmut::Plan p;
    lens[i] = wtfmut::materialise(seed, indices[i], c, ncorpus, max_len, out + i * stride, &p);
    if (info) {
      info[3 * i] = p.op;
      info[3 * i + 1] = p.tries;
      info[3 * i + 2] = p.failed_ops;
    }
  }
}
}
