// sim_distill.cc — TEST INFRASTRUCTURE ONLY: the corpus distiller's rule
// (wtf_amd/csrc/engine_distill.h, distill_host) built for the host, behind a
// C interface for tests/test_distill.py and tests/native/sim_distill_main.cc.
#include "../../wtf_amd/csrc/engine_distill.h"

extern "C" int sim_distill(uint32_t n, const uint64_t *offsets, const uint64_t *values, const uint8_t *eligible,
                           uint32_t *out_index, uint32_t *out_gain, uint32_t *kept, uint64_t *universe) {
  return wtfdis::distill_host(n, offsets, values, eligible, out_index, out_gain, kept, universe);
}
