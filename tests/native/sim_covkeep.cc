// sim_covkeep.cc — TEST INFRASTRUCTURE ONLY: the coverage-keeping rule
// (wtf_amd/csrc/engine_covkeep.h) built for the host, behind a C interface for
// tests/test_minimize_coverage.py and tests/native/sim_covkeep_main.cc.
#include "../../wtf_amd/csrc/engine_covkeep.h"

extern "C" {

uint64_t sim_covkeep_mix64(uint64_t x) { return wtfkeep::mix64(x); }
uint32_t sim_covkeep_cap(uint32_t H) { return wtfkeep::cap(H); }

// present[i] = the probe's answer for t[i]; returns missing(S, T)
uint32_t sim_covkeep_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g, const uint64_t *t,
                           uint32_t nt, uint8_t *present) {
  for (uint32_t i = 0; i < nt; i++) present[i] = wtfkeep::table_has(rip, gen, H, g, t[i]);
  return wtfkeep::missing_table(rip, gen, H, g, t, nt);
}

uint64_t sim_covkeep_sorted(const uint64_t *s, uint64_t ns, const uint64_t *t, uint64_t nt) {
  return wtfkeep::missing_sorted(s, ns, t, nt);
}

int sim_covkeep_keeps(int ok, int error, int overflow, uint64_t missing) {
  return wtfkeep::keeps(ok != 0, error != 0, overflow != 0, missing);
}

}  // extern "C"
