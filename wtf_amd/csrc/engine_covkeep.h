// engine_covkeep.h — the coverage-keeping rule of `minimize --keep-coverage`
// (wtfgpu_coverage_contains): one definition of
//
//   (a lane's coverage set S, the target set T) -> missing = |T \ S|
//
// and of what makes a candidate keep, compiled three times, as
// engine_minimize.h is: by hipcc into k_cov_contains (engine_kernels.h), by
// the host compiler into libwtfhost.a (host/minimize.cc: the session's own
// check, for executors without the kernel) and into the test library
// tests/native/sim_covkeep.cc. Plain C++ when hipcc is not the compiler.
// tests/covkeep_model.py restates this comment, not the code.
//
// Nothing here is the reference's (it has no minimiser).
//
// ---- the rule
//   T is the input's own whole coverage set, from one run of the input as it
//   is with full coverage: rips, or with --edges rips and edge values, as
//   opaque 64-bit values, sorted and unique. T is fixed for the whole session
//   (a winner's set never replaces it), so coverage cannot erode round after
//   round.
//
//   missing(S, T) = |T \ S|: the values of T that S lacks.
//
//   A candidate keeps iff all of
//     - its result is Ok_t,
//     - there is no engine error,
//     - its lane's set did not overflow,
//     - missing(S, T) == 0.
//   Keeping is a superset, not equality: a candidate that also reaches code
//   the input did not still keeps, and the output covers at least T.
//
// ---- a lane's set as a table
//   An open-addressed table of H slots (H a power of two): rip[H] values and
//   gen[H] generations, and the lane's current generation g. A slot is live
//   iff gen[slot] == g; every other slot is empty, whatever it holds (a
//   restore or a collection empties the set by changing g). A value v is
//   inserted (log_value, engine_run.h) at the first slot that is not live
//   among mix64(v) & (H - 1), +1, +2, ... (mod H), unless a live slot holding
//   v comes first. A set holds at most cap(H) = H - H / 4 values: inserting a
//   value it lacks into a set of cap(H) values drops the value and raises the
//   lane's overflow flag.
//
// ---- the probe: is v in the table
//   Start at mix64(v) & (H - 1) and go on linearly (mod H), at most H slots:
//     - a slot that is not live ends the probe: absent (log_value would have
//       put v there). That slot may hold v itself, from an earlier
//       generation: still absent;
//     - a live slot holding v: present;
//     - any other live slot: the next one.
//   H slots without an answer: absent.
//
// mix64 is the finaliser engine_device.h defines for the engine (the two must
// stay the same function; the GPU test compares this probe with tables that
// k_run filled):
//   x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
//   x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33     (64-bit wrap-around)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KEEP_HD __host__ __device__ inline
#else
#define KEEP_HD inline
#endif

namespace wtfkeep {

KEEP_HD uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// The most values a table of H slots holds
KEEP_HD uint32_t cap(uint32_t H) { return H - H / 4; }

// The probe. rip / gen are the lane's H slots, g its generation.
KEEP_HD bool table_has(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g, uint64_t v) {
  uint32_t h = (uint32_t)mix64(v) & (H - 1);
  for (uint32_t probe = 0; probe < H; probe++) {
    if (gen[h] != g) return false;
    if (rip[h] == v) return true;
    h = (h + 1) & (H - 1);
  }
  return false;
}

// A candidate keeps
KEEP_HD bool keeps(bool ok, bool error, bool overflow, uint64_t missing) {
  return ok && !error && !overflow && missing == 0;
}

// ---- for the host

// missing(S, T) for S as a table
inline uint32_t missing_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g, const uint64_t *t,
                              uint32_t nt) {
  uint32_t m = 0;
  for (uint32_t i = 0; i < nt; i++) m += !table_has(rip, gen, H, g, t[i]);
  return m;
}

// missing(S, T) for S and T as sorted unique lists
inline uint64_t missing_sorted(const uint64_t *s, size_t ns, const uint64_t *t, size_t nt) {
  uint64_t m = 0;
  size_t i = 0;
  for (size_t j = 0; j < nt; j++) {
    while (i < ns && s[i] < t[j]) i++;
    m += !(i < ns && s[i] == t[j]);
  }
  return m;
}

}  // namespace wtfkeep
