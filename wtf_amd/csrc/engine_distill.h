// engine_distill.h — the corpus distiller's rule (wtfgpu_distill, `wtfgpu
// distill`): one definition of
//
//   (sets in rank order, eligible flags) -> (taken indices, gains, universe)
//
// compiled by hipcc into engine.hip (the argument check, the selection key and
// the gain of one set, shared with k_distill_gain / k_distill_take in
// engine_kernels.h) and by the host compiler into libwtfhost.a
// (host/distill.cc: distill_host is the twin's path and the A/B path) and into
// the test program tests/native/sim_distill.cc. Plain C++ when hipcc is not
// the compiler. tests/distill_model.py restates this comment, not the code.
//
// Nothing here is the reference's: its corpus minimiser is a master with
// --runs 0, which keeps an input iff it shows coverage no earlier input
// showed. This is the greedy cover instead.
//
// ---- the rule
// There are n sets S_0..S_{n-1} in rank order. Each is a strictly ascending
// list of 64-bit values. The values are opaque: rips, or --edges hashes. Each
// set carries an `eligible` flag.
//
//   covered = {}
//   loop:
//     g_i = |S_i \ covered| for every eligible i not yet taken
//     if max g_i == 0: stop
//     take the lowest i whose g_i is the maximum; record (i, g_i); covered |= S_i
//
// - The output is the taken indices in the order taken and their gains.
// - `universe` is the number of distinct values over the eligible sets. Sort
//   and deduplicate them to count it.
// - Gains are non-increasing from round to round and each is >= 1.
// - The union of the taken sets equals the union of the eligible sets.
// - Running the rule again on the taken sets alone, in the same relative
//   order, takes all of them in the same order. In every round the winner
//   among all sets is a taken set, so it is still the lowest-index maximum
//   among the taken sets alone.
//
// ---- the layout
// Set i is values[offsets[i], offsets[i + 1]); offsets[0] == 0, offsets never
// decrease, and there are at most 2^32 - 1 entries in all (an entry's position
// and a dense value id each fit 32 bits). eligible == nullptr: every set is.
//
// ---- the selection key
// A round's winner is the maximum of gain << 32 | (0xFFFFFFFF - i) over the
// sets with gain >= 1: the larger gain first, then the lower index. 0 is no
// key (a gain of 0 never makes one).
//
// ---- lazy evaluation
// `covered` only grows, so a gain counted in an earlier round is an upper
// bound on the set's gain now, and so is the key made of it. A set whose stale
// key is below a key already counted this round cannot win the round and need
// not be counted again; the output is the rule's. Both builds use this:
// distill_host keeps the stale keys in a heap, k_distill_gain compares a set's
// stale key with the round's running maximum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIS_HD __host__ __device__ inline
#else
#define DIS_HD inline
#endif

#include <algorithm>
#include <new>
#include <queue>
#include <vector>

namespace wtfdis {

constexpr int kOk = 0, kInvalid = -1, kOom = -3;  // WTFGPU_OK, WTFGPU_ERR_INVALID, WTFGPU_ERR_OOM
constexpr uint64_t kMaxEntries = 0xFFFFFFFFull;

DIS_HD uint64_t make_key(uint32_t gain, uint32_t i) { return (uint64_t)gain << 32 | (0xFFFFFFFFu - i); }
DIS_HD uint32_t key_gain(uint64_t key) { return (uint32_t)(key >> 32); }
DIS_HD uint32_t key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// Is dense id `id` in the bitmap (one bit an id, 32 a word)?
DIS_HD bool covered(const uint32_t *bitmap, uint32_t id) { return (bitmap[id >> 5] >> (id & 31)) & 1; }

// ---- host only (under hipcc: the host half)

// The argument check of both builds, one O(E) pass: kInvalid for a null
// pointer with n > 0, offsets[0] != 0, offsets that decrease, more than
// 2^32 - 1 entries, or a set that is not strictly ascending.
inline int validate(uint32_t n, const uint64_t *offsets, const uint64_t *values, const uint32_t *out_index,
                    const uint32_t *out_gain, const uint32_t *kept, const uint64_t *universe) {
  if (!kept || !universe) return kInvalid;
  if (n == 0) return kOk;
  if (!offsets || !out_index || !out_gain) return kInvalid;
  if (offsets[0] != 0) return kInvalid;
  for (uint32_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] > kMaxEntries) return kInvalid;
  if (offsets[n] && !values) return kInvalid;
  for (uint32_t i = 0; i < n; i++)
    for (uint64_t j = offsets[i] + 1; j < offsets[i + 1]; j++)
      if (values[j] <= values[j - 1]) return kInvalid;
  return kOk;
}

// The rule on the host. out_index / out_gain have room for n entries each;
// *kept of them are written. kOk, kInvalid (validate) or kOom.
inline int distill_host(uint32_t n, const uint64_t *offsets, const uint64_t *values, const uint8_t *eligible,
                        uint32_t *out_index, uint32_t *out_gain, uint32_t *kept, uint64_t *universe) {
  if (const int rc = validate(n, offsets, values, out_index, out_gain, kept, universe)) return rc;
  *kept = 0;
  *universe = 0;
  if (n == 0) return kOk;
  try {
    // dense ids: the eligible sets' values sorted and deduplicated
    std::vector<uint64_t> uniq;
    for (uint32_t i = 0; i < n; i++)
      if (!eligible || eligible[i]) uniq.insert(uniq.end(), values + offsets[i], values + offsets[i + 1]);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    *universe = uniq.size();
    std::vector<uint32_t> ids(offsets[n]);
    std::priority_queue<uint64_t> heap;  // stale keys: each an upper bound on its set's key now
    for (uint32_t i = 0; i < n; i++) {
      if (eligible && !eligible[i]) continue;
      for (uint64_t j = offsets[i]; j < offsets[i + 1]; j++)
        ids[j] = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), values[j]) - uniq.begin());
      if (offsets[i + 1] > offsets[i]) heap.push(make_key((uint32_t)(offsets[i + 1] - offsets[i]), i));
    }
    std::vector<uint32_t> bitmap((uniq.size() + 31) / 32, 0);
    while (!heap.empty()) {
      const uint64_t top = heap.top();
      heap.pop();
      const uint32_t i = key_index(top);
      uint32_t gain = 0;
      for (uint64_t j = offsets[i]; j < offsets[i + 1]; j++) gain += !covered(bitmap.data(), ids[j]);
      if (gain == 0) continue;  // dead for good
      if (gain != key_gain(top)) {  // stale: every other key is at most `top`, so this one goes back
        heap.push(make_key(gain, i));
        continue;
      }
      // fresh and not below any other set's upper bound: the round's winner
      for (uint64_t j = offsets[i]; j < offsets[i + 1]; j++) bitmap[ids[j] >> 5] |= 1u << (ids[j] & 31);
      out_index[*kept] = i;
      out_gain[*kept] = gain;
      ++*kept;
    }
  } catch (const std::bad_alloc &) {
    *kept = 0;
    return kOom;
  }
  return kOk;
}

}  // namespace wtfdis
