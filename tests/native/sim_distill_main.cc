// sim_distill_main.cc — TEST INFRASTRUCTURE ONLY: a stand-alone program over
// tests/native/sim_distill.cc for tests/test_distill.py, which also builds it
// with -fsanitize=address,undefined (every buffer on the heap, of exactly its
// size). It reads cases from stdin and prints one line a case:
//   <rc> <universe> <kept> <index>:<gain> ...
//
// A case: u32 n, u32 flags (bit 0: an eligible array follows), n + 1 u64
// offsets, offsets[n] u64 values, then n eligible bytes if flagged.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

extern "C" int sim_distill(uint32_t n, const uint64_t *offsets, const uint64_t *values, const uint8_t *eligible,
                           uint32_t *out_index, uint32_t *out_gain, uint32_t *kept, uint64_t *universe);

template <typename T>
static T *read_array(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (count && fread(p, sizeof(T), count, stdin) != count) exit(2);
  return p;
}

int main() {
  uint32_t h[2];
  while (fread(h, 4, 2, stdin) == 2) {
    const uint32_t n = h[0];
    uint64_t *off = read_array<uint64_t>((size_t)n + 1);
    uint64_t *val = read_array<uint64_t>(off[n]);
    uint8_t *el = (h[1] & 1) ? read_array<uint8_t>(n) : nullptr;
    uint32_t *index = (uint32_t *)malloc(n ? n * 4 : 1), *gain = (uint32_t *)malloc(n ? n * 4 : 1);
    uint32_t kept = 0;
    uint64_t universe = 0;
    const int rc = sim_distill(n, off, val, el, index, gain, &kept, &universe);
    printf("%d %llu %u", rc, (unsigned long long)universe, kept);
    for (uint32_t k = 0; k < kept; k++) printf(" %u:%u", index[k], gain[k]);
    printf("\n");
    free(off), free(val), free(el), free(index), free(gain);
  }
  return 0;
}
