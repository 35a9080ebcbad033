// sim_covkeep_main.cc — TEST INFRASTRUCTURE ONLY: a stand-alone program over
// tests/native/sim_covkeep.cc for tests/test_minimize_coverage.py, which also
// builds it with -fsanitize=address,undefined (every table, set and target in
// a heap buffer of exactly its size). It reads cases from the file named on
// the command line and prints one line a case:
//   <missing by the table probe> <missing by the sorted lists> <present bits as 0/1>
//
// A case: u32 H, u32 g, u32 ns, u32 nt, H u64 rip slots, H u32 gen slots, ns
// u64 sorted unique values of the set, nt u64 sorted unique target values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

extern "C" uint32_t sim_covkeep_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g,
                                      const uint64_t *t, uint32_t nt, uint8_t *present);
extern "C" uint64_t sim_covkeep_sorted(const uint64_t *s, uint64_t ns, const uint64_t *t, uint64_t nt);

template <typename T>
static T *read_array(FILE *f, size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (count && fread(p, sizeof(T), count, f) != count) exit(2);
  return p;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t h[4];
  while (fread(h, 4, 4, f) == 4) {
    const uint32_t H = h[0], g = h[1], ns = h[2], nt = h[3];
    uint64_t *rip = read_array<uint64_t>(f, H);
    uint32_t *gen = read_array<uint32_t>(f, H);
    uint64_t *s = read_array<uint64_t>(f, ns);
    uint64_t *t = read_array<uint64_t>(f, nt);
    uint8_t *present = (uint8_t *)malloc(nt ? nt : 1);
    const uint32_t m = sim_covkeep_table(rip, gen, H, g, t, nt, present);
    printf("%u %llu ", m, (unsigned long long)sim_covkeep_sorted(s, ns, t, nt));
    for (uint32_t i = 0; i < nt; i++) putchar('0' + present[i]);
    putchar('\n');
    free(rip), free(gen), free(s), free(t), free(present);
  }
  fclose(f);
  return 0;
}
