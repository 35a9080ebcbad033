// sim_mutate_main.cc — TEST INFRASTRUCTURE ONLY: the cases of
// tests/test_device_mutate.py's model comparison as a program of its own, so
// that the host build of the device mutator (wtf_amd/csrc/engine_mutate.h) can
// run under -fsanitize=address,undefined.
//
//   sim_mutate_main <cases> <seed> <count>
// cases: u32 ncorpora, then per corpus u32 entries, u64 off[entries + 1], the
// bytes; then u32 nmax, u32 max_len[nmax]; u32 nnc, u32 ncorpus[nnc]. For every
// (corpus, max_len, ncorpus) the indices [0, count) are generated. The arena
// holds exactly the first ncorpus entries and the output exactly max_len
// bytes, each in a heap block of its own, so a read or a write outside either
// is reported. Prints, per case, the checksum sum((D[k] + 1) * (k + 1) * G) mod
// 2^64 over the case's stream D of u32 sizes and bytes (G = 0x9E3779B97F4A7C15),
// which the test compares with the model's, then "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim_mutate.cc"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint64_t seed = strtoull(argv[2], nullptr, 0);
  const uint32_t count = (uint32_t)strtoul(argv[3], nullptr, 0);
  uint32_t ncorpora = 0;
  if (!rd(f, &ncorpora, 4)) return 2;
  std::vector<std::vector<uint64_t>> offs(ncorpora);
  std::vector<std::vector<uint8_t>> data(ncorpora);
  for (uint32_t c = 0; c < ncorpora; c++) {
    uint32_t entries = 0;
    if (!rd(f, &entries, 4)) return 2;
    offs[c].resize(entries + 1);
    if (!rd(f, offs[c].data(), 8 * (entries + 1))) return 2;
    data[c].resize(offs[c].back());
    if (!rd(f, data[c].data(), data[c].size())) return 2;
  }
  uint32_t nmax = 0, nnc = 0;
  std::vector<uint32_t> max_lens, ncs;
  if (!rd(f, &nmax, 4)) return 2;
  max_lens.resize(nmax);
  if (!rd(f, max_lens.data(), 4 * nmax) || !rd(f, &nnc, 4)) return 2;
  ncs.resize(nnc);
  if (!rd(f, ncs.data(), 4 * nnc)) return 2;
  fclose(f);

  uint64_t h = 0, k = 0;
  const auto mixin = [&h, &k](const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) h += (uint64_t)(p[i] + 1) * (++k * 0x9E3779B97F4A7C15ull);
  };
  for (uint32_t c = 0; c < ncorpora; c++)
    for (uint32_t max_len : max_lens)
      for (uint32_t nc : ncs) {
        // exact-size copies: the arena of the first nc entries, nc + 1 offsets
        h = k = 0;
        const uint64_t used = offs[c][nc];
        uint8_t *arena = (uint8_t *)malloc(used ? used : 1);
        uint64_t *off = (uint64_t *)malloc(8 * (nc + 1));
        uint8_t *out = (uint8_t *)malloc(max_len);
        memcpy(arena, data[c].data(), used);
        memcpy(off, offs[c].data(), 8 * (nc + 1));
        for (uint64_t i = 0; i < count; i++) {
          uint32_t len = 0;
          sim_mutate_many(seed, &i, 1, arena, off, nc, max_len, out, max_len, &len, nullptr);
          if (len > max_len) {
            fprintf(stderr, "index %llu: %u bytes > max_len %u\n", (unsigned long long)i, len, max_len);
            return 1;
          }
          mixin((const uint8_t *)&len, 4);
          mixin(out, len);
        }
        free(out);
        free(off);
        free(arena);
        printf("%016llx\n", (unsigned long long)h);
      }
  puts("ok");
  return 0;
}
