// sim_packets_main.cc — TEST INFRASTRUCTURE ONLY: the cases of
// tests/test_device_packets.py's model comparison as a program of its own, so
// that the host build of the device packet mutator
// (wtf_amd/csrc/engine_mutate_packets.h) can run under
// -fsanitize=address,undefined.
//
//   sim_packets_main <cases> <seed> <count>
// cases: u32 entries, then per entry u32 len and the feed's bytes; u32
// params[6]; u32 nnc, u32 ncorpus[nnc]. For every ncorpus the indices [0, count)
// are generated. The entries are indexed here (entry_packets / entry_write, the
// gate wtfgpu_corpus_add_feed uses); the arena holds exactly the first ncorpus
// entries and the output exactly MaxFeed bytes, each in a heap block of its
// own, so a read or a write outside either is reported. Prints, per ncorpus,
// the checksum sum((D[k] + 1) * (k + 1) * G) mod 2^64 over the stream D of u32
// sizes and bytes (G = 0x9E3779B97F4A7C15), which the test compares with the
// model's, then "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim_packets.cc"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint64_t seed = strtoull(argv[2], nullptr, 0);
  const uint32_t count = (uint32_t)strtoul(argv[3], nullptr, 0);
  uint32_t entries = 0;
  if (!rd(f, &entries, 4)) return 2;
  uint32_t params[6];
  std::vector<uint8_t> arena;
  std::vector<uint64_t> offs{0};
  std::vector<std::vector<uint8_t>> feeds(entries);
  for (uint32_t e = 0; e < entries; e++) {
    uint32_t len = 0;
    if (!rd(f, &len, 4)) return 2;
    feeds[e].resize(len);
    if (!rd(f, feeds[e].data(), len)) return 2;
  }
  if (!rd(f, params, sizeof(params))) return 2;
  uint32_t nnc = 0;
  if (!rd(f, &nnc, 4)) return 2;
  std::vector<uint32_t> ncs(nnc);
  if (!rd(f, ncs.data(), 4 * nnc)) return 2;
  fclose(f);
  if (!sim_packets_params_valid(params)) return 2;
  for (uint32_t e = 0; e < entries; e++) {
    // the feed in an exact-size block of its own for the gate and the indexing
    const size_t len = feeds[e].size();
    uint8_t *feed = (uint8_t *)malloc(len ? len : 1);
    if (len) memcpy(feed, feeds[e].data(), len);
    const int64_t P = sim_packets_entry_packets(feed, len, params[5]);
    if (P < 0) {
      fprintf(stderr, "entry %u refused\n", e);
      return 1;
    }
    const uint64_t bytes = sim_packets_entry_bytes((uint64_t)P, len);
    uint8_t *entry = (uint8_t *)malloc(bytes);
    sim_packets_entry_write(feed, len, (uint64_t)P, entry);
    arena.insert(arena.end(), entry, entry + bytes);
    offs.push_back(arena.size());
    free(entry);
    free(feed);
  }

  uint64_t h = 0, k = 0;
  const auto mixin = [&h, &k](const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) h += (uint64_t)(p[i] + 1) * (++k * 0x9E3779B97F4A7C15ull);
  };
  for (uint32_t nc : ncs) {
    if (nc == 0 || nc > entries) return 2;
    h = k = 0;
    const uint64_t used = offs[nc];
    uint8_t *a = (uint8_t *)malloc(used);
    uint64_t *off = (uint64_t *)malloc(8 * (nc + 1));
    uint8_t *out = (uint8_t *)malloc(params[5]);
    memcpy(a, arena.data(), used);
    memcpy(off, offs.data(), 8 * (nc + 1));
    for (uint64_t i = 0; i < count; i++) {
      uint32_t len = 0;
      sim_packets_many(seed, &i, 1, a, off, nc, params, out, params[5], &len, nullptr);
      if (len > params[5]) {
        fprintf(stderr, "index %llu: %u bytes > MaxFeed %u\n", (unsigned long long)i, len, params[5]);
        return 1;
      }
      mixin((const uint8_t *)&len, 4);
      mixin(out, len);
    }
    free(out);
    free(off);
    free(a);
    printf("%016llx\n", (unsigned long long)h);
  }
  puts("ok");
  return 0;
}
