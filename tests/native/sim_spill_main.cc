// sim_spill_main.cc — TEST INFRASTRUCTURE ONLY: the spill scenario of
// tests/test_spill_cpu.py as a program of its own, so that the harness (and
// the engine's allocation, lookup and release code under it) can be built and
// run with -fsanitize=address,undefined on the host.
//
//   sim_spill_main <snapshot> <rdi> <store_rip> <done_rip>
// snapshot: u64 npages, u64 gpfns[npages], pages, wtfgpu_regs_t (written by the
// test). The guest loop stores rsi + address to rcx pages from rdi at a 4 KB
// stride and sums them into rax (tests/spill_lib.py).
#include <cstdio>
#include "sim_spill.cc"

static int fails;
#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
      fails++;                                           \
    }                                                    \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t npages = 0;
  if (fread(&npages, 8, 1, f) != 1) return 2;
  std::vector<uint64_t> gpfns(npages);
  std::vector<uint8_t> pages(npages * 4096);
  wtfgpu_regs_t r0;
  if (fread(gpfns.data(), 8, npages, f) != npages || fread(pages.data(), 4096, npages, f) != npages ||
      fread(&r0, sizeof(r0), 1, f) != 1)
    return 2;
  fclose(f);
  const uint64_t rdi = strtoull(argv[2], nullptr, 0), store_rip = strtoull(argv[3], nullptr, 0),
                 done_rip = strtoull(argv[4], nullptr, 0);
  const uint32_t K = 2, X = 6;
  const uint32_t ms[] = {0, 1, K, K + 1, K + X, K + X + 1};
  const uint32_t n = sizeof(ms) / sizeof(ms[0]);
  for (int pool = 1; pool >= 0; pool--) {  // with the pool, then without
    SpillSim *h = spill_sim_create(gpfns.data(), pages.data(), npages, &r0, n, K, pool ? 16 : 0, X);
    const uint32_t cap = pool ? K + X : K;
    for (int round = 0; round < 2; round++) {
      uint64_t demand = 0;
      for (uint32_t l = 0; l < n; l++) {
        const uint64_t seed = 0x1000 * round + 0x10 * l + 1;
        SpillLaneOut o;
        spill_sim_run(h, l, rdi, ms[l], seed, &o);
        const uint32_t got = ms[l] < cap ? ms[l] : cap;
        demand += got > K ? got - K : 0;
        uint64_t sum = 0;
        for (uint32_t i = 0; i < ms[l]; i++) sum += seed + rdi + 0x1000ull * i;
        if (ms[l] <= cap) {
          CHECK(o.status == WTFGPU_EXIT_INT3 && o.rip == done_rip && o.gpr[0] == sum);
        } else {
          CHECK(o.status == WTFGPU_EXIT_OVERLAY_FULL && o.rip == store_rip && o.gpr[8] == ms[l] - cap);
        }
        CHECK(o.ovn == got);
        uint64_t dirty[16];
        CHECK(spill_sim_dirty(h, l, dirty, 16) == got);
        for (uint32_t i = 0; i < got; i++) {  // every dirty page: the stored word, the snapshot's bytes around it
          uint8_t pg[4096];
          spill_sim_page(h, l, dirty[i], pg);
          uint64_t w;
          memcpy(&w, pg + (rdi & 0xfff), 8);
          CHECK(w == seed + rdi + 0x1000ull * i);
        }
      }
      uint64_t st[5];
      CHECK(spill_sim_stats(h, st) == demand && st[0] == demand && st[3] == 0);
      for (uint32_t l = 0; l < n; l++) spill_sim_restore(h, l);
      CHECK(spill_sim_stats(h, st) == 0 && st[0] == 0);
    }
    spill_sim_destroy(h);
  }
  if (fails) return 1;
  puts("ok");
  return 0;
}
