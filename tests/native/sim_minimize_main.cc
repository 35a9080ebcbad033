// sim_minimize_main.cc — TEST INFRASTRUCTURE ONLY: a stand-alone program over
// tests/native/sim_minimize.cc for the sanitizer run of tests/test_minimize.py
// (-fsanitize=address,undefined; every base and every result in a heap buffer
// of exactly its size). It reads cases from the file named on its command
// line and prints, per case, the count of candidates and the CRC-32 (zlib's)
// of the stream of little-endian u32 sizes and bytes.
//
// A case: u32 kind (0 byte buffer, 1 feed), u32 op, u32 len, u32 nidx, the
// base's bytes, then nidx u64 indices; nidx == 0xffffffff: every index.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
uint64_t sim_min_total(uint32_t U);
void sim_min_bytes(const uint8_t *base, uint32_t U, uint32_t op, const uint64_t *indices, uint32_t n, uint8_t *out,
                   uint64_t stride, uint32_t *lens);
int sim_min_feed(const uint8_t *feed, uint32_t len, const uint64_t *indices, uint32_t n, uint8_t *out, uint64_t stride,
                 uint32_t *lens);
}

static uint32_t crc_table[256];
static uint32_t crc32(uint32_t crc, const uint8_t *p, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; i++) crc = crc_table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    crc_table[i] = c;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t h[4];
  while (fread(h, 4, 4, f) == 4) {
    const uint32_t kind = h[0], op = h[1], len = h[2];
    uint8_t *base = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(base, 1, len, f) != len) return 2;
    std::vector<uint64_t> idx;
    uint32_t units = len;
    if (kind == 1) {  // a first call with no index gives the packet count
      const int P = sim_min_feed(base, len, nullptr, 0, nullptr, 0, nullptr);
      if (P < 0) return 3;
      units = (uint32_t)P;
    }
    if (h[3] == 0xffffffffu) {
      for (uint64_t i = 0; i < sim_min_total(units); i++) idx.push_back(i);
    } else {
      idx.resize(h[3]);
      if (h[3] && fread(idx.data(), 8, h[3], f) != h[3]) return 2;
    }
    uint32_t crc = 0;
    for (uint64_t i : idx) {  // one at a time: the result lands in a buffer of exactly its size
      uint32_t n = 0;
      uint8_t *out = (uint8_t *)malloc(len ? len : 1);
      if (kind == 1) sim_min_feed(base, len, &i, 1, out, len, &n);
      else sim_min_bytes(base, len, op, &i, 1, out, len, &n);
      uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
      memcpy(exact, out, n);
      const uint8_t sz[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
      crc = crc32(crc32(crc, sz, 4), exact, n);
      free(exact);
      free(out);
    }
    printf("%zu %08x\n", idx.size(), crc);
    free(base);
  }
  fclose(f);
  return 0;
}
