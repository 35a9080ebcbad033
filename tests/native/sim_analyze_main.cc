// sim_analyze_main.cc — TEST INFRASTRUCTURE ONLY: a stand-alone program over
// tests/native/sim_analyze.cc for the sanitizer run of tests/test_analyze.py
// (-fsanitize=address,undefined; every base, result, table and list in a heap
// buffer of exactly its size). It reads cases from the file named on its
// command line and prints one line a case.
//
// A case starts with four u32: kind, a, b, c.
//   kind 0  byte buffer: a = len, b = nidx; the bytes, nidx u64 indices
//           (nidx == 0xffffffff: every index). Prints the count of candidates
//           and the CRC-32 (zlib's) of their bytes, in order.
//   kind 1  feed: the same over a feed; then the framing map of its positions
//           as a string of 0 and 1.
//   kind 2  signature: a = H, b = g, c = nlive; rip[H] u64, gen[H] u32, the
//           live values as a list of nlive u64. Prints the table form's sum
//           and size, then the list form's.
//   kind 3  classes: a = count; count times five outcomes of (u32 kind, u32
//           name, u64 sig, u32 size, u32 overflow). Prints the classes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
uint64_t sim_ana_total(uint32_t U);
void sim_ana_bytes(const uint8_t *base, uint32_t U, const uint64_t *indices, uint32_t n, uint8_t *out, uint64_t stride);
int sim_ana_feed(const uint8_t *feed, uint32_t len, const uint64_t *indices, uint32_t n, uint8_t *out, uint64_t stride,
                 uint8_t *framing);
uint32_t sim_ana_sig_list(const uint64_t *v, uint64_t n, uint64_t *sum);
uint32_t sim_ana_sig_table(const uint64_t *rip, const uint32_t *gen, uint32_t H, uint32_t g, uint64_t *sum);
int sim_ana_classify(const uint32_t *kind, const uint32_t *name, const uint64_t *sig, const uint32_t *size,
                     const uint32_t *ovf);
}

static uint32_t crc_table[256];
static uint32_t crc32(uint32_t crc, const uint8_t *p, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; i++) crc = crc_table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}

template <typename T> static T *exact(FILE *f, size_t n) {  // n items in a buffer of exactly their size
  T *p = (T *)malloc(n ? n * sizeof(T) : 1);
  if (n && fread(p, sizeof(T), n, f) != n) exit(2);
  return p;
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
    if (h[0] <= 1) {
      const uint32_t len = h[1];
      uint8_t *base = exact<uint8_t>(f, len);
      std::vector<uint64_t> idx;
      if (h[2] == 0xffffffffu) {
        for (uint64_t i = 0; i < sim_ana_total(len); i++) idx.push_back(i);
      } else {
        idx.resize(h[2]);
        if (h[2] && fread(idx.data(), 8, h[2], f) != h[2]) return 2;
      }
      uint8_t *framing = (uint8_t *)malloc(len ? len : 1);
      memset(framing, 0, len);
      if (h[0] == 1 && sim_ana_feed(base, len, nullptr, 0, nullptr, 0, framing) < 0) return 3;
      uint32_t crc = 0;
      size_t made = 0;
      for (uint64_t i : idx) {  // one at a time: the result lands in a buffer of exactly its size
        if (framing[i >> 2]) continue;  // (every index of a feed: the framing ones are not candidates)
        uint8_t *out = (uint8_t *)malloc(len ? len : 1);
        if (h[0] == 1) sim_ana_feed(base, len, &i, 1, out, len, nullptr);
        else sim_ana_bytes(base, len, &i, 1, out, len);
        crc = crc32(crc, out, len);
        made++;
        free(out);
      }
      printf("%zu %08x", made, crc);
      if (h[0] == 1) {
        std::string s;
        for (uint32_t p = 0; p < len; p++) s += framing[p] ? '1' : '0';
        printf(" %s", s.c_str());
      }
      printf("\n");
      free(framing);
      free(base);
    } else if (h[0] == 2) {
      uint64_t *rip = exact<uint64_t>(f, h[1]);
      uint32_t *gen = exact<uint32_t>(f, h[1]);
      uint64_t *live = exact<uint64_t>(f, h[3]);
      uint64_t st = 0, sl = 0;
      const uint32_t nt = sim_ana_sig_table(rip, gen, h[1], h[2], &st);
      const uint32_t nl = sim_ana_sig_list(live, h[3], &sl);
      printf("%016llx %u %016llx %u\n", (unsigned long long)st, nt, (unsigned long long)sl, nl);
      free(rip);
      free(gen);
      free(live);
    } else if (h[0] == 3) {
      std::string s;
      for (uint32_t k = 0; k < h[1]; k++) {
        uint32_t kind[5], name[5], size[5], ovf[5];
        uint64_t sig[5];
        for (int j = 0; j < 5; j++) {
          uint32_t w[2], z[2];
          if (fread(w, 4, 2, f) != 2 || fread(&sig[j], 8, 1, f) != 1 || fread(z, 4, 2, f) != 2) return 2;
          kind[j] = w[0], name[j] = w[1], size[j] = z[0], ovf[j] = z[1];
        }
        s += (char)sim_ana_classify(kind, name, sig, size, ovf);
      }
      printf("%s\n", s.c_str());
    } else {
      return 2;
    }
  }
  fclose(f);
  return 0;
}
