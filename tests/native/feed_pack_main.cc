// feed_pack_main.cc — TEST INFRASTRUCTURE ONLY: the layout rule of the packed
// feed read-back (wtf_amd/csrc/engine_feedpack.h) as a program of its own, so
// that the host build of what k_feed_lens / k_feed_pack compute can be compared
// with tests/test_feed_pack.py's restatement and run under
// -fsanitize=address,undefined.
//
//   feed_pack_main pack <cases> <out>
// cases: u32 n, u32 lens[n], then the bytes of every lane whose len is not
// ~0u, in list order. Every array lives in a heap block of exactly its size
// (the lens, the offsets, each lane's bytes, the output of exactly `total`
// bytes, filled with 0xCC first), so a read or a write outside one is
// reported. out: u64 total, u64 offs[n], the bytes.
//
//   feed_pack_main lens <n> <len>
// n lanes of `len` bytes, lengths only: prints the last offset and the total.
//
//   feed_pack_main words
// chunk_len, whole_len and mask_word over their edge values, one line each.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../wtf_amd/csrc/engine_feedpack.h"

namespace fp = wtffeedpack;

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }
template <typename T>
static T *block(size_t count) {
  return (T *)malloc(count ? count * sizeof(T) : 1);
}

static int do_pack(const char *cases, const char *out_path) {
  FILE *f = fopen(cases, "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (!rd(f, &n, 4)) return 2;
  uint32_t *lens = block<uint32_t>(n);
  if (!rd(f, lens, (size_t)n * 4)) return 2;
  const uint8_t **src = block<const uint8_t *>(n);
  for (uint32_t i = 0; i < n; i++) {
    src[i] = nullptr;
    if (lens[i] == fp::kNoFeed || lens[i] == 0) continue;
    uint8_t *p = block<uint8_t>(lens[i]);
    if (!rd(f, p, lens[i])) return 2;
    src[i] = p;
  }
  fclose(f);
  uint64_t *offs = block<uint64_t>(n), *offs2 = block<uint64_t>(n);
  const uint64_t total = fp::offsets(lens, n, offs);
  uint8_t *out = block<uint8_t>(total);
  memset(out, 0xCC, total);
  if (fp::pack(lens, src, n, offs2, out) != total || (n && memcmp(offs, offs2, (size_t)n * 8))) {
    fprintf(stderr, "pack and offsets disagree\n");
    return 1;
  }
  FILE *o = fopen(out_path, "wb");
  if (!o) return 2;
  fwrite(&total, 8, 1, o);
  if (n) fwrite(offs, 8, n, o);
  if (total) fwrite(out, 1, total, o);
  fclose(o);
  for (uint32_t i = 0; i < n; i++) free((void *)src[i]);
  free(out);
  free(offs2);
  free(offs);
  free(src);
  free(lens);
  puts("ok");
  return 0;
}

static int do_lens(uint64_t n, uint32_t len) {
  uint32_t *lens = block<uint32_t>(n);
  uint64_t *offs = block<uint64_t>(n);
  for (uint64_t i = 0; i < n; i++) lens[i] = len;
  const uint64_t total = fp::offsets(lens, n, offs);
  printf("%llu %llu\nok\n", (unsigned long long)(n ? offs[n - 1] : 0), (unsigned long long)total);
  free(offs);
  free(lens);
  return 0;
}

static int do_words() {
  const uint64_t stride = 16384;
  for (uint32_t w : {0u, 1u, 16379u, 16380u, 16381u, 0x7fffffffu, 0xffffffffu})
    printf("chunk %u %u %u\n", w, fp::chunk_len(true, w, stride), fp::chunk_len(false, w, stride));
  const uint64_t region = 5 * stride;
  for (uint64_t e : {region, region + 1, region + stride - 1, region + stride, region + stride + 1, region + 3 * stride})
    printf("whole %llu %u %u\n", (unsigned long long)(e - region), fp::whole_len(true, e, region, stride),
           fp::whole_len(false, e, region, stride));
  for (uint32_t len : {0u, 1u, 2u, 3u, 4u, 5u, 16u, 17u})
    for (uint32_t at : {0u, 4u, 12u, 16u})
      printf("mask %u %u %08x\n", len, at, fp::mask_word(0xA1B2C3D4u, at, len));
  for (uint32_t v : {0u, 1u, 15u, 16u, 17u, 16383u, 16384u, 0xfffffff0u, 0xfffffffeu, 0xffffffffu})
    printf("pad %u %llu\n", v, (unsigned long long)fp::pad16(v));
  puts("ok");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "pack")) return do_pack(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "lens")) return do_lens(strtoull(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0));
  if (argc == 2 && !strcmp(argv[1], "words")) return do_words();
  return 2;
}
