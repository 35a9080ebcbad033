// engine_ptmark.h — host only: the bitmap over guest frames that says which
// of them are page-table pages of the snapshot (Dev::ptbits; a guest write to
// one drops the lane's cached translations, engine_exec.h vwrite). Walks the
// tables reachable from the initial cr3 on a host copy of the pool. Called by
// engine.hip (mark_pt_pages) and by the host build of the device code
// (tests/native/sim_lane.cc), so both run on the same marking.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace wtfgpu_host {

// page(gpfn): the frame's 4096 bytes in the snapshot, or nullptr when the
// snapshot does not hold it. maplen: frames the bitmap covers (the pfn map's
// length); a frame past it is never marked. A large leaf's frames are data.
template <typename PageFn>
inline std::vector<uint32_t> mark_pt_bits(uint64_t cr3, uint64_t maplen, PageFn page) {
  std::vector<uint32_t> bits((maplen + 31) / 32, 0);
  auto mark = [&](uint64_t gpfn) {
    if (gpfn < maplen) bits[gpfn >> 5] |= 1u << (gpfn & 31);
  };
  std::vector<std::pair<uint64_t, int>> work;
  work.push_back({cr3 >> 12 & 0xffffffffffull, 3});
  while (!work.empty()) {
    auto [pfn, level] = work.back();
    work.pop_back();
    if (pfn < maplen && (bits[pfn >> 5] >> (pfn & 31)) & 1) continue;
    mark(pfn);
    const uint8_t *pg = page(pfn);
    if (!pg || level == 0) continue;
    for (int i = 0; i < 512; i++) {
      uint64_t e;
      memcpy(&e, pg + 8 * i, 8);
      if (!(e & 1)) continue;
      if ((level == 1 || level == 2) && (e & 0x80)) continue;  // large leaf
      work.push_back({(e & 0x000ffffffffff000ull) >> 12, level - 1});
    }
  }
  return bits;
}

}  // namespace wtfgpu_host
