// sim_spill.cc — TEST INFRASTRUCTURE ONLY: several lanes of the interpreter's
// slow step (code translation, decode, exec with miss / retry, retire: the
// path that allocates copy-on-write pages) over ONE spill pool, built for the
// host. The lanes run one after another, so the pool's atomics are the plain
// host forms of engine_exec.h; what is checked here is the bookkeeping —
// which slot a page takes, the extension lists, lookups through them, the
// cap, the counters, and that restore gives every page back.
#include <cstdlib>
#include <vector>
#include "../../wtf_amd/csrc/engine_fast.h"
using namespace wtfgpu_dev;

struct SpillSim {
  uint8_t *pool = nullptr, *ov = nullptr, *sp = nullptr;
  std::vector<uint32_t> map, ptbits, ovg, ovc, ovxp, spmap;
  std::vector<uint64_t> fsb, gsb;
  std::vector<unsigned long long> stat;
  std::vector<wtfgpu_regs_t> full;
  std::vector<LaneSys> sys;
  wtfgpu_regs_t r0;
  LaneSys sys0;
  uint64_t S = 0;
  Dev P{};
};

extern "C" {

struct SpillLaneOut {
  uint64_t gpr[16], rip, rflags, icount;
  uint32_t status, ovn;
};

// K private pages per lane, a pool of S pages, X of them per lane at most
// (S == 0: no pool, as the engine without wtfgpu_alloc_spill).
SpillSim *spill_sim_create(const uint64_t *gpfns, const uint8_t *pages, uint64_t npages, const wtfgpu_regs_t *r0,
                           uint32_t nlanes, uint32_t K, uint64_t S, uint32_t X) {
  SpillSim *h = new SpillSim;
  uint64_t maxpfn = 0;
  for (uint64_t i = 0; i < npages; i++) maxpfn = gpfns[i] > maxpfn ? gpfns[i] : maxpfn;
  // page pointers carry flags in their low 12 bits: storage must be 4 KiB aligned
  h->pool = (uint8_t *)aligned_alloc(4096, (npages + 1) * 4096);
  memset(h->pool, 0, 4096);
  memcpy(h->pool + 4096, pages, npages * 4096);
  h->map.assign(maxpfn + 1, 0);
  for (uint64_t i = 0; i < npages; i++) if (!h->map[gpfns[i]]) h->map[gpfns[i]] = (uint32_t)(i + 1);
  h->ptbits.assign((maxpfn + 32) / 32, 0);
  if (!S) X = 0;
  const uint64_t N = nlanes;
  h->ov = (uint8_t *)aligned_alloc(4096, N * K * 4096);
  h->ovg.assign((uint64_t)(K + X) * N, 0);  // K rows, then the extension rows (engine.hip wtfgpu_alloc_spill)
  h->ovc.assign(N, 0);
  h->fsb.assign(N, r0->seg[WTFGPU_FS].base);
  h->gsb.assign(N, r0->seg[WTFGPU_GS].base);
  h->full.assign(N, *r0);
  h->r0 = *r0;
  LaneSys s{};  // as engine.hip make_init
  s.cr0 = r0->cr0;
  s.cr3 = r0->cr3;
  s.cr4 = r0->cr4;
  s.efer = (r0->efer & ~EFER_M32) | (compat_sel(r0->star, r0->seg[WTFGPU_CS].selector) ? EFER_M32 : 0);
  s.cpl = r0->seg[WTFGPU_CS].selector & 3;
  s.star = r0->star;
  s.lstar = r0->lstar;
  s.sfmask = r0->sfmask;
  s.kgs = r0->kernel_gs_base;
  s.cs = r0->seg[WTFGPU_CS].selector;
  s.ss = r0->seg[WTFGPU_SS].selector;
  s.idtr = r0->idtr_base;
  s.idtr_limit = r0->idtr_limit;
  s.tss = r0->seg[WTFGPU_TR].base;
  s.cr2 = r0->cr2;
  s.deliv_icount = ~0ull;
  h->sys0 = s;
  h->sys.assign(N, s);
  Dev &P = h->P;
  P.pool = h->pool;
  P.pfn_map = h->map.data();
  P.pfn_map_len = h->map.size();
  P.ptbits = h->ptbits.data();
  P.nlanes = nlanes;
  P.K = K;
  P.ov_count = h->ovc.data();
  P.ov_gpfn = h->ovg.data();
  P.ov_data = h->ov;
  P.fs_base = h->fsb.data();
  P.gs_base = h->gsb.data();
  P.full = h->full.data();
  P.sys = h->sys.data();
  if (S) {
    h->S = S;
    h->sp = (uint8_t *)aligned_alloc(4096, S * 4096);
    memset(h->sp, 0xee, S * 4096);  // a page read before its copy shows
    const uint64_t words = (S + 31) / 32;
    h->spmap.assign(words, 0);
    if (S & 31) h->spmap[words - 1] = ~0u << (S & 31);
    h->ovxp.assign((uint64_t)X * N, 0);
    h->stat.assign(SP_NSTAT, 0);
    P.X = X;
    P.sp_words = (uint32_t)words;
    P.sp_data = h->sp;
    P.sp_map = h->spmap.data();
    P.ovx_gpfn = h->ovg.data() + (uint64_t)K * N;
    P.ovx_page = h->ovxp.data();
    P.sp_stat = h->stat.data();
  }
  return h;
}

void spill_sim_destroy(SpillSim *h) {
  free(h->pool);
  free(h->ov);
  free(h->sp);
  delete h;
}

// What restore_lane does to the lane's memory and state (engine_kernels.h).
void spill_sim_restore(SpillSim *h, uint32_t lane) {
  const Dev &P = h->P;
  spill_release(P, lane, P.ov_count[lane]);
  P.ov_count[lane] = 0;
  h->full[lane] = h->r0;
  h->sys[lane] = h->sys0;
}

// One testcase on a restored lane: the initial state with rdi, rcx, rsi set.
void spill_sim_run(SpillSim *h, uint32_t lane, uint64_t rdi, uint64_t rcx, uint64_t rsi, SpillLaneOut *out) {
  const Dev &P = h->P;
  const wtfgpu_regs_t *r0 = &h->r0;
  uint32_t glo[16], ghi[16];
  Lane L{};
  L.glo = glo;
  L.ghi = ghi;
  for (int i = 0; i < 16; i++) RS(L, i, r0->gpr[i]);
  RS(L, 7, rdi);
  RS(L, 1, rcx);
  RS(L, 6, rsi);
  L.rip = r0->rip;
  L.rflags = r0->rflags;
  L.cr0 = r0->cr0;
  L.cr3 = r0->cr3;
  L.efer = h->sys0.efer;
  L.cpl = h->sys0.cpl;
  L.status = WTFGPU_RUNNING;
  L.simd = simd_bits(r0->cr0, r0->cr4, r0->xcr0);
  L.lane = lane;
  L.ovn = P.ov_count[lane];
  tlb_flush(L);
  for (uint64_t steps = 0; steps < 1000000 && L.status == WTFGPU_RUNNING; steps++) {
    const uint64_t grip = L.rip;
    uint64_t td;
    if (!tlb_get(L, grip >> 12, td) || !perm_ok(L, td, ACC_X)) {
      if (service_miss(P, L, grip & ~0xfffull, ACC_X)) tlb_get(L, grip >> 12, td);
      else td = 0;
    }
    if (!td) break;
    const uint8_t *page = (const uint8_t *)(uintptr_t)(td & ~0xfffull);
    const uint32_t off = grip & 0xfff;
    IBytes ib;
    ib.avail = 4096 - off < 16 ? 4096 - off : 16;
    uint8_t bytes[16] = {0};
    memcpy(bytes, page + off, ib.avail);
    memcpy(&ib.lo, bytes, 8);
    memcpy(&ib.hi, bytes + 8, 8);
    UOp d;
    if (decode(ib, d, false) != 0 || !d.supported) {  // (the test's code sits inside one page)
      L.status = WTFGPU_EXIT_UNIMPLEMENTED;
      break;
    }
    uint64_t next = 0;
    int x;
    L.keep = 0;
    for (int attempt = 0;; attempt++) {
      L.miss = 0;
      L.pend = 0;
      x = exec(P, L, d, grip + d.len, next);
      if (!L.miss || L.status != WTFGPU_RUNNING) break;
      if (attempt >= 16 || !service_miss(P, L, L.miss_va, (int)L.miss_acc)) break;
    }
    if (L.flush) {
      tlb_flush(L);
      L.flush = 0;
    }
    if (x == X_OK && L.status == WTFGPU_RUNNING) {
      L.rip = next;
      L.icount++;
    } else if (L.status != WTFGPU_RUNNING) {
    } else if (x == X_UNIMPL) {
      L.status = WTFGPU_EXIT_UNIMPLEMENTED;
    } else if (x == X_INT3) {
      L.status = WTFGPU_EXIT_INT3;
    } else if (x == X_HLT) {
      L.status = WTFGPU_EXIT_HLT;
    }
  }
  P.ov_count[lane] = L.ovn;  // store_lane
  for (int i = 0; i < 16; i++) out->gpr[i] = R(L, i);
  out->rip = L.rip;
  out->rflags = L.rflags;
  out->icount = L.icount;
  out->status = L.status;
  out->ovn = L.ovn;
}

// The lane's dirty list (gpas), as k_gather_dirty reads it: one array, K + X rows.
uint32_t spill_sim_dirty(SpillSim *h, uint32_t lane, uint64_t *gpas, uint32_t cap) {
  const Dev &P = h->P;
  const uint32_t n = P.ov_count[lane];
  for (uint32_t k = 0; k < n && k < cap && k < P.K + P.X; k++)
    gpas[k] = (uint64_t)P.ov_gpfn[(uint64_t)k * P.nlanes + lane] << 12;
  return n;
}

// The lane's view of a physical page (k_gather_pages).
void spill_sim_page(SpillSim *h, uint32_t lane, uint64_t gpa, uint8_t *out) {
  const Dev &P = h->P;
  const uint32_t ovn = P.ov_count[lane];
  uint64_t bloom = 0;
  for (uint32_t k = 0; k < ovn; k++) bloom |= bloom_bit(P.ov_gpfn[(uint64_t)k * P.nlanes + lane]);
  bool priv;
  memcpy(out, phys_page(P, lane, ovn, bloom, gpa >> 12, priv), 4096);
}

// in use, peak, lanes spilled, pool-empty failures, claims; returns the number
// of bits set in the ownership bitmap for pages of the pool.
uint64_t spill_sim_stats(SpillSim *h, uint64_t *out5) {
  for (int i = 0; i < 5; i++) out5[i] = h->stat.empty() ? 0 : h->stat[i];
  uint64_t owned = 0;
  for (uint64_t p = 0; p < h->S; p++) owned += (h->spmap[p >> 5] >> (p & 31)) & 1;
  return owned;
}
}
