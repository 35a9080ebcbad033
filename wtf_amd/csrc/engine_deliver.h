// engine_deliver.h — exception delivery through the guest IDT (U11 / U18):
// k_run's step loop delivers a lane's fault with it, and so does the host
// build of the lane code (tests/native/sim_lane.cc).
#pragma once
#include "engine_fast.h"

namespace wtfgpu_dev {

// One aligned 64-bit word at gpa (copy-on-write + dirty).
__device__ __forceinline__ bool lane_phys_write64(const Dev &P, Lane &L, u64 gpa, u64 v) {
  bool priv;
  const u8 *pg = phys_page(P, L.lane, L.ovn, L.bloom, gpa >> 12, priv);
  u8 *dst = (u8 *)pg;
  if (!priv) {
    dst = ov_alloc(P, L.lane, L.ovn);
    if (!dst) return false;
    cow_copy(P, L.lane, L.ovn, gpa >> 12, pg, dst);
    L.ovn++;
    L.bloom |= bloom_bit(gpa >> 12);
  }
  *(u64 *)(dst + (gpa & 0xfff)) = v;
  return true;
}

// ---------------------------------------------------------------- exception delivery
// A fault is delivered through the guest IDT when the snapshot has a present
// 64-bit interrupt / trap gate for it (SDM vol. 3 6.12-6.14): stack switch to
// TSS.RSP0 / IST on a privilege change, SS:RSP, RFLAGS, CS:RIP and the error
// code pushed, IF cleared for interrupt gates, cr2 set for #PF. Otherwise (no
// IDT: the ring-3 snapshots; a nested fault while delivering) the lane exits
// with the fault as before.
__device__ __forceinline__ bool has_error_code(u32 vec) {
  return vec == 8 || (vec >= 10 && vec <= 14) || vec == 17 || vec == 21 || vec == 29 || vec == 30;
}
__device__ __forceinline__ bool sup_xlate(const Dev &P, Lane &L, u64 va, int acc, u64 &gpa) {
  u64 td, gpfn;
  if (!walk(P, L, va, acc, td, gpfn)) return false;
  gpa = (gpfn << 12) | (va & 0xfff);
  return true;
}
__device__ __noinline__ bool deliver_fault(const Dev &P, Lane &L) {
  LaneSys &S = P.sys[L.lane];
  const u32 vec = L.exvec, err = L.exerr;
  const u64 cr2 = L.exaddr, frip = L.rip;
  const u32 st0 = L.status, cpl0 = L.cpl;
  bool ok = false;
  do {
    // a fault before any instruction retired since the last delivery (the
    // handler itself faults at once) ends as an exit: the double / triple fault
    // a CPU would raise (U18)
    if (S.deliv_icount == L.icount) break;
    if (!S.idtr || vec > 31 || (u64)vec * 16 + 15 > S.idtr_limit) break;
    u64 ga;
    if (!sup_xlate(P, L, S.idtr + vec * 16, ACC_R, ga) || (ga & 0xfff) > 4096 - 16) break;
    bool priv;
    const u8 *g = phys_page(P, L.lane, L.ovn, L.bloom, ga >> 12, priv) + (ga & 0xfff);
    const u64 lo = *(const u64 *)g, hi = *(const u64 *)(g + 8);
    const u32 attr = (u32)(lo >> 40) & 0xff, type = attr & 0xf, ist = (u32)(lo >> 32) & 7;
    if (!(attr & 0x80) || (type != 0xe && type != 0xf)) break;
    const u64 target = (lo & 0xffff) | ((lo >> 32) & 0xffff0000ull) | (hi << 32);
    const u16 sel = (u16)((lo >> 16) & 0xffff);
    const u32 ncpl = sel & 3;
    if (!canonical(target) || ncpl > L.cpl) break;
    u64 rsp = R(L, 4);
    if (ist || ncpl < L.cpl) {  // TSS64: RSP0 at +4, IST1 at +0x24
      const u64 off = ist ? 0x24 + (u64)(ist - 1) * 8 : 4 + (u64)ncpl * 8;
      u64 ta;
      if (!sup_xlate(P, L, S.tss + off, ACC_R, ta) || (ta & 0xfff) > 4096 - 8) break;
      const u8 *t = phys_page(P, L.lane, L.ovn, L.bloom, ta >> 12, priv) + (ta & 0xfff);
      u64 v = 0;
      for (int i = 0; i < 8; i++) v |= (u64)t[i] << (8 * i);
      rsp = v;
    }
    rsp &= ~0xfull;
    const bool ec = has_error_code(vec);
    const u32 n = ec ? 6 : 5;
    const u64 ors = R(L, 4), orfl = L.rflags, ocs = S.cs, oss = S.ss;
    L.cpl = 0;  // implicit supervisor accesses
    bool wr = true;
    // frame words, lowest address first: [error], rip, cs, rflags, rsp, ss
    for (u32 i = 0; i < n && wr; i++) {
      const u32 k = ec ? i : i + 1;
      const u64 w = k == 0 ? (u64)err : k == 1 ? frip : k == 2 ? ocs : k == 3 ? orfl : k == 4 ? ors : oss;
      u64 pa;
      wr = sup_xlate(P, L, rsp - 8 * n + 8 * i, ACC_W, pa) && (pa & 7) == 0 && lane_phys_write64(P, L, pa, w);
    }
    if (!wr) break;
    if (ncpl < cpl0) S.ss = (u16)ncpl;  // SS := NULL selector at the new privilege level
    set_cs(L, S, sel);
    if (vec == WTFGPU_VEC_PF) S.cr2 = cr2;
    L.cpl = S.cpl = ncpl;
    S.deliv_icount = L.icount;
    RS(L, 4, rsp - 8 * n);
    L.rflags &= ~(0x100ull | 0x4000ull | 0x10000ull | 0x20000ull | (type == 0xe ? 0x200ull : 0));
    L.rip = target;
    L.status = WTFGPU_RUNNING;
    // the frame pushes may have copied the stack page and the cpl changed:
    // drop cached translations now (the handler may run in the fast loop)
    tlb_flush(L);
    L.flush = 0;
    ok = true;
  } while (0);
  if (!ok) {  // keep the original fault
    L.cpl = cpl0;
    L.status = st0;
    L.exvec = vec;
    L.exerr = err;
    L.exaddr = cr2;
    L.nodeliver = 1;
  }
  return ok;
}

}  // namespace wtfgpu_dev
