// engine_run.h — k_run, the step loop, and what only it uses: wave helpers,
// the decoded-uop cache, breakpoint actions, slow_step, WITH_LANE_COPY
// and the stamp macros of the diagnostic build.
//
// Device half of engine.hip, which stays the single translation unit (its
// host half launches these kernels); included nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include "engine_deliver.h"
#include "engine_fast.h"

using namespace wtfgpu_dev;

namespace {

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ u64 readlane64(u64 v, int l) {
  const u32 lo = __builtin_amdgcn_readlane((u32)v, l);
  const u32 hi = __builtin_amdgcn_readlane((u32)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}
// Lane masks straight from a compare (one v_cmp writing an SGPR pair), and a
// mask back to a per-lane condition (used as the exec mask as it is): the
// step loop tests and combines groups as masks, where a per-lane bool fed to
// __ballot costs a v_cndmask + v_cmp pair to become a mask again. Every lane
// of the wave runs the step loop, so a compare's mask is the ballot's.
__device__ __forceinline__ u64 m_eq32(u32 a, u32 b) { return __builtin_amdgcn_uicmp(a, b, 32); }
__device__ __forceinline__ u64 m_ne32(u32 a, u32 b) { return __builtin_amdgcn_uicmp(a, b, 33); }
__device__ __forceinline__ u64 m_eq64(u64 a, u64 b) { return __builtin_amdgcn_uicmpl(a, b, 32); }
__device__ __forceinline__ u64 m_ne64(u64 a, u64 b) { return __builtin_amdgcn_uicmpl(a, b, 33); }
__device__ __forceinline__ u64 m_lt64(u64 a, u64 b) { return __builtin_amdgcn_uicmpl(a, b, 36); }
__device__ __forceinline__ u64 m_ge64(u64 a, u64 b) { return __builtin_amdgcn_uicmpl(a, b, 35); }
__device__ __forceinline__ u64 m_ge32(u32 a, u32 b) { return __builtin_amdgcn_uicmp(a, b, 35); }
__device__ __forceinline__ bool in_mask(u64 m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

__device__ __forceinline__ bool hash_find(const u64 *keys, u32 mask, u64 key, u32 &slot) {
  u32 h = (u32)mix64(key) & mask;
  for (u32 i = 0; i <= mask; i++) {
    const u64 k = rfl64(keys[h]);
    if (k == key) {
      slot = h;
      return true;
    }
    if (k == EMPTY_KEY) return false;
    h = (h + 1) & mask;
  }
  return false;
}

// Per-lane (non-uniform) lookup in an open-addressing u64 set.
__device__ __forceinline__ bool set_has(const u64 *keys, u32 mask, u64 key) {
  u32 h = (u32)mix64(key) & mask;
  for (u32 i = 0; i <= mask; i++) {
    const u64 k = keys[h];
    if (k == key) return true;
    if (k == EMPTY_KEY) return false;
    h = (h + 1) & mask;
  }
  return false;
}

// Rip trace: the lane's next entry (the before-execution hook's trace write,
// bochscpu_backend.cc:506-520).
__device__ __forceinline__ void trace_rip(const Dev &P, u32 lane, u64 rip) {
  const u32 n = P.trace_cnt[lane];
  if (n < P.trace_cap) P.trace[(u64)lane * P.trace_cap + n] = rip;
  P.trace_cnt[lane] = n + 1;
}

// RecordEdge's key (bochscpu_backend.cc:699-728): splitmix64's finaliser of
// the branch's rip, xor the rip that follows it.
__device__ __forceinline__ u64 edge_key(u64 rip, u64 next) {
  u64 e = rip;
  e ^= e >> 30;
  e *= 0xbf58476d1ce4e5b9ull;
  e ^= e >> 27;
  e *= 0x94d049bb133111ebull;
  e ^= e >> 31;
  return e ^ next;
}

// The branches RecordEdge sees: conditional near branches taken or not
// (cnear_branch_taken / _not_taken) and indirect near jmp / call
// (ucnear_branch with JMP_INDIRECT / CALL_INDIRECT), :235-257.
__device__ __forceinline__ bool edge_op(u32 op, u32 bsrc) {
  return op == O_JCC || op == O_LOOP || ((op == O_JMP || op == O_CALL) && bsrc != L_IMM);
}

__device__ __forceinline__ void load_lane(const Dev &P, u32 lane, Lane &L) {
  const u64 N = P.nlanes;
#pragma unroll
  for (int i = 0; i < 16; i++) RS(L, i, P.gpr[i * N + lane]);
  L.rip = P.rip[lane];
  L.rflags = P.rflags[lane];
  L.icount = P.icount[lane];
  L.nbytes = P.nbytes[lane];
  L.status = P.status[lane];
  const LaneSys s = P.sys[lane];
  L.cr0 = s.cr0;
  L.cr3 = s.cr3;
  L.efer = s.efer;  // with the 32-bit-code bit (U29)
  L.cpl = s.cpl;
  L.simd = simd_bits(s.cr0, s.cr4, P.full[lane].xcr0);
  L.ovn = P.ov_count[lane];
  L.lane = lane;
  L.cgen = P.lane_gen ? P.lane_gen[lane] : 0;
  L.ccnt = P.cov_cnt ? P.cov_cnt[lane] : 0;
  if (P.tlb_ok && P.tlb_ok[lane]) {
    const LaneTlb &t = P.tlbs[lane];
#pragma unroll
    for (int i = 0; i < TLB_N; i++) {
      L.tv[i] = t.tv[i];
      L.td[i] = t.td[i];
    }
    L.cvpn = t.cvpn;
    L.cptr = t.cptr;
    L.bloom = t.bloom;
    L.tnext = t.tnext;
  } else {
    L.bloom = 0;
    for (u32 k = 0; k < L.ovn; k++) L.bloom |= bloom_bit(P.ov_gpfn[(u64)k * N + lane]);
    tlb_flush(L);
    L.tnext = 0;
  }
  L.exvec = L.exerr = L.exop = 0;
  L.exaddr = 0;
  L.miss = L.miss_acc = L.flush = L.pend = L.keep = 0;
  L.nodeliver = 0;
  L.miss_va = 0;
}

__device__ __forceinline__ void store_tlb(const Dev &P, const Lane &L) {
  if (!P.tlb_ok) return;
  LaneTlb &t = P.tlbs[L.lane];
#pragma unroll
  for (int i = 0; i < TLB_N; i++) {
    t.tv[i] = L.tv[i];
    t.td[i] = L.td[i];
  }
  t.cvpn = L.cvpn;
  t.cptr = L.cptr;
  t.bloom = L.bloom;
  t.tnext = L.tnext;
  P.tlb_ok[L.lane] = 1;
}
__device__ __forceinline__ void tlb_stale(const Dev &P, u32 lane) {
  if (P.tlb_ok) P.tlb_ok[lane] = 0;
}

__device__ __forceinline__ void store_lane(const Dev &P, const Lane &L) {
  const u64 N = P.nlanes;
  const u32 lane = L.lane;
#pragma unroll
  for (int i = 0; i < 16; i++) P.gpr[i * N + lane] = R(L, i);
  P.rip[lane] = L.rip;
  P.rflags[lane] = L.rflags;
  P.icount[lane] = L.icount;
  P.nbytes[lane] = L.nbytes;
  P.status[lane] = L.status;
  P.ov_count[lane] = L.ovn;
  if (P.cov_cnt) P.cov_cnt[lane] = L.ccnt;
}

__device__ __forceinline__ u32 log_value(const Dev &P, u64 v, bool mine, u32 lane, u32 gen, u32 cnt);

// Coverage (bochscpu_backend.cc:501-504): a rip absent from the aggregate map
// joins the set of every lane that ran it (`mine`). The map check is uniform;
// the set insert is per lane (its own open-addressing table, no contention
// whatever wave runs the lane). Returns the lane's new entry count.
__device__ __noinline__ u32 cover(const Dev &P, u64 rip, bool mine, u32 lane, u32 gen, u32 cnt) {
  if (P.code_keys) {
    u32 s;
    if (hash_find(P.code_keys, P.code_mask, rip >> 12, s)) {
      const u32 cs = rfl32(P.code_slot[s]);
      if (rfl32(P.cov_map[(u64)cs * WTFGPU_PAGE_SIZE + (rip & 0xfff)])) return cnt;
    } else if (P.extra_keys && set_has(P.extra_keys, P.extra_mask, rip)) {
      return cnt;
    }
  }
  return log_value(P, rip, mine, lane, gen, cnt);
}

// Run stats (BochscpuRunStats_t::NumberEdges / NumberUniqueEdges,
// bochscpu_backend.h:17-45): edges recorded, and those new to the lane's set.
__device__ __forceinline__ void count_edge(const Dev &P, u32 lane, bool fresh) {
  if (!P.edge_cnt) return;
  P.edge_cnt[2 * (u64)lane] += 1;
  if (fresh) P.edge_cnt[2 * (u64)lane + 1] += 1;
}

// A branch edge (per-lane value): logged unless the aggregate has it.
__device__ __noinline__ u32 cover_edge(const Dev &P, u64 e, bool mine, u32 lane, u32 gen, u32 cnt) {
  if (!mine) return cnt;
  if (P.extra_keys && set_has(P.extra_keys, P.extra_mask, e)) return cnt;
  return log_value(P, e, true, lane, gen, cnt);
}

__device__ __forceinline__ u32 log_value(const Dev &P, u64 rip, bool mine, u32 lane, u32 gen, u32 cnt) {
  if (!mine) return cnt;
  const u32 H = P.H;
  const u64 base = (u64)lane * H;
  u32 h = (u32)mix64(rip) & (H - 1);
  for (u32 probe = 0; probe < H; probe++) {
    const u64 idx = base + h;
    if (P.cov_gen[idx] != gen) {
      if (cnt >= H - H / 4) {  // keep probes short: a full set drops the rip
        P.cov_overflow[lane] = 1;
        return cnt;
      }
      P.cov_rip[idx] = rip;
      P.cov_gen[idx] = gen;
      return cnt + 1;
    }
    if (P.cov_rip[idx] == rip) return cnt;
    h = (h + 1) & (H - 1);
  }
  return cnt;
}

// Uniform fetch of up to 16 bytes at page pointer p (within one page).
__device__ __forceinline__ void fetch_bytes(u64 pageptr, u32 off, u32 n, u64 &lo, u64 &hi) {
  // n <= 16 and off + n <= 4096
  const u64 a = (pageptr + off) & ~7ull;
  const u32 sh = (u32)((pageptr + off) & 7);
  const u64 pend = pageptr + WTFGPU_PAGE_SIZE;
  const u64 w0 = rfl64(*(const u64 *)a);
  const u64 w1 = (a + 8 < pend) ? rfl64(*(const u64 *)(a + 8)) : 0;
  const u64 w2 = (a + 16 < pend) ? rfl64(*(const u64 *)(a + 16)) : 0;
  if (sh == 0) {
    lo = w0;
    hi = w1;
  } else {
    lo = (w0 >> (8 * sh)) | (w1 << (64 - 8 * sh));
    hi = (w1 >> (8 * sh)) | (w2 << (64 - 8 * sh));
  }
  if (n < 16) {
    if (n <= 8) {
      hi = 0;
      lo = n == 8 ? lo : (lo & ((1ull << (8 * n)) - 1));
    } else {
      hi &= (1ull << (8 * (n - 8))) - 1;
    }
  }
}

// ---------------------------------------------------------------- decoded-uop cache
// Per wave, in LDS, for the lifetime of one k_run launch. Key = page pointer |
// offset of the instruction's first byte; only pages of the read-only snapshot
// pool are cached (a lane's overlay copy can be rewritten by the guest). An
// entry holds the decoded UOp (generic path), its FOp digest (fast path), the
// breakpoint lookup (the set is fixed during a launch), whether the rip is
// already in the aggregate coverage map, and the lanes this wave has already
// logged for it in this launch.
// head-only entries per wave (the UOp lives in the uop slots below):
// 4 waves x 312 x 64 bytes + the uop slots = 81,792 bytes a
// block, two blocks per CU in 160 KiB (256 entries: tlv's fill passes 16 % of
// wave-steps, 312: 12 %; profiles/r05_stamps_ucindex_ab.txt)
constexpr u32 UC_N = 312;
// uop slots per wave (power of two): 4 x 120 bytes per wave, k_run's LDS fits 160 KiB
constexpr u32 UC_U = 4;
constexpr u32 UC_BP = 1, UC_COVERED = 2, UC_CROSS = 4, UC_BADLEN = 8, UC_UNSUP = 16;
struct UCHead {
  u64 key;
  u64 logged;
  u32 flags, pad;
  FOp f;
};
// What the fast loop reads: one LDS entry per cached rip (64 bytes, so a wave
// keeps UC_N of them within the CU's LDS budget at two blocks per CU).
struct UCEntry {
  union {
    UCHead h;
    struct {
      u64 key;
      u64 logged;
      u32 flags, pad;
      FOp f;
    };
  };
  u64 rip;  // the rip that filled it (a warm image re-checks UC_COVERED with it)
};
// The decoded UOp, which only the slow step's generic exec needs: a few
// slots per wave, refilled from the shared cache (or decoded) on demand.
struct UCUop {
  u64 key;
  UOp u;
};
// The shared (device-wide) cache's payload: static flags, FOp, UOp.
struct GPayload {
  u32 flags, pad;
  FOp f;
  UOp u;
};
constexpr u32 GP_HEAD = (sizeof(u32) * 2 + sizeof(FOp)) / 4;  // dwords of flags, pad, FOp
static_assert(sizeof(UOp) % 4 == 0 && sizeof(FOp) % 4 == 0, "copied as dwords");
static_assert(sizeof(UCEntry) == 64, "LDS entry size");
// Warm start: at the end of a launch, every hardware wave stores its LDS uop
// cache as an image; at the start of the next launch on the same queue, wave
// w loads image w (logged masks cleared, UC_COVERED
// re-checked against the coverage map) instead of starting empty. UC_COVERED
// stays true until the coverage map is reset; images are dropped with the
// shared cache (pool, breakpoints, edges / trace) and on a coverage reset.
// One image per wave a launch can have (Dev::warm_n per queue): regrouping
// keeps lanes in rip order, so wave w of the next launch runs much the code
// wave w ran (measured: 64 shared images left tlv's fills at a fifth of
// wave-steps). 16 KB a wave: 32 MB a queue at 131,072 lanes.
constexpr u32 UC_QUEUES = 2;
constexpr u64 UC_IMAGE_BYTES = (u64)UC_N * sizeof(UCEntry);

// Two-way sets (entries 2s, 2s + 1); tlv's 228-instruction loop missed a fifth of
// its wave-steps direct-mapped (scripts: a trace replay gives 23 % direct,
// 14 % two-way at 256 entries).
constexpr u32 UC_WAYS = 2;
static_assert(UC_N % UC_WAYS == 0, "whole sets");
// A fill takes way 0 and moves the old way 0 to way 1, so
// the fast loop's first LDS read finds the newer entry (SYN 4 % shorter
// launches than a counter-picked way; fill passes unchanged)
__device__ __forceinline__ bool cacheable_key(u64 lptr, u64 pool_lo, u64 pool_span) {
  return !m_ge64(lptr - pool_lo, pool_span);
}
__device__ __forceinline__ u32 uc_slot(u64 key) {
  // multiplicative hash: the offset bits mix into the set index too
  // a 32-bit multiplicative hash (the page bits above 4 GiB folded in), its
  // high bits scaled to the set count by one s_mul_hi (any count); cheaper
  // than the 64-bit product and fewer tlv fill passes (13.0 -> 11.1 %)
  const u32 h = ((u32)key ^ (u32)(key >> 17)) * 0x9E3779B1u;
  return __umulhi(h, UC_N / UC_WAYS) * UC_WAYS;
}
__device__ __forceinline__ u32 uu_slot(u64 key) { return (u32)((key ^ (key >> 12) * 0x9E3779B1u) & (UC_U - 1)); }

template <typename T>
__device__ __forceinline__ void lds_uniform_read(const T *src, T &dst) {
  const u32 *s = (const u32 *)src;
  u32 *d = (u32 *)&dst;
#pragma unroll
  for (u32 i = 0; i < sizeof(T) / 4; i++) d[i] = rfl32(s[i]);
}

// The uop-cache head as the fast loop reads it (wave-uniform): key, flags
// and the FOp words fast_exec uses (not `logged` or the pads).
__device__ __forceinline__ void uc_head_read(const UCEntry *e, UCHead &h) {
  h.key = rfl64(e->key);
  h.flags = rfl32(e->flags);
  h.f.w0 = rfl32(e->f.w0);
  h.f.fl = rfl32(e->f.fl);
  h.f.w2 = rfl32(e->f.w2);
  h.f.disp = rfl64(e->f.disp);
  h.f.imm = rfl64(e->f.imm);
}

__device__ __forceinline__ bool bp_lookup(const Dev &P, u64 rip) {
  u32 s;
  return P.bp_keys && hash_find(P.bp_keys, P.bp_mask, rip, s);
}

// Fill one entry (uniform): fetch + decode from the pool page, digest, lookups.
// Write len bytes at gpa into the lane's overlay (copy-on-write + dirty).
__device__ __forceinline__ bool lane_phys_write(const Dev &P, Lane &L, u64 gpa, const u8 *src, u64 len) {
  while (len) {
    const u64 off = gpa & 0xfff;
    u64 n = 4096 - off;
    if (n > len) n = len;
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
    for (u64 i = 0; i < n; i++) dst[off + i] = src[i];
    src += n;
    gpa += n;
    len -= n;
  }
  return true;
}

constexpr u32 GUC_WORDS = 48;                                  // 3 lines x 16 dwords
constexpr u32 GUC_PAYLOAD = sizeof(GPayload) / 4;  // flags, pad, FOp, UOp
static_assert(GUC_PAYLOAD <= 3 * 14, "global uop cache entry: 3 lines of 14 payload dwords");
__device__ __forceinline__ u32 guc_slot(const Dev &P, u64 key) {
  return (u32)(mix64(key) & P.guc_mask);
}
// payload dword of lane lid (lines of 16 dwords: 14 payload, 2 key tag), or ~0u
__device__ __forceinline__ u32 guc_payload_index(u32 lid) {
  return (lid < GUC_WORDS && (lid & 15) < 14) ? (lid >> 4) * 14 + (lid & 15) : ~0u;
}

// COVERED: the rip's byte in the aggregate coverage map is set (dynamic: not
// part of a shared entry)
__device__ __forceinline__ u32 covered_flag(const Dev &P, u64 rip, u32 off) {
  if (P.code_keys) {
    u32 s;
    if (hash_find(P.code_keys, P.code_mask, rip >> 12, s)) {
      const u32 cs = rfl32(P.code_slot[s]);
      if (rfl32(P.cov_map[(u64)cs * WTFGPU_PAGE_SIZE + off])) return UC_COVERED;
    }
  }
  return 0;
}

// The same per lane (non-uniform rips: a warm image's entries).
__device__ __forceinline__ u32 covered_flag_lane(const Dev &P, u64 rip, u32 off) {
  if (!P.code_keys) return 0;
  u32 h = (u32)mix64(rip >> 12) & P.code_mask;
  for (u32 i = 0; i <= P.code_mask; i++) {
    const u64 k = P.code_keys[h];
    if (k == (rip >> 12)) return P.cov_map[(u64)P.code_slot[h] * WTFGPU_PAGE_SIZE + off] ? UC_COVERED : 0;
    if (k == EMPTY_KEY) return 0;
    h = (h + 1) & P.code_mask;
  }
  return 0;
}

// The FOp of an instruction that always runs in the slow step (its length kept).
__device__ __forceinline__ FOp generic_fop(const UOp &d) {
  FOp f{};
  f.w0 = (d.len & 0x3f) << 20;
  return f;
}

// The shared (device-wide) cache's side of a fill (uniform): one dword per
// lane, the six tag dwords checked; on a hit the head goes to `e` (when
// given) and the UOp to the uop slot `us`. Inline at k_run's fill site (a
// fill is about a fifth of tlv's wave-steps, and a call spills the caller's
// live registers); false = a miss, uc_fill decodes.
__device__ __forceinline__ bool uc_fill_shared(const Dev &P, UCEntry *e, UCUop *us, u64 key, u32 off, u64 rip,
                                               u32 lid) {
  if (!P.guc) return false;
  const u32 pj = guc_payload_index(lid);
  u32 *head = e ? (u32 *)&e->flags : nullptr, *uop = us ? (u32 *)&us->u : nullptr;  // us null: the head only
  u32 *gw = P.guc + (u64)guc_slot(P, key) * GUC_WORDS;
  const u32 w = lid < GUC_WORDS ? gw[lid] : 0;
  const bool tag = lid < GUC_WORDS && (lid & 15) >= 14;
  const bool bad = tag && w != ((lid & 1) ? (u32)(key >> 32) : (u32)key);
  if (__ballot(bad) != 0) return false;
  if (pj < GP_HEAD) {
    if (head) head[pj] = w;
  } else if (pj < GUC_PAYLOAD) {
    if (uop) uop[pj - GP_HEAD] = w;
  }
  // UC_COVERED is cached in the shared entry once seen (coverage only grows
  // until wtfgpu_reset_coverage, which clears the shared cache): most fills
  // skip the map lookup's dependent loads
  const u32 sflags = __builtin_amdgcn_readlane(w, 0);
  u32 flags = sflags;
  if (e && !(sflags & UC_COVERED)) {
    flags |= covered_flag(P, rip, off);
    if ((flags & UC_COVERED) && lid == 0) gw[0] = flags;
  }
  __builtin_amdgcn_wave_barrier();
  if (lid == 0) {
    if (us) us->key = key;
    if (e) {
      e->logged = 0;
      e->flags = flags;
      e->rip = rip;
      e->key = key;
    }
  }
  return true;
}

// Fill one entry (uniform): from the shared cache when it holds the key, else
// fetch + decode from the pool page, digest, lookups, and publish. The head
// goes to `e` (when given), the UOp to the uop slot `us`.
__device__ __noinline__ void uc_fill(const Dev &P, UCEntry *e, UCUop *us, u64 key, u64 lptr, u32 off, u64 rip,
                                     u32 lid, bool shared_checked = false) {
  const u32 pj = guc_payload_index(lid);
  u32 *uop = (u32 *)&us->u;
  if (!shared_checked && uc_fill_shared(P, e, us, key, off, rip, lid)) return;
  u32 *gw = P.guc ? P.guc + (u64)guc_slot(P, key) * GUC_WORDS : nullptr;
  IBytes ib;
  ib.avail = 4096 - off < 16 ? 4096 - off : 16;
  fetch_bytes(lptr, off, ib.avail, ib.lo, ib.hi);
  UOp d;
  const int dr = decode(ib, d);
  u32 flags = dr == 1 ? UC_CROSS : dr == 2 ? UC_BADLEN : 0;
  FOp f;
  if (dr == 0) {
    digest(d, f);
    if (P.edges && edge_op(d.op, d.bsrc)) f = generic_fop(d);  // branches whose edge is recorded run in the slow step
    if (P.trace || g_tn.buf) f = generic_fop(d);               // traced lanes log every rip in the slow step
    if (!d.supported) flags |= UC_UNSUP;
    if (bp_lookup(P, rip)) flags |= UC_BP;
  } else {
    f = FOp{};
  }
  const u32 dyn = (dr == 0 && e) ? covered_flag(P, rip, off) : 0;
  if (lid == 0) {
    us->u = d;
    us->key = key;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if (gw) {  // publish (static flags only); one coalesced store of 3 tagged lines
    u32 v = 0;
    if (pj < GP_HEAD) v = pj == 0 ? (flags | dyn) : pj == 1 ? 0u : ((const u32 *)&f)[pj - 2];
    else if (pj < GUC_PAYLOAD) v = uop[pj - GP_HEAD];
    else if (lid < GUC_WORDS && (lid & 15) >= 14) v = (lid & 1) ? (u32)(key >> 32) : (u32)key;
    if (lid < GUC_WORDS) gw[lid] = v;
  }
  if (lid == 0 && e) {
    e->logged = 0;
    e->f = f;
    e->flags = flags | dyn;
    e->rip = rip;
    e->key = key;
  }
}

// The UOp of `key` in the wave's uop slots (the slow step's generic path).
__device__ __forceinline__ const UOp *uc_uop(const Dev &P, UCUop *uu, u64 key, u64 lptr, u32 off, u64 rip, u32 lid) {
  UCUop *us = &uu[uu_slot(key)];
  if (rfl64(us->key) != key) uc_fill(P, nullptr, us, key, lptr, off, rip, lid);
  return &us->u;
}

// The uop cache (LDS entries, warm images, the shared cache) is keyed by the
// pool page, and an entry's UC_BP / UC_COVERED flags and logged mask are those
// of the rip that filled it. A pool page therefore belongs to one virtual page:
// the first that runs code from it (code_owner, claimed here). A lane that
// runs the same page at another address gets CPTR_ALIAS in its code pointer,
// which puts the pointer outside the pool as EFER_M32 does: uncached, every
// instruction through slow_step, which looks everything up by the lane's rip.
constexpr u64 CPTR_ALIAS = 1ull << 62;
__device__ __forceinline__ bool code_page_pooled(const Dev &P, u64 td, u64 &idx) {
  const u64 o = (td & ~0xfffull) - (u64)(uintptr_t)P.pool;
  idx = o >> 12;
  return !(td & T_PRIV) && P.code_owner && o < (P.npool + 1) * WTFGPU_PAGE_SIZE;
}
// the fast loop's question (a load, no claim): the page is this address's own
__device__ __forceinline__ bool code_owner_is(const Dev &P, u64 td, u64 vpn) {
  u64 idx;
  // (an atomic load: a claim another wave made is seen, not a cached 0; a stale 0 would only decline)
  return !code_page_pooled(P, td, idx) ||
         __hip_atomic_load(&P.code_owner[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == vpn + 1;
}
__device__ __forceinline__ u64 code_alias_bit(const Dev &P, u64 td, u64 vpn) {
  u64 idx;
  if (!code_page_pooled(P, td, idx)) return 0;
  const unsigned long long prev = atomicCAS((unsigned long long *)&P.code_owner[idx], 0ull, vpn + 1);
  return prev == 0 || prev == vpn + 1 ? 0 : CPTR_ALIAS;
}

// Instruction-page translation for lanes whose code-page cache missed.
__device__ __noinline__ void code_xlate(const Dev &P, Lane &L, u64 rip) {
  u64 td;
  const u64 vpn = rip >> 12;
  if (!tlb_get(L, vpn, td) || !perm_ok(L, td, ACC_X)) {
    if (service_miss(P, L, rip & ~0xfffull, ACC_X)) tlb_get(L, vpn, td);
    else td = 0;
    if (td && !perm_ok(L, td, ACC_X)) td = 0;
    if (!td && L.status == WTFGPU_EXIT_FAULT) L.exaddr = rip;
  }
  if (td) {
    L.cvpn = vpn;
    L.cptr = (td & ~0xfffull) | (L.efer & EFER_M32) | code_alias_bit(P, td, vpn);  // 32-bit code: outside the pool (U29)
  }
}

__device__ __noinline__ bool miss_service(const Dev &P, Lane &L, int attempt) {
  if (attempt >= 16 || !service_miss(P, L, L.miss_va, (int)L.miss_acc)) {
    if (attempt >= 16) set_fault(L, WTFGPU_VEC_GP, 0xffff, L.miss_va);
    return false;
  }
  return true;
}

__device__ __noinline__ int exec_generic(const Dev &P, Lane &L, const UOp *ul, u64 &next) {
  UOp d;
  lds_uniform_read(ul, d);
  return exec(P, L, d, L.rip + d.len, next);
}

// The restartable attempts at one instruction on one lane copy: a TLB miss /
// first write abandons the attempt, miss_service fills the TLB or copies the
// page, the attempt reruns.
__device__ __noinline__ int exec_retry(const Dev &P, Lane &L, const UOp *ul, u64 &next) {
  int x;
  tn_insn_begin(L.lane);
  L.keep = 0;
  for (int attempt = 0;; attempt++) {
    L.miss = 0;
    L.pend = 0;
    tn_rollback(L.lane);
    x = exec_generic(P, L, ul, next);
    if (!L.miss || L.status != WTFGPU_RUNNING) break;
    if (!miss_service(P, L, attempt)) break;
  }
  return x;
}

// Retire / exit bookkeeping after the last attempt at an instruction.
__device__ __forceinline__ void retire(const Dev &P, Lane &L, int x, u32 len, u64 next, u32 opbytes) {
  if (L.flush) {
    tlb_flush(L);
    L.flush = 0;
  }
  if ((x == X_OK || x == X_CR3) && L.status == WTFGPU_RUNNING) {
    L.rip = next;
    L.icount++;
    L.nbytes += len + L.pend;
    if (P.limit && L.icount > P.limit) L.status = WTFGPU_EXIT_TIMEOUT;
    else if (x == X_CR3) L.status = WTFGPU_EXIT_CR3;  // bochscpu_backend.cc:628-657 (U20)
  } else if (L.status != WTFGPU_RUNNING) {
    // faulted / overlay full inside exec or service_miss; rip unchanged
  } else if (x == X_UNIMPL) {
    L.status = WTFGPU_EXIT_UNIMPLEMENTED;
    L.exop = len >= 4 ? opbytes : (opbytes & ((1u << (8 * len)) - 1));
  } else if (x == X_INT3) {
    L.status = WTFGPU_EXIT_INT3;
  } else if (x == X_HLT) {
    L.status = WTFGPU_EXIT_HLT;
  }
}

// FEED action: the next chunk of the lane's feed goes to gpr[b] + window -
// size, as fuzzer_tlv_server.cc:83-166 writes the next packet. Writes go
// through the copy-on-write path (the pages are dirtied as VirtWriteDirty
// does). A missing page ends the lane with WTFGPU_EXIT_FEED_FAULT, where the
// module's handler aborts.
// A host-side VirtWriteDirty of n bytes at va (backend.cc:91-121): page by page,
// the stores run as supervisor with CR0.WP clear (translation with
// ValidateRead: only a missing translation stops it, U/S and R/W are not
// checked), through copy-on-write. false = a page did not translate (the
// pages before it are written, as VirtWrite leaves them): the lane ends with
// WTFGPU_EXIT_FEED_FAULT (the host handler's failed write, U43).
__device__ __noinline__ bool host_write(const Dev &P, Lane &L, u64 va, const u8 *__restrict__ src, u64 n) {
  const u32 cpl0 = L.cpl;
  const u64 cr00 = L.cr0;
  L.cpl = 0;
  L.cr0 &= ~(1ull << 16);
  bool ok = true;
  // page by page, as VirtWrite does: translate (copy-on-write on the first
  // write), then copy the page's part, 32 source bytes loaded per round
  for (u64 o = 0; o < n;) {
    const u64 a = va + o, room = 4096 - (a & 0xfff);
    const u32 m = (u32)(n - o < room ? n - o : room);
    u8 *d = nullptr;
    u64 td = 0;
    for (int attempt = 0;; attempt++) {
      L.miss = 0;
      if ((d = xlate(L, a, ACC_W, &td))) break;
      if (L.status != WTFGPU_RUNNING || !L.miss || !miss_service(P, L, attempt)) {
        ok = false;
        break;
      }
    }
    if (!ok) break;
    if (td & T_PT) L.flush = 1;  // a page-table page: cached translations go
    const u8 *__restrict__ sp = src + o;
    u32 k = 0;
    for (; k + 32 <= m; k += 32) {
      u8 t[32];
#pragma unroll
      for (u32 j = 0; j < 32; j++) t[j] = sp[k + j];
#pragma unroll
      for (u32 j = 0; j < 32; j++) d[k + j] = t[j];
    }
    for (; k < m; k++) d[k] = sp[k];
    o += m;
  }
  if (!ok) {
    if (L.status == WTFGPU_RUNNING || L.status == WTFGPU_EXIT_FAULT) L.status = WTFGPU_EXIT_FEED_FAULT;
    L.miss = 0;
  }
  L.cpl = cpl0;
  L.cr0 = cr00;
  L.pend = 0;
  if (ok && L.flush) {
    tlb_flush(L);
    L.flush = 0;
  }
  return ok;
}

__device__ __noinline__ bool feed_apply(const Dev &P, Lane &L, const wtfgpu_bp_action_t &a) {
  if (!P.feed_pos) return false;
  const u64 pos = P.feed_pos[L.lane];
  if (pos == ~0ull) return false;  // no feed: the host handler serves the lane
  const u64 end = P.feed_end[L.lane];
  if (pos + 4 > end) {
    L.status = WTFGPU_EXIT_STOP_OK;
    return true;
  }
  const u8 *src = P.feed_data + pos;
  const u32 n = (u32)src[0] | ((u32)src[1] << 8) | ((u32)src[2] << 16) | ((u32)src[3] << 24);
  P.feed_pos[L.lane] = pos + 4 + n;
  if (n >= a.value || pos + 4 + n > end) {
    L.status = WTFGPU_EXIT_STOP_OK;
    return true;
  }
  const u32 rb = (u32)a.gprs[0] & 15, rn = (u32)a.gprs[1] & 15;
  const u64 dst = R(L, rb) + a.value - n;
  if (!host_write(P, L, dst, src + 4, n)) return true;  // WTFGPU_EXIT_FEED_FAULT
  RS(L, rn, n);
  RS(L, rb, dst);
  return true;
}

// Declared insert (wtfgpu_set_insert; the data form of fuzzer_hevd.cc:20-59's
// InsertTestcase): the lane's feed holds one chunk, the testcase; its first 4
// bytes go to gpr[head_reg], the rest (the payload) is written at
// gpr[ptr_reg], its size goes to gpr[len_reg] and, with len_arg, to
// [rsp + 8 + 8 * len_arg] (GetArgAddress, backend.cc:160-168), in the order
// the module does it. The feed is consumed. A write that does not translate
// ends the lane with WTFGPU_EXIT_FEED_FAULT, where the host handler would
// have failed (U43).
__device__ __noinline__ void insert_apply(const Dev &P, Lane &L, const wtfgpu_insert_t &ins) {
  const u64 pos = P.feed_pos[L.lane], end = P.feed_end[L.lane];
  if (pos == ~0ull) return;
  P.feed_pos[L.lane] = end;
  if (pos + 8 > end) return;
  const u8 *src = P.feed_data + pos;
  const u32 n = (u32)src[0] | ((u32)src[1] << 8) | ((u32)src[2] << 16) | ((u32)src[3] << 24);
  if (n < 4 || pos + 4 + n > end) return;
  const u32 head = (u32)src[4] | ((u32)src[5] << 8) | ((u32)src[6] << 16) | ((u32)src[7] << 24);
  const u64 m = n - 4;
  RS(L, ins.head_reg & 15, head);
  if (!host_write(P, L, R(L, ins.ptr_reg & 15), src + 8, m)) return;
  RS(L, ins.len_reg & 15, m);
  if (ins.len_arg) {
    u8 le[8];
    for (int i = 0; i < 8; i++) le[i] = (u8)(m >> (8 * i));
    host_write(P, L, R(L, WTFGPU_RSP) + 8 + 8 * (u64)ins.len_arg, le, 8);
  }
}

// Device-side breakpoint action (wtfgpu_set_breakpoint_actions) at `grip`.
// true = applied, the lane keeps running at its new rip; false = none
// declared or it could not be applied: the lane exits to the host handler,
// registers untouched. RETURN reads [rsp] as the host's
// SimulateReturnFromFunction does (backend.cc:129-146); a read that would fault
// is left to the host path, whose translation decides the outcome.
// BLAKE3 of an 8-byte input, first 16 output bytes (one chunk, one block:
// CHUNK_START | CHUNK_END | ROOT), for Rdrand's chain.
__device__ __forceinline__ u32 rotr32(u32 x, u32 n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ void b3_g(u32 *v, int a, int b, int c, int d, u32 x, u32 y) {
  v[a] = v[a] + v[b] + x;
  v[d] = rotr32(v[d] ^ v[a], 16);
  v[c] = v[c] + v[d];
  v[b] = rotr32(v[b] ^ v[c], 12);
  v[a] = v[a] + v[b] + y;
  v[d] = rotr32(v[d] ^ v[a], 8);
  v[c] = v[c] + v[d];
  v[b] = rotr32(v[b] ^ v[c], 7);
}
__device__ __noinline__ void blake3_le64(u64 in, u64 &lo, u64 &hi) {
  const u32 iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                     0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  const u8 perm[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  u32 m[16] = {(u32)in, (u32)(in >> 32), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  u32 v[16] = {iv[0], iv[1], iv[2], iv[3], iv[4], iv[5], iv[6], iv[7], iv[0], iv[1], iv[2], iv[3], 0, 0, 8, 1 | 2 | 8};
  for (int r = 0; r < 7; r++) {
    b3_g(v, 0, 4, 8, 12, m[0], m[1]);
    b3_g(v, 1, 5, 9, 13, m[2], m[3]);
    b3_g(v, 2, 6, 10, 14, m[4], m[5]);
    b3_g(v, 3, 7, 11, 15, m[6], m[7]);
    b3_g(v, 0, 5, 10, 15, m[8], m[9]);
    b3_g(v, 1, 6, 11, 12, m[10], m[11]);
    b3_g(v, 2, 7, 8, 13, m[12], m[13]);
    b3_g(v, 3, 4, 9, 14, m[14], m[15]);
    if (r < 6) {
      u32 t[16];
      for (int i = 0; i < 16; i++) t[i] = m[perm[i]];
      for (int i = 0; i < 16; i++) m[i] = t[i];
    }
  }
  lo = (u64)(v[0] ^ v[8]) | ((u64)(v[1] ^ v[9]) << 32);
  hi = (u64)(v[2] ^ v[10]) | ((u64)(v[3] ^ v[11]) << 32);
}

__device__ __forceinline__ bool bp_apply_action(const Dev &P, Lane &L, u64 grip, const wtfgpu_bp_action_t *found) {
  u32 s;
  if (!found && (!P.act_keys || !hash_find(P.act_keys, P.act_mask, grip, s))) return false;
  const wtfgpu_bp_action_t &a = found ? *found : P.act[s];
  if (a.kind == WTFGPU_BPACT_SET_GPRS) {
    for (u32 i = 0; i < 16; i++) RS(L, i, a.gprs[i]);
    L.rip = a.gprs[16];
    return true;
  }
  if (a.kind == WTFGPU_BPACT_FEED) return feed_apply(P, L, a);
  if (a.kind == WTFGPU_BPACT_STOP_OK) {
    L.status = WTFGPU_EXIT_STOP_OK;
    return true;
  }
  if (a.kind == WTFGPU_BPACT_RDRAND) {  // Rdrand (bochscpu_backend.cc:874-885); the instruction then runs
    if (!P.rd_seed) return false;
    u64 lo, hi;
    blake3_le64(P.rd_seed[L.lane], lo, hi);
    P.rd_seed[L.lane] = lo;
    RS(L, (u32)a.gprs[0] & 15, hi);
    return true;
  }
  if (a.kind == WTFGPU_BPACT_STOP_ARGS) {  // Win64 arguments 0..5 (backend.cc:168-192), then stop
    if (!P.stop_args) return false;
    const u64 rsp = R(L, WTFGPU_RSP);
    u64 v[6] = {R(L, 1), R(L, 2), R(L, 8), R(L, 9), 0, 0};
    for (u32 i = 4; i < 6 && i < a.value; i++) {
      for (int attempt = 0;; attempt++) {
        L.miss = 0;
        if (vread(L, rsp + 8 + 8 * (u64)i, 8, v[i])) break;
        if (L.status != WTFGPU_RUNNING || !L.miss || !miss_service(P, L, attempt)) {
          L.status = WTFGPU_RUNNING;  // undo a fault: the host handler decides
          L.miss = 0;
          L.pend = 0;
          return false;
        }
      }
    }
    L.pend = 0;
    for (u32 i = 0; i < 6; i++) P.stop_args[(u64)L.lane * 6 + i] = i < a.value ? v[i] : 0;
    L.status = WTFGPU_EXIT_STOP_ARGS;
    return true;
  }
  if (a.kind != WTFGPU_BPACT_RETURN) return false;
  if (a.gprs[0]) {
    // the handler first reads a C string at gpr[gprs[0] - 1], at most gprs[1]
    // bytes (VirtReadString, backend.h:333-430): a byte that does not
    // translate before the terminator leaves the hit to the host handler,
    // whose read then decides (U43)
    // (read as aligned 32-byte blocks, the four words of a block loaded at
    // once: a block never crosses a page, so it translates exactly when the
    // first byte of it the scan needs does)
    const u64 s = R(L, (u32)(a.gprs[0] - 1) & 15);
    const u64 lim = a.gprs[1];
    for (u64 i = 0; i < lim;) {
      const u64 va = s + i, al = va & ~31ull;
      const u8 *p = nullptr;
      for (int attempt = 0;; attempt++) {
        L.miss = 0;
        if ((p = xlate(L, al, ACC_R))) break;
        if (L.status != WTFGPU_RUNNING || !L.miss || !miss_service(P, L, attempt)) {
          L.status = WTFGPU_RUNNING;  // undo a fault: the host handler decides
          L.miss = 0;
          return false;
        }
      }
      const u64 *w = (const u64 *)p;
      const u64 c0 = w[0], c1 = w[1], c2 = w[2], c3 = w[3];
      bool term = false;
      for (u32 b = (u32)(va - al); b < 32 && i < lim && !term; b++, i++) {
        const u64 c = b < 8 ? c0 : b < 16 ? c1 : b < 24 ? c2 : c3;
        term = ((c >> (8 * (b & 7))) & 0xff) == 0;
      }
      if (term) break;
    }
  }
  const u64 rsp = R(L, WTFGPU_RSP);
  u64 ra = 0;
  for (int attempt = 0;; attempt++) {
    L.miss = 0;
    if (vread(L, rsp, 8, ra)) break;
    if (L.status != WTFGPU_RUNNING || !L.miss || !miss_service(P, L, attempt)) {
      L.status = WTFGPU_RUNNING;  // undo a fault: the host handler decides
      L.miss = 0;
      L.pend = 0;
      return false;
    }
  }
  L.pend = 0;
  RS(L, WTFGPU_RAX, a.value);
  RS(L, WTFGPU_RSP, rsp + 8);
  L.rip = ra;
  return true;
}

// The action stands in for a host handler, whose guest-memory reads and writes
// (VirtRead / VirtWrite) are no CPU accesses: Tenet does not log them
// (bochscpu_backend.cc:1215-1323 logs the lin_access hook only).
// found: the action k_run already looked up (nullptr: look it up)
__device__ __noinline__ bool bp_apply(const Dev &P, Lane &L, u64 grip, const wtfgpu_bp_action_t *found = nullptr) {
  tn_mute(L.lane);
  const bool r = bp_apply_action(P, L, grip, found);
  tn_unmute(L.lane, 0, 0, 0, false);
  return r;
}

// A step the uop cache cannot serve: code on a lane overlay page, or an
// instruction that crosses into the next page (translated per lane).
__device__ __noinline__ void slow_step(const Dev &P, Lane &L, u64 grip, u64 lptr, bool ing, bool &skip) {
  const u32 off = (u32)(grip & 0xfff);
  const bool m32 = (lptr & EFER_M32) != 0;  // the group's lanes run 32-bit code (U29)
  lptr &= ~(EFER_M32 | CPTR_ALIAS);
  IBytes ib;
  ib.avail = 4096 - off < 16 ? 4096 - off : 16;
  fetch_bytes(lptr, off, ib.avail, ib.lo, ib.hi);
  UOp d;
  int dr = decode(ib, d, m32);
  if (dr == 1) {
    u64 nptr = 0;
    if (ing) {
      const u64 va2 = (grip & ~0xfffull) + 4096;
      u64 td;
      if (!tlb_get(L, va2 >> 12, td) || !perm_ok(L, td, ACC_X)) {
        if (service_miss(P, L, va2, ACC_X)) tlb_get(L, va2 >> 12, td);
        else td = 0;
      }
      if (td) nptr = td & ~0xfffull;
      else ing = false;
    }
    const u64 cm = __ballot(ing);
    if (cm == 0) return;
    const int leader = __ffsll((long long)cm) - 1;
    const u64 lnptr = readlane64(nptr, leader);
    ing = ing && nptr == lnptr;
    const u32 n0 = ib.avail;
    u64 lo2, hi2;
    fetch_bytes(lnptr, 0, 16 - n0, lo2, hi2);
    // splice: bytes [0,n0) from page 1, [n0,16) from page 2
    if (n0 >= 8) {
      ib.hi = (n0 == 8 ? 0 : ib.hi) | (n0 == 8 ? lo2 : (lo2 << (8 * (n0 - 8))));
    } else {
      ib.lo = ib.lo | (lo2 << (8 * n0));
      ib.hi = (lo2 >> (64 - 8 * n0)) | (hi2 << (8 * n0));
    }
    ib.avail = 16;
    dr = decode(ib, d, m32);
  }
  if (dr == 2) {
    if (ing) set_fault(L, WTFGPU_VEC_GP, 0, 0);
    return;
  }
  const u64 gmask = __ballot(ing);
  if (gmask == 0) return;
  if (P.cov_rip) L.ccnt = cover(P, grip, ing, L.lane, L.cgen, L.ccnt);
  if (P.trace && ing && !skip) trace_rip(P, L.lane, grip);  // a resumed breakpoint was logged at its hit
  const bool isbp = bp_lookup(P, grip);
  if (ing) {
    if (isbp && !skip) {
      // breakpoint hit (bochscpu_backend.cc:545-547): device action or host exit;
      // an action that left rip unchanged runs the instruction next step (skip)
      const bool applied = bp_apply(P, L, grip);
      if (!applied) L.status = WTFGPU_EXIT_BREAKPOINT;
      skip = applied && L.rip == grip;
      if (applied && !skip && g_tn.buf) tn_regs(P, L);  // Tenet: the action moved rip
      ing = false;
    } else {
      skip = false;
    }
  }
  if (!d.supported) {
    if (ing) {
      L.status = WTFGPU_EXIT_UNIMPLEMENTED;
      L.exop = d.len >= 4 ? d.opbytes : (d.opbytes & ((1u << (8 * d.len)) - 1));
    }
    return;
  }
  if (ing) {
    u64 next = 0;
    int x;
    tn_insn_begin(L.lane);
    L.keep = 0;
    for (int attempt = 0;; attempt++) {
      L.miss = 0;
      L.pend = 0;
      tn_rollback(L.lane);
      x = exec(P, L, d, grip + d.len, next);
      if (!L.miss || L.status != WTFGPU_RUNNING) break;
      if (!miss_service(P, L, attempt)) break;
    }
    retire(P, L, x, d.len, next, d.opbytes);
    if (g_tn.buf && (x == X_OK || x == X_CR3)) tn_regs(P, L);
    // RecordEdge (bochscpu_backend.cc:699-728): the branch ran, whatever the retire hook decided
    if (P.edges && P.cov_rip && edge_op(d.op, d.bsrc) && x == X_OK) {
      const u32 c0 = L.ccnt;
      L.ccnt = cover_edge(P, edge_key(grip, next), true, L.lane, L.cgen, L.ccnt);
      count_edge(P, L.lane, L.ccnt != c0);
    }
  }
}

// Runs `call` on a copy T of lane L whose registers live in arrays of their
// own, so the kernel's register arrays never escape into a called function
// (they stay in VGPRs). The copy lives in a per-lane slot in HBM (L2-resident
// while the lane runs), which leaves LDS to a second resident wave per SIMD:
// k_run launches take 1.25-1.35x less time per lane than with the copy in LDS
// (one slot per thread, one wave per SIMD; MI355X, tlv). On the stack, i.e.
// in scratch, its write-backs were most of k_run's HBM traffic.
struct LaneCopy {
  Lane l;
  u32 r[32];
};
#define WITH_LANE_COPY(call)                      \
  do {                                            \
    LaneCopy &C_ = ((LaneCopy *)P.lcopy)[lane];   \
    Lane &T = C_.l;                               \
    u32 *const tlo_ = C_.r, *const thi_ = C_.r + 16; \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; i_++) { \
      tlo_[i_] = glo[i_];                         \
      thi_[i_] = ghi[i_];                         \
    }                                             \
    T = L;                                        \
    T.glo = tlo_;                                 \
    T.ghi = thi_;                                 \
    call;                                         \
    L = T;                                        \
    L.glo = glo;                                  \
    L.ghi = ghi;                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; i_++) { \
      glo[i_] = tlo_[i_];                         \
      ghi[i_] = thi_[i_];                         \
    }                                             \
  } while (0)

// Diagnostic build only (-DWTFGPU_STAMPS, `make stamps`): per-phase s_memtime
// cycle totals of the step loop, summed into stat[4..11] (never in the product).
#ifdef WTFGPU_STAMPS
#define STAMP(k)                                   \
  do {                                             \
    const u64 t_ = __builtin_amdgcn_s_memtime();   \
    stamp_[k] += t_ - tprev_;                      \
    tprev_ = t_;                                   \
  } while (0)
// why the fast loop handed the wave to the slow step, counted in stat[12..15]:
// 0 a fast attempt missed (TLB, first write, page crossing, state), 1 the
// code page changed, 2 the rip is not in the wave's LDS uop cache, 3 other
// (generic op, breakpoint, coverage, code outside the pool)
#define WHY(k) why_ = (k)
// and which generic ops the slow step executed (O_* / O_SYS2 etc.), one count per
// group, in stat[16..528): index op | why << 6 | covered << 8
#define OPHIST(op) ophist_[((op) & 63) | (why_ & 3) << 6 | ((op) & 64 ? 256 : 0)]++
constexpr u32 STAT_N = 536;  // + stat[528..535]: cycles in bp_apply by action kind
#else
constexpr u32 STAT_N = 16;
#define OPHIST(op) \
  do {             \
  } while (0)
#define STAMP(k) \
  do {           \
  } while (0)
#define WHY(k) \
  do {         \
  } while (0)
#endif

// The lanes of a per-lane `if` meet again here, before a `continue` or the
// end of the step loop's body. Without it the loop latch is the join of that
// divergent branch, which makes every value the latch merges (the step count,
// the group, `have`) divergent to the compiler, and the step loops become
// exec-masked divergent loops. No instruction is emitted.
#define RECONVERGE() __builtin_amdgcn_wave_barrier()

// ---------------------------------------------------------------- main kernel
// One hardware wave runs P.lpw lanes (64, or 32 / 16 to put more waves on
// each SIMD when the batch is small: the step loop is latency-bound).
// entries a fill pass also brings in after the missed one (profiles/r06_ab_fill_prefetch.txt)
constexpr u32 FILL_PREFETCH = 8;
// The register allocation allows two waves per SIMD: at 3 / 4 k_run spills
// and loses (profiles/r06_ab_occupancy.txt).
__global__ __launch_bounds__(256, 2) void k_run(Dev P, u32 first, u32 count, u64 max_steps) {
  if (P.perm && rfl64(P.stat[3]) == 0) return;  // regrouped launch with no running lane
  const u32 lid = threadIdx.x & 63;
  const u32 hw = rfl32(blockIdx.x * 4 + (threadIdx.x >> 6));  // hardware wave in the launch (uniform)
  const u32 tid = hw * P.lpw + lid;
  const bool inrange = lid < P.lpw && tid < count && first + tid < P.nlanes;
  // the lane this position runs: identity, or the regrouping order (lanes at
  // the same rip side by side, k_regroup_keys + radix sort)
  const u32 lane = inrange ? (P.perm ? P.perm[first + tid] : first + tid) : 0;
  // a lane that is not running has its final exit already (or waits for the
  // host): it is neither loaded nor stored
  const bool valid = inrange && P.status[lane] == WTFGPU_RUNNING;
  __shared__ UCEntry sUC[4][UC_N];
  __shared__ UCUop sUU[4][UC_U];
  UCEntry *uc = sUC[threadIdx.x >> 6];
  UCUop *uu = sUU[threadIdx.x >> 6];
  // the LDS uop cache: the warm image of an earlier launch, or empty
  const bool wave_live = __ballot(valid) != 0;
  const UCEntry *img = (P.warm && wave_live) ? (const UCEntry *)P.warm + (u64)(hw % P.warm_n) * UC_N : nullptr;
  if (img) {
    for (u32 i = lid; i < UC_N; i += 64) {
      UCEntry t = img[i];
      t.logged = 0;
      if (P.cov_rip && t.key != EMPTY_KEY && !(t.flags & (UC_COVERED | UC_CROSS | UC_BADLEN)))
        t.flags |= covered_flag_lane(P, t.rip, (u32)(t.rip & 0xfff));
      uc[i] = t;
    }
  } else {
    for (u32 i = lid; i < UC_N; i += 64) uc[i].key = EMPTY_KEY;
  }
  if (lid < UC_U) uu[lid].key = EMPTY_KEY;
  u32 glo[16], ghi[16];
  Lane L;
  L.glo = glo;
  L.ghi = ghi;
  if (valid) {
    load_lane(P, lane, L);
  } else {
    L.status = WTFGPU_EXIT_IDLE;
    L.lane = 0;
    L.rip = 0;
    L.icount = 0;
    L.cvpn = EMPTY_KEY;
  }
  const u64 icount0 = L.icount;
  bool skip = valid && (P.lflags[lane] & 1);
  // Tenet: the registers at the start (first entry), or after a host handler
  // moved rip (resume without skip, lflags bit 1)
  if (valid && g_tn.buf && (g_tn.pos[lane] == 0 || (P.lflags[lane] & 2))) WITH_LANE_COPY(tn_regs(P, T));
  // The fields the step loops read, once: P is address-taken (the rare-path
  // calls take it by reference), so a field read in the loop would be a
  // scratch load each step, and its vmcnt(0) wait would also wait for the
  // previous step's guest stores. A flag that steers uniform control flow
  // goes through readfirstlane (a load from that private copy counts as
  // divergent, and a loop exit on one made the step loop an exec-masked
  // divergent loop). The loop-invariant bounds are kept in VGPRs (the
  // compiler is told nothing of their uniformity) and compared as lane
  // masks: SGPRs are the step loop's scarce registers, and these were
  // spilled to VGPR lanes and reloaded on every wave-step.
  const bool cov_on = rfl32(P.cov_rip != nullptr ? 1u : 0u) != 0;
  u64 pool_lo = (u64)(uintptr_t)P.pool, pool_span = (P.npool + 1) * WTFGPU_PAGE_SIZE;
  u64 limit_v = P.limit ? P.limit : ~0ull;  // icount above it: timeout
  // wave-steps of this launch (a launch is bounded far below 2^32 wave-steps)
  u32 max32 = max_steps > 0xffffffffull ? 0xffffffffu : (u32)max_steps;
  asm volatile("" : "+v"(pool_lo), "+v"(pool_span), "+v"(limit_v), "+v"(max32));
  const FastMem fm = fast_mem(P);
  u32 steps = 0;
#ifdef WTFGPU_STAMPS
  u64 stamp_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 tprev_ = __builtin_amdgcn_s_memtime();
  u64 whyc_[4] = {0, 0, 0, 0};
  u32 why_ = 3;
  u32 ophist_[512] = {};
  u64 bpcyc_[8] = {};
#endif

  for (;;) {
    // ================= fast loop: the common step, no calls. Leaves with
    // `have` set and `grip` = the group it could not serve.
    u64 grip = 0;
    bool have = false;
    for (;;) {
      if (m_ge32(steps, max32)) break;
      // (a position with no lane is EXIT_IDLE, never running)
      const u64 am = m_eq32(L.status, WTFGPU_RUNNING);
      if (am == 0) break;
      // group = lanes at the min rip; when the wave is converged (the common
      // case) the first active lane's rip is that min and the reduction is skipped
      grip = readlane64(L.rip, __ffsll((long long)am) - 1);
      u64 gm = am & m_eq64(L.rip, grip);
      if (gm != am) {
        for (u64 lo = am & m_lt64(L.rip, grip); lo; lo = am & m_lt64(L.rip, grip))
          grip = readlane64(L.rip, __ffsll((long long)lo) - 1);
        gm = am & m_eq64(L.rip, grip);
      }
      have = true;
      WHY(1);
      // a new code page: the lane's TLB, else a walk, in registers (what
      // code_xlate does); a translation that would fault goes to the slow step
      if (const u64 cxm = gm & m_ne64(L.cvpn, grip >> 12)) {
        if (in_mask(cxm)) {
          u64 td, gp;
          bool ok = tlb_get(L, grip >> 12, td) && perm_ok(L, td, ACC_X);
          if (!ok && fast_walk(P, L, grip & ~0xfffull, ACC_X, td, gp) && perm_ok(L, td, ACC_X)) {
            tlb_put(L, grip >> 12, td);
            ok = true;
          }
          // (a pool page this address does not own yet, or shares: code_xlate claims it or marks the alias)
          if (ok && code_owner_is(P, td, grip >> 12)) {
            L.cvpn = grip >> 12;
            L.cptr = (td & ~0xfffull) | (L.efer & EFER_M32);  // 32-bit code: to slow_step (U29)
          }
        }
        if (gm & m_ne64(L.cvpn, grip >> 12)) break;
      }
      WHY(3);
      const u64 lptr = readlane64(L.cptr, __ffsll((long long)gm) - 1);
      if (m_ge64(lptr - pool_lo, pool_span)) break;
      const u64 ingm = gm & m_eq64(L.cptr, lptr);
      const bool ing = in_mask(ingm);
      const u64 key = lptr | (grip & 0xfff);
      UCEntry *e = &uc[uc_slot(key)];
      // one LDS round trip: key, logged mask, flags and the FOp are contiguous;
      // the second way only when the first misses (reading both at once kept
      // twice the head in flight on every step: SYN 8 % slower than one way)
      // (the words the step needs only: the logged mask is read when the rip
      // is not yet covered, the pads never)
      UCHead h;
      uc_head_read(e, h);
      if (h.key != key) uc_head_read(++e, h);
      WHY(2);
      if (h.key != key) break;
      WHY(3);
      const u32 flags = h.flags;
      if (flags & (UC_CROSS | UC_BADLEN | UC_UNSUP)) break;
      // a breakpoint: the slow step runs its handler; lanes that resume at it
      // (skip: a device action that left rip there, or a host handler's
      // resume) run the instruction here, as the slow step would without
      // calling the handler again
      if ((flags & UC_BP) && (ingm & ~__ballot(skip))) break;
      if (cov_on && !(flags & UC_COVERED) && (ingm & ~rfl64(e->logged))) break;
      const FOp &f = h.f;
      if (fo_op(f) == FO_GENERIC) break;
      // a form that touches no memory cannot miss: one pass, no retry rounds
      if (!(f.fl & (FF_PUSH | FF_POP | FF_MR_A | FF_MR_B | FF_MW)) && fo_op(f) < FO_VLD) {
        steps++;
        have = false;
        if (ing) {
          skip = false;
          const u32 len = fo_len(f);
          FOp fr = f;
          asm volatile("" : "+s"(fr.w0), "+s"(fr.fl), "+s"(fr.w2), "+s"(fr.disp), "+s"(fr.imm));
          u64 next;
          fast_exec<true>(fm, L, fr, grip + len, next);
          L.rip = next;
          L.icount++;
          L.nbytes += len;
          if (L.icount > limit_v) L.status = WTFGPU_EXIT_TIMEOUT;
        }
        RECONVERGE();
        continue;
      }
      steps++;
      have = false;
      STAMP(6);
      // a TLB miss or a first write (fxlate: miss 2) is served here, on the
      // lane in registers, and the instruction retried at once, so the group
      // still takes one wave-step (at most 3 fill rounds); anything else (a
      // fault to raise, a page-table write, a page-crossing operand, ...) is
      // left to the slow step, whose exec() raises what it raises. A first
      // write's page copy is made by the whole wave, 64 bytes a position: one
      // memory round trip instead of a lane's 64 dependent ones
      const u32 len = fo_len(f);
      u64 next = 0;
      u64 wantm = ingm;
      if (ing) skip = false;
      for (u32 round = 0;; round++) {
        if (in_mask(wantm)) {
          L.miss = 0;
          L.pend = 0;
          // the FOp as an opaque value each round: otherwise everything
          // fast_exec derives from it (masks, shift counts, every op's
          // conditions) is hoisted out of this loop as invariant, stays live
          // across it and spills to VGPR lanes: ~100 v_writelane and ~280
          // v_readlane on every wave-step
          FOp fr = f;
          asm volatile("" : "+s"(fr.w0), "+s"(fr.fl), "+s"(fr.w2), "+s"(fr.disp), "+s"(fr.imm));
          fast_exec(fm, L, fr, grip + len, next);
        }
        RECONVERGE();
        // lanes to serve and retry: a TLB miss or first write (miss 2), 3 rounds at most
        wantm = round >= 3 ? 0 : wantm & m_eq32(L.miss, 2);
        if (wantm == 0) break;
        u64 csrc = 0, cdst = 0, cgpfn = 0, ctd = 0;
        bool want = in_mask(wantm);
        if (want && !fast_fill_prep(P, L, csrc, cdst, cgpfn, ctd)) {
          want = false;
          fast_fault(P, L);  // the lane stops with the fault (delivered after the loop)
        }
        for (u64 cm = __ballot(want && cdst); cm; cm &= cm - 1) {
          const int l = __ffsll((long long)cm) - 1;
          const uint4 *s4 = (const uint4 *)(uintptr_t)readlane64(csrc, l) + lid * 4;
          uint4 *d4 = (uint4 *)(uintptr_t)readlane64(cdst, l) + lid * 4;
          const uint4 a = s4[0], b = s4[1], c = s4[2], d = s4[3];
          d4[0] = a;
          d4[1] = b;
          d4[2] = c;
          d4[3] = d;
        }
        // the copies land before the lanes read their pages (one wave, one CU)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (want && cdst) fast_fill_finish(P, L, cdst, cgpfn, ctd);
        wantm = __ballot(want);
      }
      const u64 missm = ingm & m_ne32(L.miss, 0);
      if (in_mask(ingm & ~missm)) {
        L.rip = next;
        L.icount++;
        L.nbytes += len + L.pend;
        if (L.icount > limit_v) L.status = WTFGPU_EXIT_TIMEOUT;
      }
      RECONVERGE();
      STAMP(7);
      // lanes that still missed keep their rip: the slow step services them.
      // The attempt is not a wave-step of its own (the slow step counts the
      // group once): a slice's length in wave-steps must not depend on which
      // path ran a group, since that depends on when other queues' coverage
      // commits landed (U44: fixed-seed campaigns reproduce)
      if (missm & m_eq32(L.status, WTFGPU_RUNNING)) {
        WHY(0);
        steps--;
        have = true;
        break;
      }
      // lanes whose fill raised a fault here (fast_fault): the step counted
      // (as the slow step's would have), the fault is delivered next
      if (missm) break;
    }
    STAMP(0);
    // faults raised by the last slow step: deliver through the guest IDT when
    // it has a gate (the lane resumes at the handler), else the lane exits
    if (__ballot(L.status == WTFGPU_EXIT_FAULT && !L.nodeliver)) {
      if (L.status == WTFGPU_EXIT_FAULT && !L.nodeliver) {
        bool dv;
        WITH_LANE_COPY(dv = deliver_fault(P, T));
        if (dv && g_tn.buf) WITH_LANE_COPY(tn_regs(P, T));  // Tenet: the delivered exception
      }
      RECONVERGE();
      continue;
    }
    if (!have) break;

    // ================= slow step for group `grip`: translation misses, cache
    // fills, page-crossing / overlay code, coverage logging, breakpoints,
    // generic instructions, TLB misses and copy-on-write
    steps++;
#ifdef WTFGPU_STAMPS
    whyc_[why_ & 3]++;
#endif
    const bool active = L.status == WTFGPU_RUNNING;
    bool cand = active && L.rip == grip;
    if (cand && (grip >> 12) != L.cvpn) WITH_LANE_COPY(code_xlate(P, T, grip));
    cand = cand && (grip >> 12) == L.cvpn;
    const u64 cm = __ballot(cand);
    if (cm == 0) continue;
    const int leader = __ffsll((long long)cm) - 1;
    const u64 lptr = readlane64(L.cptr, leader);
    bool ing = cand && L.cptr == lptr;

    const u32 off = (u32)(grip & 0xfff);
    const u64 key = lptr | off;
    UCEntry *e = &uc[uc_slot(key)];
    if (rfl64(e->key) != key) {
      if (rfl64(e[1].key) == key) e += 1;
      else if (cacheable_key(lptr, pool_lo, pool_span)) {
        // the newest fill takes way 0 (the fast loop's first read), the old
        // way 0 moves to way 1 (whose entry is the one dropped)
        if (lid < 16) ((u32 *)&e[1])[lid] = ((const u32 *)e)[lid];
        __builtin_amdgcn_wave_barrier();
      }
    }
    const bool cacheable = !m_ge64(lptr - pool_lo, pool_span);
    if (cacheable && rfl64(e->key) != key) {
      // the shared-cache hit path inline (uc_fill_shared), else the full fill
      if (!uc_fill_shared(P, e, &uu[uu_slot(key)], key, off, grip, lid))
        uc_fill(P, e, &uu[uu_slot(key)], key, lptr, off, grip, lid, true);
      // sequential prefetch: the instructions after this one in the page, from
      // the shared cache into their sets' second (older) way, while the wave
      // is in the slow step anyway; stops at the first that is cached, absent
      // from the shared cache, or crosses the page
      const UCEntry *pe = e;
      u64 prip = grip;
      for (u32 k = 0; k < FILL_PREFETCH; k++) {
        const u32 pf = rfl32(pe->flags), pw0 = rfl32(pe->f.w0), plen = (pw0 >> 20) & 0x3f;
        if ((pf & (UC_CROSS | UC_BADLEN)) || !plen) break;
        const u64 nxt = prip + plen;  // the fall-through (same page only)
        if ((nxt >> 12) != (grip >> 12) || (nxt & 0xfff) > 4096 - 16) break;
        const u32 poff = (u32)(nxt & 0xfff);
        const u64 pkey = lptr | poff;
        UCEntry *ps = &uc[uc_slot(pkey)];
        if (rfl64(ps->key) == pkey || rfl64(ps[1].key) == pkey) break;
        if (!uc_fill_shared(P, ps + 1, nullptr, pkey, poff, nxt, lid)) break;
        pe = ps + 1;
        prip = nxt;
      }
      // an entry the fast loop can run (a common op, nothing to log, no
      // breakpoint): back to it, this pass was only the fill
      const u32 ff = rfl32(e->flags);
      if (!(ff & (UC_BP | UC_CROSS | UC_BADLEN | UC_UNSUP)) && (!cov_on || (ff & UC_COVERED)) &&
          (rfl32(e->f.w0) & 0xff) != FO_GENERIC) {  // read uniformly: a divergent exit here made the whole step loop divergent
        steps--;
        STAMP(2);
        continue;
      }
    }
    STAMP(2);
    const u32 flags = cacheable ? rfl32(e->flags) : UC_CROSS;
    if (flags & (UC_CROSS | UC_BADLEN)) {
      if (flags & UC_BADLEN) {
        if (ing) set_fault(L, WTFGPU_VEC_GP, 0, 0);
      } else if (L.status != WTFGPU_EXIT_IDLE) {  // a position with no lane has no copy slot of its own
        bool sk = skip;  // skip stays a register (a reference would put it in scratch for the whole loop)
        WITH_LANE_COPY(slow_step(P, T, grip, lptr, ing, sk));
        skip = sk;
      }
      RECONVERGE();
      STAMP(5);
      continue;
    }
    const u32 len = (rfl32(e->f.w0) >> 20) & 0x3f;  // fo_len, read once for the wave
    const u64 gmask = __ballot(ing);

    // ---- coverage, then breakpoint (bochscpu_backend.cc:501-547)
    if (P.trace && ing && !skip) trace_rip(P, L.lane, grip);  // a resumed breakpoint was logged at its hit
    bool logged_now = false;  // wave-uniform
    if (cov_on && !(flags & UC_COVERED)) {
      const u64 logged = rfl64(e->logged);
      if (gmask & ~logged) {
        L.ccnt = cover(P, grip, ing && !((logged >> lid) & 1), L.lane, L.cgen, L.ccnt);
        if (lid == 0) e->logged = logged | gmask;
        logged_now = true;
      }
    }
    STAMP(3);
    // the group has just logged the rip (its lanes are all in the entry's mask
    // now): an op the fast loop runs goes back to it, not to the generic exec.
    // Only right after logging, so a group the fast loop hands back (a miss
    // to serve) finds nothing to log and takes the generic path: no ping-pong
    if (logged_now && !(flags & (UC_BP | UC_UNSUP)) && (rfl32(e->f.w0) & 0xff) != FO_GENERIC) {
      steps--;
      continue;
    }
    // a register-only device action (SetGprs, StopOk: the same for every lane)
    // is applied here, without the lane copy and call the others take
    u32 act_kind = ~0u;
    const wtfgpu_bp_action_t *act = nullptr;
    if ((flags & UC_BP) && P.act_keys && !g_tn.buf) {
      u32 slot;
      if (hash_find(P.act_keys, P.act_mask, grip, slot)) {
        act = &P.act[slot];
        act_kind = rfl32(act->kind);
      }
    }
#ifdef WTFGPU_STAMPS
    // breakpoint hits by action kind (56 + kind; 63: none found)
    if (__ballot(ing && (flags & UC_BP) && !skip)) OPHIST(56 + (act_kind < 7 ? act_kind : 7));
#endif
    // (one block per kind: with the two kinds nested in one per-lane if/else
    // the build ran wrong on MI355X, tlv's lanes stopping Ok at their SetGprs
    // breakpoint, although either kind alone ran right: do not merge these
    // two blocks; the A/B is in DESIGN.md §3)
    if (act_kind == WTFGPU_BPACT_SET_GPRS && ing && !skip) {
#pragma unroll
      for (u32 i = 0; i < 16; i++) RS(L, i, act->gprs[i]);
      L.rip = act->gprs[16];
      skip = L.rip == grip;
      ing = false;
    }
    if (act_kind == WTFGPU_BPACT_STOP_OK && ing && !skip) {
      L.status = WTFGPU_EXIT_STOP_OK;
      skip = true;
      ing = false;
    }
    // a Feed action about to write a packet (feed_apply's checks) whose first
    // page is not yet the lane's own: that page's copy-on-write is made here
    // by the whole wave, 64 bytes a position (as the fast loop's first writes),
    // instead of by each lane's 16-round copy inside host_write. Same walk
    // (supervisor, CR0.WP clear, as host_write), same overlay slot, same page:
    // host_write then finds it private. Anything else is left to host_write.
    if (act_kind == WTFGPU_BPACT_FEED && P.feed_pos) {
      bool want = false;
      if (ing && !skip) {
        const u64 pos = P.feed_pos[L.lane];
        const u64 end = P.feed_end[L.lane];
        if (pos != ~0ull && pos + 4 <= end) {
          const u8 *src = P.feed_data + pos;
          const u32 n = (u32)src[0] | ((u32)src[1] << 8) | ((u32)src[2] << 16) | ((u32)src[3] << 24);
          const u64 win = act->value;
          if (n && n < win && pos + 4 + n <= end) {
            const u64 va = R(L, (u32)act->gprs[0] & 15) + win - n;
            u64 td;
            if (!(tlb_get(L, va >> 12, td) && (td & T_PRIV))) {
              L.miss_va = va;
              L.miss_acc = ACC_W;
              want = true;
            }
          }
        }
      }
      u64 csrc = 0, cdst = 0, cgpfn = 0, ctd = 0;
      if (want) {
        const u32 cpl0 = L.cpl;
        const u64 cr00 = L.cr0;
        L.cpl = 0;
        L.cr0 &= ~(1ull << 16);
        want = fast_fill_prep(P, L, csrc, cdst, cgpfn, ctd);
        L.cpl = cpl0;
        L.cr0 = cr00;
      }
      RECONVERGE();
      for (u64 cm = __ballot(want && cdst); cm; cm &= cm - 1) {
        const int l = __ffsll((long long)cm) - 1;
        const uint4 *s4 = (const uint4 *)(uintptr_t)readlane64(csrc, l) + lid * 4;
        uint4 *d4 = (uint4 *)(uintptr_t)readlane64(cdst, l) + lid * 4;
        const uint4 a = s4[0], b = s4[1], c = s4[2], d = s4[3];
        d4[0] = a;
        d4[1] = b;
        d4[2] = c;
        d4[3] = d;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (want && cdst) fast_fill_finish(P, L, cdst, cgpfn, ctd);
      RECONVERGE();
    }
    if (ing) {
      if ((flags & UC_BP) && !skip) {
        // breakpoint hit: device action (the lane keeps running) or host exit
        bool applied = false;
#ifdef WTFGPU_STAMPS
        const u64 tb_ = __builtin_amdgcn_s_memtime();
#endif
        if (P.act_keys) WITH_LANE_COPY(applied = bp_apply(P, T, grip, act));
#ifdef WTFGPU_STAMPS
        bpcyc_[act_kind < 7 ? act_kind : 7] += __builtin_amdgcn_s_memtime() - tb_;
#endif
        if (!applied) L.status = WTFGPU_EXIT_BREAKPOINT;
        skip = applied && L.rip == grip;
        if (applied && !skip && g_tn.buf) WITH_LANE_COPY(tn_regs(P, T));  // Tenet: the action moved rip
        ing = false;
      } else {
        skip = false;
      }
    }
    STAMP(4);
    // the UOp for the generic path (wave-uniform: the slot fill is a wave operation)
    const UOp *u = nullptr;
    if (__ballot(ing)) u = uc_uop(P, uu, key, lptr, off, grip, lid);
    if (__ballot(ing) && !(flags & UC_UNSUP)) OPHIST(rfl32(u->op) + (flags & UC_COVERED ? 64 : 0));
    if (ing && (flags & UC_UNSUP)) {
      const u32 ob = u->opbytes, n = len;
      L.status = WTFGPU_EXIT_UNIMPLEMENTED;
      L.exop = n >= 4 ? ob : (ob & ((1u << (8 * n)) - 1));
      ing = false;
    }
    if (ing) {
      // restartable attempts (exec_retry), all on one copy of the lane
      u64 next = 0;
      int x;
      WITH_LANE_COPY(x = exec_retry(P, T, u, next));
      u32 opbytes = 0;
      if (x == X_UNIMPL) opbytes = u->opbytes;
      retire(P, L, x, len, next, opbytes);
      if (g_tn.buf && (x == X_OK || x == X_CR3)) WITH_LANE_COPY(tn_regs(P, T));  // Tenet: the retired instruction
      // RecordEdge (bochscpu_backend.cc:699-728): the branch ran, whatever the retire hook decided
      if (P.edges && P.cov_rip && x == X_OK && edge_op(rfl32(u->op), rfl32(u->bsrc))) {
        const u32 c0 = L.ccnt;
        L.ccnt = cover_edge(P, edge_key(grip, next), true, L.lane, L.cgen, L.ccnt);
        count_edge(P, L.lane, L.ccnt != c0);
      }
    }
    RECONVERGE();
    STAMP(1);
  }

  if (P.warm && wave_live && hw < P.warm_n) {  // this wave's cache for the next launch
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    UCEntry *out = (UCEntry *)P.warm + (u64)hw * UC_N;
    for (u32 i = lid; i < UC_N; i += 64) out[i] = uc[i];
  }
  // Tenet: a lane that stopped with accesses still open (an undelivered fault,
  // an unimplemented instruction) closes them with a REGS entry
  if (valid && g_tn.buf && L.status != WTFGPU_RUNNING && L.status != WTFGPU_EXIT_BREAKPOINT &&
      g_tn.pos[lane] > g_tn.ipos[lane])
    WITH_LANE_COPY(tn_regs(P, T));
  if (valid) {
    store_lane(P, L);
    store_tlb(P, L);
    if (L.status == WTFGPU_EXIT_FAULT || L.status == WTFGPU_EXIT_UNIMPLEMENTED) {
      ExitInfo ei;
      ei.vector = L.exvec;
      ei.error = L.exerr;
      ei.opcode = L.exop;
      ei.cpl = L.cpl;
      ei.addr = L.exaddr;
      P.exinfo[lane] = ei;
    }
    P.lflags[lane] = skip ? 1u : 0u;
  }
  const u64 retired = wave_sum(valid ? L.icount - icount0 : 0);
  const u64 running = wave_sum((valid && L.status == WTFGPU_RUNNING) ? 1 : 0);
  if (lid == 0) {
    atomicAdd((unsigned long long *)&P.stat[0], (unsigned long long)steps);
    atomicAdd((unsigned long long *)&P.stat[1], (unsigned long long)retired);
    if (running) atomicAdd((unsigned long long *)&P.stat[2], (unsigned long long)running);
#ifdef WTFGPU_STAMPS
    for (int k = 0; k < 8; k++) atomicAdd((unsigned long long *)&P.stat[4 + k], (unsigned long long)stamp_[k]);
    for (int k = 0; k < 4; k++) atomicAdd((unsigned long long *)&P.stat[12 + k], (unsigned long long)whyc_[k]);
    for (int k = 0; k < 512; k++)
      if (ophist_[k]) atomicAdd((unsigned long long *)&P.stat[16 + k], (unsigned long long)ophist_[k]);
    for (int k = 0; k < 8; k++) atomicAdd((unsigned long long *)&P.stat[528 + k], (unsigned long long)bpcyc_[k]);
#endif
  }
}

}  // namespace
