// engine_kernels.h — the plumbing kernels around k_run: lane restore,
// host-driven lane memory, bulk lane services and coverage services.
//
// Device half of engine.hip (see engine_run.h); included nowhere else.
#pragma once
#include "engine_run.h"
#include "engine_mutate.h"
#include "engine_mutate_packets.h"
#include "engine_minimize.h"
#include "engine_distill.h"
#include "engine_covkeep.h"
#include "engine_analyze.h"
#include "engine_feedpack.h"

namespace {

// ---------------------------------------------------------------- restore
struct InitState {
  u64 g[16];
  u64 rip, rflags, fsb, gsb;
  LaneSys sys;
};

// Registers, system state and overlay of one lane back to the snapshot (the
// dirty-list reset: overlays dropped, nothing copied).
__device__ __forceinline__ void restore_lane(const Dev &P, const InitState &s, const wtfgpu_regs_t *full0,
                                             wtfgpu_regs_t *full, u32 lane) {
  const u64 N = P.nlanes;
  full[lane] = *full0;
#pragma unroll
  for (int i = 0; i < 16; i++) P.gpr[i * N + lane] = s.g[i];
  P.rip[lane] = s.rip;
  P.rflags[lane] = s.rflags;
  P.fs_base[lane] = s.fsb;
  P.gs_base[lane] = s.gsb;
  P.icount[lane] = 0;
  P.nbytes[lane] = 0;
  P.status[lane] = WTFGPU_RUNNING;
  P.lflags[lane] = 0;
  P.sys[lane] = s.sys;
  spill_release(P, lane, P.ov_count[lane]);  // pool pages back (the one place: engine_exec.h rule 2)
  P.ov_count[lane] = 0;
  tlb_stale(P, lane);
  if (P.rd_seed) P.rd_seed[lane] = P.rd_seed0;  // bochscpu_backend.cc:1030
  if (P.trace_cnt) P.trace_cnt[lane] = 0;
  if (P.edge_cnt) P.edge_cnt[2 * (u64)lane] = P.edge_cnt[2 * (u64)lane + 1] = 0;
  if (g_tn.buf) {
    g_tn.pos[lane] = g_tn.ipos[lane] = g_tn.cpos[lane] = 0;
    g_tn.last[lane] = ~0ull;
    g_tn.mute[lane] = 0;
  }
  if (P.cov_rip) {
    P.lane_gen[lane] += 1;
    P.cov_cnt[lane] = 0;
    P.cov_overflow[lane] = 0;
  }
}

// Streaming form: a lane list.
__global__ void k_restore_list(Dev P, const InitState *S, const wtfgpu_regs_t *full0, wtfgpu_regs_t *full,
                               const u32 *lanes, u32 n) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const InitState s = *S;
  restore_lane(P, s, full0, full, lanes[t]);
}

__global__ void k_restore(Dev P, const InitState *S, const wtfgpu_regs_t *full0, wtfgpu_regs_t *full, u32 first,
                          u32 count) {
  const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lane = first + tid;
  if (tid >= count || lane >= P.nlanes) return;
  const u64 N = P.nlanes;
  const InitState s = *S;
  full[lane] = *full0;  // cold architectural state (read/write_regs only)
#pragma unroll
  for (int i = 0; i < 16; i++) P.gpr[i * N + lane] = s.g[i];
  P.rip[lane] = s.rip;
  P.rflags[lane] = s.rflags;
  P.fs_base[lane] = s.fsb;
  P.gs_base[lane] = s.gsb;
  P.icount[lane] = 0;
  P.nbytes[lane] = 0;
  P.status[lane] = WTFGPU_RUNNING;
  P.lflags[lane] = 0;
  P.sys[lane] = s.sys;
  spill_release(P, lane, P.ov_count[lane]);  // pool pages back (the one place: engine_exec.h rule 2)
  P.ov_count[lane] = 0;  // the dirty-list reset: overlays dropped, nothing copied
  tlb_stale(P, lane);
  if (P.rd_seed) P.rd_seed[lane] = P.rd_seed0;  // bochscpu_backend.cc:1030
  if (P.trace_cnt) P.trace_cnt[lane] = 0;
  if (P.edge_cnt) P.edge_cnt[2 * (u64)lane] = P.edge_cnt[2 * (u64)lane + 1] = 0;
  if (g_tn.buf) {
    g_tn.pos[lane] = g_tn.ipos[lane] = g_tn.cpos[lane] = 0;
    g_tn.last[lane] = ~0ull;
    g_tn.mute[lane] = 0;
  }
  if (P.cov_rip) {       // the lane's coverage set empties
    P.lane_gen[lane] += 1;
    P.cov_cnt[lane] = 0;
    P.cov_overflow[lane] = 0;
  }
}

// ---------------------------------------------------------------- host-driven lane memory
// One thread per lane with pending writes (records sorted by lane). op: 0 write virt.
struct WriteRec {
  u32 lane, len;
  u64 gva, data_off;
};

__device__ __forceinline__ void lane_min_load(const Dev &P, u32 lane, Lane &L) {
  const LaneSys s = P.sys[lane];
  L.cr0 = s.cr0;
  L.cr3 = s.cr3;
  L.efer = s.efer;
  L.cpl = 0;  // host accesses are not subject to user checks (VirtTranslate has none)
  L.simd = 0;
  L.ovn = P.ov_count[lane];
  L.bloom = 0;
  for (u32 k = 0; k < L.ovn; k++) L.bloom |= bloom_bit(P.ov_gpfn[(u64)k * P.nlanes + lane]);
  L.lane = lane;
  L.status = WTFGPU_RUNNING;
  L.nbytes = 0;
  tlb_flush(L);
  L.tnext = 0;
  L.miss = L.miss_acc = L.flush = L.pend = L.keep = 0;
  L.nodeliver = 0;
}

// Host-side translation (bochscpu_mem_virt_translate semantics: present bits
// only, no permission checks).
__device__ __forceinline__ bool host_walk(const Dev &P, Lane &L, u64 va, u64 &gpa) {
  u64 table = L.cr3 & 0x000ffffffffff000ull;
  bool priv;
  u64 e = 0, pmask = 0xfff;
  for (int level = 3; level >= 0; level--) {
    const u8 *pg = phys_page(P, L.lane, L.ovn, L.bloom, table >> 12, priv);
    e = *(const u64 *)(pg + ((va >> (12 + 9 * level)) & 0x1ff) * 8);
    if (!(e & 1)) return false;
    if ((level == 1 || level == 2) && (e & 0x80)) {
      pmask = level == 2 ? 0x3fffffffull : 0x1fffffull;
      break;
    }
    table = e & 0x000ffffffffff000ull;
  }
  gpa = ((e & 0x000ffffffffff000ull) & ~pmask) | (va & pmask);
  return true;
}

// The same write by one 64-thread block (the control is uniform, every
// thread computes it; the page copy and the bytes are spread over the block).
__device__ __forceinline__ bool lane_phys_write_block(const Dev &P, Lane &L, u64 gpa, const u8 *src, u64 len, u32 lid) {
  while (len) {
    const u64 off = gpa & 0xfff;
    u64 n = 4096 - off;
    if (n > len) n = len;
    bool priv;
    const u8 *pg = phys_page(P, L.lane, L.ovn, L.bloom, gpa >> 12, priv);
    u8 *dst = (u8 *)pg;
    if (!priv) {
      // one thread takes the slot (a pool page past K: one claim), all copy
      __shared__ u8 *slot_page;
      if (lid == 0) slot_page = ov_alloc(P, L.lane, L.ovn);
      __syncthreads();
      dst = slot_page;
      __syncthreads();  // (read before the next round's write)
      if (!dst) return false;
      const uint4 *s4 = (const uint4 *)pg;
      uint4 *d4 = (uint4 *)dst;
      for (u32 i = lid; i < 256; i += 64) d4[i] = s4[i];
      if (lid == 0) P.ov_gpfn[(u64)L.ovn * P.nlanes + L.lane] = (u32)(gpa >> 12);
      __syncthreads();  // the copy before the patch (and the slot before later lookups)
      L.ovn++;
      L.bloom |= bloom_bit(gpa >> 12);
    }
    for (u64 i = lid; i < n; i += 64) dst[off + i] = src[i];
    __syncthreads();
    src += n;
    gpa += n;
    len -= n;
  }
  return true;
}

// Host-handler writes, one 64-thread block per lane, records in order.
__global__ void k_apply_writes(Dev P, const WriteRec *recs, const u32 *starts, u32 nlanes_w, const u8 *data,
                               i32 *status_out, u32 phys) {
  const u32 t = blockIdx.x, lid = threadIdx.x;
  if (t >= nlanes_w) return;
  const u32 r0 = starts[t], r1 = starts[t + 1];
  const u32 lane = recs[r0].lane;
  Lane L;
  lane_min_load(P, lane, L);
  for (u32 r = r0; r < r1; r++) {
    const WriteRec w = recs[r];
    u64 va = w.gva, left = w.len;
    const u8 *src = data + w.data_off;
    i32 st = 0;
    while (left) {
      const u64 off = va & 0xfff;
      u64 n = 4096 - off;
      if (n > left) n = left;
      u64 gpa = va;
      if (!phys && !host_walk(P, L, va, gpa)) {
        st = WTFGPU_ERR_TRANSLATE;
        break;
      }
      if (!lane_phys_write_block(P, L, gpa, src, n, lid)) {
        st = WTFGPU_ERR_OOM;
        break;
      }
      va += n;
      src += n;
      left -= n;
    }
    if (lid == 0) status_out[r] = st;
  }
  if (lid == 0) {
    P.ov_count[lane] = L.ovn;
    tlb_stale(P, lane);
  }
}

// Host-injected exception per lane (PageFaultsMemoryIfNeeded): delivered
// through the guest IDT now; the lane resumes at the handler.
__global__ void k_inject_fault(Dev P, const u32 *lanes, const u64 *addrs, u32 n, u32 vector, u32 error, i32 *ok) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 lane = lanes[t];
  u32 glo[16], ghi[16];
  Lane L;
  L.glo = glo;
  L.ghi = ghi;
  load_lane(P, lane, L);
  L.status = WTFGPU_EXIT_FAULT;
  L.exvec = vector;
  L.exerr = error;
  L.exaddr = addrs[t];
  const bool d = deliver_fault(P, L);
  ok[t] = d ? 1 : 0;
  if (d && g_tn.buf) {  // Tenet: the injected exception
    g_tn.ipos[lane] = g_tn.pos[lane];
    tn_regs(P, L);
  }
  if (d) {
    store_lane(P, L);
    tlb_stale(P, lane);
    P.lflags[lane] = 0;
  } else if (L.ovn > P.K && L.ovn != P.ov_count[lane]) {
    // the failed delivery claimed pool pages for the frame: they stay on the
    // lane's list (as k_run keeps them), so restore gives them back
    P.ov_count[lane] = L.ovn;
    tlb_stale(P, lane);
  }
}

// The declared insert of a lane list (wtfgpu_set_insert), after the feed
// scatter: lanes without a feed are left alone. The writes are not CPU
// accesses (Tenet does not log them).
__global__ void k_insert(Dev P, wtfgpu_insert_t ins, const u32 *lanes, u32 first, u32 n) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 lane = lanes ? lanes[t] : first + t;
  if (P.feed_pos[lane] == ~0ull || P.status[lane] != WTFGPU_RUNNING) return;
  u32 glo[16], ghi[16];
  Lane L;
  L.glo = glo;
  L.ghi = ghi;
  load_lane(P, lane, L);
  if (g_tn.buf) tn_mute(lane);
  insert_apply(P, L, ins);
  if (g_tn.buf) tn_unmute(lane, 0, 0, 0, false);
  store_lane(P, L);
  store_tlb(P, L);
}

// Lane status (+ skip-breakpoint-once flag) for a lane list (resume / stop).
__global__ void k_set_status(Dev P, const u32 *lanes, u32 n, u32 status, const u8 *skip) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 lane = lanes[t];
  P.status[lane] = status;
  if (skip) P.lflags[lane] = skip[t] ? 1u : (g_tn.buf ? 2u : 0u);  // 2: Tenet entry at the next launch
}

// Single-lane memory services for the host proxy.
// op 0: translate (out u64 gpa), 1: read phys, 2: write phys, 3: read virt, 4: write virt
__global__ void k_lane_mem(Dev P, u32 lane, u32 op, u64 addr, u64 len, u8 *buf, i64 *result) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Lane L;
  lane_min_load(P, lane, L);
  i64 rc = 0;
  if (op == 0) {
    u64 gpa;
    rc = host_walk(P, L, addr, gpa) ? (i64)gpa : -1;
  } else if (op == 1 || op == 3) {
    u64 a = addr;
    for (u64 i = 0; i < len;) {
      u64 gpa = a;
      if (op == 3 && !host_walk(P, L, a, gpa)) {
        rc = -1;
        break;
      }
      u64 n = 4096 - (a & 0xfff);
      if (n > len - i) n = len - i;
      bool priv;
      const u8 *pg = phys_page(P, L.lane, L.ovn, L.bloom, gpa >> 12, priv);
      for (u64 k = 0; k < n; k++) buf[i + k] = pg[(gpa & 0xfff) + k];
      i += n;
      a += n;
    }
  } else {
    u64 a = addr;
    for (u64 i = 0; i < len;) {
      u64 gpa = a;
      if (op == 4 && !host_walk(P, L, a, gpa)) {
        rc = -1;
        break;
      }
      u64 n = 4096 - (a & 0xfff);
      if (n > len - i) n = len - i;
      if (!lane_phys_write(P, L, gpa, buf + i, n)) {
        rc = -2;
        break;
      }
      i += n;
      a += n;
    }
    P.ov_count[lane] = L.ovn;
    tlb_stale(P, lane);
  }
  *result = rc;
}

// ---------------------------------------------------------------- bulk lane services
// GPRs + rip + rflags (18 u64, that order) of a lane list, gathered / scattered.
__global__ void k_gather_gprs(Dev P, const u32 *lanes, u32 n, u64 *out) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u64 N = P.nlanes, l = lanes[t];
  for (int i = 0; i < 16; i++) out[(u64)t * 18 + i] = P.gpr[i * N + l];
  out[(u64)t * 18 + 16] = P.rip[l];
  out[(u64)t * 18 + 17] = P.rflags[l];
}
__global__ void k_scatter_gprs(Dev P, const u32 *lanes, u32 n, const u64 *in) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u64 N = P.nlanes, l = lanes[t];
  for (int i = 0; i < 16; i++) P.gpr[i * N + l] = in[(u64)t * 18 + i];
  P.rip[l] = in[(u64)t * 18 + 16];
  P.rflags[l] = in[(u64)t * 18 + 17];
}
// Dirty lists of a lane list: out[t * (K + X + 1)] = count, then the gpfns
// (ov_gpfn's rows run on into the extension list).
__global__ void k_gather_dirty(Dev P, const u32 *lanes, u32 n, u32 *out) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 l = lanes[t], cnt = P.ov_count[l];
  u32 *o = out + (u64)t * (P.K + P.X + 1);
  o[0] = cnt;
  for (u32 k = 0; k < cnt && k < P.K + P.X; k++) o[1 + k] = P.ov_gpfn[(u64)k * P.nlanes + l];
}
// Lane views of physical pages (overlay copy, else snapshot, else zeros): one
// 256-thread block per (lane, gpa) request, 16 bytes per thread.
// `len` bytes (<= 256, within one page) at (lane, gpa) from each lane's view:
// one 64-thread block per record, 4 bytes per thread.
__global__ void k_gather_bytes(Dev P, const u32 *lanes, const u64 *gpas, u32 n, u32 len, u8 *out) {
  const u32 r = blockIdx.x;
  if (r >= n) return;
  const u32 l = lanes[r];
  const u64 gpa = gpas[r];
  const u32 ovn = P.ov_count[l];
  u64 bloom = 0;
  for (u32 k = 0; k < ovn; k++) bloom |= bloom_bit(P.ov_gpfn[(u64)k * P.nlanes + l]);
  bool priv;
  const u8 *src = phys_page(P, l, ovn, bloom, gpa >> 12, priv) + (gpa & 0xfff);
  for (u32 i = threadIdx.x; i < len; i += blockDim.x) out[(u64)r * len + i] = src[i];
}

__global__ void k_gather_pages(Dev P, const u32 *lanes, const u64 *gpas, u32 n, u8 *out) {
  const u32 r = blockIdx.x;
  if (r >= n) return;
  const u32 l = lanes[r];
  const u64 gpfn = gpas[r] >> 12;
  const u32 ovn = P.ov_count[l];
  u64 bloom = 0;
  for (u32 k = 0; k < ovn; k++) bloom |= bloom_bit(P.ov_gpfn[(u64)k * P.nlanes + l]);
  bool priv;
  const uint4 *src = (const uint4 *)phys_page(P, l, ovn, bloom, gpfn, priv);
  ((uint4 *)(out + (u64)r * WTFGPU_PAGE_SIZE))[threadIdx.x] = src[threadIdx.x];
}

// ---------------------------------------------------------------- coverage services
// The coverage sets of a lane list (lanes == nullptr: lanes first + i), one
// block per lane, compacted into (lane, rip) pairs.
__global__ void k_cov_collect(Dev P, const u32 *lanes, u32 first, u32 n, u32 *out_lane, u64 *out_rip, u64 cap,
                              unsigned long long *n_out, u32 *ovf) {
  const u32 i = blockIdx.x;
  if (i >= n) return;
  const u32 lane = lanes ? lanes[i] : first + i;
  const u32 g = P.lane_gen[lane];
  const u64 base = (u64)lane * P.H;
  for (u32 k = threadIdx.x; k < P.H; k += blockDim.x) {
    if (P.cov_gen[base + k] != g) continue;
    const unsigned long long pos = atomicAdd(n_out, 1ull);
    if (pos < cap) {
      out_lane[pos] = lane;
      out_rip[pos] = P.cov_rip[base + k];
    }
  }
  if (threadIdx.x == 0 && P.cov_overflow[lane]) atomicOr(ovf, 1u);
}

// The coverage sets of the stopped lanes of [first, first + count) (status
// neither RUNNING nor IDLE: the lanes a slice finished or left at a host
// breakpoint), compacted as k_cov_collect does (wtfgpu_prefetch_coverage).
// One wave per lane; an empty set (cov_cnt 0, the common case once the
// coverage has settled) costs one load.
__global__ void k_cov_collect_stopped(Dev P, u32 first, u32 count, u32 *out_lane, u64 *out_rip, u64 cap,
                                      unsigned long long *n_out, u32 *ovf) {
  const u32 i = blockIdx.x * 4 + (threadIdx.x >> 6), lid = threadIdx.x & 63;
  if (i >= count) return;
  const u32 lane = first + i;
  const u32 st = P.status[lane];
  if (st == WTFGPU_RUNNING || st == WTFGPU_EXIT_IDLE) return;
  if (P.cov_overflow[lane] && lid == 0) atomicOr(ovf, 1u);
  if (P.cov_cnt[lane] == 0) return;
  const u32 g = P.lane_gen[lane];
  const u64 base = (u64)lane * P.H;
  for (u32 k = lid; k < P.H; k += 64) {
    if (P.cov_gen[base + k] != g) continue;
    const unsigned long long pos = atomicAdd(n_out, 1ull);
    if (pos < cap) {
      out_lane[pos] = lane;
      out_rip[pos] = P.cov_rip[base + k];
    }
  }
}

// Rdrand seeds of a lane list: gathered into / scattered from buf.
__global__ void k_lane_seeds(Dev P, const u32 *lanes, u32 n, u64 *buf, int write) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (write) P.rd_seed[lanes[i]] = buf[i];
  else buf[i] = P.rd_seed[lanes[i]];
}

// STOP_ARGS arguments of a lane list (6 u64 each).
__global__ void k_stop_args(Dev P, const u32 *lanes, u32 n, u64 *out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6) return;
  out[i] = P.stop_args[(u64)lanes[i / 6] * 6 + i % 6];
}

// Exit records of lanes [first, first + count) (wtfgpu_read_exits).
__global__ void k_pack_exits(Dev P, u32 first, u32 count, wtfgpu_exit_t *out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u32 lane = first + i;
  wtfgpu_exit_t e;
  e.status = P.status[lane];
  e.vector = e.error = e.opcode = 0;
  e.addr = 0;
  if (e.status == WTFGPU_EXIT_FAULT) {
    const ExitInfo x = P.exinfo[lane];
    e.vector = x.vector;
    e.error = x.error;
    e.addr = x.addr;
    e.opcode = x.cpl;
  } else if (e.status == WTFGPU_EXIT_UNIMPLEMENTED) {
    e.opcode = P.exinfo[lane].opcode;
  }
  e.rip = P.rip[lane];
  e.icount = P.icount[lane];
  out[i] = e;
}

// Regrouping keys: running lanes by rip (lanes at one rip become neighbours,
// so one wave step serves them all), every other lane after them (their
// waves find nothing to run and leave at once).
// They also count the running lanes (P.stat[3]): a launch with none returns at once.
__global__ void k_regroup_keys(Dev P, u32 first, u32 count, u32 *keys, u32 *lanes) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < count;
  const u32 lane = first + (in ? i : 0);
  const bool run = in && P.status[lane] == WTFGPU_RUNNING;
  const u64 m = __ballot(run);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long *)&P.stat[3], (unsigned long long)__popcll(m));
  if (!in) return;
  const u32 r = (u32)P.rip[lane] & 0xffffffu;  // 24 key bits: three radix passes
  keys[i] = run ? (r == 0xffffffu ? r - 1 : r) : 0xffffffu;
  lanes[i] = lane;
}

// Empty the coverage sets of a lane list (generation bump: O(1) per lane).
__global__ void k_cov_clear(Dev P, const u32 *lanes, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 lane = lanes[i];
  P.lane_gen[lane] += 1;
  P.cov_cnt[lane] = 0;
  P.cov_overflow[lane] = 0;
}

// Bytes set in the coverage map but not in its shadow (what a MAX all-reduce
// brought in from other shards since the last look), as byte indices; with
// `write`, the shadow catches up with the map. Sixteen bytes per thread.
__global__ void k_cov_absorb(const u8 *map, u8 *shadow, u64 n16, u64 *out_idx, u64 cap,
                             unsigned long long *count, int write) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n16) return;
  const uint4 m = ((const uint4 *)map)[t], s = ((const uint4 *)shadow)[t];
  if (m.x == s.x && m.y == s.y && m.z == s.z && m.w == s.w) return;
  const u32 mw[4] = {m.x, m.y, m.z, m.w}, sw[4] = {s.x, s.y, s.z, s.w};
  for (int w = 0; w < 4; w++)
    for (int b = 0; b < 4; b++)
      if (((mw[w] >> (8 * b)) & 0xff) && !((sw[w] >> (8 * b)) & 0xff)) {
        const unsigned long long pos = atomicAdd(count, 1ull);
        if (write && pos < cap) out_idx[pos] = t * 16 + w * 4 + b;
      }
  if (write) ((uint4 *)shadow)[t] = m;
}

// A merged map from the other shards (bytes are 0 / 1, so OR is the MAX):
// the deferred shard merge (CoverageExchange_t::MergeEnd); k_cov_absorb then
// reports what it added.
__global__ void k_cov_merge_in(uint4 *map, const uint4 *src, u64 n16) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n16) return;
  const uint4 a = map[t], b = src[t];
  if ((b.x & ~a.x) | (b.y & ~a.y) | (b.z & ~a.z) | (b.w & ~a.w)) map[t] = uint4{a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w};
}

// Per-lane feed regions (streaming): `n` lanes, lane lanes[i] gets
// len[i] bytes from src + off[i] at its region.
// Lane i's feed: bytes [off[i], off[i + 1]) of src into the lane's region, its
// read position and end set; a lane without a feed (has[i] = 0) or with one
// larger than its region keeps none (the host handler serves it).
__global__ void k_feed_scatter(u8 *feed, u64 stride, const u32 *lanes, const u64 *off, const u8 *has, u32 n,
                               const u8 *src, u64 *feed_pos, u64 *feed_end) {
  const u32 i = blockIdx.x;
  if (i >= n) return;
  const u32 lane = lanes[i];
  const u64 o = off[i], len = off[i + 1] - o;
  const bool keep = (!has || has[i]) && len <= stride;
  if (threadIdx.x == 0) {
    feed_pos[lane] = keep ? (u64)lane * stride : ~0ull;
    feed_end[lane] = keep ? (u64)lane * stride + len : 0;
  }
  if (!keep) return;
  u8 *dst = feed + (u64)lane * stride;
  const u8 *sp = src + o;
  for (u64 k = threadIdx.x; k < len; k += blockDim.x) dst[k] = sp[k];
}

// The device mutator (wtfgpu_mutate_feed_lanes; engine_mutate.h defines the
// stream): one wave per testcase, MUT_WAVES testcases a block. Testcase i is
// (seed, index[i]) over the first ncorpus[i] corpus entries; every decision
// of its plan depends on those alone, so all 64 lanes compute the same plan
// and then write the chunk k_feed_scatter would have copied, a little-endian
// u32 size and the bytes, four bytes a lane a round (the region and the bytes
// after the size are 4-aligned; the last word is zero-padded, inside the
// region: size <= max_len <= stride - 4).
constexpr u32 MUT_WAVES = 4;
__global__ __launch_bounds__(64 * MUT_WAVES) void k_mutate_feeds(u8 *feed, u64 stride, const u32 *lanes,
                                                                 const u64 *index, const u32 *ncorpus, u32 n, u64 seed,
                                                                 u32 max_len, const u8 *arena, const u64 *arena_off,
                                                                 u64 *feed_pos, u64 *feed_end) {
  const u32 i = blockIdx.x * MUT_WAVES + threadIdx.x / 64, l = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = lanes[i];
  wtfmut::Plan p;
  wtfmut::make_plan(p, seed, index[i], wtfmut::Corpus{arena, arena_off}, ncorpus[i], max_len);
  u8 *dst = feed + (u64)lane * stride;
  if (l == 0) {
    feed_pos[lane] = (u64)lane * stride;
    feed_end[lane] = (u64)lane * stride + 4 + p.size;
    *(u32 *)dst = p.size;
  }
  for (u32 j = 4 * l; j < p.size; j += 256) {
    u32 w = 0;
    for (u32 k = 0; k < 4; k++)
      if (j + k < p.size) w |= (u32)wtfmut::plan_byte(p, j + k) << (8 * k);
    *(u32 *)(dst + 4 + j) = w;
  }
}

// wtfgpu_read_feed_lanes: the first chunk of each listed lane's feed region
// (the testcase, which stays there after k_insert has consumed the feed), cut
// to `room` bytes, one block a lane. len ~0u: the lane has no feed.
__global__ void k_feed_gather(const u8 *feed, u64 stride, const u32 *lanes, u32 n, const u64 *feed_pos, u32 *lens,
                              u8 *out, u64 room) {
  const u32 i = blockIdx.x;
  if (i >= n) return;
  const u32 lane = lanes[i];
  const bool has = feed_pos[lane] != ~0ull;
  const u8 *src = feed + (u64)lane * stride;
  u64 len = has ? (u64)src[0] | ((u64)src[1] << 8) | ((u64)src[2] << 16) | ((u64)src[3] << 24) : 0;
  if (len > stride - 4) len = stride - 4;
  if (threadIdx.x == 0) lens[i] = has ? (u32)len : ~0u;
  if (len > room) len = room;
  for (u64 k = threadIdx.x; k < len; k += blockDim.x) out[(u64)i * room + k] = src[4 + k];
}

// The device packet mutator (wtfgpu_mutate_packets_lanes;
// engine_mutate_packets.h defines the stream): one wave per testcase,
// MUT_WAVES a block, as k_mutate_feeds. The feed is the chunks themselves from
// the region's first byte, four bytes a lane a round. Chunks are 12 + body
// bytes long, so neither a chunk nor a source run is 4-aligned: every word is
// composed byte by byte through the plan. The last word is zero-padded and
// stays inside the region: size <= MaxFeed <= stride, a multiple of 4.
//
// A mutated testcase is a wave-uniform plan over the base entry. A generated
// one has no base: lane p < N computes packet p's three header words from its
// four direct draws, an exclusive prefix over the chunk sizes gives each chunk
// its place (lanes >= N hold the end), and each output word finds its chunk by
// a search over the lanes' places; what is not a header byte is zero. Every
// cross-lane read happens with all 64 lanes active (the round loops are
// wave-uniform; only the store is predicated).
__global__ __launch_bounds__(64 * MUT_WAVES) void k_mutate_packets(u8 *feed, u64 stride, const u32 *lanes,
                                                                   const u64 *index, const u32 *ncorpus, u32 n,
                                                                   u64 seed, wtfpkt::Params q, const u8 *arena,
                                                                   const u64 *arena_off, u64 *feed_pos,
                                                                   u64 *feed_end) {
  const u32 i = blockIdx.x * MUT_WAVES + threadIdx.x / 64, l = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = lanes[i];
  u8 *dst = feed + (u64)lane * stride;
  wtfmut::Rng g(seed, index[i]);
  const u64 s0 = g.s;
  u32 size;
  if (g.R(5) == 4) {
    const u32 N = (u32)g.R(q.GenMaxPackets) + 1;
    const wtfpkt::GenPacket k = wtfpkt::gen_packet(s0, l, q);
    const u32 len = l < N ? 4 + k.w[0] : 0;
    u32 incl = len;  // inclusive prefix over the wave
    for (u32 d = 1; d < 64; d <<= 1) {
      const u32 up = __shfl_up(incl, d);
      if (l >= d) incl += up;
    }
    size = __shfl(incl, 63);
    const u32 at = l < N ? incl - len : ~0u;  // this lane's chunk starts here; no chunk: past every byte
    for (u32 j0 = 0; j0 < size; j0 += 256) {
      const u32 j = j0 + 4 * l;
      u32 c = 0;  // the last chunk that starts at or before byte j (chunk 0 starts at 0)
      for (u32 d = 32; d; d >>= 1)
        if (__shfl(at, c + d) <= j) c += d;
      const u32 c1 = c < 63 ? c + 1 : 63;  // a word meets at most one boundary: chunks have 12 bytes or more
      const u32 at0 = __shfl(at, c), at1 = __shfl(at, c1);
      const u32 a0 = __shfl(k.w[0], c), a1 = __shfl(k.w[1], c), a2 = __shfl(k.w[2], c);
      const u32 b0 = __shfl(k.w[0], c1), b1 = __shfl(k.w[1], c1), b2 = __shfl(k.w[2], c1);
      u32 w = 0;
      for (u32 b = 0; b < 4; b++) {
        const u32 pos = j + b;
        if (pos >= size) break;
        const bool nx = c1 != c && pos >= at1;
        const u32 r = pos - (nx ? at1 : at0);
        if (r < 12) {
          const u32 h = r < 4 ? (nx ? b0 : a0) : r < 8 ? (nx ? b1 : a1) : (nx ? b2 : a2);
          w |= ((h >> (8 * (r & 3))) & 0xff) << (8 * b);
        }
      }
      if (j < size) *(u32 *)(dst + j) = w;
    }
  } else {
    wtfpkt::Plan p;
    wtfpkt::make_plan(p, g, wtfmut::Corpus{arena, arena_off}, ncorpus[i], q);
    size = p.size;
    for (u32 j = 4 * l; j < size; j += 256) {
      u32 w = 0;
      for (u32 k = 0; k < 4; k++)
        if (j + k < size) w |= (u32)wtfpkt::plan_byte(p, j + k) << (8 * k);
      *(u32 *)(dst + j) = w;
    }
  }
  if (l == 0) {
    feed_pos[lane] = (u64)lane * stride;
    feed_end[lane] = (u64)lane * stride + size;
  }
}

// The minimiser's candidates (wtfgpu_minimize_feed_lanes; engine_minimize.h
// defines the stream): one wave per candidate, MUT_WAVES a block, as the two
// mutators. Candidate i is index[i] of `op` over arena entry `entry`; its
// level, range and plan depend on those alone, so all 64 lanes compute the
// same plan and then write four bytes a lane a round. A byte-buffer arena
// (feeds == 0) gets the chunk k_mutate_feeds writes: a little-endian u32 size
// and the bytes from region + 4, the last word zero-padded inside the region
// (size <= stride - 4: the call refuses a longer entry). A feed arena gets the
// whole feed from the region's first byte, as k_mutate_packets writes it
// (size <= stride). The tail is the base shifted by any byte count, so its
// words are composed byte by byte through the plan; a head word is loaded
// whole only where it lies wholly in the head and its source is 4-aligned
// (the destination always is). No LDS, and the plan stays in registers.
__global__ __launch_bounds__(64 * MUT_WAVES) void k_minimize_feeds(u8 *feed, u64 stride, const u32 *lanes,
                                                                   const u64 *index, u32 n, u32 entry, u32 op,
                                                                   u32 feeds, const u8 *arena, const u64 *arena_off,
                                                                   u64 *feed_pos, u64 *feed_end) {
  const u32 i = blockIdx.x * MUT_WAVES + threadIdx.x / 64, l = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = lanes[i];
  wtfmin::Plan p;
  wtfmin::make_plan(p, wtfmut::Corpus{arena, arena_off}, entry, feeds != 0, op, index[i]);
  const u32 skip = feeds ? 0 : 4;
  u8 *dst = feed + (u64)lane * stride;
  if (l == 0) {
    feed_pos[lane] = (u64)lane * stride;
    feed_end[lane] = (u64)lane * stride + skip + p.size;
    if (!feeds) *(u32 *)dst = p.size;
  }
  const bool aligned = ((u64)p.base & 3) == 0;
  for (u32 j = 4 * l; j < p.size; j += 256) {
    u32 w = 0;
    if (aligned && j + 4 <= p.a) {
      w = *(const u32 *)(p.base + j);
    } else {
      for (u32 k = 0; k < 4; k++)
        if (j + k < p.size) w |= (u32)wtfmin::plan_byte(p, j + k) << (8 * k);
    }
    *(u32 *)(dst + skip + j) = w;
  }
}

// The analyzer's candidates (wtfgpu_analyze_feed_lanes; engine_analyze.h
// defines the stream): one wave per candidate, MUT_WAVES a block, four bytes a
// lane a round, into the two layouts k_minimize_feeds writes. Candidate i is
// the base (arena entry `entry`) with byte index[i] / 4 replaced by variant
// index[i] % 4 of it, so the size is the base's and all 64 lanes share the
// plan. The changed byte lies in exactly one destination word, and that word
// is composed byte by byte, as is the last, partial word (zero-padded inside
// the region: size <= stride - 4 for a byte buffer, the call refuses a longer
// entry; size <= stride for a feed) and every word of a base that is not
// 4-aligned in the arena; all other words are loaded whole. No LDS, and the
// plan stays in registers.
__global__ __launch_bounds__(64 * MUT_WAVES) void k_analyze_feeds(u8 *feed, u64 stride, const u32 *lanes,
                                                                  const u64 *index, u32 n, u32 entry, u32 feeds,
                                                                  const u8 *arena, const u64 *arena_off,
                                                                  u64 *feed_pos, u64 *feed_end) {
  const u32 i = blockIdx.x * MUT_WAVES + threadIdx.x / 64, l = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = lanes[i];
  wtfana::Plan p;
  wtfana::make_plan(p, wtfmut::Corpus{arena, arena_off}, entry, feeds != 0, index[i]);
  const u32 skip = feeds ? 0 : 4;
  u8 *dst = feed + (u64)lane * stride;
  if (l == 0) {
    feed_pos[lane] = (u64)lane * stride;
    feed_end[lane] = (u64)lane * stride + skip + p.size;
    if (!feeds) *(u32 *)dst = p.size;
  }
  const bool aligned = ((u64)p.base & 3) == 0;
  for (u32 j = 4 * l; j < p.size; j += 256) {
    u32 w = 0;
    if (aligned && j + 4 <= p.size && (p.p & ~3u) != j) {
      w = *(const u32 *)(p.base + j);
    } else {
      for (u32 k = 0; k < 4; k++)
        if (j + k < p.size) w |= (u32)wtfana::plan_byte(p, j + k) << (8 * k);
    }
    *(u32 *)(dst + skip + j) = w;
  }
}

// wtfgpu_read_whole_feed_lanes: each listed lane's whole feed, from its
// region's first byte to feed_end (which nothing moves after the feed is
// written: k_run and k_insert advance feed_pos only), cut to `room` bytes, one
// block a lane. len ~0u: the lane has no feed.
__global__ void k_feed_gather_whole(const u8 *feed, u64 stride, const u32 *lanes, u32 n, const u64 *feed_pos,
                                    const u64 *feed_end, u32 *lens, u8 *out, u64 room) {
  const u32 i = blockIdx.x;
  if (i >= n) return;
  const u32 lane = lanes[i];
  const bool has = feed_pos[lane] != ~0ull;
  const u8 *src = feed + (u64)lane * stride;
  u64 len = has ? feed_end[lane] - (u64)lane * stride : 0;
  if (len > stride) len = stride;
  if (threadIdx.x == 0) lens[i] = has ? (u32)len : ~0u;
  if (len > room) len = room;
  for (u64 k = threadIdx.x; k < len; k += blockDim.x) out[(u64)i * room + k] = src[k];
}

// wtfgpu_read_feeds_packed (engine_feedpack.h defines the layout): each listed
// lane's length, as k_feed_gather (whole == 0) or k_feed_gather_whole gives
// it, and its padded length for the scan; padded[n] = 0, so that the
// exclusive sum over n + 1 values ends with the total.
__global__ void k_feed_lens(const u8 *feed, u64 stride, const u32 *lanes, u32 n, const u64 *feed_pos,
                            const u64 *feed_end, u32 whole, u32 *lens, u64 *padded) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    padded[n] = 0;
    return;
  }
  const u32 lane = lanes[i];
  const u64 region = (u64)lane * stride;
  const bool has = feed_pos[lane] != ~0ull;
  const u32 len = whole ? wtffeedpack::whole_len(has, has ? feed_end[lane] : 0, region, stride)
                        : wtffeedpack::chunk_len(has, has ? *(const u32 *)(feed + region) : 0, stride);
  lens[i] = len;
  padded[i] = wtffeedpack::pad16(len);
}

// The copy: one wave per listed lane, MUT_WAVES a block, 16 bytes a thread a
// round, exactly pad16(lens[i]) bytes at out + offs[i] (lens and offs are what
// k_feed_lens and the scan left, not read again from the feed: what is
// written is what was sized). A region is 16 KiB-aligned and a place
// 16-aligned, so whole feeds move as 16-byte loads and stores; a chunk starts
// at region + 4, 4-aligned only, and is loaded a word at a time. A word is
// loaded only if it starts below len, which keeps every load inside the
// region (len <= stride - skip, a multiple of 4), and the bytes at and after
// len are masked to zero: the padding. The round loop is wave-uniform.
__global__ __launch_bounds__(64 * MUT_WAVES) void k_feed_pack(const u8 *feed, u64 stride, const u32 *lanes, u32 n,
                                                              u32 whole, const u32 *lens, const u64 *offs, u8 *out) {
  const u32 i = blockIdx.x * MUT_WAVES + threadIdx.x / 64, l = threadIdx.x & 63;
  if (i >= n) return;
  const u32 len = lens[i];
  if (len == wtffeedpack::kNoFeed) return;
  const u32 padded = (u32)wtffeedpack::pad16(len);
  const u8 *src = feed + (u64)lanes[i] * stride + (whole ? 0 : 4);
  u8 *dst = out + offs[i];
  for (u32 j0 = 0; j0 < padded; j0 += 16 * 64) {
    const u32 j = j0 + 16 * l;
    if (j >= padded) continue;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (whole) {
      v = *(const uint4 *)(src + j);  // j < padded <= stride: inside the region
    } else {
      if (j < len) v.x = *(const u32 *)(src + j);
      if (j + 4 < len) v.y = *(const u32 *)(src + j + 4);
      if (j + 8 < len) v.z = *(const u32 *)(src + j + 8);
      if (j + 12 < len) v.w = *(const u32 *)(src + j + 12);
    }
    v.x = wtffeedpack::mask_word(v.x, j, len);
    v.y = wtffeedpack::mask_word(v.y, j + 4, len);
    v.z = wtffeedpack::mask_word(v.z, j + 8, len);
    v.w = wtffeedpack::mask_word(v.w, j + 12, len);
    *(uint4 *)(dst + j) = v;
  }
}

__global__ void k_cov_commit(Dev P, const u64 *rips, u64 n) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || !P.code_keys) return;
  const u64 rip = rips[t];
  u32 h = (u32)mix64(rip >> 12) & P.code_mask;
  for (u32 i = 0; i <= P.code_mask; i++) {
    const u64 k = P.code_keys[h];
    if (k == rip >> 12) {
      const u64 at = (u64)P.code_slot[h] * WTFGPU_PAGE_SIZE + (rip & 0xfff);
      P.cov_map[at] = 1;
      P.cov_shadow[at] = 1;  // this shard's own find: not reported by absorb
      return;
    }
    if (k == EMPTY_KEY) break;
    h = (h + 1) & P.code_mask;
  }
  // not a code byte of a code page (a rip elsewhere, an edge): the extra set,
  // kept at most 3/4 full (a value that does not fit is logged again later)
  if (!P.extra_keys || rip == EMPTY_KEY) return;
  u32 g = (u32)mix64(rip) & P.extra_mask;
  for (u32 i = 0; i <= P.extra_mask / 4; i++) {
    const unsigned long long prev = atomicCAS((unsigned long long *)&P.extra_keys[g], EMPTY_KEY, rip);
    if (prev == EMPTY_KEY || prev == rip) return;
    g = (g + 1) & P.extra_mask;
  }
}

// ---------------------------------------------------------------- coverage attribution
// wtfgpu_attribute_coverage: the listed lanes' new values, attributed in list
// order against the device aggregate. Position i of the list owns the values
// of lane lanes[i]; every kernel here runs one wave per position or one thread
// per candidate, and no result depends on which wave wins an atomic.

// Is v in the device aggregate: its byte of cov_map when its page is a code
// page, the extra set otherwise (where k_cov_commit put it).
__device__ __forceinline__ bool cov_has(const Dev &P, u64 v) {
  if (P.code_keys) {
    u32 h = (u32)mix64(v >> 12) & P.code_mask;
    for (u32 i = 0; i <= P.code_mask; i++) {
      const u64 k = P.code_keys[h];
      if (k == v >> 12) return P.cov_map[(u64)P.code_slot[h] * WTFGPU_PAGE_SIZE + (v & 0xfff)] != 0;
      if (k == EMPTY_KEY) break;
      h = (h + 1) & P.code_mask;
    }
  }
  return P.extra_keys && v != EMPTY_KEY && set_has(P.extra_keys, P.extra_mask, v);
}

// Pass 1 (out == nullptr): cnt[i] = the candidates of position i (live entries
// absent from the aggregate; with `all`, every live entry), plus the raw live
// entries and the overflow flags of the list. An empty set costs one load.
// Pass 2 (out != nullptr): the same walk writes the candidates to
// out[off[i] ...], in slot order (ballot prefix: one order whatever the timing).
__global__ void k_attr_scan(Dev P, const u32 *lanes, u32 n, u32 all, u32 *cnt, const u32 *off, u64 *out,
                            unsigned long long *entries, u32 *ovf) {
  const u32 i = rfl32(blockIdx.x * 4 + (threadIdx.x >> 6)), lid = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = rfl32(lanes[i]);
  if (!out && lid == 0 && P.cov_overflow[lane]) atomicOr(ovf, 1u);
  u32 live = 0, keep = 0;
  if (P.cov_cnt[lane]) {
    const u32 g = P.lane_gen[lane], H = P.H;
    const u64 base = (u64)lane * H;
    const u32 at = out ? off[i] : 0, end = out ? off[i + 1] : 0;  // (off has n + 1 entries)
    for (u32 k0 = 0; k0 < H; k0 += 64) {
      const u32 k = k0 + lid;
      const bool lv = k < H && P.cov_gen[base + k] == g;
      const u64 v = lv ? P.cov_rip[base + k] : 0;
      const bool kp = lv && (all || !cov_has(P, v));
      const u64 mk = __ballot(kp);
      const u32 to = at + keep + __popcll(mk & ((1ull << lid) - 1));
      if (out && kp && to < end) out[to] = v;
      live += __popcll(__ballot(lv));
      keep += __popcll(mk);
    }
  }
  if (out || lid) return;
  cnt[i] = keep;
  if (live) atomicAdd(entries, (unsigned long long)live);
}

// Position i's candidates sorted: each one's rank among them is its place (a
// set holds a value once; equal values would keep their slot order). The
// candidates of a lane are a handful once a campaign has warmed up.
__global__ void k_attr_sort(const u32 *cnt, const u32 *off, u32 n, const u64 *in, u64 *vals, u32 *pos) {
  const u32 i = rfl32(blockIdx.x * 4 + (threadIdx.x >> 6)), lid = threadIdx.x & 63;
  if (i >= n) return;
  const u32 c = rfl32(cnt[i]);
  const u64 o = rfl32(off[i]);
  for (u32 e = lid; e < c; e += 64) {
    const u64 v = in[o + e];
    u32 r = 0;
    for (u32 j = 0; j < c; j++) {
      const u64 w = in[o + j];
      r += (w < v || (w == v && j < e)) ? 1u : 0u;
    }
    vals[o + r] = v;
    pos[o + r] = i;
  }
}

// First owner: own[slot of v] = the smallest position among v's owners that
// are not revoked (~0: none). keys / own are T + 1 entries, all bits set; the
// last serves the one value that equals the empty key. T >= 2 * s.
__global__ void k_attr_owner(const u64 *vals, const u32 *pos, u32 s, const u8 *revoke, u64 *keys, u32 *own, u32 T,
                             u32 *slot_of) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s) return;
  const u64 v = vals[j];
  u32 h = T;
  if (v != EMPTY_KEY) {
    h = (u32)mix64(v) & (T - 1);
    for (u32 t = 0; t < T; t++) {
      const unsigned long long prev = atomicCAS((unsigned long long *)&keys[h], EMPTY_KEY, v);
      if (prev == EMPTY_KEY || prev == v) break;
      h = (h + 1) & (T - 1);
    }
  }
  slot_of[j] = h;
  if (!revoke[pos[j]]) atomicMin(&own[h], pos[j]);
}

// Candidate j is emitted iff its position is at most its value's first owner.
__global__ void k_attr_keep(const u32 *pos, const u32 *slot_of, const u32 *own, u32 s, u32 *flag) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > s) return;
  flag[j] = j < s && pos[j] <= own[slot_of[j]] ? 1u : 0u;  // flag[s] = 0: the scan's last sum is the total
}

// The emitted candidates keep their (position, value) order: at[] is the
// exclusive scan of flag[].
__global__ void k_attr_emit(const u64 *vals, const u32 *pos, const u32 *flag, const u32 *at, u32 s, u32 *out_pos,
                            u64 *out_vals) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s || !flag[j]) return;
  out_pos[at[j]] = pos[j];
  out_vals[at[j]] = vals[j];
}

// ---- keeping coverage (wtfgpu_coverage_contains; engine_covkeep.h defines the rule)
// For position i of the list: how many of the target's nt values lane
// lanes[i]'s set lacks, the set's live entries and its overflow flag. One wave
// per position, four a block; the lane, its generation and its entry count are
// the wave's. The wave strides over the target 64 values a step, each thread
// probing the lane's table for its value (engine_covkeep.h's probe, as
// log_value inserts); the ballot of "absent" is the step's count, the same in
// every thread. The count is exact (no early exit). An empty set (cov_cnt 0)
// costs one load: everything is missing. It reads the sets and changes
// nothing; the caller checked the list and the target.
__global__ __launch_bounds__(256) void k_cov_contains(Dev P, const u32 *lanes, u32 n, const u64 *target, u32 nt,
                                                      u32 *missing, u32 *size, u32 *overflow) {
  const u32 i = rfl32(blockIdx.x * 4 + (threadIdx.x >> 6)), lid = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = rfl32(lanes[i]);
  const u32 cnt = rfl32(P.cov_cnt[lane]);
  u32 miss = nt;
  if (cnt) {
    const u32 g = rfl32(P.lane_gen[lane]), H = P.H;
    const u64 *rip = P.cov_rip + (u64)lane * H;
    const u32 *gen = P.cov_gen + (u64)lane * H;
    miss = 0;
    for (u32 t0 = 0; t0 < nt; t0 += 64) {
      const u32 t = t0 + lid;
      const bool absent = t < nt && !wtfkeep::table_has(rip, gen, H, g, target[t]);
      miss += (u32)__popcll(__ballot(absent));
    }
  }
  if (lid) return;
  missing[i] = miss;
  size[i] = cnt;
  overflow[i] = P.cov_overflow[lane] ? 1u : 0u;
}

// ---- a set's signature (wtfgpu_coverage_signature; engine_analyze.h defines it)
// For position i of the list: the wrap-around sum of mix64 over the values of
// lane lanes[i]'s set, the set's live entries and its overflow flag. One wave
// per position, four a block; the lane, its generation and its entry count are
// the wave's. The wave strides over the lane's H slots 64 a step, gen then
// rip, both coalesced; a thread adds mix64(rip) of its slot to a private sum
// where the slot is live (gen == g). The ballot of "live" is the step's count,
// the same in every thread, and the scan stops once the running count reaches
// cov_cnt (the set's live slots, as log_value counts them). One 64-lane
// shuffle reduction at the end. An empty set (cov_cnt 0) costs one load and
// gives (0, 0). It reads the sets and changes nothing; the caller checked the
// list.
__global__ __launch_bounds__(256) void k_cov_signature(Dev P, const u32 *lanes, u32 n, u64 *sig, u32 *size,
                                                       u32 *overflow) {
  const u32 i = rfl32(blockIdx.x * 4 + (threadIdx.x >> 6)), lid = threadIdx.x & 63;
  if (i >= n) return;
  const u32 lane = rfl32(lanes[i]);
  const u32 cnt = rfl32(P.cov_cnt[lane]);
  u64 sum = 0;
  if (cnt) {
    const u32 g = rfl32(P.lane_gen[lane]), H = P.H;
    const u64 *rip = P.cov_rip + (u64)lane * H;
    const u32 *gen = P.cov_gen + (u64)lane * H;
    u32 seen = 0;
    for (u32 h0 = 0; h0 < H && seen < cnt; h0 += 64) {
      const u32 h = h0 + lid;
      const bool live = h < H && gen[h] == g;
      if (live) sum += wtfkeep::mix64(rip[h]);
      seen += (u32)__popcll(__ballot(live));
    }
    for (u32 d = 32; d; d >>= 1) {
      const u32 lo = __shfl_xor((u32)sum, d, 64), hi = __shfl_xor((u32)(sum >> 32), d, 64);
      sum += ((u64)hi << 32) | lo;
    }
  }
  if (lid) return;
  sig[i] = sum;
  size[i] = cnt;
  overflow[i] = P.cov_overflow[lane] ? 1u : 0u;
}

// ---- the corpus distiller (wtfgpu_distill; engine_distill.h defines the rule)
// The words a call's kernels share: the round's running maximum key (0: none
// yet), `done` once a round found no gain, and how many sets are taken.
struct DistillState {
  u64 key;
  u32 done, kept;
};
constexpr u32 DIS_GROUP = 16;   // lanes that count one set
constexpr u32 DIS_BLOCK = 256;  // 16 sets a block
constexpr u32 DIS_BATCH = 64;   // rounds queued between two looks at `done`

// Each entry's dense id: its value's place in the sorted unique values.
__global__ __launch_bounds__(DIS_BLOCK) void k_distill_ids(const u64 *vals, u64 entries, const u64 *uniq, u32 universe,
                                                           u32 *ids) {
  const u64 e = (u64)blockIdx.x * DIS_BLOCK + threadIdx.x;
  if (e >= entries) return;
  const u64 v = vals[e];
  u32 lo = 0, hi = universe;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (uniq[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  ids[e] = lo;
}

// One round's gains. DIS_GROUP lanes count one set: sets run from none to
// 8,192 entries and most hold a few hundred, so a wave a set would idle most
// lanes on the short ones, while 16 lanes still read 64 contiguous bytes of
// ids a step and four sets share a wave. A group leaves at one load when its
// set is dead (gain 0: `covered` only grows, so it stays 0) and at two when
// the set's stale key is below the round's running maximum (engine_distill.h,
// lazy evaluation; a running maximum read late only prunes less). The group's
// lanes stay together (every condition is the group's), so a ballot's 16 bits
// of the group are the step's absent ids. One atomicMax a counted set.
__global__ __launch_bounds__(DIS_BLOCK) void k_distill_gain(const u32 *off, const u32 *ids, u32 sets,
                                                            const u32 *bitmap, u32 *gain, DistillState *st) {
  if (st->done) return;
  const u64 t = (u64)blockIdx.x * DIS_BLOCK + threadIdx.x;
  const u32 s = (u32)(t / DIS_GROUP), l = threadIdx.x % DIS_GROUP, shift = (threadIdx.x & 63) / DIS_GROUP * DIS_GROUP;
  if (s >= sets) return;
  const u32 stale = gain[s];
  if (stale == 0) return;
  const u64 running = __hip_atomic_load(&st->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wtfdis::make_key(stale, s) < running) return;
  const u64 lo = off[s], hi = off[s + 1];
  u32 g = 0;
  for (u64 b = lo; b < hi; b += DIS_GROUP) {
    const u64 j = b + l;
    const bool absent = j < hi && !wtfdis::covered(bitmap, ids[j]);
    g += __popcll((__ballot(absent) >> shift) & ((1ull << DIS_GROUP) - 1));
  }
  if (l == 0) {
    gain[s] = g;
    if (g) atomicMax((unsigned long long *)&st->key, (unsigned long long)wtfdis::make_key(g, s));
  }
}

// One round's take, one block: the key's set joins `covered` (ids of one set
// share bitmap words: atomicOr), is appended to the output and marked dead;
// no key means the cover is complete. The bitmap reaches the next round's
// k_distill_gain through the kernel boundary.
__global__ __launch_bounds__(DIS_BLOCK) void k_distill_take(const u32 *off, const u32 *ids, u32 *bitmap, u32 *gain,
                                                            DistillState *st, u32 *out_index, u32 *out_gain) {
  if (st->done) return;
  const u64 key = st->key;
  __syncthreads();  // every thread has the key before thread 0 clears it
  if (key == 0) {
    if (threadIdx.x == 0) st->done = 1;
    return;
  }
  const u32 s = wtfdis::key_index(key);
  for (u64 j = (u64)off[s] + threadIdx.x; j < off[s + 1]; j += DIS_BLOCK) atomicOr(&bitmap[ids[j] >> 5], 1u << (ids[j] & 31));
  if (threadIdx.x == 0) {
    const u32 k = st->kept;
    out_index[k] = s;
    out_gain[k] = wtfdis::key_gain(key);
    st->kept = k + 1;
    gain[s] = 0;
    st->key = 0;
  }
}

}  // namespace
