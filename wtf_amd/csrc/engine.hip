// engine.hip — kernels + host implementation of the C ABI in include/wtfgpu.h.
// The one translation unit: the kernels live in two headers and are launched
// from the host half below.
//
// Hot kernel: k_run, the RIP-grouped lane-per-testcase x86-64 interpreter
// (engine_run.h; engine_device.h explains the scheme). Everything else is
// plumbing (engine_kernels.h):
// lane restore (the dirty-list reset that replaces bochscpu's per-page memcpy,
// bochscpu_backend.cc:730-797), batched guest-memory writes for host-side
// handlers, coverage log compaction and the aggregate coverage map.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>
#include <hipcub/device/device_scan.hpp>
#include <hipcub/device/device_select.hpp>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "engine_run.h"
#include "engine_kernels.h"
#include "engine_ptmark.h"

using namespace wtfgpu_dev;

// ====================================================================== host
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "wtfgpu: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, \
              __LINE__);                                                                 \
      return WTFGPU_ERR_HIP;                                                             \
    }                                                                                    \
  } while (0)

// What a queue owns (wtfgpu_select_queue): its stream and the scratch a call
// on it stages through, so that work queued on one (a k_run slice) runs while
// the host drives the other. The only home of per-queue state: the context
// holds two of these and a pointer to the selected one (wtfgpu_ctx::q), so a
// new member is declared here and nowhere else.
struct QueueRes {
  u32 index = 0;  // 0 or 1: picks the queue's set of warm LDS images (run_params)
  hipStream_t stream = nullptr;
  u8 *d_scratch = nullptr;
  u64 scratch_bytes = 0;
  u8 *h_stage = nullptr;  // pinned host staging of the queue's asynchronous uploads
  u64 stage_bytes = 0;
  u64 *d_stat = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  u32 *d_rkeys = nullptr, *d_rkeys2 = nullptr, *d_rlanes = nullptr;
  void *d_rtemp = nullptr;
  size_t rtemp_bytes = 0;
  u32 async_launches = 0;  // wtfgpu_run_async in flight (0 = none)
  u8 rg_used = 2;          // its run in flight regroups (1), not (0), unmeasured (2): regroup_now
  // asynchronous plumbing (see ring_put / wtfgpu_prefetch_*): the pinned
  // upload ring, the prefetched exits / coverage entries, the event after the
  // queue's plumbing of its last run (another queue's work is ordered after it)
  u8 *h_ring = nullptr;
  u64 ring_cap = 0, ring_off = 0;
  wtfgpu_exit_t *d_exq = nullptr;
  u64 exq_cap = 0;
  u8 *d_pcov = nullptr;
  hipEvent_t ev_pre = nullptr;
  bool pre_valid = false;
  // wtfgpu_read_feeds_packed: the pinned bytes k_feed_pack writes and the
  // caller reads until the queue's next packed read
  u8 *h_pack = nullptr;
  u64 h_pack_cap = 0;
};

struct wtfgpu_ctx {
  int device = 0;
  Dev P{};
  // pool
  u8 *d_pool = nullptr;
  u32 *d_pfnmap = nullptr;
  u32 *d_ptbits = nullptr;
  u64 *d_codeowner = nullptr;
  u64 npool = 0;
  // lanes
  u64 *d_gpr = nullptr, *d_rip = nullptr, *d_rflags = nullptr, *d_fsb = nullptr, *d_gsb = nullptr,
      *d_icount = nullptr, *d_nbytes = nullptr;
  u32 *d_status = nullptr, *d_lflags = nullptr, *d_ovcount = nullptr, *d_ovgpfn = nullptr;
  ExitInfo *d_exinfo = nullptr;
  LaneSys *d_sys = nullptr;
  u32 *d_guc = nullptr;       // device-wide decoded-uop cache (Dev::guc)
  u8 *d_warm = nullptr;       // LDS uop-cache images, UC_QUEUES sets of warm_n (Dev::warm)
  u32 warm_n = 0;
  u64 *d_rdseed = nullptr;    // per-lane Rdrand seeds (Dev::rd_seed)
  u64 *d_stopargs = nullptr;  // per-lane STOP_ARGS arguments (Dev::stop_args)
  u64 *d_extra = nullptr;     // coverage values outside code pages (Dev::extra_keys)
  u8 *d_attr = nullptr;       // wtfgpu_attribute_coverage's candidates, owner table and result
  u64 attr_bytes = 0;
  u64 *d_covtarget = nullptr;  // wtfgpu_coverage_target's copy (both queues read it)
  u32 covtarget_n = 0;
  bool covtarget_set = false;
  u8 *d_tn_buf = nullptr;     // Tenet traces (g_tn)
  u64 *d_tn_pos = nullptr, *d_tn_cpos = nullptr, *d_tn_ipos = nullptr, *d_tn_last = nullptr;
  u32 *d_tn_mute = nullptr;
  u64 tn_cap = 0;
  u64 *d_trace = nullptr;     // rip traces (Dev::trace)
  u32 *d_tracecnt = nullptr;
  u32 *d_edgecnt = nullptr;  // [nlanes][2] (wtfgpu_set_edges)
  LaneTlb *d_tlbs = nullptr;  // translation state kept between k_run launches
  u8 *d_lcopy = nullptr;      // the rare path's lane copies (LaneCopy)
  u32 *d_tlbok = nullptr;
  u8 *d_ovdata = nullptr;
  // spill pool (wtfgpu_alloc_spill): pages, ownership bitmap, extension page
  // indices, counters (the extension gpfns are d_ovgpfn's rows K..)
  u8 *d_spdata = nullptr;
  u32 *d_spmap = nullptr, *d_ovxpage = nullptr;
  unsigned long long *d_spstat = nullptr;
  u64 sp_pages = 0;
  wtfgpu_regs_t *d_full = nullptr;  // full per-lane architectural state (cold fields)
  // breakpoints
  u64 *d_bp = nullptr;
  u64 *d_actkeys = nullptr;
  wtfgpu_bp_action_t *d_act = nullptr;
  u64 *d_feedpos = nullptr, *d_feedend = nullptr;
  u8 *d_feeddata = nullptr;
  u64 feed_cap = 0;
  u64 feed_stride = 0;  // streaming: bytes of feed region per lane (0 = one packed feed)
  bool ins_on = false;  // a declared insert (wtfgpu_set_insert) runs after each feed upload
  wtfgpu_insert_t ins{};
  // device corpus (wtfgpu_corpus_alloc): an append-only arena and its offset
  // table (entries + 1 values; the host keeps a copy for the argument checks)
  u8 *d_corpus = nullptr;
  u64 *d_corpus_off = nullptr;
  u64 corpus_max_entries = 0, corpus_max_bytes = 0;
  std::vector<u64> corpus_off;
  // each entry's units (a byte buffer's bytes, a feed's packets): the index
  // check of wtfgpu_minimize_feed_lanes (engine_minimize.h)
  std::vector<u32> corpus_units;
  // each feed entry's chunk offsets (coff[0 .. P], as the entry holds them):
  // wtfgpu_analyze_feed_lanes refuses framing positions with them
  // (engine_analyze.h); an arena of byte buffers keeps none
  std::vector<std::vector<u32>> corpus_coff;
  // what the arena holds, fixed by its first add: byte buffers
  // (wtfgpu_corpus_add) or indexed feeds (wtfgpu_corpus_add_feed)
  enum CorpusKind : u32 { kCorpusEmpty, kCorpusBytes, kCorpusFeeds } corpus_kind = kCorpusEmpty;
  // coverage
  u64 *d_codekeys = nullptr;
  u32 *d_codeslot = nullptr;
  u8 *d_covmap = nullptr;
  u8 *d_covshadow = nullptr;  // the map as of the last absorb / own commit
  u64 ncovslots = 0;
  u64 *d_covrip = nullptr;
  u32 *d_covgen = nullptr, *d_lanegen = nullptr, *d_covcnt = nullptr, *d_covovf = nullptr;
  std::vector<u64> code_vpns;
  // host copy of the pool (page-table marking, host-side reads)
  std::vector<u8> h_pool;
  std::vector<u32> h_map;
  // misc
  InitState *d_init = nullptr;
  wtfgpu_regs_t *d_init_full = nullptr;  // initial architectural state, copied per lane by k_restore
  wtfgpu_regs_t initial{};
  bool have_initial = false;
  // cross-wave regrouping (wtfgpu_run): the lane order, shared by the queues
  // (each sorts its own lanes' part; keys and radix-sort scratch are per queue)
  u32 *d_perm = nullptr;
  u64 regroup_steps = 1024;
  // regrouping pays only while lanes diverge from their wave neighbours:
  // regroup_now() measures both schedules (lanes retired per wave-step) and
  // runs the better one, probing the other every kProbe-th run; all counts,
  // no clocks, so a fixed-seed campaign schedules the same way every time
  // (WTFGPU_REGROUP_AUTO=0: always regroup)
  // A synchronous run to completion (wtfgpu_run with no step bound) ends
  // with the same lane states in either order, so there the choice is by
  // measured kernel time per retired instruction instead: a run whose longest
  // lane sets its length (SYN) gains nothing from denser wave-steps and pays
  // for the sorts and the shorter launches.
  bool regroup_auto = true;
  double lps_sched[2] = {0, 0};  // lanes per wave-step, EMA: [0] fixed order, [1] regrouped
  u64 rg_runs = 0;
  double nspi_sched[2] = {0, 0};  // run-to-completion runs: kernel ns per retired instruction, EMA
  u64 rg_sync_runs = 0;
  // queue 1 is created at its first selection; every call works on *q
  QueueRes queues[2];
  QueueRes *q = &queues[0];  // the selected queue (wtfgpu_select_queue)
};

namespace {

template <typename T>
int dalloc(T **p, u64 count) {
  *p = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void **)p, count * sizeof(T));
  if (e != hipSuccess) {
    fprintf(stderr, "wtfgpu: hipMalloc(%llu bytes) failed: %s\n", (unsigned long long)(count * sizeof(T)),
            hipGetErrorString(e));
    return WTFGPU_ERR_OOM;
  }
  return WTFGPU_OK;
}
template <typename T>
void dfree(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// The current queue's device scratch, at least `bytes`. Growth is geometric
// and stream-ordered (hipFreeAsync / hipMallocAsync on the queue's stream):
// the old buffer is released after the queue's earlier work that reads it
// (e.g. an asynchronous k_feed_scatter) and nothing synchronises the device,
// so the other queue's k_run slice keeps running.
int ensure_scratch(wtfgpu_ctx *c, u64 bytes) {
  QueueRes &q = *c->q;
  if (q.scratch_bytes >= bytes) return WTFGPU_OK;
  const u64 want = std::max<u64>(std::max<u64>(bytes, 2 * q.scratch_bytes), 1ull << 20);
  if (q.d_scratch) HIPCHK(hipFreeAsync(q.d_scratch, q.stream));
  q.d_scratch = nullptr;
  q.scratch_bytes = 0;
  if (hipMallocAsync((void **)&q.d_scratch, want, q.stream) != hipSuccess) return WTFGPU_ERR_OOM;
  q.scratch_bytes = want;
  return WTFGPU_OK;
}

// Pinned staging for an asynchronous upload on the current queue: the bytes
// are copied into the queue's pinned ring and the caller queues the DMA from
// there, so the call returns without waiting for the queue's stream (whose
// earlier kernels may wait behind the other queue's k_run for free compute
// units: every VGPR of a SIMD is taken by two k_run waves). The ring restarts
// after each synchronisation of the stream (wtfgpu_run_wait, or here when
// full): no DMA still reads it then.
u8 *ring_put(wtfgpu_ctx *c, const void *src, u64 bytes) {
  QueueRes &q = *c->q;
  const u64 need = (bytes + 255) & ~255ull;
  if (q.ring_off + need > q.ring_cap) {
    if (hipStreamSynchronize(q.stream) != hipSuccess) return nullptr;
    q.ring_off = 0;
    if (need > q.ring_cap) {
      if (q.h_ring) (void)hipHostFree(q.h_ring);
      q.h_ring = nullptr;
      q.ring_cap = 0;
      const u64 want = std::max<u64>(need * 2, 4ull << 20);
      if (hipHostMalloc((void **)&q.h_ring, want, hipHostMallocDefault) != hipSuccess) return nullptr;
      q.ring_cap = want;
    }
  }
  u8 *p = q.h_ring + q.ring_off;
  if (src && bytes) memcpy(p, src, bytes);
  q.ring_off += need;
  return p;
}
// the current queue's stream is idle: the ring may be reused from its start
void ring_reset(wtfgpu_ctx *c) { c->q->ring_off = 0; }

int queue_create(QueueRes &q, u32 index) {
  q.index = index;
  HIPCHK(hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&q.ev0));
  HIPCHK(hipEventCreate(&q.ev1));
  HIPCHK(hipEventCreateWithFlags(&q.ev_pre, hipEventDisableTiming));
  if (dalloc(&q.d_stat, STAT_N)) return WTFGPU_ERR_OOM;
  return WTFGPU_OK;
}
// a queue's regrouping buffers (sized by the lane count)
void regroup_free(QueueRes &q) {
  dfree(q.d_rkeys);
  dfree(q.d_rkeys2);
  dfree(q.d_rlanes);
  dfree(q.d_rtemp);
  q.rtemp_bytes = 0;
}
void queue_destroy(QueueRes &q) {
  if (q.stream) (void)hipStreamSynchronize(q.stream);
  regroup_free(q);
  dfree(q.d_stat);
  dfree(q.d_scratch);
  dfree(q.d_exq);
  dfree(q.d_pcov);
  if (q.h_pack) (void)hipHostFree(q.h_pack);
  q.h_pack = nullptr;
  if (q.h_stage) (void)hipHostFree(q.h_stage);
  q.h_stage = nullptr;
  if (q.h_ring) (void)hipHostFree(q.h_ring);
  q.h_ring = nullptr;
  if (q.ev_pre) (void)hipEventDestroy(q.ev_pre);
  if (q.ev0) (void)hipEventDestroy(q.ev0);
  if (q.ev1) (void)hipEventDestroy(q.ev1);
  if (q.stream) (void)hipStreamDestroy(q.stream);
  q = QueueRes{};
}

u64 hmix(u64 x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

u32 table_size(u64 n) {
  u32 s = 16;
  while (s < 2 * n + 2) s <<= 1;
  return s;
}

InitState make_init(const wtfgpu_regs_t &r) {
  InitState s{};
  for (int i = 0; i < 16; i++) s.g[i] = r.gpr[i];
  s.rip = r.rip;
  s.rflags = r.rflags;
  s.fsb = r.seg[WTFGPU_FS].base;
  s.gsb = r.seg[WTFGPU_GS].base;
  s.sys.cr0 = r.cr0;
  s.sys.cr3 = r.cr3;
  s.sys.cr4 = r.cr4;
  s.sys.efer = (r.efer & ~EFER_M32) | (compat_sel(r.star, r.seg[WTFGPU_CS].selector) ? EFER_M32 : 0);  // U29
  s.sys.cpl = r.seg[WTFGPU_CS].selector & 3;
  s.sys.star = r.star;
  s.sys.lstar = r.lstar;
  s.sys.sfmask = r.sfmask;
  s.sys.kgs = r.kernel_gs_base;
  s.sys.cs = r.seg[WTFGPU_CS].selector;
  s.sys.idtr = r.idtr_base;
  s.sys.idtr_limit = r.idtr_limit;
  s.sys.tss = r.seg[WTFGPU_TR].base;
  s.sys.cr2 = r.cr2;
  s.sys.deliv_icount = ~0ull;
  s.sys.ss = r.seg[WTFGPU_SS].selector;
  return s;
}

bool lanes_ok(wtfgpu_ctx *c, u32 first, u32 count) {
  return c && c->d_gpr && (u64)first + count <= c->P.nlanes;
}

template <typename T>
int d2h(wtfgpu_ctx *c, T *dst, const T *src, u64 n) {
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->q->stream));
  return WTFGPU_OK;
}
template <typename T>
int h2d(wtfgpu_ctx *c, T *dst, const T *src, u64 n) {
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, c->q->stream));
  return WTFGPU_OK;
}

// ---- lane-list calls: a list of lanes (plus side arrays) -> the queue's
// scratch -> one kernel over the list. Each call keeps its own argument
// checks, in its own order (tests/test_gpu_abi_queues.py pins the return
// codes), its own launch, and names its upload route at the stage_lanes call.

// Every lane of the list is below the lane count. One branch-light pass: the
// step thread hands over lists of a whole slice's lanes.
bool lane_list_in_range(const wtfgpu_ctx *c, const u32 *lanes, u32 n) {
  u32 bad = 0;
  for (u32 i = 0; i < n; i++) bad |= (u32)(lanes[i] >= c->P.nlanes);
  return !bad;
}
int check_lane_list(const wtfgpu_ctx *c, const u32 *lanes, u32 n) {
  if (!c || !c->d_gpr || (n && !lanes) || !lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  return WTFGPU_OK;
}

// A region of the scratch after the lane list: an input uploaded with the
// list (src null: its place is kept, nothing is copied) or room the kernel
// writes / the call fills itself. stage_lanes sets `off`.
struct Side {
  u64 bytes;
  const void *src;
  bool room;
  u64 align;
  u64 off;
};
Side side_in(const void *src, u64 bytes) { return Side{bytes, src, false, 256, 0}; }
Side side_room(u64 bytes, u64 align = 256) { return Side{bytes, nullptr, true, align, 0}; }

enum class Upload {
  // Through the queue's pinned ring (ring_put), one DMA of the list and the
  // inputs: the call returns without a wait, ordered before the queue's later
  // work. For the calls that only change lane state; the step thread's
  // overlap with the other queue's slice depends on it.
  Ring,
  // Straight from the caller's memory, a copy per array: for the calls that
  // return data, which synchronise the queue before they return.
  Direct,
};

// Lays the list (lanes null: no list) and the sides out in the current
// queue's scratch, grown as needed, and queues the upload of the list and the
// inputs on the queue's stream. Never waits for the stream (ring_put apart).
int stage_lanes(wtfgpu_ctx *c, Upload route, const u32 *lanes, u32 n, Side *sides = nullptr, u32 nsides = 0) {
  const u64 list = lanes ? (u64)n * 4 : 0;
  u64 end = list, in_end = list;  // of everything, of the list and the inputs
  for (u32 i = 0; i < nsides; i++) {
    Side &s = sides[i];
    s.off = (end + s.align - 1) & ~(s.align - 1);
    end = s.off + s.bytes;
    if (!s.room) in_end = end;
  }
  if (ensure_scratch(c, end)) return WTFGPU_ERR_OOM;
  QueueRes &q = *c->q;
  u8 *to = q.d_scratch;
  if (route == Upload::Ring) {
    to = ring_put(c, nullptr, in_end);
    if (!to) return WTFGPU_ERR_OOM;
  }
  // Ring: host copies into the ring, then the one DMA; Direct: the DMAs themselves
  const auto put = [&](u64 off, const void *src, u64 bytes) -> int {
    if (!src || !bytes) return WTFGPU_OK;
    if (route == Upload::Ring) memcpy(to + off, src, bytes);
    else HIPCHK(hipMemcpyAsync(to + off, src, bytes, hipMemcpyHostToDevice, q.stream));
    return WTFGPU_OK;
  };
  if (int rc = put(0, lanes, list)) return rc;
  for (u32 i = 0; i < nsides; i++)
    if (!sides[i].room)
      if (int rc = put(sides[i].off, sides[i].src, sides[i].bytes)) return rc;
  // (the place of an input without a source goes up as the ring holds it: its kernel gets no pointer to it)
  if (route == Upload::Ring && in_end)
    HIPCHK(hipMemcpyAsync(q.d_scratch, to, in_end, hipMemcpyHostToDevice, q.stream));
  return WTFGPU_OK;
}

// The end of a Direct call that returns data: the region copied to the
// caller, then the wait its caller relies on.
int read_back(wtfgpu_ctx *c, void *dst, const Side &s) {
  HIPCHK(hipMemcpyAsync(dst, c->q->d_scratch + s.off, s.bytes, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// The per-lane feed regions (wtfgpu_set_feed_lanes, wtfgpu_mutate_feed_lanes),
// made at their first use.
int feed_regions(wtfgpu_ctx *c) {
  const u64 N = c->P.nlanes;
  // first use: buffers change under every queue
  if (!c->d_feedpos || c->feed_stride == 0) HIPCHK(hipDeviceSynchronize());
  if (!c->d_feedpos) {
    if (dalloc(&c->d_feedpos, N) || dalloc(&c->d_feedend, N)) return WTFGPU_ERR_OOM;
    std::vector<u64> none(N, ~0ull);
    HIPCHK(hipMemcpy(c->d_feedpos, none.data(), N * 8, hipMemcpyHostToDevice));
  }
  if (c->feed_stride == 0) {  // switch to per-lane regions (a packed feed's lanes are finished by now)
    const u64 stride = WTFGPU_FEED_STRIDE;
    dfree(c->d_feeddata);
    c->feed_cap = 0;
    if (dalloc(&c->d_feeddata, N * stride)) return WTFGPU_ERR_OOM;
    c->feed_cap = N * stride;
    c->feed_stride = stride;
  }
  return WTFGPU_OK;
}

constexpr u32 kExtraEntries = 1u << 20;

// The warm images of every queue dropped (rare: setup-time changes). Every
// queue is drained first: a launch in flight on another queue reads or
// writes its set.
int warm_clear(wtfgpu_ctx *c) {
  if (!c->d_warm) return WTFGPU_OK;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(c->d_warm, 0xff, UC_IMAGE_BYTES * c->warm_n * UC_QUEUES));
  return WTFGPU_OK;
}

// Entries depend on the pool pages and the breakpoint set: cleared with them.
int guc_clear(wtfgpu_ctx *c) {
  if (c->d_guc) HIPCHK(hipMemsetAsync(c->d_guc, 0, (u64)(c->P.guc_mask + 1) * GUC_WORDS * 4, c->q->stream));
  return warm_clear(c);
}

}  // namespace

extern "C" {

int wtfgpu_abi_version(void) { return WTFGPU_ABI_VERSION; }

int wtfgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int wtfgpu_create(int device, wtfgpu_ctx **out) {
  if (!out) return WTFGPU_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return WTFGPU_ERR_NODEV;
  HIPCHK(hipSetDevice(device));
  wtfgpu_ctx *c = new (std::nothrow) wtfgpu_ctx();
  if (!c) return WTFGPU_ERR_OOM;
  c->device = device;
  // regrouped launches of 1024 wave-steps by default (measured on MI355X:
  // HEVD 0.73M -> 1.9M execs/s, tlv 2.0M -> 2.1-2.3M, SYN 0.88M -> 0.81M)
  c->regroup_steps = 1024;
  if (const char *e = getenv("WTFGPU_REGROUP_STEPS")) c->regroup_steps = strtoull(e, nullptr, 0);
  if (const char *e = getenv("WTFGPU_REGROUP_AUTO")) c->regroup_auto = e[0] != '0';
  {
    // shared decoded-uop cache: 256K entries of 192 bytes, 48 MB (WTFGPU_GUC=0:
    // off; 32K entries had HEVD I/O launches 2-3 % longer, profiles/r06_ab_guc_size.txt)
    const char *e = getenv("WTFGPU_GUC");
    const u32 n = e ? (u32)strtoul(e, nullptr, 0) : 262144u;
    if (n && !(n & (n - 1))) {
      if (dalloc(&c->d_guc, (u64)n * GUC_WORDS)) {
        delete c;
        return WTFGPU_ERR_OOM;
      }
      HIPCHK(hipMemset(c->d_guc, 0, (u64)n * GUC_WORDS * 4));
      c->P.guc = c->d_guc;
      c->P.guc_mask = n - 1;
    }
  }
  if (queue_create(c->queues[0], 0) || dalloc(&c->d_init, 1) || dalloc(&c->d_init_full, 1)) {
    wtfgpu_destroy(c);
    return WTFGPU_ERR_OOM;
  }
  *out = c;
  return WTFGPU_OK;
}

void *wtfgpu_stream(wtfgpu_ctx *c) { return c ? (void *)c->q->stream : nullptr; }

static void free_spill(wtfgpu_ctx *c) {
  dfree(c->d_spdata);
  dfree(c->d_spmap);
  dfree(c->d_ovxpage);
  dfree(c->d_spstat);
  c->sp_pages = 0;
  Dev &P = c->P;
  P.X = P.sp_words = 0;
  P.sp_data = nullptr;
  P.sp_map = P.ovx_gpfn = P.ovx_page = nullptr;
  P.sp_stat = nullptr;
}

static void free_lanes(wtfgpu_ctx *c) {
  dfree(c->d_feedpos);  // sized by the lane count
  dfree(c->d_feedend);
  c->P.feed_pos = nullptr;
  c->P.feed_end = nullptr;
  dfree(c->d_gpr);
  dfree(c->d_rip);
  dfree(c->d_rflags);
  dfree(c->d_fsb);
  dfree(c->d_gsb);
  dfree(c->d_icount);
  dfree(c->d_nbytes);
  dfree(c->d_status);
  dfree(c->d_lflags);
  dfree(c->d_ovcount);
  dfree(c->d_ovgpfn);
  dfree(c->d_exinfo);
  dfree(c->d_sys);
  dfree(c->d_tlbs);
  dfree(c->d_lcopy);
  dfree(c->d_tlbok);
  dfree(c->d_rdseed);
  dfree(c->d_stopargs);
  dfree(c->d_extra);
  dfree(c->d_trace);
  dfree(c->d_tracecnt);
  dfree(c->d_edgecnt);
  c->P.trace = nullptr;
  c->P.trace_cnt = nullptr;
  c->P.edge_cnt = nullptr;
  c->P.trace_cap = 0;
  if (c->d_tn_buf) {  // Tenet buffers are sized by the lane count
    dfree(c->d_tn_buf);
    dfree(c->d_tn_pos);
    dfree(c->d_tn_cpos);
    dfree(c->d_tn_ipos);
    dfree(c->d_tn_last);
    dfree(c->d_tn_mute);
    c->tn_cap = 0;
    const TenetDev T{};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tn), &T, sizeof(T));
  }
  dfree(c->d_ovdata);
  free_spill(c);
  dfree(c->d_full);
  dfree(c->d_perm);
  // regrouping buffers are sized by the lane count: every queue's
  for (QueueRes &q : c->queues) regroup_free(q);
  dfree(c->d_covrip);
  dfree(c->d_covgen);
  dfree(c->d_lanegen);
  dfree(c->d_covcnt);
  dfree(c->d_covovf);
}

// The spill pool sits on top of the lane storage: allocated after
// wtfgpu_alloc_lanes, dropped with it. Lanes that hold pool pages must have
// been restored (or are about to be discarded with the lanes).
int wtfgpu_alloc_spill(wtfgpu_ctx *c, uint64_t pool_pages, uint32_t lane_max) {
  if (!c || !c->P.nlanes || !c->d_ovgpfn) return WTFGPU_ERR_INVALID;
  if ((pool_pages == 0) != (lane_max == 0) || pool_pages > 0xffffffe0ull) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  for (QueueRes &q : c->queues)
    if (q.stream) HIPCHK(hipStreamSynchronize(q.stream));
  Dev &P = c->P;
  const u64 N = P.nlanes;
  // a pool that is replaced must be empty (its owners' lists would dangle)
  if (c->d_spstat) {
    unsigned long long st[SP_NSTAT];
    HIPCHK(hipMemcpy(st, c->d_spstat, sizeof(st), hipMemcpyDeviceToHost));
    if (st[SP_INUSE]) return WTFGPU_ERR_INVALID;
  }
  free_spill(c);
  // the dirty list keeps one allocation: K rows, then the X extension rows
  u32 *gp = nullptr;
  if (dalloc(&gp, ((u64)P.K + lane_max) * N)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpy(gp, c->d_ovgpfn, (u64)P.K * N * 4, hipMemcpyDeviceToDevice));
  dfree(c->d_ovgpfn);
  c->d_ovgpfn = P.ov_gpfn = gp;
  if (!pool_pages) return WTFGPU_OK;
  const u64 words = (pool_pages + 31) / 32;
  int rc = dalloc(&c->d_spdata, pool_pages * WTFGPU_PAGE_SIZE);
  rc |= dalloc(&c->d_spmap, words);
  rc |= dalloc(&c->d_ovxpage, (u64)lane_max * N);
  rc |= dalloc(&c->d_spstat, (u64)SP_NSTAT);
  if (rc || ((uintptr_t)c->d_spdata & 0xfff)) {
    free_spill(c);
    return WTFGPU_ERR_OOM;
  }
  std::vector<u32> map(words, 0);  // bits past the last page stay owned for ever
  if (pool_pages & 31) map[words - 1] = ~0u << (pool_pages & 31);
  HIPCHK(hipMemcpy(c->d_spmap, map.data(), words * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_spstat, 0, SP_NSTAT * sizeof(unsigned long long)));
  HIPCHK(hipMemset(c->d_ovxpage, 0, (u64)lane_max * N * 4));
  c->sp_pages = pool_pages;
  P.X = lane_max;
  P.sp_words = (u32)words;
  P.sp_data = c->d_spdata;
  P.sp_map = c->d_spmap;
  P.ovx_gpfn = c->d_ovgpfn + (u64)P.K * N;
  P.ovx_page = c->d_ovxpage;
  P.sp_stat = c->d_spstat;
  return WTFGPU_OK;
}

uint32_t wtfgpu_dirty_capacity(wtfgpu_ctx *c) { return c ? c->P.K + c->P.X : 0; }

int wtfgpu_spill_stats(wtfgpu_ctx *c, wtfgpu_spill_stats_t *out) {
  if (!c || !out) return WTFGPU_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  if (!c->d_spstat) return WTFGPU_OK;  // no pool: all zero
  HIPCHK(hipSetDevice(c->device));
  unsigned long long st[SP_NSTAT];  // (on the queue's stream: after its queued runs and restores)
  HIPCHK(hipMemcpyAsync(st, c->d_spstat, sizeof(st), hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  out->pool_pages = c->sp_pages;
  out->lane_max = c->P.X;
  out->in_use = st[SP_INUSE];
  out->peak = st[SP_PEAK];
  out->lanes_spilled = st[SP_LANES];
  out->pool_empty = st[SP_EMPTY];
  out->claims = st[SP_CLAIMS];
  return WTFGPU_OK;
}

int wtfgpu_destroy(wtfgpu_ctx *c) {
  if (!c) return WTFGPU_OK;
  (void)hipSetDevice(c->device);
  for (QueueRes &q : c->queues)
    if (q.stream) (void)hipStreamSynchronize(q.stream);
  free_lanes(c);
  dfree(c->d_attr);
  dfree(c->d_covtarget);
  dfree(c->d_guc);
  if (c->d_warm) (void)hipFree(c->d_warm);
  dfree(c->d_pool);
  dfree(c->d_pfnmap);
  dfree(c->d_ptbits);
  dfree(c->d_codeowner);
  dfree(c->d_bp);
  dfree(c->d_actkeys);
  dfree(c->d_act);
  dfree(c->d_feeddata);
  dfree(c->d_corpus);
  dfree(c->d_corpus_off);
  dfree(c->d_codekeys);
  dfree(c->d_codeslot);
  dfree(c->d_covmap);
  dfree(c->d_covshadow);
  dfree(c->d_init);
  dfree(c->d_init_full);
  for (QueueRes &q : c->queues) queue_destroy(q);
  delete c;
  return WTFGPU_OK;
}

static int mark_pt_pages(wtfgpu_ctx *c);

// Snapshot page pool. Also marks page-table pages reachable from the
// initial cr3 (set later by wtfgpu_set_initial_state).
int wtfgpu_load_pool(wtfgpu_ctx *c, const uint64_t *gpfns, const uint8_t *pages, uint64_t npages) {
  if (!c || (npages && (!gpfns || !pages))) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  dfree(c->d_pool);
  dfree(c->d_pfnmap);
  dfree(c->d_ptbits);
  dfree(c->d_codeowner);
  u64 maxpfn = 0;
  for (u64 i = 0; i < npages; i++) maxpfn = std::max<u64>(maxpfn, gpfns[i]);
  const u64 maplen = npages ? maxpfn + 1 : 1;
  std::vector<u32> map(maplen, 0);
  for (u64 i = 0; i < npages; i++)
    if (map[gpfns[i]] == 0) map[gpfns[i]] = (u32)(i + 1);  // first occurrence wins (try_emplace)
  if (dalloc(&c->d_pool, (npages + 1) * WTFGPU_PAGE_SIZE)) return WTFGPU_ERR_OOM;
  // TLB entries pack permission bits into the low 12 bits of page pointers
  if ((uintptr_t)c->d_pool & 0xfff) {
    fprintf(stderr, "wtfgpu: page pool not 4 KiB aligned\n");
    return WTFGPU_ERR_OOM;
  }
  if (dalloc(&c->d_pfnmap, maplen)) return WTFGPU_ERR_OOM;
  if (dalloc(&c->d_ptbits, (maplen + 31) / 32)) return WTFGPU_ERR_OOM;
  if (dalloc(&c->d_codeowner, npages + 1)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemsetAsync(c->d_pool, 0, WTFGPU_PAGE_SIZE, c->q->stream));
  if (npages)
    HIPCHK(hipMemcpyAsync(c->d_pool + WTFGPU_PAGE_SIZE, pages, npages * WTFGPU_PAGE_SIZE, hipMemcpyHostToDevice,
                          c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_pfnmap, map.data(), maplen * 4, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_ptbits, 0, (maplen + 31) / 32 * 4, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_codeowner, 0, (npages + 1) * 8, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));

  c->npool = npages;
  c->h_pool.assign(pages, pages + npages * WTFGPU_PAGE_SIZE);
  c->h_map = std::move(map);
  c->P.pool = c->d_pool;
  c->P.pfn_map = c->d_pfnmap;
  c->P.pfn_map_len = maplen;
  c->P.npool = npages;
  c->P.ptbits = c->d_ptbits;
  c->P.code_owner = c->d_codeowner;
  if (c->d_tlbok) HIPCHK(hipMemsetAsync(c->d_tlbok, 0, (u64)c->P.nlanes * 4, c->q->stream));  // old page pointers
  if (guc_clear(c)) return WTFGPU_ERR_HIP;
  HIPCHK(hipStreamSynchronize(c->q->stream));
  if (c->have_initial) return mark_pt_pages(c);
  return WTFGPU_OK;
}

int wtfgpu_alloc_lanes(wtfgpu_ctx *c, uint32_t nlanes, uint32_t overlay_pages, uint32_t cov_entries) {
  if (!c || nlanes == 0 || overlay_pages == 0) return WTFGPU_ERR_INVALID;
  if (cov_entries & (cov_entries - 1)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  free_lanes(c);
  const u64 N = nlanes;
  // lanes per wave: 64. Measured on MI355X (SYN, 64K lanes): 32 and 16 lanes
  // per wave take 2x / 4x the time: the step loop's cost is per wave-step,
  // more resident waves do not overlap it (WTFGPU_LPW overrides, for tests)
  u32 lpw = 64;
  if (const char *e = getenv("WTFGPU_LPW")) {
    const u32 v = (u32)atoi(e);
    if (v == 64 || v == 32 || v == 16) lpw = v;
  }
  int rc = 0;
  rc |= dalloc(&c->d_gpr, 16 * N);
  rc |= dalloc(&c->d_rip, N);
  rc |= dalloc(&c->d_rflags, N);
  rc |= dalloc(&c->d_fsb, N);
  rc |= dalloc(&c->d_gsb, N);
  rc |= dalloc(&c->d_icount, N);
  rc |= dalloc(&c->d_nbytes, N);
  rc |= dalloc(&c->d_status, N);
  rc |= dalloc(&c->d_lflags, N);
  rc |= dalloc(&c->d_ovcount, N);
  rc |= dalloc(&c->d_ovgpfn, (u64)overlay_pages * N);
  rc |= dalloc(&c->d_exinfo, N);
  rc |= dalloc(&c->d_sys, N);
  rc |= dalloc(&c->d_ovdata, N * overlay_pages * WTFGPU_PAGE_SIZE);
  if (!rc && ((uintptr_t)c->d_ovdata & 0xfff)) {
    fprintf(stderr, "wtfgpu: overlay pages not 4 KiB aligned\n");
    return WTFGPU_ERR_OOM;
  }
  rc |= dalloc(&c->d_full, N);
  rc |= dalloc(&c->d_tlbs, N);
  rc |= dalloc(&c->d_lcopy, N * sizeof(LaneCopy));
  rc |= dalloc(&c->d_tlbok, N);
  rc |= dalloc(&c->d_rdseed, N);
  rc |= dalloc(&c->d_stopargs, 6 * N);
  if (!c->d_extra) {  // the aggregate's values outside code pages (Dev::extra_keys): 1M entries
    rc |= dalloc(&c->d_extra, (u64)kExtraEntries);
    if (!rc) HIPCHK(hipMemset(c->d_extra, 0xff, (u64)kExtraEntries * 8));
  }
  if (cov_entries) {
    rc |= dalloc(&c->d_covrip, N * cov_entries);
    rc |= dalloc(&c->d_covgen, N * cov_entries);
    rc |= dalloc(&c->d_lanegen, N);
    rc |= dalloc(&c->d_covcnt, N);
    rc |= dalloc(&c->d_covovf, N);
  }
  if (rc) return WTFGPU_ERR_OOM;
  std::vector<u32> idle(N, WTFGPU_EXIT_IDLE);
  HIPCHK(hipMemcpyAsync(c->d_status, idle.data(), N * 4, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_ovcount, 0, N * 4, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_lflags, 0, N * 4, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_tlbok, 0, N * 4, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_rdseed, 0, N * 8, c->q->stream));  // CpuState_t::Seed = 0 (globals.h:1084)
  HIPCHK(hipMemsetAsync(c->d_icount, 0, N * 8, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_nbytes, 0, N * 8, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_exinfo, 0, N * sizeof(ExitInfo), c->q->stream));
  if (cov_entries) {
    HIPCHK(hipMemsetAsync(c->d_covgen, 0, N * cov_entries * 4, c->q->stream));
    std::vector<u32> one(N, 1);  // generation 1: every entry (0) is empty
    HIPCHK(hipMemcpyAsync(c->d_lanegen, one.data(), N * 4, hipMemcpyHostToDevice, c->q->stream));
    HIPCHK(hipMemsetAsync(c->d_covcnt, 0, N * 4, c->q->stream));
    HIPCHK(hipMemsetAsync(c->d_covovf, 0, N * 4, c->q->stream));
  }
  HIPCHK(hipStreamSynchronize(c->q->stream));
  Dev &P = c->P;
  P.nlanes = nlanes;
  P.K = overlay_pages;
  P.lpw = lpw;
  P.gpr = c->d_gpr;
  P.rip = c->d_rip;
  P.rflags = c->d_rflags;
  P.fs_base = c->d_fsb;
  P.gs_base = c->d_gsb;
  P.icount = c->d_icount;
  P.nbytes = c->d_nbytes;
  P.status = c->d_status;
  P.lflags = c->d_lflags;
  P.exinfo = c->d_exinfo;
  P.sys = c->d_sys;
  P.tlbs = c->d_tlbs;
  P.lcopy = c->d_lcopy;
  P.tlb_ok = c->d_tlbok;
  P.rd_seed = c->d_rdseed;
  P.stop_args = c->d_stopargs;
  P.extra_keys = c->d_extra;
  P.extra_mask = kExtraEntries - 1;
  P.rd_seed0 = 0;
  P.ov_count = c->d_ovcount;
  P.ov_gpfn = c->d_ovgpfn;
  P.ov_data = c->d_ovdata;
  P.full = c->d_full;
  P.cov_rip = c->d_covrip;
  P.cov_gen = c->d_covgen;
  P.lane_gen = c->d_lanegen;
  P.cov_cnt = c->d_covcnt;
  P.cov_overflow = c->d_covovf;
  P.H = cov_entries;
  P.stat = c->q->d_stat;
  if (P.edges) return wtfgpu_set_edges(c, 1);  // the counters follow the lane count
  return WTFGPU_OK;
}

uint32_t wtfgpu_lane_count(wtfgpu_ctx *c) { return c ? c->P.nlanes : 0; }

// Walks the initial page tables on the host copy of the pool to mark
// page-table pages (a guest write to one invalidates the lane TLB).
static int mark_pt_pages(wtfgpu_ctx *c) {
  if (!c->d_ptbits) return WTFGPU_OK;
  const u64 maplen = c->h_map.size();
  if (maplen == 0) return WTFGPU_OK;
  auto page = [&](u64 gpfn) -> const u8 * {
    const u32 idx = gpfn < maplen ? c->h_map[gpfn] : 0;
    return idx ? c->h_pool.data() + (u64)(idx - 1) * WTFGPU_PAGE_SIZE : nullptr;
  };
  const std::vector<u32> bits = wtfgpu_host::mark_pt_bits(c->initial.cr3, maplen, page);  // engine_ptmark.h
  HIPCHK(hipMemcpyAsync(c->d_ptbits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_set_initial_state(wtfgpu_ctx *c, const wtfgpu_regs_t *regs) {
  if (!c || !regs) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  c->initial = *regs;
  c->have_initial = true;
  c->P.cr3_0 = regs->cr3;
  if (c->d_tlbok) HIPCHK(hipMemsetAsync(c->d_tlbok, 0, (u64)c->P.nlanes * 4, c->q->stream));  // page-table pages change
  const InitState s = make_init(*regs);
  HIPCHK(hipMemcpyAsync(c->d_init, &s, sizeof(s), hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_init_full, regs, sizeof(*regs), hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return mark_pt_pages(c);
}

int wtfgpu_set_regroup(wtfgpu_ctx *c, uint64_t steps) {
  if (!c) return WTFGPU_ERR_INVALID;
  c->regroup_steps = steps;
  return WTFGPU_OK;
}

int wtfgpu_set_limit(wtfgpu_ctx *c, uint64_t limit) {
  if (!c) return WTFGPU_ERR_INVALID;
  c->P.limit = limit;
  return WTFGPU_OK;
}

int wtfgpu_set_breakpoints(wtfgpu_ctx *c, const uint64_t *gvas, uint32_t n) {
  if (!c || (n && !gvas)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  dfree(c->d_bp);
  c->P.bp_keys = nullptr;
  c->P.bp_mask = 0;
  if (guc_clear(c)) return WTFGPU_ERR_HIP;  // shared entries carry the breakpoint flag
  if (n == 0) {
    HIPCHK(hipStreamSynchronize(c->q->stream));
    return WTFGPU_OK;
  }
  const u32 sz = table_size(n);
  std::vector<u64> t(sz, EMPTY_KEY);
  for (u32 i = 0; i < n; i++) {
    u32 h = (u32)hmix(gvas[i]) & (sz - 1);
    while (t[h] != EMPTY_KEY && t[h] != gvas[i]) h = (h + 1) & (sz - 1);
    t[h] = gvas[i];
  }
  if (dalloc(&c->d_bp, sz)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpyAsync(c->d_bp, t.data(), sz * 8, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  c->P.bp_keys = c->d_bp;
  c->P.bp_mask = sz - 1;
  return WTFGPU_OK;
}

int wtfgpu_set_breakpoint_actions(wtfgpu_ctx *c, const wtfgpu_bp_action_t *acts, uint32_t n) {
  if (!c || (n && !acts)) return WTFGPU_ERR_INVALID;
  for (u32 i = 0; i < n; i++) {
    if (acts[i].kind > WTFGPU_BPACT_STOP_ARGS || acts[i].gva == EMPTY_KEY) return WTFGPU_ERR_INVALID;
    if (acts[i].kind == WTFGPU_BPACT_STOP_ARGS && acts[i].value > 6) return WTFGPU_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  dfree(c->d_actkeys);
  dfree(c->d_act);
  c->P.act_keys = nullptr;
  c->P.act = nullptr;
  c->P.act_mask = 0;
  if (n == 0) return WTFGPU_OK;
  const u32 sz = table_size(n);
  std::vector<u64> t(sz, EMPTY_KEY);
  std::vector<wtfgpu_bp_action_t> a(sz);
  memset(a.data(), 0, sz * sizeof(wtfgpu_bp_action_t));
  for (u32 i = 0; i < n; i++) {
    u32 h = (u32)hmix(acts[i].gva) & (sz - 1);
    while (t[h] != EMPTY_KEY && t[h] != acts[i].gva) h = (h + 1) & (sz - 1);
    t[h] = acts[i].gva;
    a[h] = acts[i];
  }
  if (dalloc(&c->d_actkeys, sz) || dalloc(&c->d_act, sz)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpyAsync(c->d_actkeys, t.data(), sz * 8, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_act, a.data(), sz * sizeof(wtfgpu_bp_action_t), hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  c->P.act_keys = c->d_actkeys;
  c->P.act = c->d_act;
  c->P.act_mask = sz - 1;
  return WTFGPU_OK;
}

int wtfgpu_set_feed(wtfgpu_ctx *c, uint32_t first, uint32_t count, const uint64_t *offsets, const uint8_t *has_feed,
                    const uint8_t *bytes, uint64_t nbytes) {
  if (!lanes_ok(c, first, count) || !offsets || (nbytes && !bytes)) return WTFGPU_ERR_INVALID;
  for (u32 i = 0; i < count; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] > nbytes) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  const u64 N = c->P.nlanes;
  if (!c->d_feedpos) {
    if (dalloc(&c->d_feedpos, N) || dalloc(&c->d_feedend, N)) return WTFGPU_ERR_OOM;
    std::vector<u64> none(N, ~0ull);
    HIPCHK(hipMemcpy(c->d_feedpos, none.data(), N * 8, hipMemcpyHostToDevice));
  }
  // the data of one call is the whole feed (earlier feeds are replaced)
  c->feed_stride = 0;  // packed layout (per-lane regions: wtfgpu_set_feed_lanes)
  if (nbytes > c->feed_cap) {
    dfree(c->d_feeddata);
    c->feed_cap = 0;
    if (dalloc(&c->d_feeddata, nbytes)) return WTFGPU_ERR_OOM;
    c->feed_cap = nbytes;
  }
  std::vector<u64> pos(count), end(count);
  for (u32 i = 0; i < count; i++) {
    const bool has = !has_feed || has_feed[i];
    pos[i] = has ? offsets[i] : ~0ull;
    end[i] = offsets[i + 1];
  }
  if (nbytes) HIPCHK(hipMemcpyAsync(c->d_feeddata, bytes, nbytes, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_feedpos + first, pos.data(), count * 8ull, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_feedend + first, end.data(), count * 8ull, hipMemcpyHostToDevice, c->q->stream));
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  if (c->ins_on && count) {
    k_insert<<<(count + 63) / 64, 64, 0, c->q->stream>>>(c->P, c->ins, nullptr, first, count);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_set_insert(wtfgpu_ctx *c, const wtfgpu_insert_t *ins) {
  if (!c) return WTFGPU_ERR_INVALID;
  if (ins && (ins->head_reg > 15 || ins->ptr_reg > 15 || ins->len_reg > 15 || ins->len_arg > 64))
    return WTFGPU_ERR_INVALID;
  c->ins_on = ins != nullptr;
  if (ins) c->ins = *ins;
  return WTFGPU_OK;
}

int wtfgpu_set_code_pages(wtfgpu_ctx *c, const uint64_t *vpns, uint32_t n) {
  if (!c || (n && !vpns)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  dfree(c->d_codekeys);
  dfree(c->d_codeslot);
  dfree(c->d_covmap);
  dfree(c->d_covshadow);
  c->P.code_keys = nullptr;
  c->P.code_slot = nullptr;
  c->P.cov_map = nullptr;
  c->P.cov_shadow = nullptr;
  c->P.code_mask = 0;
  c->code_vpns.assign(vpns, vpns + n);
  c->ncovslots = n;
  if (n == 0) return WTFGPU_OK;
  const u32 sz = table_size(n);
  std::vector<u64> keys(sz, EMPTY_KEY);
  std::vector<u32> slots(sz, 0);
  for (u32 i = 0; i < n; i++) {
    u32 h = (u32)hmix(vpns[i]) & (sz - 1);
    while (keys[h] != EMPTY_KEY && keys[h] != vpns[i]) h = (h + 1) & (sz - 1);
    keys[h] = vpns[i];
    slots[h] = i;
  }
  if (dalloc(&c->d_codekeys, sz) || dalloc(&c->d_codeslot, sz) || dalloc(&c->d_covmap, (u64)n * WTFGPU_PAGE_SIZE) ||
      dalloc(&c->d_covshadow, (u64)n * WTFGPU_PAGE_SIZE))
    return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpyAsync(c->d_codekeys, keys.data(), sz * 8, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->d_codeslot, slots.data(), sz * 4, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_covmap, 0, (u64)n * WTFGPU_PAGE_SIZE, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_covshadow, 0, (u64)n * WTFGPU_PAGE_SIZE, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  if (int rc = warm_clear(c)) return rc;  // images carry UC_COVERED
  c->P.cov_shadow = c->d_covshadow;
  c->P.code_keys = c->d_codekeys;
  c->P.code_slot = c->d_codeslot;
  c->P.code_mask = sz - 1;
  c->P.cov_map = c->d_covmap;
  return WTFGPU_OK;
}

int wtfgpu_restore(wtfgpu_ctx *c, uint32_t first, uint32_t count) {
  if (!lanes_ok(c, first, count) || !c->have_initial) return WTFGPU_ERR_STATE;
  if (count == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  k_restore<<<(count + 255) / 256, 256, 0, c->q->stream>>>(c->P, c->d_init, c->d_init_full, c->d_full, first, count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_restore_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n) {
  if (!c || !c->have_initial) return WTFGPU_ERR_INVALID;
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n)) return rc;
  k_restore_list<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, c->d_init, c->d_init_full, c->d_full,
                                                         (const u32 *)c->q->d_scratch, n);
  HIPCHK(hipGetLastError());
  return WTFGPU_OK;
}

int wtfgpu_set_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, const uint64_t *offsets,
                          const uint8_t *has_feed, const uint8_t *bytes, uint64_t nbytes) {
  if (!c || !c->d_gpr || (n && (!lanes || !offsets)) || (nbytes && !bytes) || !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  {  // one branch-light pass: offsets ascending within the bytes
    u32 bad = 0;
    for (u32 i = 0; i < n; i++) bad |= (u32)(offsets[i + 1] < offsets[i]) | (u32)(offsets[i + 1] > nbytes);
    if (bad) return WTFGPU_ERR_INVALID;
  }
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = feed_regions(c)) return rc;
  // one staging upload of the lane list, the offsets and the flags (the
  // scatter derives each lane's length, position and end), one of the bytes
  // (straight from the caller's buffer: pinned memory DMAs), then one scatter
  Side s[] = {side_in(offsets, (u64)(n + 1) * 8), side_in(has_feed, n), side_room(nbytes)};
  const Side &off = s[0], &has = s[1], &data = s[2];
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, s, 3)) return rc;
  u8 *const S = c->q->d_scratch;
  if (nbytes) HIPCHK(hipMemcpyAsync(S + data.off, bytes, nbytes, hipMemcpyHostToDevice, c->q->stream));
  k_feed_scatter<<<n, 128, 0, c->q->stream>>>(c->d_feeddata, c->feed_stride, (const u32 *)S,
                                              (const u64 *)(S + off.off), has_feed ? S + has.off : nullptr, n,
                                              S + data.off, c->d_feedpos, c->d_feedend);
  HIPCHK(hipGetLastError());
  // no wait: the queue's later work (its k_run slice) is ordered after the
  // scatter. Nothing here or in the queue's next call waits for the DMA of
  // `bytes`: the caller keeps them unchanged until a call of its own waits for
  // the queue (wtfgpu_run_wait, or any call that returns data).
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  if (c->ins_on) {  // the declared insert of the listed lanes, ordered after the scatter
    k_insert<<<(n + 63) / 64, 64, 0, c->q->stream>>>(c->P, c->ins, (const u32 *)c->q->d_scratch, 0, n);
    HIPCHK(hipGetLastError());
  }
  return WTFGPU_OK;
}

// ---- device corpus and mutator (engine_mutate.h)

int wtfgpu_corpus_alloc(wtfgpu_ctx *c, uint64_t max_entries, uint64_t max_bytes) {
  if (!c || (max_entries == 0) != (max_bytes == 0) || max_entries > 0xffffffffull) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());  // a mutation in flight on either queue reads the old arena
  dfree(c->d_corpus);
  dfree(c->d_corpus_off);
  c->corpus_max_entries = c->corpus_max_bytes = 0;
  c->corpus_off.clear();
  c->corpus_units.clear();
  c->corpus_coff.clear();
  c->corpus_kind = wtfgpu_ctx::kCorpusEmpty;
  if (max_entries == 0) return WTFGPU_OK;
  if (dalloc(&c->d_corpus, max_bytes) || dalloc(&c->d_corpus_off, max_entries + 1)) {
    dfree(c->d_corpus);
    dfree(c->d_corpus_off);
    return WTFGPU_ERR_OOM;
  }
  HIPCHK(hipMemset(c->d_corpus_off, 0, 8));
  c->corpus_max_entries = max_entries;
  c->corpus_max_bytes = max_bytes;
  c->corpus_off.assign(1, 0);
  return WTFGPU_OK;
}

int wtfgpu_corpus_add(wtfgpu_ctx *c, const uint8_t *bytes, uint64_t len, uint32_t *index) {
  if (!c || !c->d_corpus || (len && !bytes)) return WTFGPU_ERR_INVALID;
  if (c->corpus_kind == wtfgpu_ctx::kCorpusFeeds) return WTFGPU_ERR_STATE;
  const u64 count = c->corpus_off.size() - 1, used = c->corpus_off.back();
  if (count >= c->corpus_max_entries || len > c->corpus_max_bytes - used) return WTFGPU_ERR_FULL;
  HIPCHK(hipSetDevice(c->device));
  // Blocking copies on the null stream (the queues' streams do not wait for
  // it): complete on return, so a mutation ordered later sees the entry, and
  // one in flight reads only entries below its own ncorpus, written before.
  if (len) HIPCHK(hipMemcpy(c->d_corpus + used, bytes, len, hipMemcpyHostToDevice));
  const u64 end = used + len;
  HIPCHK(hipMemcpy(c->d_corpus_off + count + 1, &end, 8, hipMemcpyHostToDevice));
  c->corpus_off.push_back(end);
  c->corpus_units.push_back((u32)std::min<u64>(len, 0xffffffffull));
  c->corpus_kind = wtfgpu_ctx::kCorpusBytes;
  if (index) *index = (u32)count;
  return WTFGPU_OK;
}

int wtfgpu_corpus_add_feed(wtfgpu_ctx *c, const uint8_t *feed, uint64_t len, uint32_t *index) {
  if (!c || !c->d_corpus || (len && !feed)) return WTFGPU_ERR_INVALID;
  // the only gate: k_mutate_packets trusts every offset of an entry
  const int64_t packets = wtfpkt::entry_packets(feed, len, WTFGPU_FEED_STRIDE);
  if (packets < 0) return WTFGPU_ERR_INVALID;
  if (c->corpus_kind == wtfgpu_ctx::kCorpusBytes) return WTFGPU_ERR_STATE;
  const u64 count = c->corpus_off.size() - 1, used = c->corpus_off.back();
  const u64 bytes = wtfpkt::entry_bytes((u64)packets, len);
  if (count >= c->corpus_max_entries || bytes > c->corpus_max_bytes - used) return WTFGPU_ERR_FULL;
  HIPCHK(hipSetDevice(c->device));
  std::vector<u8> entry(bytes);
  wtfpkt::entry_write(feed, len, (u64)packets, entry.data());
  // blocking copies, as wtfgpu_corpus_add; entries stay 4-aligned (every size is a multiple of 4)
  HIPCHK(hipMemcpy(c->d_corpus + used, entry.data(), bytes, hipMemcpyHostToDevice));
  const u64 end = used + bytes;
  HIPCHK(hipMemcpy(c->d_corpus_off + count + 1, &end, 8, hipMemcpyHostToDevice));
  c->corpus_off.push_back(end);
  c->corpus_units.push_back((u32)packets);
  {  // the entry's words 1 .. P + 1
    std::vector<u32> coff((size_t)packets + 1);
    memcpy(coff.data(), entry.data() + 4, coff.size() * 4);
    c->corpus_coff.push_back(std::move(coff));
  }
  c->corpus_kind = wtfgpu_ctx::kCorpusFeeds;
  if (index) *index = (u32)count;
  return WTFGPU_OK;
}

int wtfgpu_mutate_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t seed, const uint64_t *indices,
                             const uint32_t *ncorpus, uint32_t max_len) {
  if (!c || !c->d_gpr || !c->d_corpus || (n && (!lanes || !indices || !ncorpus)) ||
      max_len > WTFGPU_FEED_STRIDE - 4 || !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  {  // every order reads entries that exist: the kernel checks nothing
    const u64 count = c->corpus_off.size() - 1;
    u32 bad = 0;
    for (u32 i = 0; i < n; i++) bad |= (u32)(ncorpus[i] == 0) | (u32)(ncorpus[i] > count);
    if (bad) return WTFGPU_ERR_INVALID;
  }
  if (c->corpus_kind == wtfgpu_ctx::kCorpusFeeds) return WTFGPU_ERR_STATE;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = feed_regions(c)) return rc;
  // one staging upload of the lane list and the orders; no caller's buffer is
  // read after the call returns (unlike wtfgpu_set_feed_lanes' `bytes`)
  Side s[] = {side_in(indices, (u64)n * 8), side_in(ncorpus, (u64)n * 4)};
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_mutate_feeds<<<(n + MUT_WAVES - 1) / MUT_WAVES, 64 * MUT_WAVES, 0, c->q->stream>>>(
      c->d_feeddata, c->feed_stride, (const u32 *)S, (const u64 *)(S + s[0].off), (const u32 *)(S + s[1].off), n, seed,
      max_len, c->d_corpus, c->d_corpus_off, c->d_feedpos, c->d_feedend);
  HIPCHK(hipGetLastError());
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  if (c->ins_on) {  // the declared insert of the listed lanes, ordered after the mutation
    k_insert<<<(n + 63) / 64, 64, 0, c->q->stream>>>(c->P, c->ins, (const u32 *)S, 0, n);
    HIPCHK(hipGetLastError());
  }
  return WTFGPU_OK;
}

int wtfgpu_read_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t *lens, uint8_t *bytes,
                           uint64_t stride) {
  if (!c || !c->d_gpr || (n && (!lanes || !lens)) || (n && stride && !bytes) || !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  if (!c->d_feedpos || c->feed_stride == 0) {  // no per-lane regions yet: no lane has a feed in one
    for (u32 i = 0; i < n; i++) lens[i] = ~0u;
    return WTFGPU_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  Side s[] = {side_room((u64)n * 4), side_room((u64)n * stride)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_feed_gather<<<n, 128, 0, c->q->stream>>>(c->d_feeddata, c->feed_stride, (const u32 *)S, n, c->d_feedpos,
                                             (u32 *)(S + s[0].off), S + s[1].off, stride);
  HIPCHK(hipGetLastError());
  // gathered on the device, so the copy back is the listed lanes' bytes only; one wait
  HIPCHK(hipMemcpyAsync(lens, S + s[0].off, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  if (stride) return read_back(c, bytes, s[1]);
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_mutate_packets_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t seed,
                                const uint64_t *indices, const uint32_t *ncorpus,
                                const wtfgpu_packet_params_t *params) {
  if (!c || !c->d_gpr || !c->d_corpus || !params || (n && (!lanes || !indices || !ncorpus)) ||
      !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  const wtfpkt::Params q{params->gen_max_packets, params->gen_commands,       params->gen_max_body,
                         params->flip_one_in,     params->insert_max_packets, WTFGPU_FEED_STRIDE};
  if (!wtfpkt::params_valid(q)) return WTFGPU_ERR_INVALID;
  {  // every order reads entries that exist: the kernel checks nothing
    const u64 count = c->corpus_off.size() - 1;
    u32 bad = 0;
    for (u32 i = 0; i < n; i++) bad |= (u32)(ncorpus[i] == 0) | (u32)(ncorpus[i] > count);
    if (bad) return WTFGPU_ERR_INVALID;
  }
  if (c->corpus_kind == wtfgpu_ctx::kCorpusBytes) return WTFGPU_ERR_STATE;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = feed_regions(c)) return rc;
  Side s[] = {side_in(indices, (u64)n * 8), side_in(ncorpus, (u64)n * 4)};
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_mutate_packets<<<(n + MUT_WAVES - 1) / MUT_WAVES, 64 * MUT_WAVES, 0, c->q->stream>>>(
      c->d_feeddata, c->feed_stride, (const u32 *)S, (const u64 *)(S + s[0].off), (const u32 *)(S + s[1].off), n, seed,
      q, c->d_corpus, c->d_corpus_off, c->d_feedpos, c->d_feedend);
  HIPCHK(hipGetLastError());
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  return WTFGPU_OK;
}

// The minimiser's candidates (engine_minimize.h): as wtfgpu_mutate_feed_lanes,
// with the orders checked against the entry's unit count the host keeps.
int wtfgpu_minimize_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t entry, uint32_t op,
                               const uint64_t *indices) {
  if (!c || !c->d_gpr || !c->d_corpus || (n && (!lanes || !indices)) || op >= wtfmin::kNumOps ||
      entry >= c->corpus_units.size() || !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  const bool feeds = c->corpus_kind == wtfgpu_ctx::kCorpusFeeds;
  const u32 units = c->corpus_units[entry];
  // a byte buffer goes out as one chunk behind its u32 size: the kernel checks nothing
  if (!feeds && c->corpus_off[entry + 1] - c->corpus_off[entry] > WTFGPU_FEED_STRIDE - 4) return WTFGPU_ERR_INVALID;
  {
    const u64 total = wtfmin::total(units);
    u32 bad = 0;
    for (u32 i = 0; i < n; i++) bad |= (u32)(indices[i] >= total);
    if (bad) return WTFGPU_ERR_INVALID;
  }
  if (feeds && op == wtfmin::kZero) return WTFGPU_ERR_STATE;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = feed_regions(c)) return rc;
  Side s[] = {side_in(indices, (u64)n * 8)};
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, s, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  k_minimize_feeds<<<(n + MUT_WAVES - 1) / MUT_WAVES, 64 * MUT_WAVES, 0, c->q->stream>>>(
      c->d_feeddata, c->feed_stride, (const u32 *)S, (const u64 *)(S + s[0].off), n, entry, op, feeds ? 1u : 0u,
      c->d_corpus, c->d_corpus_off, c->d_feedpos, c->d_feedend);
  HIPCHK(hipGetLastError());
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  if (c->ins_on) {  // the declared insert of the listed lanes, ordered after the candidates
    k_insert<<<(n + 63) / 64, 64, 0, c->q->stream>>>(c->P, c->ins, (const u32 *)S, 0, n);
    HIPCHK(hipGetLastError());
  }
  return WTFGPU_OK;
}

// The corpus distiller (engine_distill.h): what one call allocates, freed
// whatever way the call ends.
struct DistillBufs {
  u64 *vals = nullptr, *sorted = nullptr, *uniq = nullptr, *count = nullptr;
  u8 *temp = nullptr;
  u32 *ids = nullptr, *off = nullptr, *gain = nullptr, *bitmap = nullptr, *out_index = nullptr, *out_gain = nullptr;
  DistillState *st = nullptr;
  ~DistillBufs() {
    dfree(vals), dfree(sorted), dfree(uniq), dfree(count), dfree(temp), dfree(ids), dfree(off), dfree(gain);
    dfree(bitmap), dfree(out_index), dfree(out_gain), dfree(st);
  }
};

// The eligible sets go up packed, in rank order, so the device sees no flag
// and its set k is the host's pick[k]: the lowest k among equal gains is the
// lowest i. Dense ids: radix sort of a copy, unique, binary search. Then
// rounds of k_distill_gain + k_distill_take, DIS_BATCH of them queued between
// two looks at `done`; a call of m sets ends after at most m + 1 rounds.
int wtfgpu_distill(wtfgpu_ctx *c, uint32_t n, const uint64_t *offsets, const uint64_t *values, const uint8_t *eligible,
                   uint32_t *out_index, uint32_t *out_gain, uint32_t *kept, uint64_t *universe) {
  if (!c) return WTFGPU_ERR_INVALID;
  if (int rc = wtfdis::validate(n, offsets, values, out_index, out_gain, kept, universe)) return rc;
  *kept = 0;
  *universe = 0;
  if (n == 0) return WTFGPU_OK;
  std::vector<u32> pick, off(1, 0), size;
  try {
    for (u32 i = 0; i < n; i++) {
      if (eligible && !eligible[i]) continue;
      pick.push_back(i);
      size.push_back((u32)(offsets[i + 1] - offsets[i]));
      off.push_back(off.back() + size.back());
    }
  } catch (const std::bad_alloc &) {
    return WTFGPU_ERR_OOM;
  }
  const u32 m = (u32)pick.size();
  const u64 E = off.back();
  if (E == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t stream = c->q->stream;
  DistillBufs B;
  size_t sort_bytes = 0, uniq_bytes = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const u64 *)nullptr, (u64 *)nullptr, E, 0, 64, stream));
  HIPCHK(hipcub::DeviceSelect::Unique(nullptr, uniq_bytes, (const u64 *)nullptr, (u64 *)nullptr, (u64 *)nullptr,
                                      (int64_t)E, stream));
  if (dalloc(&B.vals, E) || dalloc(&B.sorted, E) || dalloc(&B.uniq, E) || dalloc(&B.count, 1) || dalloc(&B.ids, E) ||
      dalloc(&B.off, (u64)m + 1) || dalloc(&B.gain, m) || dalloc(&B.out_index, m) || dalloc(&B.out_gain, m) ||
      dalloc(&B.st, 1) || dalloc(&B.temp, std::max(sort_bytes, uniq_bytes)))
    return WTFGPU_ERR_OOM;
  for (u32 k = 0; k < m;) {  // a run of eligible neighbours is one copy
    u32 e = k + 1;
    while (e < m && pick[e] == pick[e - 1] + 1) e++;
    if (off[e] > off[k])
      HIPCHK(hipMemcpyAsync(B.vals + off[k], values + offsets[pick[k]], (u64)(off[e] - off[k]) * 8,
                            hipMemcpyHostToDevice, stream));
    k = e;
  }
  HIPCHK(hipMemcpyAsync(B.off, off.data(), ((u64)m + 1) * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(B.gain, size.data(), (u64)m * 4, hipMemcpyHostToDevice, stream));  // a set's size bounds its gain
  HIPCHK(hipMemsetAsync(B.st, 0, sizeof(DistillState), stream));
  HIPCHK(hipcub::DeviceRadixSort::SortKeys(B.temp, sort_bytes, (const u64 *)B.vals, B.sorted, E, 0, 64, stream));
  HIPCHK(hipcub::DeviceSelect::Unique(B.temp, uniq_bytes, (const u64 *)B.sorted, B.uniq, B.count, (int64_t)E, stream));
  u64 U = 0;
  HIPCHK(hipMemcpyAsync(&U, B.count, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (U == 0 || U > E) return WTFGPU_ERR_HIP;
  const u64 words = U / 32 + 1;
  if (dalloc(&B.bitmap, words)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemsetAsync(B.bitmap, 0, words * 4, stream));
  k_distill_ids<<<(u32)((E + DIS_BLOCK - 1) / DIS_BLOCK), DIS_BLOCK, 0, stream>>>(B.vals, E, B.uniq, (u32)U, B.ids);
  HIPCHK(hipGetLastError());
  const u32 gain_blocks = (u32)(((u64)m * DIS_GROUP + DIS_BLOCK - 1) / DIS_BLOCK);
  DistillState st{};
  for (u64 rounds = 0; !st.done;) {
    if (rounds > m) return WTFGPU_ERR_HIP;  // (m sets end in m + 1 rounds)
    const u64 batch = std::min<u64>(DIS_BATCH, (u64)m + 1 - rounds);
    for (u64 r = 0; r < batch; r++) {
      k_distill_gain<<<gain_blocks, DIS_BLOCK, 0, stream>>>(B.off, B.ids, m, B.bitmap, B.gain, B.st);
      k_distill_take<<<1, DIS_BLOCK, 0, stream>>>(B.off, B.ids, B.bitmap, B.gain, B.st, B.out_index, B.out_gain);
    }
    HIPCHK(hipGetLastError());
    rounds += batch;
    HIPCHK(hipMemcpyAsync(&st, B.st, sizeof(st), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  if (st.kept > m) return WTFGPU_ERR_HIP;
  HIPCHK(hipMemcpyAsync(out_index, B.out_index, (u64)st.kept * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(out_gain, B.out_gain, (u64)st.kept * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (u32 k = 0; k < st.kept; k++) out_index[k] = pick[out_index[k]];
  *kept = st.kept;
  *universe = U;
  return WTFGPU_OK;
}

// The analyzer's candidates (engine_analyze.h): as wtfgpu_minimize_feed_lanes,
// with the orders checked against the entry's length and, for a feed, against
// the chunk offsets the host keeps (a framing position is refused).
int wtfgpu_analyze_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t entry,
                              const uint64_t *indices) {
  if (!c || !c->d_gpr || !c->d_corpus || (n && (!lanes || !indices)) || entry >= c->corpus_units.size() ||
      !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  const bool feeds = c->corpus_kind == wtfgpu_ctx::kCorpusFeeds;
  if (feeds && entry >= c->corpus_coff.size()) return WTFGPU_ERR_INVALID;
  u64 bytes = c->corpus_off[entry + 1] - c->corpus_off[entry];
  // a byte buffer goes out as one chunk behind its u32 size: the kernel checks nothing
  if (!feeds && bytes > WTFGPU_FEED_STRIDE - 4) return WTFGPU_ERR_INVALID;
  {
    const u32 *coff = feeds ? c->corpus_coff[entry].data() : nullptr;
    const u32 P = feeds ? c->corpus_units[entry] : 0;
    if (feeds) bytes = coff[P];
    const u64 total = wtfana::total((u32)bytes);
    u32 bad = 0;
    for (u32 i = 0; i < n; i++)
      bad |= (u32)(indices[i] >= total || (feeds && wtfana::is_framing(coff, P, (u32)(indices[i] >> 2))));
    if (bad) return WTFGPU_ERR_INVALID;
  }
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = feed_regions(c)) return rc;
  Side s[] = {side_in(indices, (u64)n * 8)};
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, s, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  k_analyze_feeds<<<(n + MUT_WAVES - 1) / MUT_WAVES, 64 * MUT_WAVES, 0, c->q->stream>>>(
      c->d_feeddata, c->feed_stride, (const u32 *)S, (const u64 *)(S + s[0].off), n, entry, feeds ? 1u : 0u,
      c->d_corpus, c->d_corpus_off, c->d_feedpos, c->d_feedend);
  HIPCHK(hipGetLastError());
  c->P.feed_pos = c->d_feedpos;
  c->P.feed_end = c->d_feedend;
  c->P.feed_data = c->d_feeddata;
  if (c->ins_on) {  // the declared insert of the listed lanes, ordered after the candidates
    k_insert<<<(n + 63) / 64, 64, 0, c->q->stream>>>(c->P, c->ins, (const u32 *)S, 0, n);
    HIPCHK(hipGetLastError());
  }
  return WTFGPU_OK;
}

int wtfgpu_read_whole_feed_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t *lens, uint8_t *bytes,
                                 uint64_t stride) {
  if (!c || !c->d_gpr || (n && (!lanes || !lens)) || (n && stride && !bytes) || !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  if (!c->d_feedpos || c->feed_stride == 0) {  // no per-lane regions yet: no lane has a feed in one
    for (u32 i = 0; i < n; i++) lens[i] = ~0u;
    return WTFGPU_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  Side s[] = {side_room((u64)n * 4), side_room((u64)n * stride)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_feed_gather_whole<<<n, 128, 0, c->q->stream>>>(c->d_feeddata, c->feed_stride, (const u32 *)S, n, c->d_feedpos,
                                                   c->d_feedend, (u32 *)(S + s[0].off), S + s[1].off, stride);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(lens, S + s[0].off, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  if (stride) return read_back(c, bytes, s[1]);
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// The packed read-back (engine_feedpack.h): lengths, a 64-bit scan and the
// first wait give the caller lens, offs and the total; then k_feed_pack writes
// exactly `total` bytes into the queue's pinned buffer, grown to the total
// (known only now, and not n x stride), and the second wait returns them.
int wtfgpu_read_feeds_packed(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t whole, uint32_t *lens,
                             uint64_t *offs, const uint8_t **bytes, uint64_t *total) {
  if (!c || !c->d_gpr || !bytes || !total || (n && (!lanes || !lens || !offs)) || whole > 1 ||
      !lane_list_in_range(c, lanes, n))
    return WTFGPU_ERR_INVALID;
  *total = 0;
  *bytes = c->q->h_pack;
  if (n == 0) return WTFGPU_OK;
  if (!c->d_feedpos || c->feed_stride == 0) {  // no per-lane regions yet: no lane has a feed in one
    for (u32 i = 0; i < n; i++) {
      lens[i] = ~0u;
      offs[i] = 0;
    }
    return WTFGPU_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  QueueRes &q = *c->q;
  size_t tmp_n = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_n, (u64 *)nullptr, (u64 *)nullptr, (int)(n + 1), q.stream));
  Side s[] = {side_room((u64)n * 4), side_room((u64)(n + 1) * 8), side_room((u64)(n + 1) * 8), side_room(tmp_n)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 4)) return rc;
  u8 *const S = q.d_scratch;
  u32 *const d_lens = (u32 *)(S + s[0].off);
  u64 *const d_pad = (u64 *)(S + s[1].off), *const d_offs = (u64 *)(S + s[2].off);
  k_feed_lens<<<n / 256 + 1, 256, 0, q.stream>>>(c->d_feeddata, c->feed_stride, (const u32 *)S, n, c->d_feedpos,
                                                 c->d_feedend, whole, d_lens, d_pad);
  HIPCHK(hipGetLastError());
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(S + s[3].off, tmp_n, d_pad, d_offs, (int)(n + 1), q.stream));
  u64 sum = 0;
  HIPCHK(hipMemcpyAsync(lens, d_lens, (u64)n * 4, hipMemcpyDeviceToHost, q.stream));
  HIPCHK(hipMemcpyAsync(offs, d_offs, (u64)n * 8, hipMemcpyDeviceToHost, q.stream));
  HIPCHK(hipMemcpyAsync(&sum, d_offs + n, 8, hipMemcpyDeviceToHost, q.stream));
  HIPCHK(hipStreamSynchronize(q.stream));
  if (sum > (u64)n * c->feed_stride) return WTFGPU_ERR_STATE;  // (cannot be: every place is at most a region)
  if (sum == 0) return WTFGPU_OK;
  if (q.h_pack_cap < sum) {  // geometric; the bytes of the queue's last packed read end here, as declared
    const u64 want = std::max<u64>(std::max<u64>(sum, 2 * q.h_pack_cap), 1ull << 20);
    if (q.h_pack) (void)hipHostFree(q.h_pack);
    q.h_pack = nullptr;
    q.h_pack_cap = 0;
    if (hipHostMalloc((void **)&q.h_pack, want, hipHostMallocDefault) != hipSuccess) return WTFGPU_ERR_OOM;
    q.h_pack_cap = want;
  }
  // k_feed_pack writes the pinned buffer itself: no device staging, no DMA
  // (measured against staging plus one hipMemcpyAsync: profiles/packed_readback_ab.txt)
  u8 *d_out = nullptr;
  HIPCHK(hipHostGetDevicePointer((void **)&d_out, q.h_pack, 0));
  k_feed_pack<<<(n + MUT_WAVES - 1) / MUT_WAVES, 64 * MUT_WAVES, 0, q.stream>>>(
      c->d_feeddata, c->feed_stride, (const u32 *)S, n, whole, d_lens, d_offs, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(q.stream));
  *bytes = q.h_pack;
  *total = sum;
  return WTFGPU_OK;
}

// ---- register I/O

int wtfgpu_read_gprs(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint64_t *out18) {
  if (!lanes_ok(c, first, count) || !out18) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  const u64 N = c->P.nlanes;
  std::vector<u64> tmp((u64)18 * count);
  int rc = 0;
  for (int i = 0; i < 16; i++) rc |= d2h(c, tmp.data() + (u64)i * count, c->d_gpr + i * N + first, count);
  rc |= d2h(c, tmp.data() + (u64)16 * count, c->d_rip + first, count);
  rc |= d2h(c, tmp.data() + (u64)17 * count, c->d_rflags + first, count);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->q->stream));
  for (u64 l = 0; l < count; l++)
    for (int i = 0; i < 18; i++) out18[l * 18 + i] = tmp[(u64)i * count + l];
  return WTFGPU_OK;
}

int wtfgpu_write_gprs(wtfgpu_ctx *c, uint32_t first, uint32_t count, const uint64_t *in18) {
  if (!lanes_ok(c, first, count) || !in18) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  const u64 N = c->P.nlanes;
  std::vector<u64> tmp((u64)18 * count);
  for (u64 l = 0; l < count; l++)
    for (int i = 0; i < 18; i++) tmp[(u64)i * count + l] = in18[l * 18 + i];
  int rc = 0;
  for (int i = 0; i < 16; i++) rc |= h2d(c, c->d_gpr + i * N + first, tmp.data() + (u64)i * count, count);
  rc |= h2d(c, c->d_rip + first, tmp.data() + (u64)16 * count, count);
  rc |= h2d(c, c->d_rflags + first, tmp.data() + (u64)17 * count, count);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_regs(wtfgpu_ctx *c, uint32_t first, uint32_t count, wtfgpu_regs_t *out) {
  if (!lanes_ok(c, first, count) || !out) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  std::vector<u64> g((u64)18 * count);
  int rc = wtfgpu_read_gprs(c, first, count, g.data());
  if (rc) return rc;
  std::vector<u64> fsb(count), gsb(count);
  std::vector<LaneSys> sys(count);
  rc |= d2h(c, out, c->d_full + first, count);
  rc |= d2h(c, fsb.data(), c->d_fsb + first, count);
  rc |= d2h(c, gsb.data(), c->d_gsb + first, count);
  rc |= d2h(c, sys.data(), c->d_sys + first, count);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->q->stream));
  for (u64 l = 0; l < count; l++) {
    wtfgpu_regs_t &r = out[l];
    for (int i = 0; i < 16; i++) r.gpr[i] = g[l * 18 + i];
    r.rip = g[l * 18 + 16];
    r.rflags = g[l * 18 + 17];
    r.seg[WTFGPU_FS].base = fsb[l];
    r.seg[WTFGPU_GS].base = gsb[l];
    r.cr0 = sys[l].cr0;
    r.cr3 = sys[l].cr3;
    r.cr4 = sys[l].cr4;
    r.efer = sys[l].efer & ~EFER_M32;
    r.kernel_gs_base = sys[l].kgs;
    r.star = sys[l].star;
    r.lstar = sys[l].lstar;
    r.sfmask = sys[l].sfmask;
    r.cr2 = sys[l].cr2;
    r.seg[WTFGPU_CS].selector = sys[l].cs;
    r.seg[WTFGPU_SS].selector = sys[l].ss;
  }
  return WTFGPU_OK;
}

int wtfgpu_write_regs(wtfgpu_ctx *c, uint32_t first, uint32_t count, const wtfgpu_regs_t *in) {
  if (!lanes_ok(c, first, count) || !in) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  std::vector<u64> g((u64)18 * count), fsb(count), gsb(count);
  std::vector<LaneSys> sys(count);
  for (u64 l = 0; l < count; l++) {
    const wtfgpu_regs_t &r = in[l];
    for (int i = 0; i < 16; i++) g[l * 18 + i] = r.gpr[i];
    g[l * 18 + 16] = r.rip;
    g[l * 18 + 17] = r.rflags;
    fsb[l] = r.seg[WTFGPU_FS].base;
    gsb[l] = r.seg[WTFGPU_GS].base;
    sys[l] = make_init(r).sys;
  }
  int rc = wtfgpu_write_gprs(c, first, count, g.data());
  if (rc) return rc;
  rc |= h2d(c, c->d_full + first, in, count);
  rc |= h2d(c, c->d_fsb + first, fsb.data(), count);
  rc |= h2d(c, c->d_gsb + first, gsb.data(), count);
  rc |= h2d(c, c->d_sys + first, sys.data(), count);
  if (c->d_tlbok) HIPCHK(hipMemsetAsync(c->d_tlbok + first, 0, (u64)count * 4, c->q->stream));
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_exits(wtfgpu_ctx *c, uint32_t first, uint32_t count, wtfgpu_exit_t *out) {
  if (!lanes_ok(c, first, count) || !out) return WTFGPU_ERR_INVALID;
  if (count == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  // packed on the device, one copy back
  const u64 bytes = (u64)count * sizeof(wtfgpu_exit_t);
  if (ensure_scratch(c, bytes)) return WTFGPU_ERR_OOM;
  k_pack_exits<<<(count + 255) / 256, 256, 0, c->q->stream>>>(c->P, first, count, (wtfgpu_exit_t *)c->q->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->q->d_scratch, bytes, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

static int set_status_list(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t status, const uint8_t *skip) {
  if (!c || !c->d_status || (n && !lanes) || !lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  // lane list (+ skip flags) -> scratch, one scatter kernel: no whole-array round trips
  Side sk = side_in(skip, n);
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n, &sk, 1)) return rc;
  k_set_status<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)c->q->d_scratch, n, status,
                                                          skip ? c->q->d_scratch + sk.off : nullptr);
  HIPCHK(hipGetLastError());
  return WTFGPU_OK;
}

int wtfgpu_resume(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, const uint8_t *skip_bp) {
  std::vector<u8> zeros;
  if (!skip_bp) {
    zeros.assign(n, 0);
    skip_bp = zeros.data();
  }
  return set_status_list(c, lanes, n, WTFGPU_RUNNING, skip_bp);
}

int wtfgpu_stop(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t status) {
  return set_status_list(c, lanes, n, status, nullptr);
}

// Regrouping buffers of the current queue (sized by the lane count).
static int regroup_buffers(wtfgpu_ctx *c) {
  QueueRes &q = *c->q;
  if (q.d_rkeys) return WTFGPU_OK;
  const u64 N = c->P.nlanes;
  if (!c->d_perm && dalloc(&c->d_perm, N)) return WTFGPU_ERR_OOM;
  if (dalloc(&q.d_rkeys, N) || dalloc(&q.d_rkeys2, N) || dalloc(&q.d_rlanes, N)) return WTFGPU_ERR_OOM;
  size_t bytes = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, q.d_rkeys, q.d_rkeys2, q.d_rlanes, c->d_perm, (int)N, 0, 24,
                                            q.stream));
  HIPCHK(hipMalloc(&q.d_rtemp, bytes));
  q.rtemp_bytes = bytes;
  return WTFGPU_OK;
}

// The kernel parameters of a run on the current queue.
static Dev run_params(wtfgpu_ctx *c, bool regroup) {
  Dev Q = c->P;
  Q.perm = regroup ? c->d_perm : nullptr;
  Q.stat = c->q->d_stat;
  // warm-started LDS uop caches (WTFGPU_WARM=0: every launch starts empty)
  const char *w = getenv("WTFGPU_WARM");
  if (!(w && atoi(w) == 0)) {
    const u32 need = (u32)((c->P.nlanes + c->P.lpw - 1) / c->P.lpw);  // the most waves a launch can have
    if (c->d_warm && c->warm_n < need) {
      (void)hipDeviceSynchronize();
      (void)hipFree(c->d_warm);
      c->d_warm = nullptr;
    }
    if (!c->d_warm) {
      c->warm_n = need;
      const u64 bytes = UC_IMAGE_BYTES * need * UC_QUEUES;
      if (hipMalloc((void **)&c->d_warm, bytes) != hipSuccess) {
        c->d_warm = nullptr;
      } else if (hipMemset(c->d_warm, 0xff, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(c->d_warm);
        c->d_warm = nullptr;
      }
    }
    Q.warm = c->d_warm ? c->d_warm + (u64)(c->q->index % UC_QUEUES) * UC_IMAGE_BYTES * c->warm_n : nullptr;
    Q.warm_n = c->warm_n;
  } else {
    Q.warm = nullptr;
  }
  return Q;
}

// Whether this run regroups (see wtfgpu_ctx::regroup_auto): measure each
// schedule once, then run the one that retires more lanes per wave-step
// (regrouping must win by kMargin: its sorts and shorter launches cost time a
// wave-step count does not show), probing the other every kProbe-th run.
static u64 regroup_now(wtfgpu_ctx *c, u32 count) {
  c->q->rg_used = 2;  // not a measured choice
  if (!c->regroup_steps || count < 2 * c->P.lpw) return 0;
  if (!c->regroup_auto) return c->regroup_steps;
  static constexpr double kMargin = 1.1;
  static constexpr u64 kProbe = 32;
  const u64 i = c->rg_runs++;
  bool on;
  if (c->lps_sched[1] == 0) on = true;
  else if (c->lps_sched[0] == 0) on = false;
  else {
    on = c->lps_sched[1] > kMargin * c->lps_sched[0];
    if (i % kProbe == kProbe - 1) on = !on;
  }
  c->q->rg_used = on;
  return on ? c->regroup_steps : 0;
}
// The same choice for a synchronous run to completion, by kernel time per
// retired instruction (its result does not depend on the lane order).
static u64 regroup_now_timed(wtfgpu_ctx *c, u32 count, int &used) {
  used = 2;
  if (!c->regroup_steps || count < 2 * c->P.lpw) return 0;
  if (!c->regroup_auto) return c->regroup_steps;
  static constexpr u64 kProbe = 32;
  const u64 i = c->rg_sync_runs++;
  bool on;
  if (c->nspi_sched[1] == 0) on = true;
  else if (c->nspi_sched[0] == 0) on = false;
  else {
    on = c->nspi_sched[1] < c->nspi_sched[0];
    if (i % kProbe == kProbe - 1) on = !on;
  }
  used = on;
  return on ? c->regroup_steps : 0;
}
static void regroup_observe_timed(wtfgpu_ctx *c, int used, double ms, u64 retired) {
  if (used > 1 || retired < 4096) return;
  const double v = ms * 1e6 / (double)retired;
  double &e = c->nspi_sched[used];
  e = e == 0 ? v : 0.75 * e + 0.25 * v;
}
static void regroup_observe(wtfgpu_ctx *c, u64 group_steps, u64 retired) {
  const u8 used = c->q->rg_used;
  if (used > 1 || group_steps < 64) return;
  const double lps = (double)retired / (double)group_steps;
  double &e = c->lps_sched[used];
  e = e == 0 ? lps : 0.75 * e + 0.25 * lps;
}

// One k_run launch of `steps` wave-steps over [first, first + count), after
// the regrouping sort when on.
static int launch_chunk(wtfgpu_ctx *c, const Dev &Q, u32 first, u32 count, u64 steps, bool regroup) {
  QueueRes &q = *c->q;
  const u32 hwaves = (count + c->P.lpw - 1) / c->P.lpw;
  if (regroup) {
    HIPCHK(hipMemsetAsync(q.d_stat + 2, 0, 16, q.stream));  // running lanes: this launch's (2: after, 3: before)
    k_regroup_keys<<<(count + 255) / 256, 256, 0, q.stream>>>(Q, first, count, q.d_rkeys, q.d_rlanes);
    HIPCHK(hipGetLastError());
    size_t bytes = q.rtemp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(q.d_rtemp, bytes, q.d_rkeys, q.d_rkeys2, q.d_rlanes, c->d_perm + first,
                                              (int)count, 0, 24, q.stream));
  }
  k_run<<<(hwaves + 3) / 4, 256, 0, q.stream>>>(Q, first, count, steps);
  HIPCHK(hipGetLastError());
  return WTFGPU_OK;
}

// Diagnostic build only: the per-phase cycle totals of one run (stat[4..11]).
static void print_stamps(const u64 *s) {
#ifdef WTFGPU_STAMPS
  if (s[0])
    fprintf(stderr,
            "wtfgpu stamps (cycles per wave-step, %llu steps): fast loop %.0f, slow: xlate+fill %.0f, coverage %.0f, "
            "exec %.0f, cross-page %.0f; slow steps: miss %llu, codepage %llu, ucmiss %llu, other %llu; "
            "fast lookup %.0f, fast exec %.0f, bp %.0f\n",
            (unsigned long long)s[0], (double)s[4] / s[0], (double)s[6] / s[0], (double)s[7] / s[0],
            (double)s[5] / s[0], (double)s[9] / s[0], (unsigned long long)s[12], (unsigned long long)s[13],
            (unsigned long long)s[14], (unsigned long long)s[15], (double)s[10] / s[0], (double)s[11] / s[0], (double)s[8] / s[0]);
  fprintf(stderr, "wtfgpu stamps generic ops:");
  for (int k = 0; k < 512; k++)
    if (s[16 + k]) fprintf(stderr, " %d:%llu", k, (unsigned long long)s[16 + k]);
  fprintf(stderr, "\n");
  fprintf(stderr, "wtfgpu stamps bp_apply cycles by kind:");
  for (int k = 0; k < 8; k++) fprintf(stderr, " %d:%llu", k, (unsigned long long)s[528 + k]);
  fprintf(stderr, "\n");
#else
  (void)s;
#endif
}

// Up to `group` k_run launches of `chunk` wave-steps each, until `done`
// reaches max_steps, queued between the queue's ev0 and ev1 over zeroed
// statistics. Nothing waits.
static int queue_launches(wtfgpu_ctx *c, const Dev &Q, u32 first, u32 count, u64 chunk, u64 max_steps, u64 group,
                          bool regroup, u64 &done, u32 &launches) {
  QueueRes &q = *c->q;
  HIPCHK(hipMemsetAsync(q.d_stat, 0, STAT_N * 8, q.stream));
  HIPCHK(hipEventRecord(q.ev0, q.stream));
  for (launches = 0; launches < group && done < max_steps; launches++) {
    const u64 steps = std::min<u64>(chunk, max_steps - done);
    if (int rc = launch_chunk(c, Q, first, count, steps, regroup)) return rc;
    done += steps;
  }
  HIPCHK(hipEventRecord(q.ev1, q.stream));
  return WTFGPU_OK;
}

// The statistics of the launches queued last, added to `st`, after a wait for
// them; `running`: the lanes still running after the last launch.
static int collect_stats(wtfgpu_ctx *c, u32 launches, wtfgpu_run_stats_t &st, u64 &running) {
  QueueRes &q = *c->q;
  u64 s[STAT_N];
  HIPCHK(hipMemcpyAsync(s, q.d_stat, sizeof(s), hipMemcpyDeviceToHost, q.stream));
  HIPCHK(hipStreamSynchronize(q.stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, q.ev0, q.ev1));
  st.kernel_launches += launches;
  st.group_steps += s[0];
  st.lane_retired += s[1];
  st.kernel_ms += ms;
  running = s[2];
  print_stamps(s);
  return WTFGPU_OK;
}

int wtfgpu_run(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint64_t max_steps, wtfgpu_run_stats_t *stats) {
  if (!lanes_ok(c, first, count) || (first % c->P.lpw)) return WTFGPU_ERR_INVALID;
  if (!c->P.pool) return WTFGPU_ERR_STATE;
  if (c->q->async_launches) return WTFGPU_ERR_STATE;  // wtfgpu_run_wait first
  HIPCHK(hipSetDevice(c->device));
  wtfgpu_run_stats_t st{};
  u64 chunk = 1ull << 20;  // wave-steps per launch: keeps every launch short
  // Cross-wave regrouping: launches of `regroup` wave-steps, between them the
  // lanes are sorted by rip so that lanes that diverged from their wave
  // neighbours meet lanes at the same rip in another wave (wtfgpu_set_regroup,
  // WTFGPU_REGROUP_STEPS; 0 = fixed lane order; regroup_now).
  // (no step bound: a run to completion, see wtfgpu_ctx::nspi_sched)
  const bool to_end = max_steps >= (1ull << 32);
  int used_timed = 2;
  const u64 regroup = to_end ? regroup_now_timed(c, count, used_timed) : regroup_now(c, count);
  if (regroup) {
    chunk = regroup;
    if (int rc = regroup_buffers(c)) return rc;
  }
  const Dev Q = run_params(c, regroup != 0);
  // launches per host synchronisation: regrouped chunks are short, so a
  // group of them is queued at once (one stats read-back per group)
  const u32 group = regroup ? (u32)std::max<u64>(1, 4096 / regroup) : 1;
  u64 done = 0, running = 0;
  do {  // a statistics read-back per group; ends when no lane is running
    u32 k = 0;
    if (int rc = queue_launches(c, Q, first, count, chunk, max_steps, group, regroup != 0, done, k)) return rc;
    if (int rc = collect_stats(c, k, st, running)) return rc;
  } while (running && done < max_steps);
  if (to_end) regroup_observe_timed(c, used_timed, st.kernel_ms, st.lane_retired);
  else regroup_observe(c, st.group_steps, st.lane_retired);
  if (stats) *stats = st;
  return WTFGPU_OK;
}

int wtfgpu_run_async(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint64_t max_steps) {
  if (!lanes_ok(c, first, count) || (first % c->P.lpw) || max_steps == 0 || max_steps > (1ull << 32))
    return WTFGPU_ERR_INVALID;
  if (!c->P.pool) return WTFGPU_ERR_STATE;
  if (c->q->async_launches) return WTFGPU_ERR_STATE;
  HIPCHK(hipSetDevice(c->device));
  const u64 regroup = regroup_now(c, count);
  const u64 chunk = regroup ? regroup : max_steps;
  if (regroup)
    if (int rc = regroup_buffers(c)) return rc;
  const Dev Q = run_params(c, regroup != 0);
  HIPCHK(hipEventRecord(c->q->ev_pre, c->q->stream));  // the plumbing before this run (wtfgpu_select_queue)
  c->q->pre_valid = true;
  u64 done = 0;
  u32 k = 0;  // every launch of the run in one group: wtfgpu_run_wait reads the statistics
  if (int rc = queue_launches(c, Q, first, count, chunk, max_steps, ~0ull, regroup != 0, done, k)) return rc;
  c->q->async_launches = k;
  return WTFGPU_OK;
}

int wtfgpu_run_wait(wtfgpu_ctx *c, wtfgpu_run_stats_t *stats) {
  if (!c) return WTFGPU_ERR_INVALID;
  wtfgpu_run_stats_t st{};
  if (c->q->async_launches) {
    HIPCHK(hipSetDevice(c->device));
    u64 running = 0;
    if (int rc = collect_stats(c, c->q->async_launches, st, running)) return rc;
    ring_reset(c);  // the stream is idle
    c->q->async_launches = 0;
    regroup_observe(c, st.group_steps, st.lane_retired);
  }
  if (stats) *stats = st;
  return WTFGPU_OK;
}

int wtfgpu_prefetch_results(wtfgpu_ctx *c, uint32_t first, uint32_t count, wtfgpu_exit_t *exits, uint64_t *bytes,
                            uint32_t *dirty, uint64_t *stop_args) {
  if (!lanes_ok(c, first, count) || !exits) return WTFGPU_ERR_INVALID;
  if (count == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (c->q->exq_cap < count) {  // stream-ordered, as ensure_scratch
    if (c->q->d_exq) HIPCHK(hipFreeAsync(c->q->d_exq, c->q->stream));
    c->q->d_exq = nullptr;
    c->q->exq_cap = 0;
    if (hipMallocAsync((void **)&c->q->d_exq, (u64)count * sizeof(wtfgpu_exit_t), c->q->stream) != hipSuccess)
      return WTFGPU_ERR_OOM;
    c->q->exq_cap = count;
  }
  k_pack_exits<<<(count + 255) / 256, 256, 0, c->q->stream>>>(c->P, first, count, c->q->d_exq);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(exits, c->q->d_exq, (u64)count * sizeof(wtfgpu_exit_t), hipMemcpyDeviceToHost, c->q->stream));
  if (bytes) HIPCHK(hipMemcpyAsync(bytes, c->d_nbytes + first, (u64)count * 8, hipMemcpyDeviceToHost, c->q->stream));
  if (dirty) HIPCHK(hipMemcpyAsync(dirty, c->d_ovcount + first, (u64)count * 4, hipMemcpyDeviceToHost, c->q->stream));
  if (stop_args && c->d_stopargs)
    HIPCHK(hipMemcpyAsync(stop_args, c->d_stopargs + (u64)first * 6, (u64)count * 48, hipMemcpyDeviceToHost,
                          c->q->stream));
  return WTFGPU_OK;
}

constexpr u64 kPcovCap = 1ull << 22;  // prefetched coverage entries per queue
constexpr u64 kPcovLanes = 256, kPcovRips = kPcovLanes + kPcovCap * 4;

int wtfgpu_prefetch_coverage(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint64_t *hdr) {
  if (!lanes_ok(c, first, count) || !hdr) return WTFGPU_ERR_INVALID;
  if (!c->d_covrip || count == 0) {
    hdr[0] = hdr[1] = 0;
    return WTFGPU_ERR_STATE;  // nothing to prefetch: the caller reads the sets itself
  }
  HIPCHK(hipSetDevice(c->device));
  if (!c->q->d_pcov && hipMallocAsync((void **)&c->q->d_pcov, kPcovRips + kPcovCap * 8, c->q->stream) != hipSuccess) {
    c->q->d_pcov = nullptr;
    return WTFGPU_ERR_OOM;
  }
  HIPCHK(hipMemsetAsync(c->q->d_pcov, 0, 16, c->q->stream));
  k_cov_collect_stopped<<<(count + 3) / 4, 256, 0, c->q->stream>>>(
      c->P, first, count, (u32 *)(c->q->d_pcov + kPcovLanes), (u64 *)(c->q->d_pcov + kPcovRips), kPcovCap,
      (unsigned long long *)c->q->d_pcov, (u32 *)(c->q->d_pcov + 8));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hdr, c->q->d_pcov, 16, hipMemcpyDeviceToHost, c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_prefetched_coverage(wtfgpu_ctx *c, uint32_t *out_lanes, uint64_t *out_rips, uint64_t n) {
  if (!c || (n && (!out_lanes || !out_rips)) || n > kPcovCap || (n && !c->q->d_pcov)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out_lanes, c->q->d_pcov + kPcovLanes, n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(out_rips, c->q->d_pcov + kPcovRips, n * 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_clear_coverage_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n) {
  if (!c || (n && !lanes)) return WTFGPU_ERR_INVALID;
  if (!c->d_covrip || n == 0) return WTFGPU_OK;  // (without coverage sets a lane out of range passes: kept)
  if (!lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = stage_lanes(c, Upload::Ring, lanes, n)) return rc;
  k_cov_clear<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)c->q->d_scratch, n);
  HIPCHK(hipGetLastError());
  return WTFGPU_OK;
}

int wtfgpu_lane_seeds(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t *seeds, int write) {
  if (!c || (n && (!lanes || !seeds)) || !c->d_rdseed || !lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side s = side_in(write ? seeds : nullptr, (u64)n * 8);
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &s, 1)) return rc;
  k_lane_seeds<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)c->q->d_scratch, n,
                                                          (u64 *)(c->q->d_scratch + s.off), write);
  HIPCHK(hipGetLastError());
  if (!write) return read_back(c, seeds, s);
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_stop_args(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t *out6) {
  if (!c || (n && (!lanes || !out6)) || !c->d_stopargs || !lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side out = side_room((u64)n * 48);
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &out, 1)) return rc;
  k_stop_args<<<(n * 6 + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)c->q->d_scratch, n,
                                                             (u64 *)(c->q->d_scratch + out.off));
  HIPCHK(hipGetLastError());
  return read_back(c, out6, out);
}

int wtfgpu_select_queue(wtfgpu_ctx *c, uint32_t queue) {
  if (!c || queue >= 2) return WTFGPU_ERR_INVALID;
  QueueRes &cur = *c->q, &next = c->queues[queue];
  if (&next == &cur) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (!next.stream)
    if (int rc = queue_create(next, queue)) return rc;
  // The plumbing queued on the old queue without a wait (restores, status
  // and feed uploads, wtfgpu_restore_lanes ...) may touch lanes the new
  // queue runs: the new queue's later work is ordered after it. Only after
  // the plumbing: with a run in flight, after the event wtfgpu_run_async
  // recorded before its launches (the two queues' slices still overlap);
  // without one, after everything the old queue holds.
  if (!cur.async_launches) {
    HIPCHK(hipEventRecord(cur.ev_pre, cur.stream));
    cur.pre_valid = true;
  }
  if (cur.pre_valid) HIPCHK(hipStreamWaitEvent(next.stream, cur.ev_pre, 0));
  c->q = &next;
  return WTFGPU_OK;
}

// ---- lane memory services
static int lane_mem(wtfgpu_ctx *c, uint32_t lane, u32 op, u64 addr, void *buf, u64 len, i64 *result) {
  if (!c || lane >= c->P.nlanes) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  if (ensure_scratch(c, len + 64)) return WTFGPU_ERR_OOM;
  i64 *d_res = (i64 *)c->q->d_scratch;
  u8 *d_buf = c->q->d_scratch + 64;
  if ((op == 2 || op == 4) && len) HIPCHK(hipMemcpyAsync(d_buf, buf, len, hipMemcpyHostToDevice, c->q->stream));
  k_lane_mem<<<1, 64, 0, c->q->stream>>>(c->P, lane, op, addr, len, d_buf, d_res);
  HIPCHK(hipGetLastError());
  if ((op == 1 || op == 3) && len) HIPCHK(hipMemcpyAsync(buf, d_buf, len, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(result, d_res, 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_lane_translate(wtfgpu_ctx *c, uint32_t lane, uint64_t gva, uint64_t *gpa) {
  i64 r = 0;
  int rc = lane_mem(c, lane, 0, gva, nullptr, 0, &r);
  if (rc) return rc;
  if (r < 0) return WTFGPU_ERR_TRANSLATE;
  if (gpa) *gpa = (u64)r;
  return WTFGPU_OK;
}
int wtfgpu_lane_read_phys(wtfgpu_ctx *c, uint32_t lane, uint64_t gpa, void *buf, uint64_t len) {
  i64 r = 0;
  int rc = lane_mem(c, lane, 1, gpa, buf, len, &r);
  return rc ? rc : (r < 0 ? WTFGPU_ERR_TRANSLATE : WTFGPU_OK);
}
int wtfgpu_lane_write_phys(wtfgpu_ctx *c, uint32_t lane, uint64_t gpa, const void *buf, uint64_t len) {
  i64 r = 0;
  int rc = lane_mem(c, lane, 2, gpa, (void *)buf, len, &r);
  return rc ? rc : (r == -2 ? WTFGPU_ERR_OOM : (r < 0 ? WTFGPU_ERR_TRANSLATE : WTFGPU_OK));
}
int wtfgpu_lane_read_virt(wtfgpu_ctx *c, uint32_t lane, uint64_t gva, void *buf, uint64_t len) {
  i64 r = 0;
  int rc = lane_mem(c, lane, 3, gva, buf, len, &r);
  return rc ? rc : (r < 0 ? WTFGPU_ERR_TRANSLATE : WTFGPU_OK);
}
int wtfgpu_lane_write_virt(wtfgpu_ctx *c, uint32_t lane, uint64_t gva, const void *buf, uint64_t len) {
  i64 r = 0;
  int rc = lane_mem(c, lane, 4, gva, (void *)buf, len, &r);
  return rc ? rc : (r == -2 ? WTFGPU_ERR_OOM : (r < 0 ? WTFGPU_ERR_TRANSLATE : WTFGPU_OK));
}

static int apply_writes(wtfgpu_ctx *c, const wtfgpu_write_t *writes, uint32_t n, const uint8_t *data,
                        uint64_t data_len, int32_t *status_out, u32 phys) {
  if (!c || (n && (!writes || !data))) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<u32> order(n);
  for (u32 i = 0; i < n; i++) {
    order[i] = i;
    if (writes[i].lane >= c->P.nlanes || writes[i].data_off + writes[i].len > data_len) return WTFGPU_ERR_INVALID;
  }
  bool grouped = true;  // records of a lane already consecutive and lanes ascending: no sort
  for (u32 i = 1; i < n && grouped; i++) grouped = writes[i - 1].lane <= writes[i].lane;
  if (!grouped)
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return writes[a].lane < writes[b].lane; });
  std::vector<WriteRec> recs(n);
  std::vector<u32> starts;
  for (u32 i = 0; i < n; i++) {
    const wtfgpu_write_t &w = writes[order[i]];
    recs[i] = WriteRec{w.lane, w.len, w.gva, w.data_off};
    if (i == 0 || w.lane != recs[i - 1].lane) starts.push_back(i);
  }
  const u32 nl = (u32)starts.size();
  starts.push_back(n);
  const u64 b_recs = (u64)n * sizeof(WriteRec), b_starts = starts.size() * 4ull, b_st = (u64)n * 4;
  const u64 o_starts = (b_recs + 255) & ~255ull, o_st = (o_starts + b_starts + 255) & ~255ull,
            o_data = (o_st + b_st + 255) & ~255ull;
  if (ensure_scratch(c, o_data + data_len)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpyAsync(c->q->d_scratch, recs.data(), b_recs, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->q->d_scratch + o_starts, starts.data(), b_starts, hipMemcpyHostToDevice, c->q->stream));
  HIPCHK(hipMemcpyAsync(c->q->d_scratch + o_data, data, data_len, hipMemcpyHostToDevice, c->q->stream));
  k_apply_writes<<<nl, 64, 0, c->q->stream>>>(c->P, (const WriteRec *)c->q->d_scratch,
                                                       (const u32 *)(c->q->d_scratch + o_starts), nl,
                                                       c->q->d_scratch + o_data, (i32 *)(c->q->d_scratch + o_st), phys);
  HIPCHK(hipGetLastError());
  std::vector<i32> st(n);
  HIPCHK(hipMemcpyAsync(st.data(), c->q->d_scratch + o_st, b_st, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  int rc = WTFGPU_OK;
  for (u32 i = 0; i < n; i++) {
    if (status_out) status_out[order[i]] = st[i];
    if (st[i]) rc = st[i];
  }
  return rc;
}

int wtfgpu_apply_writes(wtfgpu_ctx *c, const wtfgpu_write_t *writes, uint32_t n, const uint8_t *data,
                        uint64_t data_len, int32_t *status_out) {
  return apply_writes(c, writes, n, data, data_len, status_out, 0);
}
int wtfgpu_apply_phys_writes(wtfgpu_ctx *c, const wtfgpu_write_t *writes, uint32_t n, const uint8_t *data,
                             uint64_t data_len, int32_t *status_out) {
  return apply_writes(c, writes, n, data, data_len, status_out, 1);
}

int wtfgpu_read_gprs_list(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t *out18) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side out = side_room((u64)n * 18 * 8);
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &out, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  k_gather_gprs<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n, (u64 *)(S + out.off));
  HIPCHK(hipGetLastError());
  return read_back(c, out18, out);
}

int wtfgpu_write_gprs_list(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, const uint64_t *in18) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side in = side_in(in18, (u64)n * 18 * 8);
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &in, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  k_scatter_gprs<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n, (const u64 *)(S + in.off));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_dirty_list(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t *out) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side o = side_room((u64)n * ((u64)c->P.K + c->P.X + 1) * 4);
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &o, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  k_gather_dirty<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n, (u32 *)(S + o.off));
  HIPCHK(hipGetLastError());
  return read_back(c, out, o);
}

uint32_t wtfgpu_overlay_pages(wtfgpu_ctx *c) { return c ? c->P.K : 0; }

int wtfgpu_gather_pages(wtfgpu_ctx *c, const uint32_t *lanes, const uint64_t *gpas, uint32_t n, uint8_t *out) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  if (!gpas || !out || !c->P.pool) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  Side s[] = {side_in(gpas, (u64)n * 8), side_room((u64)n * WTFGPU_PAGE_SIZE, 4096)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_gather_pages<<<n, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, (const u64 *)(S + s[0].off), n, S + s[1].off);
  HIPCHK(hipGetLastError());
  return read_back(c, out, s[1]);
}

int wtfgpu_inject_fault(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t vector, uint32_t error,
                        const uint64_t *addrs, int32_t *delivered) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  if (!addrs || !delivered || vector > 31) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  Side s[] = {side_in(addrs, (u64)n * 8), side_room((u64)n * 4)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_inject_fault<<<(n + 63) / 64, 64, 0, c->q->stream>>>(c->P, (const u32 *)S, (const u64 *)(S + s[0].off), n, vector,
                                                         error, (i32 *)(S + s[1].off));
  HIPCHK(hipGetLastError());
  return read_back(c, delivered, s[1]);
}

int wtfgpu_gather_bytes(wtfgpu_ctx *c, const uint32_t *lanes, const uint64_t *gpas, uint32_t n, uint32_t len,
                        uint8_t *out) {
  if (int rc = check_lane_list(c, lanes, n)) return rc;
  if (n == 0) return WTFGPU_OK;
  if (!gpas || !out || !c->P.pool || len == 0 || len > 256) return WTFGPU_ERR_INVALID;
  for (u32 i = 0; i < n; i++)
    if ((gpas[i] & 0xfff) + len > WTFGPU_PAGE_SIZE) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  Side s[] = {side_in(gpas, (u64)n * 8), side_room((u64)n * len)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 2)) return rc;
  u8 *const S = c->q->d_scratch;
  k_gather_bytes<<<n, 64, 0, c->q->stream>>>(c->P, (const u32 *)S, (const u64 *)(S + s[0].off), n, len, S + s[1].off);
  HIPCHK(hipGetLastError());
  return read_back(c, out, s[1]);
}

static int lane_cr_ptr(wtfgpu_ctx *c, uint32_t lane, uint32_t cr, u8 **p) {
  if (!c || !c->d_sys || lane >= c->P.nlanes || (cr != 2 && cr != 3)) return WTFGPU_ERR_INVALID;
  *p = (u8 *)(c->d_sys + lane) + (cr == 2 ? offsetof(LaneSys, cr2) : offsetof(LaneSys, cr3));
  return WTFGPU_OK;
}

int wtfgpu_lane_get_cr(wtfgpu_ctx *c, uint32_t lane, uint32_t cr, uint64_t *value) {
  u8 *p = nullptr;
  if (!value || lane_cr_ptr(c, lane, cr, &p)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(value, p, 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_lane_set_cr(wtfgpu_ctx *c, uint32_t lane, uint32_t cr, uint64_t value) {
  u8 *p = nullptr;
  if (lane_cr_ptr(c, lane, cr, &p)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(p, &value, 8, hipMemcpyHostToDevice, c->q->stream));
  if (cr == 3) HIPCHK(hipMemsetAsync(c->d_tlbok + lane, 0, 4, c->q->stream));  // translations of the old cr3
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// Page-locked host memory for staging buffers: device<->host copies into it
// are plain DMA (no bounce through a driver staging buffer).
int wtfgpu_host_alloc(wtfgpu_ctx *c, uint64_t bytes, void **out) {
  if (!c || !out || !bytes) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) return WTFGPU_ERR_OOM;
  return WTFGPU_OK;
}

int wtfgpu_host_free(wtfgpu_ctx *c, void *p) {
  if (!c) return WTFGPU_ERR_INVALID;
  if (p) HIPCHK(hipHostFree(p));
  return WTFGPU_OK;
}

int wtfgpu_read_dirty(wtfgpu_ctx *c, uint32_t lane, uint64_t *gpas, uint32_t cap, uint32_t *n) {
  if (!c || lane >= c->P.nlanes || !n) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  u32 cnt = 0;  // (on the queue's stream: after its queued restores)
  HIPCHK(hipMemcpyAsync(&cnt, c->d_ovcount + lane, 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  *n = cnt;
  for (u32 k = 0; k < cnt && k < cap; k++) {
    u32 g = 0;
    HIPCHK(hipMemcpyAsync(&g, c->d_ovgpfn + (u64)k * c->P.nlanes + lane, 4, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipStreamSynchronize(c->q->stream));
    gpas[k] = (u64)g << 12;
  }
  return WTFGPU_OK;
}

// The coverage sets of a lane list (lanes == nullptr: first .. first+n),
// compacted into (lane, rip) pairs; `clear` empties the sets read.
static int collect_sets(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t first, uint32_t n, uint32_t *out_lanes,
                        uint64_t *out_rips, uint64_t cap, uint64_t *total, uint32_t *overflow, int clear) {
  HIPCHK(hipSetDevice(c->device));
  const u64 room = std::max<u64>(cap, 1);
  // header (total, overflow) | lanes out | rips out
  Side s[] = {side_room(256), side_room(room * 4), side_room(room * 8)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, s, 3)) return rc;
  u8 *const S = c->q->d_scratch, *const H = S + s[0].off;
  HIPCHK(hipMemsetAsync(H, 0, 16, c->q->stream));
  k_cov_collect<<<n, 256, 0, c->q->stream>>>(c->P, lanes ? (const u32 *)S : nullptr, first, n, (u32 *)(S + s[1].off),
                                             (u64 *)(S + s[2].off), cap, (unsigned long long *)H, (u32 *)(H + 8));
  HIPCHK(hipGetLastError());
  u64 hdr[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hdr, H, 16, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  if (clear && lanes && hdr[0] <= cap) {  // everything was read: the sets empty (ordered before later work)
    k_cov_clear<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n);
    HIPCHK(hipGetLastError());
  }
  const u64 m = std::min(hdr[0], cap);
  if (m) {
    HIPCHK(hipMemcpyAsync(out_lanes, S + s[1].off, m * 4, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipMemcpyAsync(out_rips, S + s[2].off, m * 8, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipStreamSynchronize(c->q->stream));
  }
  if (overflow) *overflow = (u32)hdr[1] & 1;
  *total = hdr[0];
  return WTFGPU_OK;
}

int wtfgpu_read_coverage(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint32_t *lanes, uint64_t *rips,
                         uint64_t cap, uint64_t *n, uint32_t *overflow) {
  if (!lanes_ok(c, first, count) || !n || (cap && (!lanes || !rips))) return WTFGPU_ERR_INVALID;
  *n = 0;
  if (overflow) *overflow = 0;
  if (!c->d_covrip || count == 0) return WTFGPU_OK;
  return collect_sets(c, nullptr, first, count, lanes, rips, cap, n, overflow, 0);
}

int wtfgpu_collect_coverage_lanes(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t *out_lanes,
                                  uint64_t *out_rips, uint64_t cap, uint64_t *total, uint32_t *overflow) {
  if (!c || !total || (n && !lanes) || (cap && (!out_lanes || !out_rips))) return WTFGPU_ERR_INVALID;
  *total = 0;
  if (overflow) *overflow = 0;
  // the range check comes after the look for the sets here and before it in
  // wtfgpu_attribute_coverage: an accident, kept (callers see the return codes)
  if (!c->d_covrip || n == 0) return WTFGPU_OK;
  if (!lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  return collect_sets(c, lanes, 0, n, out_lanes, out_rips, cap, total, overflow, 1);
}

// The target set of wtfgpu_coverage_contains (engine_covkeep.h): a device copy
// that replaces the earlier one. Rare (once a session): every queue is drained
// first, since a check in flight on either reads the copy it replaces.
int wtfgpu_coverage_target(wtfgpu_ctx *c, const uint64_t *values, uint64_t n) {
  if (!c || (n && !values) || n > 0xFFFFFFFFull) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  dfree(c->d_covtarget);
  c->covtarget_n = 0;
  c->covtarget_set = false;
  if (dalloc(&c->d_covtarget, std::max<u64>(n, 1))) return WTFGPU_ERR_OOM;
  if (n) HIPCHK(hipMemcpy(c->d_covtarget, values, n * 8, hipMemcpyHostToDevice));
  c->covtarget_n = (u32)n;
  c->covtarget_set = true;
  return WTFGPU_OK;
}

// How much of the target each listed lane's set lacks (k_cov_contains); the
// sets stay as they are.
int wtfgpu_coverage_contains(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint32_t *missing, uint32_t *size,
                             uint32_t *overflow) {
  if (!c || (n && (!lanes || !missing || !size || !overflow))) return WTFGPU_ERR_INVALID;
  if (!c->d_gpr || !c->d_covrip || !c->covtarget_set) return WTFGPU_ERR_STATE;
  if (!lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side out = side_room((u64)n * 12);  // missing[n] | size[n] | overflow[n]
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &out, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  u32 *const o = (u32 *)(S + out.off);
  k_cov_contains<<<(n + 3) / 4, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n, c->d_covtarget, c->covtarget_n, o,
                                                        o + n, o + 2 * (u64)n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(missing, o, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(size, o + n, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(overflow, o + 2 * (u64)n, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// Each listed lane's set as a signature (k_cov_signature; engine_analyze.h);
// the sets stay as they are.
int wtfgpu_coverage_signature(wtfgpu_ctx *c, const uint32_t *lanes, uint32_t n, uint64_t *sig, uint32_t *size,
                              uint32_t *overflow) {
  if (!c || (n && (!lanes || !sig || !size || !overflow))) return WTFGPU_ERR_INVALID;
  if (!c->d_gpr || !c->d_covrip) return WTFGPU_ERR_STATE;
  if (!lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;
  if (n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  Side out = side_room((u64)n * 16);  // sig[n] | size[n] | overflow[n]
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, &out, 1)) return rc;
  u8 *const S = c->q->d_scratch;
  u64 *const o = (u64 *)(S + out.off);
  u32 *const o32 = (u32 *)(o + n);
  k_cov_signature<<<(n + 3) / 4, 256, 0, c->q->stream>>>(c->P, (const u32 *)S, n, o, o32, o32 + n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sig, o, (u64)n * 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(size, o32, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(overflow, o32 + n, (u64)n * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// The new values of a lane list attributed in list order on the device (see
// wtfgpu.h). Two device passes with one look at their counts between them:
// most calls of a warmed-up campaign end at the first (no candidate left
// after the filter against the aggregate).
int wtfgpu_attribute_coverage(wtfgpu_ctx *c, const uint32_t *lanes, const uint8_t *revoke, uint32_t n, uint32_t flags,
                              uint32_t *out_pos, uint64_t *out_vals, uint64_t cap, uint64_t *total, uint64_t *entries,
                              uint32_t *overflow) {
  if (!c || !total || (n && !lanes) || (cap && (!out_pos || !out_vals)) || (flags & ~(uint32_t)WTFGPU_ATTRIB_ALL))
    return WTFGPU_ERR_INVALID;
  *total = 0;
  if (entries) *entries = 0;
  if (overflow) *overflow = 0;
  if (!lane_list_in_range(c, lanes, n)) return WTFGPU_ERR_INVALID;  // (before the look for the sets: see above)
  if (!c->d_covrip || n == 0) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const u32 all = flags & WTFGPU_ATTRIB_ALL ? 1 : 0;
  const auto up = [](u64 v) { return (v + 255) & ~255ull; };
  size_t tmp_n = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_n, (u32 *)nullptr, (u32 *)nullptr, (int)(n + 1), c->q->stream));
  // queue scratch: lanes | revoke | cnt[n + 1] | off[n + 1] | header (entries, overflow) | scan scratch
  const bool rev = revoke && !all;
  Side sc[] = {side_in(rev ? revoke : nullptr, n), side_room((u64)(n + 1) * 4), side_room((u64)(n + 1) * 4),
               side_room(256), side_room(tmp_n)};
  if (int rc = stage_lanes(c, Upload::Direct, lanes, n, sc, 5)) return rc;
  const u64 o_rev = sc[0].off, o_cnt = sc[1].off, o_off = sc[2].off, o_hdr = sc[3].off, o_tmp = sc[4].off;
  u8 *const S = c->q->d_scratch;
  const u32 *d_lanes = (const u32 *)S;
  const u8 *d_rev = S + o_rev;
  u32 *d_cnt = (u32 *)(S + o_cnt), *d_off = (u32 *)(S + o_off);
  if (!rev) HIPCHK(hipMemsetAsync(S + o_rev, 0, n, c->q->stream));
  HIPCHK(hipMemsetAsync(S + o_cnt, 0, (u64)(n + 1) * 4, c->q->stream));
  HIPCHK(hipMemsetAsync(S + o_hdr, 0, 16, c->q->stream));
  const u32 wblocks = (n + 3) / 4;
  k_attr_scan<<<wblocks, 256, 0, c->q->stream>>>(c->P, d_lanes, n, all, d_cnt, nullptr, nullptr,
                                              (unsigned long long *)(S + o_hdr), (u32 *)(S + o_hdr + 8));
  HIPCHK(hipGetLastError());
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(S + o_tmp, tmp_n, d_cnt, d_off, (int)(n + 1), c->q->stream));
  u64 hdr[2] = {0, 0};
  u32 s = 0;  // candidates (the scan's last sum; 32 bits hold nlanes * H of any context that fits the device)
  HIPCHK(hipMemcpyAsync(hdr, S + o_hdr, 16, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipMemcpyAsync(&s, d_off + n, 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  if (entries) *entries = hdr[0];
  if (overflow) *overflow = (u32)hdr[1] & 1;
  const auto clear = [&]() -> int {  // everything was read: the sets empty (ordered before later work)
    k_cov_clear<<<(n + 255) / 256, 256, 0, c->q->stream>>>(c->P, d_lanes, n);
    HIPCHK(hipGetLastError());
    return WTFGPU_OK;
  };
  if (s == 0) return clear();
  if (all && cap < s) {  // parity mode emits every candidate: nothing more to learn without room
    *total = s;
    return WTFGPU_OK;
  }
  // own buffer: raw | vals | pos | slot | keys[T + 1] | own[T + 1] | flag[s + 1] | at[s + 1] | out_pos | out_vals | scan scratch
  u32 T = 64;
  while (T < 2ull * s && T < (1u << 31)) T <<= 1;
  if (T < 2ull * s) return WTFGPU_ERR_OOM;
  size_t tmp_s = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_s, (u32 *)nullptr, (u32 *)nullptr, (int)(s + 1), c->q->stream));
  const u64 a_vals = up((u64)s * 8), a_pos = a_vals + up((u64)s * 8), a_slot = a_pos + up((u64)s * 4),
            a_keys = a_slot + up((u64)s * 4), a_own = a_keys + up(((u64)T + 1) * 8),
            a_flag = a_own + up(((u64)T + 1) * 4), a_at = a_flag + up(((u64)s + 1) * 4),
            a_opos = a_at + up(((u64)s + 1) * 4), a_oval = a_opos + up((u64)s * 4), a_tmp = a_oval + up((u64)s * 8),
            a_end = a_tmp + tmp_s;
  if (c->attr_bytes < a_end) {
    dfree(c->d_attr);
    c->attr_bytes = 0;
    const u64 want = std::max<u64>(a_end + a_end / 2, 1ull << 20);
    if (hipMalloc((void **)&c->d_attr, want) != hipSuccess) return WTFGPU_ERR_OOM;
    c->attr_bytes = want;
  }
  u8 *const A = c->d_attr;
  u64 *d_raw = (u64 *)A, *d_vals = (u64 *)(A + a_vals);
  u32 *d_pos = (u32 *)(A + a_pos);
  k_attr_scan<<<wblocks, 256, 0, c->q->stream>>>(c->P, d_lanes, n, all, nullptr, d_off, d_raw, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  k_attr_sort<<<wblocks, 256, 0, c->q->stream>>>(d_cnt, d_off, n, d_raw, d_vals, d_pos);
  HIPCHK(hipGetLastError());
  const u32 *d_rpos = d_pos;  // the result, on the device
  const u64 *d_rvals = d_vals;
  u32 m = s;
  if (!all) {
    u32 *d_slot = (u32 *)(A + a_slot), *d_own = (u32 *)(A + a_own), *d_flag = (u32 *)(A + a_flag),
        *d_at = (u32 *)(A + a_at);
    HIPCHK(hipMemsetAsync(A + a_keys, 0xff, a_flag - a_keys, c->q->stream));  // keys and own: all bits set
    k_attr_owner<<<(s + 255) / 256, 256, 0, c->q->stream>>>(d_vals, d_pos, s, d_rev, (u64 *)(A + a_keys), d_own, T,
                                                            d_slot);
    HIPCHK(hipGetLastError());
    k_attr_keep<<<s / 256 + 1, 256, 0, c->q->stream>>>(d_pos, d_slot, d_own, s, d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(A + a_tmp, tmp_s, d_flag, d_at, (int)(s + 1), c->q->stream));
    k_attr_emit<<<(s + 255) / 256, 256, 0, c->q->stream>>>(d_vals, d_pos, d_flag, d_at, s, (u32 *)(A + a_opos),
                                                        (u64 *)(A + a_oval));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&m, d_at + s, 4, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipStreamSynchronize(c->q->stream));
    d_rpos = (const u32 *)(A + a_opos);
    d_rvals = (const u64 *)(A + a_oval);
  }
  *total = m;
  if (cap < m) return WTFGPU_OK;  // nothing emptied: the caller calls again with room
  if (m) {
    HIPCHK(hipMemcpyAsync(out_pos, d_rpos, (u64)m * 4, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipMemcpyAsync(out_vals, d_rvals, (u64)m * 8, hipMemcpyDeviceToHost, c->q->stream));
  }
  const int rc = clear();
  HIPCHK(hipStreamSynchronize(c->q->stream));  // d_attr serves both queues: idle at every return
  return rc;
}

int wtfgpu_commit_coverage(wtfgpu_ctx *c, const uint64_t *rips, uint64_t n) {
  if (!c || (n && !rips)) return WTFGPU_ERR_INVALID;
  if (n == 0 || !c->d_covmap) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (ensure_scratch(c, n * 8)) return WTFGPU_ERR_OOM;
  HIPCHK(hipMemcpyAsync(c->q->d_scratch, rips, n * 8, hipMemcpyHostToDevice, c->q->stream));
  k_cov_commit<<<(u32)((n + 255) / 256), 256, 0, c->q->stream>>>(c->P, (const u64 *)c->q->d_scratch, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_reset_coverage(wtfgpu_ctx *c) {
  if (!c) return WTFGPU_ERR_INVALID;
  if (!c->d_covmap) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(c->d_covmap, 0, c->ncovslots * WTFGPU_PAGE_SIZE, c->q->stream));
  HIPCHK(hipMemsetAsync(c->d_covshadow, 0, c->ncovslots * WTFGPU_PAGE_SIZE, c->q->stream));
  if (c->d_extra) HIPCHK(hipMemsetAsync(c->d_extra, 0xff, (u64)kExtraEntries * 8, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return guc_clear(c);  // shared entries and images carry UC_COVERED
}

int wtfgpu_set_trace(wtfgpu_ctx *c, uint32_t per_lane) {
  if (!c || !c->P.nlanes) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  dfree(c->d_trace);
  dfree(c->d_tracecnt);
  c->P.trace = nullptr;
  c->P.trace_cnt = nullptr;
  c->P.trace_cap = 0;
  if (per_lane) {
    const u64 N = c->P.nlanes;
    if (dalloc(&c->d_trace, N * per_lane) || dalloc(&c->d_tracecnt, N)) return WTFGPU_ERR_OOM;
    HIPCHK(hipMemset(c->d_tracecnt, 0, N * 4));
    c->P.trace = c->d_trace;
    c->P.trace_cnt = c->d_tracecnt;
    c->P.trace_cap = per_lane;
  }
  return guc_clear(c);  // cached entries were digested for the other setting
}

int wtfgpu_read_trace(wtfgpu_ctx *c, uint32_t lane, uint64_t *rips, uint64_t cap, uint64_t *n) {
  if (!c || !n || (cap && !rips) || lane >= c->P.nlanes || !c->d_trace) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  u32 cnt = 0;
  HIPCHK(hipMemcpyAsync(&cnt, c->d_tracecnt + lane, 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  *n = cnt;
  const u64 k = std::min<u64>(std::min<u64>(cnt, c->P.trace_cap), cap);
  if (k)
    HIPCHK(hipMemcpyAsync(rips, c->d_trace + (u64)lane * c->P.trace_cap, k * 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

// Tenet traces (engine_exec.h TenetDev): bytes_per_lane of entries per lane, 0 = off.
int wtfgpu_set_tenet(wtfgpu_ctx *c, uint64_t bytes_per_lane) {
  if (!c || !c->d_gpr || (bytes_per_lane & 7)) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  dfree(c->d_tn_buf);
  dfree(c->d_tn_pos);
  dfree(c->d_tn_cpos);
  dfree(c->d_tn_ipos);
  dfree(c->d_tn_last);
  dfree(c->d_tn_mute);
  TenetDev T{};
  c->tn_cap = 0;
  if (bytes_per_lane) {
    const u64 N = c->P.nlanes;
    if (dalloc(&c->d_tn_buf, N * bytes_per_lane) || dalloc(&c->d_tn_pos, N) || dalloc(&c->d_tn_cpos, N) ||
        dalloc(&c->d_tn_ipos, N) || dalloc(&c->d_tn_last, N) || dalloc(&c->d_tn_mute, N))
      return WTFGPU_ERR_OOM;
    HIPCHK(hipMemset(c->d_tn_pos, 0, N * 8));
    HIPCHK(hipMemset(c->d_tn_cpos, 0, N * 8));
    HIPCHK(hipMemset(c->d_tn_ipos, 0, N * 8));
    HIPCHK(hipMemset(c->d_tn_last, 0xff, N * 8));
    HIPCHK(hipMemset(c->d_tn_mute, 0, N * 4));
    T = TenetDev{c->d_tn_buf, bytes_per_lane, c->d_tn_pos, c->d_tn_cpos, c->d_tn_ipos, c->d_tn_last, c->d_tn_mute};
    c->tn_cap = bytes_per_lane;
  }
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tn), &T, sizeof(T)));
  return guc_clear(c);  // cached entries were digested for the other setting
}

int wtfgpu_read_tenet(wtfgpu_ctx *c, uint32_t lane, uint8_t *buf, uint64_t cap, uint64_t *n) {
  if (!c || !n || (cap && !buf) || lane >= c->P.nlanes || !c->d_tn_buf) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  u64 pos = 0;
  HIPCHK(hipMemcpyAsync(&pos, c->d_tn_pos + lane, 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  *n = pos;
  const u64 k = std::min<u64>(std::min<u64>(pos, c->tn_cap), cap);
  if (k) HIPCHK(hipMemcpyAsync(buf, c->d_tn_buf + (u64)lane * c->tn_cap, k, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_set_edges(wtfgpu_ctx *c, int on) {
  if (!c) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  c->P.edges = on ? 1 : 0;
  if (on && !c->d_edgecnt && c->P.nlanes) {
    if (dalloc(&c->d_edgecnt, 2ull * c->P.nlanes)) return WTFGPU_ERR_OOM;
    HIPCHK(hipMemset(c->d_edgecnt, 0, 8ull * c->P.nlanes));
  }
  c->P.edge_cnt = on ? c->d_edgecnt : nullptr;
  return guc_clear(c);  // cached entries were digested for the other setting
}

int wtfgpu_coverage_absorb(wtfgpu_ctx *c, uint64_t *rips, uint64_t cap, uint64_t *n) {
  if (!c || !n || (cap && !rips)) return WTFGPU_ERR_INVALID;
  *n = 0;
  if (!c->d_covmap || !c->ncovslots) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const u64 bytes = c->ncovslots * WTFGPU_PAGE_SIZE, n16 = bytes / 16;
  if (ensure_scratch(c, 256 + cap * 8)) return WTFGPU_ERR_OOM;
  unsigned long long *d_count = (unsigned long long *)c->q->d_scratch;
  u64 *d_idx = (u64 *)(c->q->d_scratch + 256);
  HIPCHK(hipMemsetAsync(d_count, 0, 8, c->q->stream));
  k_cov_absorb<<<(u32)((n16 + 255) / 256), 256, 0, c->q->stream>>>(c->d_covmap, c->d_covshadow, n16, d_idx, cap,
                                                                   d_count, cap ? 1 : 0);
  HIPCHK(hipGetLastError());
  u64 total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_count, 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  const u64 m = std::min(total, cap);
  if (m) {
    std::vector<u64> idx(m);
    HIPCHK(hipMemcpyAsync(idx.data(), d_idx, m * 8, hipMemcpyDeviceToHost, c->q->stream));
    HIPCHK(hipStreamSynchronize(c->q->stream));
    std::sort(idx.begin(), idx.end());
    for (u64 i = 0; i < m; i++) rips[i] = (c->code_vpns[idx[i] / WTFGPU_PAGE_SIZE] << 12) | (idx[i] % WTFGPU_PAGE_SIZE);
  }
  *n = total;
  return WTFGPU_OK;
}

int wtfgpu_coverage_merge_in(wtfgpu_ctx *c, const void *dev_src, uint64_t bytes) {
  if (!c || (bytes && !dev_src)) return WTFGPU_ERR_INVALID;
  if (!c->d_covmap || !c->ncovslots) return bytes ? WTFGPU_ERR_INVALID : WTFGPU_OK;
  const u64 mb = c->ncovslots * WTFGPU_PAGE_SIZE, n16 = mb / 16;
  if (bytes != mb) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  k_cov_merge_in<<<(u32)((n16 + 255) / 256), 256, 0, c->q->stream>>>((uint4 *)c->d_covmap, (const uint4 *)dev_src, n16);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_coverage_device_map(wtfgpu_ctx *c, void **dev_ptr, uint64_t *bytes) {
  if (!c || !dev_ptr || !bytes) return WTFGPU_ERR_INVALID;
  *dev_ptr = c->d_covmap;
  *bytes = c->ncovslots * WTFGPU_PAGE_SIZE;
  return WTFGPU_OK;
}

int wtfgpu_coverage_rips(wtfgpu_ctx *c, uint64_t *rips, uint64_t cap, uint64_t *n) {
  if (!c || !n) return WTFGPU_ERR_INVALID;
  *n = 0;
  if (!c->d_covmap) return WTFGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<u8> m(c->ncovslots * WTFGPU_PAGE_SIZE);
  HIPCHK(hipMemcpyAsync(m.data(), c->d_covmap, m.size(), hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  u64 k = 0;
  for (u64 s = 0; s < c->ncovslots; s++)
    for (u64 o = 0; o < WTFGPU_PAGE_SIZE; o++)
      if (m[s * WTFGPU_PAGE_SIZE + o]) {
        if (k < cap && rips) rips[k] = (c->code_vpns[s] << 12) | o;
        k++;
      }
  *n = k;
  return WTFGPU_OK;
}

int wtfgpu_read_bytes(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint64_t *out) {
  if (!lanes_ok(c, first, count) || !out) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, c->d_nbytes + first, (u64)count * 8, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_edge_counts(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint32_t *out2) {
  if (!lanes_ok(c, first, count) || !out2) return WTFGPU_ERR_INVALID;
  if (!c->d_edgecnt) {
    memset(out2, 0, 8ull * count);
    return WTFGPU_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out2, c->d_edgecnt + 2ull * first, 8ull * count, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

int wtfgpu_read_dirty_counts(wtfgpu_ctx *c, uint32_t first, uint32_t count, uint32_t *out) {
  if (!lanes_ok(c, first, count) || !out) return WTFGPU_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, c->d_ovcount + first, (u64)count * 4, hipMemcpyDeviceToHost, c->q->stream));
  HIPCHK(hipStreamSynchronize(c->q->stream));
  return WTFGPU_OK;
}

}  // extern "C"
