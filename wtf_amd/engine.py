"""Python handle on the HIP engine (libwtfgpu.so) through its C ABI.

Used by tests and bench.py to drive lanes directly; the C++ GpuBackend_t
(wtf_amd/host) is the drop-in for wtf's Backend_t. Every call goes to the HIP
library; a missing library or device raises instead of falling back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class EngineError(RuntimeError):
    pass


class DeviceCorpusFull(EngineError):
    pass


def _chk(rc, what):
    if rc != 0:
        raise EngineError(f"{what} failed: {rc}")


class Engine:
    def __init__(self, device: int = 0):
        self.L = abi.load_hip_library()
        ctx = C.c_void_p()
        _chk(self.L.wtfgpu_create(device, C.byref(ctx)), "wtfgpu_create")
        self.ctx = ctx
        self.nlanes = 0

    def close(self):
        if self.ctx:
            self.L.wtfgpu_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup
    def load_pool(self, pfns, blob: bytes):
        arr = (C.c_uint64 * max(1, len(pfns)))(*pfns)
        _chk(self.L.wtfgpu_load_pool(self.ctx, arr, blob, len(pfns)), "load_pool")

    def alloc_lanes(self, n, overlay_pages=16, cov_entries=1024):
        _chk(self.L.wtfgpu_alloc_lanes(self.ctx, n, overlay_pages, cov_entries), "alloc_lanes")
        self.nlanes = n

    def alloc_spill(self, pool_pages, lane_max):
        """A device-wide pool of pool_pages copy-on-write pages for lanes whose
        overlay_pages private ones are full, lane_max of them per lane at most
        (wtfgpu_alloc_spill; after alloc_lanes)."""
        _chk(self.L.wtfgpu_alloc_spill(self.ctx, pool_pages, lane_max), "alloc_spill")

    def spill_stats(self) -> dict:
        """The pool's counters: pool_pages, lane_max, in_use, peak,
        lanes_spilled, pool_empty, claims (all zero without a pool)."""
        st = abi.SpillStats()
        _chk(self.L.wtfgpu_spill_stats(self.ctx, C.byref(st)), "spill_stats")
        return {k: getattr(st, k) for k, _ in abi.SpillStats._fields_}

    def dirty_capacity(self) -> int:
        """Dirty pages a lane can hold: overlay_pages + the spill cap."""
        return self.L.wtfgpu_dirty_capacity(self.ctx)

    def restore_lanes(self, lanes):
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        _chk(self.L.wtfgpu_restore_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la)),
             "restore_lanes")

    def set_initial_state(self, regs: abi.Regs):
        _chk(self.L.wtfgpu_set_initial_state(self.ctx, C.byref(regs)), "set_initial_state")

    def set_limit(self, n):
        _chk(self.L.wtfgpu_set_limit(self.ctx, n), "set_limit")

    def set_breakpoints(self, gvas):
        arr = (C.c_uint64 * max(1, len(gvas)))(*gvas)
        _chk(self.L.wtfgpu_set_breakpoints(self.ctx, arr, len(gvas)), "set_breakpoints")

    def set_edges(self, on: bool):
        _chk(self.L.wtfgpu_set_edges(self.ctx, 1 if on else 0), "set_edges")

    def set_code_pages(self, vpns):
        arr = (C.c_uint64 * max(1, len(vpns)))(*vpns)
        _chk(self.L.wtfgpu_set_code_pages(self.ctx, arr, len(vpns)), "set_code_pages")

    def restore(self, first=0, count=None):
        count = self.nlanes - first if count is None else count
        _chk(self.L.wtfgpu_restore(self.ctx, first, count), "restore")

    # ---- feeds, the declared insert, the device corpus and mutator
    def set_insert(self, head_reg, ptr_reg, len_reg, len_arg=0):
        ins = abi.Insert(head_reg, ptr_reg, len_reg, len_arg)
        _chk(self.L.wtfgpu_set_insert(self.ctx, C.byref(ins)), "set_insert")

    def set_feed_lanes(self, lanes, testcases):
        """One chunk per lane (a u32 size, then the bytes), as the streaming
        refill uploads them. The bytes are kept until the next call."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        chunks = [len(t).to_bytes(4, "little") + bytes(t) for t in testcases]
        off = np.zeros(len(la) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in chunks])
        self._feed_keep = b"".join(chunks)
        _chk(self.L.wtfgpu_set_feed_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la),
                                          off.ctypes.data_as(C.POINTER(C.c_uint64)), None, self._feed_keep,
                                          len(self._feed_keep)), "set_feed_lanes")

    def corpus_alloc(self, max_entries, max_bytes):
        _chk(self.L.wtfgpu_corpus_alloc(self.ctx, max_entries, max_bytes), "corpus_alloc")

    def corpus_add(self, data: bytes) -> int:
        """Index of the new entry; raises DeviceCorpusFull when it does not fit."""
        idx = C.c_uint32()
        rc = self.L.wtfgpu_corpus_add(self.ctx, bytes(data), len(data), C.byref(idx))
        if rc == abi.ERR_FULL:
            raise DeviceCorpusFull(f"corpus_add: no room for {len(data)} bytes")
        _chk(rc, "corpus_add")
        return idx.value

    def mutate_feed_lanes_rc(self, lanes, seed, indices, ncorpus, max_len) -> int:
        """wtfgpu_mutate_feed_lanes' return code (asynchronous on the queue)."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint64)
        nc = np.ascontiguousarray(ncorpus, dtype=np.uint32)
        assert len(ix) == len(la) and len(nc) == len(la)
        return self.L.wtfgpu_mutate_feed_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la), seed,
                                               ix.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               nc.ctypes.data_as(C.POINTER(C.c_uint32)), max_len)

    def mutate_feed_lanes(self, lanes, seed, indices, ncorpus, max_len):
        _chk(self.mutate_feed_lanes_rc(lanes, seed, indices, ncorpus, max_len), "mutate_feed_lanes")

    def read_feed_lanes(self, lanes, stride=abi.FEED_STRIDE - 4):
        """Each listed lane's testcase (None: the lane has no feed)."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        lens = np.zeros(len(la), dtype=np.uint32)
        out = np.zeros((len(la), stride), dtype=np.uint8)
        _chk(self.L.wtfgpu_read_feed_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la),
                                           lens.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.c_void_p),
                                           stride), "read_feed_lanes")
        return [None if n == 0xffffffff else out[i, :min(int(n), stride)].tobytes() for i, n in enumerate(lens)]

    # ---- the device packet mutator (csrc/engine_mutate_packets.h)
    def corpus_add_feed_rc(self, feed: bytes):
        """(return code, index) of wtfgpu_corpus_add_feed."""
        idx = C.c_uint32(0xffffffff)
        rc = self.L.wtfgpu_corpus_add_feed(self.ctx, bytes(feed), len(feed), C.byref(idx))
        return rc, idx.value

    def corpus_add_feed(self, feed: bytes) -> int:
        """Index of the new entry; raises DeviceCorpusFull when it does not fit."""
        rc, idx = self.corpus_add_feed_rc(feed)
        if rc == abi.ERR_FULL:
            raise DeviceCorpusFull(f"corpus_add_feed: no room for {len(feed)} bytes")
        _chk(rc, "corpus_add_feed")
        return idx

    def mutate_packets_lanes_rc(self, lanes, seed, indices, ncorpus, params) -> int:
        """wtfgpu_mutate_packets_lanes' return code (asynchronous on the queue);
        params: the five wtfgpu_packet_params_t values, in order."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint64)
        nc = np.ascontiguousarray(ncorpus, dtype=np.uint32)
        assert len(ix) == len(la) and len(nc) == len(la)
        pp = abi.PacketParams(*params)
        return self.L.wtfgpu_mutate_packets_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la), seed,
                                                  ix.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  nc.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pp))

    def mutate_packets_lanes(self, lanes, seed, indices, ncorpus, params):
        _chk(self.mutate_packets_lanes_rc(lanes, seed, indices, ncorpus, params), "mutate_packets_lanes")

    # ---- the minimiser's candidates (csrc/engine_minimize.h)
    def minimize_feed_lanes_rc(self, lanes, entry, op, indices) -> int:
        """wtfgpu_minimize_feed_lanes' return code (asynchronous on the queue);
        op: abi.MIN_REMOVE or abi.MIN_ZERO. lanes / indices None: a null pointer."""
        la = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.uint32)
        ix = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint64)
        n = len(la) if la is not None else len(ix)
        assert la is None or ix is None or len(ix) == len(la)
        return self.L.wtfgpu_minimize_feed_lanes(self.ctx,
                                                 None if la is None else la.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                                 entry, op,
                                                 None if ix is None else ix.ctypes.data_as(C.POINTER(C.c_uint64)))

    def minimize_feed_lanes(self, lanes, entry, op, indices):
        _chk(self.minimize_feed_lanes_rc(lanes, entry, op, indices), "minimize_feed_lanes")

    # ---- the corpus distiller (csrc/engine_distill.h)
    def distill_rc(self, n, offsets, values, eligible, want_out=True, want_counts=True):
        """wtfgpu_distill's return code and outputs: (rc, index, gain, universe).
        offsets / values / eligible None: a null pointer; want_out / want_counts
        False: null output pointers."""
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        val = None if values is None else np.ascontiguousarray(values, dtype=np.uint64)
        el = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
        oi, og = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        kept, uni = C.c_uint32(0), C.c_uint64(0)
        p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        rc = self.L.wtfgpu_distill(self.ctx, n,
                                   None if off is None else off.ctypes.data_as(p64),
                                   None if val is None else val.ctypes.data_as(p64),
                                   None if el is None else el.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   oi.ctypes.data_as(p32) if want_out else None,
                                   og.ctypes.data_as(p32) if want_out else None,
                                   C.byref(kept) if want_counts else None, C.byref(uni) if want_counts else None)
        k = kept.value
        return rc, oi[:k].tolist(), og[:k].tolist(), uni.value

    def distill(self, sets, eligible=None):
        """The greedy cover of `sets` (each a strictly ascending sequence of
        64-bit values, in rank order): (taken indices in the order taken, their
        gains, the number of distinct values over the eligible sets)."""
        sets = [np.ascontiguousarray(s, dtype=np.uint64) for s in sets]
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        if sets:
            off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
        val = np.concatenate(sets) if sets else np.zeros(0, dtype=np.uint64)
        if len(val) == 0:
            val = np.zeros(1, dtype=np.uint64)
        rc, index, gain, universe = self.distill_rc(len(sets), off, val, eligible)
        _chk(rc, "distill")
        return index, gain, universe

    # ---- the analyzer's candidates and set signatures (csrc/engine_analyze.h)
    def analyze_feed_lanes_rc(self, lanes, entry, indices) -> int:
        """wtfgpu_analyze_feed_lanes' return code (asynchronous on the queue).
        lanes / indices None: a null pointer."""
        la = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.uint32)
        ix = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint64)
        n = len(la) if la is not None else len(ix)
        assert la is None or ix is None or len(ix) == len(la)
        return self.L.wtfgpu_analyze_feed_lanes(self.ctx,
                                                None if la is None else la.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                                entry,
                                                None if ix is None else ix.ctypes.data_as(C.POINTER(C.c_uint64)))

    def analyze_feed_lanes(self, lanes, entry, indices):
        _chk(self.analyze_feed_lanes_rc(lanes, entry, indices), "analyze_feed_lanes")

    def coverage_signature_rc(self, lanes, want_out=True):
        """wtfgpu_coverage_signature's return code and outputs: (rc, sig, size,
        overflow), one entry a listed lane. lanes None: a null pointer (with
        n = 1); want_out False: null output pointers."""
        la = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.uint32)
        n = 1 if la is None else len(la)
        sig = np.zeros(max(n, 1), dtype=np.uint64)
        out = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2)]
        p32 = C.POINTER(C.c_uint32)
        ptrs = [sig.ctypes.data_as(C.POINTER(C.c_uint64)) if want_out else None]
        ptrs += [o.ctypes.data_as(p32) if want_out else None for o in out]
        rc = self.L.wtfgpu_coverage_signature(self.ctx, None if la is None else la.ctypes.data_as(p32), n, *ptrs)
        return (rc, sig[:n], out[0][:n], out[1][:n])

    def coverage_signature(self, lanes):
        """For each listed lane: its coverage set's signature (u64), the set's
        entries and whether it overflowed (u32 arrays). The sets are not
        emptied."""
        rc, sig, size, overflow = self.coverage_signature_rc(lanes)
        _chk(rc, "coverage_signature")
        return sig, size, overflow

    # ---- keeping coverage (csrc/engine_covkeep.h)
    def coverage_target_rc(self, values) -> int:
        """wtfgpu_coverage_target's return code. values None: a null pointer
        (with n = 1); an empty sequence is the empty target."""
        if values is None:
            return self.L.wtfgpu_coverage_target(self.ctx, None, 1)
        v = np.ascontiguousarray(values, dtype=np.uint64)
        return self.L.wtfgpu_coverage_target(self.ctx, v.ctypes.data_as(C.POINTER(C.c_uint64)), len(v))

    def coverage_target(self, values):
        """The target set the following coverage_contains calls check against."""
        _chk(self.coverage_target_rc(values), "coverage_target")

    def coverage_contains_rc(self, lanes, want_out=True):
        """wtfgpu_coverage_contains' return code and outputs: (rc, missing,
        size, overflow), one entry a listed lane. lanes None: a null pointer
        (with n = 1); want_out False: null output pointers."""
        la = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.uint32)
        n = 1 if la is None else len(la)
        out = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3)]
        p32 = C.POINTER(C.c_uint32)
        ptrs = [o.ctypes.data_as(p32) if want_out else None for o in out]
        rc = self.L.wtfgpu_coverage_contains(self.ctx, None if la is None else la.ctypes.data_as(p32), n, *ptrs)
        return (rc, *[o[:n] for o in out])

    def coverage_contains(self, lanes):
        """For each listed lane: how many of the target's values its coverage
        set lacks, the set's entries, and whether it overflowed (u32 arrays).
        The sets are not emptied."""
        rc, missing, size, overflow = self.coverage_contains_rc(lanes)
        _chk(rc, "coverage_contains")
        return missing, size, overflow

    def clear_coverage_lanes(self, lanes):
        """Empties the listed lanes' coverage sets (queued on the current queue)."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        _chk(self.L.wtfgpu_clear_coverage_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la)),
             "clear_coverage_lanes")

    def read_whole_feed_lanes(self, lanes, stride=abi.FEED_STRIDE):
        """Each listed lane's whole feed (None: the lane has no feed)."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        lens = np.zeros(len(la), dtype=np.uint32)
        out = np.zeros((len(la), stride), dtype=np.uint8)
        _chk(self.L.wtfgpu_read_whole_feed_lanes(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la),
                                                 lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 out.ctypes.data_as(C.c_void_p), stride), "read_whole_feed_lanes")
        return [None if n == 0xffffffff else out[i, :min(int(n), stride)].tobytes() for i, n in enumerate(lens)]

    def read_feeds_packed_raw(self, lanes, whole=True, null_lens=False):
        """wtfgpu_read_feeds_packed as it answers: (rc, lens, offs, a copy of the
        pinned buffer's first `total` bytes, total, the buffer's address).
        `whole` goes through as an integer; null_lens: a null `lens`."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        n = len(la)
        lens = np.zeros(n, dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        ptr, total = C.c_void_p(), C.c_uint64()
        rc = self.L.wtfgpu_read_feeds_packed(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), n, int(whole),
                                             None if null_lens else lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ptr), C.byref(total))
        buf = C.string_at(ptr.value, total.value) if rc == 0 and total.value else b""
        return rc, lens, offs, buf, total.value, ptr.value

    def read_feeds_packed(self, lanes, whole=True):
        """Each listed lane's whole feed (whole=False: its first chunk without the
        size), read back packed; None: the lane has no feed."""
        rc, lens, offs, buf, _, _ = self.read_feeds_packed_raw(lanes, whole)
        _chk(rc, "read_feeds_packed")
        return [None if n == 0xffffffff else buf[int(o):int(o) + int(n)] for n, o in zip(lens, offs)]

    # ---- registers
    def read_gprs(self, first=0, count=None) -> np.ndarray:
        count = self.nlanes - first if count is None else count
        out = np.zeros((count, 18), dtype=np.uint64)
        _chk(self.L.wtfgpu_read_gprs(self.ctx, first, count, out.ctypes.data_as(C.POINTER(C.c_uint64))),
             "read_gprs")
        return out

    def write_gprs(self, g: np.ndarray, first=0):
        g = np.ascontiguousarray(g, dtype=np.uint64)
        _chk(self.L.wtfgpu_write_gprs(self.ctx, first, g.shape[0], g.ctypes.data_as(C.POINTER(C.c_uint64))),
             "write_gprs")

    def read_regs(self, first=0, count=1):
        arr = (abi.Regs * count)()
        _chk(self.L.wtfgpu_read_regs(self.ctx, first, count, arr), "read_regs")
        return list(arr)

    def write_regs(self, regs, first=0):
        arr = (abi.Regs * len(regs))(*regs)
        _chk(self.L.wtfgpu_write_regs(self.ctx, first, len(regs), arr), "write_regs")

    # ---- run
    def run(self, first=0, count=None, max_steps=1 << 40) -> abi.RunStats:
        count = self.nlanes - first if count is None else count
        st = abi.RunStats()
        _chk(self.L.wtfgpu_run(self.ctx, first, count, max_steps, C.byref(st)), "run")
        return st

    def set_regroup(self, steps):
        """Wave-steps per launch between regrouping sorts (0: fixed lane order)."""
        _chk(self.L.wtfgpu_set_regroup(self.ctx, steps), "set_regroup")

    def run_async(self, first=0, count=None, max_steps=1 << 32):
        """Queues a run of at most max_steps wave-steps; run_wait() collects it."""
        count = self.nlanes - first if count is None else count
        _chk(self.L.wtfgpu_run_async(self.ctx, first, count, max_steps), "run_async")

    def run_wait(self) -> abi.RunStats:
        st = abi.RunStats()
        _chk(self.L.wtfgpu_run_wait(self.ctx, C.byref(st)), "run_wait")
        return st

    def select_queue(self, queue: int):
        """Every later call is issued on queue 0 or 1 (wtfgpu_select_queue)."""
        _chk(self.L.wtfgpu_select_queue(self.ctx, queue), "select_queue")

    def exits(self, first=0, count=None):
        count = self.nlanes - first if count is None else count
        arr = (abi.Exit * count)()
        _chk(self.L.wtfgpu_read_exits(self.ctx, first, count, arr), "read_exits")
        return list(arr)

    EXIT_DTYPE = np.dtype([("status", "<u4"), ("vector", "<u4"), ("error", "<u4"), ("opcode", "<u4"),
                           ("addr", "<u8"), ("rip", "<u8"), ("icount", "<u8")])

    def exits_np(self, first=0, count=None) -> np.ndarray:
        """read_exits as a numpy structured array (one record per lane)."""
        count = self.nlanes - first if count is None else count
        out = np.zeros(count, dtype=self.EXIT_DTYPE)
        assert out.itemsize == C.sizeof(abi.Exit)
        _chk(self.L.wtfgpu_read_exits(self.ctx, first, count, out.ctypes.data_as(C.POINTER(abi.Exit))),
             "read_exits")
        return out

    def resume(self, lanes, skip):
        n = len(lanes)
        la = (C.c_uint32 * max(1, n))(*lanes)
        sk = (C.c_uint8 * max(1, n))(*[1 if s else 0 for s in skip])
        _chk(self.L.wtfgpu_resume(self.ctx, la, n, sk), "resume")

    def inject_fault(self, lanes, vector, error, addrs) -> list[bool]:
        n = len(lanes)
        la = (C.c_uint32 * max(1, n))(*lanes)
        aa = (C.c_uint64 * max(1, n))(*addrs)
        ok = (C.c_int32 * max(1, n))()
        _chk(self.L.wtfgpu_inject_fault(self.ctx, la, n, vector, error, aa, ok), "inject_fault")
        return [bool(ok[i]) for i in range(n)]

    def stop(self, lanes, status=abi.EXIT_STOPPED):
        n = len(lanes)
        la = (C.c_uint32 * max(1, n))(*lanes)
        _chk(self.L.wtfgpu_stop(self.ctx, la, n, status), "stop")

    # ---- memory
    def apply_writes(self, writes, phys=False, check=True):
        """writes: list of (lane, gva, bytes); phys: the addresses are guest
        physical (wtfgpu_apply_phys_writes). Returns each write's status;
        check=False returns them also when a write failed instead of raising."""
        if not writes:
            return []
        recs = (abi.Write * len(writes))()
        blob = bytearray()
        for i, (lane, gva, data) in enumerate(writes):
            recs[i].lane, recs[i].len, recs[i].gva, recs[i].data_off = lane, len(data), gva, len(blob)
            blob += data
        st = (C.c_int32 * len(writes))()
        fn = self.L.wtfgpu_apply_phys_writes if phys else self.L.wtfgpu_apply_writes
        rc = fn(self.ctx, recs, len(writes), bytes(blob), len(blob), st)
        if check:
            _chk(rc, "apply_writes")
        return list(st)

    def dirty_list(self, lanes) -> np.ndarray:
        """[n, dirty_capacity + 1] u32: each lane's dirty count, then its gpfns."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        out = np.zeros((len(la), self.dirty_capacity() + 1), dtype=np.uint32)
        _chk(self.L.wtfgpu_read_dirty_list(self.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la),
                                           out.ctypes.data_as(C.POINTER(C.c_uint32))), "read_dirty_list")
        return out

    def read_virt(self, lane, gva, n) -> bytes:
        b = C.create_string_buffer(n)
        _chk(self.L.wtfgpu_lane_read_virt(self.ctx, lane, gva, b, n), "read_virt")
        return b.raw

    def write_virt(self, lane, gva, data: bytes):
        _chk(self.L.wtfgpu_lane_write_virt(self.ctx, lane, gva, data, len(data)), "write_virt")

    def read_phys(self, lane, gpa, n) -> bytes:
        b = C.create_string_buffer(n)
        _chk(self.L.wtfgpu_lane_read_phys(self.ctx, lane, gpa, b, n), "read_phys")
        return b.raw

    def translate(self, lane, gva):
        out = C.c_uint64()
        rc = self.L.wtfgpu_lane_translate(self.ctx, lane, gva, C.byref(out))
        return None if rc else out.value

    def dirty(self, lane) -> list[int]:
        n = C.c_uint32()
        cap = 4096
        arr = (C.c_uint64 * cap)()
        _chk(self.L.wtfgpu_read_dirty(self.ctx, lane, arr, cap, C.byref(n)), "read_dirty")
        return list(arr[: min(n.value, cap)])

    def coverage(self, first=0, count=None, cap=None):
        """{lane: set(rips)} of rips absent from the coverage map when executed
        (a first call sizes the buffers: after warm-up the log is usually empty)."""
        count = self.nlanes - first if count is None else count
        n = C.c_uint64()
        ovf = C.c_uint32()
        dummy_l, dummy_r = (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
        _chk(self.L.wtfgpu_read_coverage(self.ctx, first, count, dummy_l, dummy_r, 0, C.byref(n), C.byref(ovf)),
             "read_coverage")
        out: dict[int, set] = {}
        total = n.value
        if total:
            lanes = np.zeros(total, dtype=np.uint32)
            rips = np.zeros(total, dtype=np.uint64)
            _chk(self.L.wtfgpu_read_coverage(self.ctx, first, count, lanes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             rips.ctypes.data_as(C.POINTER(C.c_uint64)), total, C.byref(n),
                                             C.byref(ovf)), "read_coverage")
            for ln, rp in zip(lanes.tolist(), rips.tolist()):
                out.setdefault(ln, set()).add(rp)
        return out, bool(ovf.value)

    def commit_coverage(self, rips):
        arr = np.ascontiguousarray(np.array(sorted(rips), dtype=np.uint64))
        _chk(self.L.wtfgpu_commit_coverage(self.ctx, arr.ctypes.data_as(C.POINTER(C.c_uint64)), len(arr)),
             "commit_coverage")

    def attribute_coverage(self, lanes, revoke=None, full=False):
        """New coverage of `lanes` attributed in the given order on the device
        (wtfgpu_attribute_coverage): (pos u32[], vals u64[], entries, overflow),
        sorted by (position in lanes, value). A first call with cap=0 sizes the
        buffers; the call that has room empties the lanes' sets."""
        la = np.ascontiguousarray(lanes, dtype=np.uint32)
        n = len(la)
        rv = None if revoke is None else np.ascontiguousarray(np.asarray(revoke) != 0, dtype=np.uint8)
        assert rv is None or len(rv) == n
        flags = abi.ATTRIB_ALL if full else 0
        total, entries, ovf = C.c_uint64(), C.c_uint64(), C.c_uint32()
        lp = la.ctypes.data_as(C.POINTER(C.c_uint32))
        rp = None if rv is None else rv.ctypes.data_as(C.POINTER(C.c_uint8))

        def call(pos, vals, room):
            _chk(self.L.wtfgpu_attribute_coverage(
                self.ctx, lp, rp, n, flags, None if pos is None else pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                None if vals is None else vals.ctypes.data_as(C.POINTER(C.c_uint64)), room, C.byref(total),
                C.byref(entries), C.byref(ovf)), "attribute_coverage")

        call(None, None, 0)
        room = total.value
        pos = np.zeros(room, dtype=np.uint32)
        vals = np.zeros(room, dtype=np.uint64)
        if room:
            call(pos, vals, room)
        return pos[: total.value], vals[: total.value], entries.value, bool(ovf.value)

    def nbytes(self, first=0, count=None) -> np.ndarray:
        count = self.nlanes - first if count is None else count
        out = np.zeros(count, dtype=np.uint64)
        _chk(self.L.wtfgpu_read_bytes(self.ctx, first, count, out.ctypes.data_as(C.POINTER(C.c_uint64))),
             "read_bytes")
        return out

    def dirty_counts(self, first=0, count=None) -> np.ndarray:
        count = self.nlanes - first if count is None else count
        out = np.zeros(count, dtype=np.uint32)
        _chk(self.L.wtfgpu_read_dirty_counts(self.ctx, first, count, out.ctypes.data_as(C.POINTER(C.c_uint32))),
             "read_dirty_counts")
        return out

    def gather_pages(self, lanes, gpas) -> np.ndarray:
        """[n, 4096] u8: each lane's current view of each guest-physical page."""
        lanes = np.ascontiguousarray(lanes, dtype=np.uint32)
        gpas = np.ascontiguousarray(gpas, dtype=np.uint64)
        out = np.zeros((len(lanes), 4096), dtype=np.uint8)
        _chk(self.L.wtfgpu_gather_pages(self.ctx, lanes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        gpas.ctypes.data_as(C.POINTER(C.c_uint64)), len(lanes),
                                        out.ctypes.data_as(C.c_void_p)), "gather_pages")
        return out

    def get_cr(self, lane, cr) -> int:
        out = C.c_uint64()
        _chk(self.L.wtfgpu_lane_get_cr(self.ctx, lane, cr, C.byref(out)), "lane_get_cr")
        return out.value

    def set_cr(self, lane, cr, value):
        _chk(self.L.wtfgpu_lane_set_cr(self.ctx, lane, cr, value), "lane_set_cr")
