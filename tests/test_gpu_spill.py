"""The spill pool on the GPU: lanes whose K private copy-on-write pages are
full take further pages from a shared pool (wtfgpu_alloc_spill), and nothing a
guest or a read-back call sees depends on where a page lives.

Shapes are tiny on purpose: K = 2 private pages, X = 6 pool pages per lane.
The guest loop of tests/spill_lib.py dirties M pages; the oracle, which has no
page limit, is the reference, and hand-written values are where the engine
stops and the oracle does not (a full overlay, host writes, a Feed)."""
import ctypes as C
import functools
import os
import shutil
import statistics
import struct

import numpy as np
import pytest

from wtf_amd import abi
from wtf_amd.abi import regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, seg, user_state

from tests import spill_lib as S
from tests import sysprog2 as S2
from tests import tlv_harness as H
from tests.oracle_lib import Oracle

pytestmark = pytest.mark.gpu

K, X, CAP = S.K, S.X, S.K + S.X
EXIT_HLT, EXIT_STOP_OK, ERR_OOM = 4, 11, -3
# M lane by lane: 15 values, so the pattern shifts from wave to wave; lanes
# that never spill (M <= K), lanes that spill, lanes at the cap (K + X) and
# lanes past it (K + X + 1) sit side by side in every wave
MCYCLE = (0, 1, 2, 3, 5, 8, 9, 4, 8, 2, 9, 6, 1, 7, 3)
MASK64 = 2**64 - 1


def _seed(lane, rnd=0):
    return ((rnd << 40) | (lane << 12) | 0x5A1) * 0x9E3779B97F4A7C15 & MASK64


def _engine(sp, regs, lanes, pool, k=K, x=X):
    from wtf_amd.engine import Engine
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(lanes, overlay_pages=k, cov_entries=64)
    if pool:
        eng.alloc_spill(pool, x)
    eng.set_initial_state(regs)
    eng.set_limit(0)
    return eng


def _state(eng, first, count):
    """Every lane's result as spill_lib.want() gives the oracle's: status,
    rip, GPRs, rflags, retired count, dirty set and every dirty page's bytes."""
    g = eng.read_gprs(first, count)
    ex = eng.exits_np(first, count)
    dl = eng.dirty_list(np.arange(first, first + count))
    assert dl.shape[1] == eng.dirty_capacity() + 1
    pl, pg = [], []
    for i in range(count):
        for gp in dl[i, 1:1 + dl[i, 0]]:
            pl.append(first + i)
            pg.append(int(gp) << 12)
    data = eng.gather_pages(pl, pg) if pl else np.zeros((0, 4096), dtype=np.uint8)
    out, at = [], 0
    for i in range(count):
        n = int(dl[i, 0])
        out.append({"status": int(ex["status"][i]), "rip": int(ex["rip"][i]),
                    "gpr": tuple(int(v) for v in g[i, :16]), "rflags": int(g[i, 17]),
                    "icount": int(ex["icount"][i]), "dirty": tuple(sorted(pg[at:at + n])),
                    "pages": {pg[at + j]: data[at + j].tobytes() for j in range(n)}})
        at += n
    return out


def _diff(got, want):
    return [k for k in want if got[k] != want[k]]


def _check(got, m, seed, held=None):
    """One lane of the loop over m pages. held: the dirty pages it ended with
    when that is fewer than the loop wanted (the cap, or an empty pool)."""
    if held is None:
        held = min(m, CAP)
    if held == m:
        return _diff(got, S.want(m, seed))
    w = S.want_full(held, seed, m)
    bad = _diff(got, {k: w[k] for k in ("status", "rip", "icount", "dirty", "pages")})
    if got["gpr"][2] != w["rdx"] or got["gpr"][8] != w["r8"]:
        bad.append("gpr")
    return bad


def _start_loop(eng, first, ms, seeds):
    g = eng.read_gprs(first, len(ms))
    g[:, 7], g[:, 1], g[:, 6] = S.BASE, ms, np.array(seeds, dtype=np.uint64)
    eng.write_gprs(g, first)


# ---------------------------------------------------------------- 1: a mixed wave
def test_mixed_wave_matches_the_oracle():
    """416 lanes: one full 256-thread block, then two full waves and a partial
    one. On an engine without the pool every lane with M > K ends as
    EXIT_OVERLAY_FULL."""
    n = 416
    sp, r0, _ = S.space()
    ms = [MCYCLE[l % len(MCYCLE)] for l in range(n)]
    seeds = [_seed(l) for l in range(n)]
    demand = sum(min(m, CAP) - K for m in ms if m > K)
    eng = _engine(sp, r0, n, pool=demand + 37)  # (not a multiple of 32: the bitmap's last word is partial)
    try:
        assert eng.dirty_capacity() == CAP and eng.L.wtfgpu_overlay_pages(eng.ctx) == K
        eng.restore()
        _start_loop(eng, 0, ms, seeds)
        eng.run()
        got = _state(eng, 0, n)
        bad = [(l, ms[l], d) for l in range(n) if (d := _check(got[l], ms[l], seeds[l]))]
        assert not bad, f"{len(bad)}/{n} lanes differ, first: {bad[:5]}"
        assert {g["status"] for g in got} == {S.EXIT_INT3, S.EXIT_OVERLAY_FULL}
        # single-lane reads see spilled pages too
        deep = ms.index(CAP)
        assert sorted(eng.dirty(deep)) == list(got[deep]["dirty"])
        va = S.BASE + 0x1000 * (CAP - 1)
        assert eng.read_virt(deep, va, 8) == ((seeds[deep] + va) & MASK64).to_bytes(8, "little")
        assert list(eng.dirty_counts()) == [min(m, CAP) for m in ms]
        st = eng.spill_stats()
        assert st["pool_pages"] == demand + 37 and st["lane_max"] == X
        assert st["peak"] >= demand and st["in_use"] == demand and st["claims"] == demand
        assert st["lanes_spilled"] == sum(m > K for m in ms) and st["pool_empty"] == 0
        eng.restore()
        assert eng.spill_stats()["in_use"] == 0 and not eng.dirty_counts().any()
    finally:
        eng.close()


# ---------------------------------------------------------------- 2: every allocation site at a lane holding K pages
KCODE, KSTACK, KDATA, PTWIN = 0xFFFFF80000600000, 0xFFFFF80000300000, 0xFFFFF80000800000, 0xFFFFF80000A00000
KSP = KSTACK + 0x1800
_TWO = b"\x48\x89\x37" + b"\x48\x89\xb7\x00\x10\x00\x00"  # mov [rdi], rsi; mov [rdi + 0x1000], rsi: K pages held
KPROGS = {
    # a store across a page boundary into two untouched pages (service_miss, twice for one instruction)
    "cross": _TWO + b"\x49\x89\x31" + b"\xf4",             # mov [r9], rsi; hlt
    # int 0x80: the frame lands on an untouched stack page (soft_int: sup_write_pa)
    "int": _TWO + b"\xcd\x80" + b"\xf4",
    # #UD delivered through the IDT, the same stack page (deliver_fault: lane_phys_write64)
    "ud": _TWO + b"\x0f\x0b" + b"\xf4",
    # a write to a page-table page, which is copied into the pool, then a load
    # and a store through the changed mapping: the walk reads the pool's copy
    "pt": _TWO + b"\x48\x8b\x03" + b"\x48\x8b\x53\x08" + b"\x48\x89\x13"  # mov rax,[rbx]; mov rdx,[rbx+8]; mov [rbx],rdx
          + b"\x49\x8b\x09" + b"\x49\x89\x71\x08" + b"\xf4",               # mov rcx,[r9]; mov [r9+8],rsi; hlt
}
KSLOT = {n: KCODE + 0x40 * i for i, n in enumerate(KPROGS)}
KHANDLER = KCODE + 0x200
_HANDLER = b"\x4c\x8b\x04\x24" + b"\x4c\x8b\x54\x24\x10" + b"\xf4"  # mov r8,[rsp]; mov r10,[rsp+16]; hlt
KDIRTY = {"cross": K + 2, "int": K + 1, "ud": K + 1, "pt": K + 2}


@functools.lru_cache(maxsize=None)
def _kspace():
    sp = AddressSpace()
    code = bytearray(b"\xf4" * 0x1000)
    for n, b in KPROGS.items():
        code[KSLOT[n] - KCODE:KSLOT[n] - KCODE + len(b)] = b
    code[KHANDLER - KCODE:KHANDLER - KCODE + len(_HANDLER)] = _HANDLER
    sp.map(KCODE, bytes(code), user=False, write=False)
    idt = bytearray(0x1000)
    for v in (0x80, 6):
        idt[v * 16:v * 16 + 16] = S2._gate(KHANDLER)
    sp.map(S2.IDT, bytes(idt), user=False, write=False, nx=True)
    sp.map(S2.GDT, S2.gdt_page(), user=False, nx=True)
    sp.map(S2.TSS, bytes(0x1000), user=False, nx=True)
    for i in range(2):
        sp.map(KSTACK + 0x1000 * i, b"", user=False, nx=True)
    for i in range(6):
        sp.map(KDATA + 0x1000 * i, S.data_page(i), user=False, nx=True)
    table = sp.cr3 >> 12  # the leaf page table of KDATA, mapped at PTWIN
    for level in (3, 2, 1):
        table = (sp._entry(table, (KDATA >> (12 + 9 * level)) & 0x1FF) & 0x000FFFFFFFFFF000) >> 12
    sp.map_pfn(PTWIN, table, user=False, nx=True)
    st = user_state(KCODE, KSP, sp.cr3)
    st.update({"cs": seg(0x10, 0, 0, 0x209B), "ss": seg(0x18, 0, 0xFFFFFFFF, 0xC93), "rflags": 0x202,
               "gdtr": {"base": S2.GDT, "limit": S2.GDT_LIMIT}, "idtr": {"base": S2.IDT, "limit": 0xFFF},
               "tr": seg(0x40, S2.TSS, 0x67, 0x8B)})
    return sp, regs_from_state(st)


def _kregs(name, seed):
    _, r0 = _kspace()
    r = type(r0).from_buffer_copy(r0)
    r.rip = KSLOT[name]
    r.gpr[7], r.gpr[6] = KDATA + 0x10, seed
    r.gpr[9] = KDATA + 0x3000 - 4 if name == "cross" else KDATA + 0x4000
    r.gpr[3] = PTWIN + 8 * (((KDATA + 0x4000) >> 12) & 0x1FF)
    return r


@functools.lru_cache(maxsize=None)
def _kwant(name, seed):
    sp, _ = _kspace()
    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    o.restore(_kregs(name, seed))
    e = o.run()
    r = o.regs()
    dirty = sorted(o.dirty())
    return {"status": e.status, "rip": e.rip, "gpr": tuple(r.gpr[i] for i in range(16)), "rflags": r.rflags,
            "icount": o.icount(), "dirty": tuple(dirty), "pages": {g: o.read_phys(g, 4096) for g in dirty}}


def test_guest_allocation_sites_past_k():
    n = 160
    sp, r0 = _kspace()
    names = list(KPROGS)
    prog = [names[l % len(names)] for l in range(n)]
    seeds = [_seed(l % 8, 2) for l in range(n)]
    # the oracle does what the cases are about (so a pass says something)
    for name in names:
        w = _kwant(name, seeds[0])
        assert w["status"] == EXIT_HLT and len(w["dirty"]) == KDIRTY[name], (name, w["status"], hex(w["rip"]))
        assert (w["rip"] == KHANDLER + len(_HANDLER) - 1) == (name in ("int", "ud")), name
    pt = _kwant("pt", seeds[0])  # the load went through the changed mapping: page 5's bytes
    assert pt["gpr"][1] == int.from_bytes(S.data_page(5)[:8], "little")
    eng = _engine(sp, r0, n, pool=2 * n)
    try:
        eng.restore()
        g = eng.read_gprs()
        for l in range(n):
            r = _kregs(prog[l], seeds[l])
            g[l, :16] = [r.gpr[i] for i in range(16)]
            g[l, 16] = r.rip
        eng.write_gprs(g)
        eng.run()
        got = _state(eng, 0, n)
        bad = [(l, prog[l], d) for l in range(n) if (d := _diff(got[l], _kwant(prog[l], seeds[l])))]
        assert not bad, f"{len(bad)}/{n} lanes differ, first: {bad[:5]}"
        st = eng.spill_stats()
        assert st["in_use"] == sum(KDIRTY[p] - K for p in prog) and st["pool_empty"] == 0
    finally:
        eng.close()


def test_host_writes_past_k():
    """apply_writes and apply_phys_writes on lanes that hold K pages: pages
    2 .. 7 come from the pool, a ninth page is WTFGPU_ERR_OOM. Then the loop
    runs over the 8 pages the host dirtied, against an oracle given the same
    writes."""
    n = 160
    sp, r0, gpas = S.space()
    eng = _engine(sp, r0, n, pool=n * X)
    try:
        eng.restore()

        def val(l, i):
            return struct.pack("<QQ", l * 0x0101010101 + i, ~(l + (i << 20)) & MASK64)

        va = [S.DATA_VA + 0x1000 * i for i in range(S.NDATA)]
        eng.apply_writes([(l, va[i] + 0x40, val(l, i)) for l in range(n) for i in range(K)])
        assert list(eng.dirty_counts()) == [K] * n
        virt = [(l, a, d) for l in range(n) for a, d in ((va[2] + 0x40, val(l, 2)),
                                                          (va[4] - 8, val(l, 3)),       # across pages 3 and 4
                                                          (va[6] + 0x40, val(l, 6)))]
        assert set(eng.apply_writes(virt)) == {0}
        phys = [(l, a, d) for l in range(n) for a, d in ((gpas[5] + 0x40, val(l, 5)), (gpas[7] + 0x40, val(l, 7)))]
        assert set(eng.apply_writes(phys, phys=True)) == {0}
        over = eng.apply_writes([(l, va[8] + 0x40, val(l, 8)) for l in range(n)], check=False)
        assert set(over) == {ERR_OOM}
        seeds = [_seed(l, 3) for l in range(n)]
        _start_loop(eng, 0, [CAP] * n, seeds)
        eng.run()
        got = _state(eng, 0, n)
        bad = []
        pfns, blob = sp.phys()
        o = Oracle(pfns=pfns, blob=blob)
        for l in range(0, n, 7):  # (every seventh lane has its own oracle run; the rest are checked by hand below)
            o.restore(S.lane_regs(CAP, seeds[l]))
            for i in (0, 1, 2, 5, 6, 7):
                o.write_virt(va[i] + 0x40, val(l, i))
            o.write_virt(va[4] - 8, val(l, 3))
            e = o.run()
            w = {"status": e.status, "rip": e.rip, "gpr": tuple(o.regs().gpr[i] for i in range(16)),
                 "icount": o.icount(), "dirty": tuple(sorted(o.dirty()))}
            w["pages"] = {g: o.read_phys(g, 4096) for g in w["dirty"]}
            if d := _diff(got[l], w):
                bad.append((l, d))
        for l in range(n):
            p = {gpas[i]: bytearray(S.data_page(i)) for i in range(CAP)}
            for i in (0, 1, 2, 5, 6, 7):
                p[gpas[i]][0x40:0x50] = val(l, i)
            p[gpas[3]][0xFF8:], p[gpas[4]][:8] = val(l, 3)[:8], val(l, 3)[8:]
            for i in range(CAP):
                a = S.BASE + 0x1000 * i
                p[gpas[i]][S.STORE_OFF:S.STORE_OFF + 8] = ((seeds[l] + a) & MASK64).to_bytes(8, "little")
            if got[l]["status"] != S.EXIT_INT3 or got[l]["pages"] != {g: bytes(b) for g, b in p.items()}:
                bad.append((l, "pages"))
        assert not bad, bad[:5]
        assert eng.spill_stats()["in_use"] == n * X
    finally:
        eng.close()


def test_feed_chunk_lands_on_untouched_pages_past_k():
    """A Feed action on lanes that hold K pages: the chunk crosses from one
    untouched page into the next, both come from the pool (the fast loop's
    pre-fault declines past K; the action's own write allocates)."""
    n = 160
    sp, r0, _ = S.space()
    eng = _engine(sp, r0, n, pool=3 * n)
    try:
        eng.set_breakpoints([S.FEED_HOOK, S.FEED_RET])
        acts = (abi.BpAction * 2)()
        acts[0].gva, acts[0].kind, acts[0].value = S.FEED_HOOK, abi.BPACT_FEED, 0x900
        acts[0].gprs[0], acts[0].gprs[1] = 3, 2  # buffer in rbx, size to rdx
        acts[1].gva, acts[1].kind = S.FEED_RET, 5  # STOP_OK
        assert eng.L.wtfgpu_set_breakpoint_actions(eng.ctx, acts, 2) == 0
        eng.restore()
        eng.apply_writes([(l, S.DATA_VA + 0x1000 * i, bytes([l & 0xFF, i])) for l in range(n) for i in range(K)])
        rbx = S.DATA_VA + 0x2800  # the window [rbx, rbx + 0x900) crosses from page 2 into page 3
        g = eng.read_gprs()
        g[:, 3], g[:, 16] = rbx, S.FEED_CALL
        eng.write_gprs(g)
        rng = np.random.default_rng(17)
        chunks, blob, offs = [], b"", [0]
        for _ in range(n):
            size = int(rng.integers(0x101, 0x8FF))  # every chunk starts on page 2 and reaches page 3
            chunks.append(rng.integers(0, 256, size=size, dtype=np.uint8).tobytes())
            blob += size.to_bytes(4, "little") + chunks[-1]
            offs.append(len(blob))
        o = (C.c_uint64 * (n + 1))(*offs)
        assert eng.L.wtfgpu_set_feed(eng.ctx, 0, n, o, None, blob, len(blob)) == 0
        eng.run()
        ex = eng.exits_np()
        out = eng.read_gprs()
        bad = []
        for l, data in enumerate(chunks):
            dst = rbx + 0x900 - len(data)
            page2 = S.data_page(2)
            if (int(ex["status"][l]), int(ex["rip"][l])) != (EXIT_STOP_OK, S.FEED_RET) or \
                    eng.read_virt(l, dst, len(data)) != data or int(out[l, 3]) != dst or int(out[l, 2]) != len(data) or \
                    eng.read_virt(l, dst - 8, 8) != page2[(dst - 8) & 0xFFF:][:8]:
                bad.append((l, len(data), int(ex["status"][l])))
        assert not bad, bad[:5]
        # (the call's return address dirtied the stack page first: three pool pages a lane)
        assert list(eng.dirty_counts()) == [K + 3] * n
        st = eng.spill_stats()
        assert st["in_use"] == 3 * n and st["pool_empty"] == 0
    finally:
        eng.close()


# ---------------------------------------------------------------- 3: reuse across queues
def test_pages_are_reused_across_queues():
    """Two queues, lanes 0 .. 63 and 64 .. 159 (a run starts at a wave
    boundary), six rounds; a pool no larger than the two queues' largest
    demands together, so pages must go round. Every word of every dirty page
    is read back after every round."""
    n, rounds = 160, 6
    first, count = (0, 64), (64, 96)
    sp, r0, _ = S.space()

    def ms(q, r):  # nobody past the cap here: no lane may fail
        return [min(MCYCLE[(l + 3 * r) % len(MCYCLE)], CAP) for l in range(first[q], first[q] + count[q])]

    def demand(q, r):
        return sum(m - K for m in ms(q, r) if m > K)

    pool = max(demand(0, r) for r in range(rounds)) + max(demand(1, r) for r in range(rounds))
    eng = _engine(sp, r0, n, pool=pool)
    bad = []

    def collect(q, r):
        eng.run_wait()
        got = _state(eng, first[q], count[q])
        m = ms(q, r)
        for i in range(count[q]):
            if d := _check(got[i], m[i], _seed(first[q] + i, r)):
                bad.append((r, first[q] + i, m[i], d))

    try:
        for r in range(rounds):
            for q in (0, 1):  # while this queue's lanes are read, restored and refilled, the other's run
                eng.select_queue(q)
                if r:
                    collect(q, r - 1)
                eng.restore(first[q], count[q])
                _start_loop(eng, first[q], ms(q, r), [_seed(first[q] + i, r) for i in range(count[q])])
                eng.run_async(first[q], count[q])
        for q in (0, 1):
            eng.select_queue(q)
            collect(q, rounds - 1)
        assert not bad, f"{len(bad)} lane results differ, first: {bad[:5]}"
        for q in (0, 1):
            eng.select_queue(q)
            eng.restore(first[q], count[q])
            assert not eng.dirty_counts(first[q], count[q]).any()  # (a read on this queue: its restore has run)
        st = eng.spill_stats()
        assert st["pool_empty"] == 0 and st["in_use"] == 0
        assert st["claims"] == sum(demand(q, r) for q in (0, 1) for r in range(rounds)) > pool  # pages were reused
        assert st["peak"] <= pool
    finally:
        eng.close()


# ---------------------------------------------------------------- 4: the pool runs dry
def test_pool_exhaustion_fails_lanes_cleanly():
    """32 of 160 lanes spill: 24 want K + X pages and 8 want one more. The pool
    has 169 pages for a demand of 192. A lane fails for want of a page only
    while the pool is empty and it holds at most X - 1 = 5 pages; had all 24
    lanes with M = K + X failed that way, at most 24 * 5 + 8 * 6 = 168 pages
    would be held, and the pool would not be empty: so at least one of them
    succeeds whatever the order, and since 192 > 169 at least one lane fails."""
    n, pool = 160, 169
    sp, r0, _ = S.space()
    ms = [(CAP + 1 if l % 20 == 0 else CAP) if l % 5 == 0 else MCYCLE[l % len(MCYCLE)] % (K + 1) for l in range(n)]
    assert sum(m == CAP for m in ms) == 24 and sum(m == CAP + 1 for m in ms) == 8 and max(
        m for m in ms if m < CAP) <= K
    seeds = [_seed(l, 9) for l in range(n)]
    eng = _engine(sp, r0, n, pool=pool)
    try:
        eng.restore()
        _start_loop(eng, 0, ms, seeds)
        eng.run()
        got = _state(eng, 0, n)
        held = [len(g["dirty"]) for g in got]
        bad = [(l, ms[l], held[l], d) for l in range(n) if (d := _check(got[l], ms[l], seeds[l], held[l]))]
        assert not bad, f"{len(bad)}/{n} lanes are neither right nor a clean EXIT_OVERLAY_FULL, first: {bad[:5]}"
        starved = [l for l in range(n) if got[l]["status"] == S.EXIT_OVERLAY_FULL and held[l] < CAP]
        st = eng.spill_stats()
        assert st["pool_empty"] == len(starved) > 0
        assert any(got[l]["status"] == S.EXIT_INT3 for l in range(n) if ms[l] == CAP)
        assert st["in_use"] == sum(h - K for h in held if h > K) <= pool
        eng.restore()
        assert eng.spill_stats()["in_use"] == 0
        ms2 = [K + 1] * n  # 160 pages: everyone fits
        _start_loop(eng, 0, ms2, seeds)
        eng.run()
        got = _state(eng, 0, n)
        bad = [(l, d) for l in range(n) if (d := _check(got[l], K + 1, seeds[l]))]
        assert not bad, bad[:5]
        st2 = eng.spill_stats()
        assert st2["pool_empty"] == st["pool_empty"] and st2["in_use"] == n
    finally:
        eng.close()


# ---------------------------------------------------------------- 5: a campaign with a small K and a pool
_SAME = ("execs", "retired", "coverage", "corpus", "crashes", "unique_crashes", "timeouts", "cr3", "errors")
K_SMALL = 3


@pytest.mark.parametrize("edges", [False, True], ids=["rips", "edges"])
def test_tlv_campaign_is_the_same_with_a_small_k_and_a_pool(tmp_path, edges):
    """A fixed-seed tlv campaign (1,024 lanes, 4 batches) with --overlay-pages
    32 and no pool, then with K = 3 private pages and a pool that cannot run
    dry (1,024 lanes x 29 pages, the same 32-page cap per lane): the same
    counts, crash names, corpus and coverage. On an engine without the pool the
    second run ends its spilling testcases as engine errors (err_overlay > 0).

    K = 3 is below the median of the first run's dirty pages per testcase.
    Measured on an MI355X from the first run's corpus, replayed: 2, 4, 5, 5, 5
    and 11 pages (rips: 6 testcases, median 5); with --edges 2, 4, 5 x 6, 7,
    11, 13, 15 (12 testcases, median 5). The test replays the corpus itself and
    checks the median it finds, so a drifting target cannot make it vacuous."""
    base = H.build_target(str(tmp_path / "tlv"))
    flag = ("--edges",) if edges else ()
    out = []
    for tag, extra in (("k32", ("--overlay-pages", "32")),
                       ("spill", ("--overlay-pages", str(K_SMALL), "--spill-pages", str(1024 * (32 - K_SMALL)),
                                  "--spill-lane-max", str(32 - K_SMALL)))):
        t = str(tmp_path / tag)
        shutil.copytree(base, t)
        st = H.fuzz(H.WTFGPU, t, runs=4096, lanes=1024, seed=1337, extra=(*flag, *extra))
        out.append((st, sorted(os.listdir(os.path.join(t, "crashes"))), sorted(os.listdir(os.path.join(t, "outputs"))), t))
    (a, ca, oa, ta), (b, cb, ob, _) = out
    assert a["execs"] == 4096 and a["backend"]["err_overlay"] == 0 and a["backend"]["spill_lanes"] == 0
    # the small K is below the median of the first run's own dirty counts (its corpus, replayed)
    rows = H.run(H.WTFGPU, ta, os.path.join(ta, "outputs"), str(tmp_path / "replay.jsonl"), lanes=1024,
                 full_coverage=False, extra=("--overlay-pages", "32"))
    dirty = sorted(r["dirty"] for r in rows)
    print("dirty pages per corpus testcase:", {d: dirty.count(d) for d in sorted(set(dirty))})
    assert K_SMALL < statistics.median(dirty)
    assert {k: a[k] for k in _SAME} == {k: b[k] for k in _SAME}
    assert ca == cb and oa == ob and oa
    assert b["backend"]["spill_lanes"] > 0 and b["backend"]["spill_pool_empty"] == 0 and b["backend"]["err_overlay"] == 0
    assert b["backend"]["spill_peak"] > 0
