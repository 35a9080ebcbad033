"""The page walk on the GPU: the cases of tests/paging_cases.py, one lane each
in waves that mix rings, paths and verdicts, then each page-copying case across
a whole wave (the fast loop's whole-wave copy-on-write), under two more launch
shapes, and the host's accesses (translate, read_virt, write_virt,
apply_writes) on the same address space. Expectations come from
tests/paging_model.py (SDM vol. 3 4.5 - 4.7), as in tests/test_paging.py.

Guest #PF / #GP are lane exits. No case leaves the page pool: a frame outside
the dump reads as the zero page (tests/test_paging.py::test_table_shape)."""
import random
import struct

import numpy as np
import pytest

from wtf_amd import abi

from tests import launch_shapes as shared
from tests import paging_cases as Z
from tests import paging_model as M
from tests.oracle_lib import Oracle

pytestmark = pytest.mark.gpu

LIMIT = 1000
K = 8
CODE_ON_LEAF = {"t-x-2m-cross4k": [Z.L2 + 0xFFD], "t-x-2m-out-present": [Z.L2 + Z.MIB2 - 3],
                "t-ign-2m-x": [Z.L2_IGN + Z.TGT], "r-2m-clean-ux": [Z.L2 + Z.TGT]}


def _mixed():
    """Every case on a lane of its own, shuffled with a fixed seed, padded with
    repeats to whole waves: [(case, salt)]."""
    lanes = [(c, 0) for c in Z.ASSERTED]
    rnd = random.Random(20260401)
    while len(lanes) % 64:
        lanes.append((rnd.choice(Z.ASSERTED), 1 + len(lanes) % 200))
    rnd.shuffle(lanes)
    assert len(lanes) >= 256
    rings = [{c.cpl for c, _ in lanes[i:i + 64]} for i in range(0, len(lanes), 64)]
    assert all(r == {0, 3} for r in rings)   # every wave mixes the rings
    return lanes


# the cases that copy a page, by the model's word: every case that ends with a dirty frame (stores through
# aliases, CR0.WP = 0 stores, stores into and out of large leaves and into the frame the dump does not
# hold, table edits)
UNIFORM = [c for c in Z.ASSERTED if Z.expect(c).dirty]
NLANES = max(len(_mixed()), 64 * len(UNIFORM))


def _new_engine():
    from wtf_amd.engine import Engine
    sp, r0, _ = Z.zoo()
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    return eng, r0


@pytest.fixture(scope="module")
def eng():
    e, r0 = _new_engine()
    e.alloc_lanes(NLANES, overlay_pages=K, cov_entries=64)
    e.set_initial_state(r0)
    e.set_limit(LIMIT)
    e.set_code_pages(sorted({va >> 12 for vas in CODE_ON_LEAF.values() for va in vas} | {Z.AFTER >> 12}))
    yield e
    e.close()


def load(eng, lanes):
    eng.restore(0, len(lanes))
    eng.write_regs([Z.lane_regs(c, salt) for c, salt in lanes])


def collect(eng, lanes, views=False):
    n = len(lanes)
    ex = eng.exits_np(0, n)
    regs = eng.read_regs(0, n)
    dl = eng.dirty_list(np.arange(n))
    pl = [i for i in range(n) for _ in range(int(dl[i, 0]))]
    pg = [int(g) << 12 for i in range(n) for g in dl[i, 1:1 + int(dl[i, 0])]]
    data = eng.gather_pages(pl, pg) if pl else np.zeros((0, 4096), dtype=np.uint8)
    out, at = [], 0
    for i, (c, _) in enumerate(lanes):
        k = int(dl[i, 0])
        r = regs[i]
        v = {}
        if views:
            for _, va, _ in c.ops:
                try:
                    v[va] = eng.read_virt(i, va, 8)
                except Exception:   # EngineError: does not translate
                    v[va] = None
        out.append({"status": int(ex["status"][i]), "vector": int(ex["vector"][i]), "error": int(ex["error"][i]),
                    "addr": int(ex["addr"][i]), "rip": int(ex["rip"][i]), "icount": int(ex["icount"][i]),
                    "gpr": list(r.gpr), "dirty": sorted(p >> 12 for p in pg[at:at + k]),
                    "vec": {j: struct.pack("<QQQQ", r.xmm[j][0], r.xmm[j][1], r.ymmh[j][0], r.ymmh[j][1]) for j in range(8)},
                    "mem": {pg[at + j] >> 12: data[at + j].tobytes() for j in range(k)}, "views": v})
        at += k
    return out


def check(got, lanes, what):
    want = {}
    bad = []
    for i, (c, salt) in enumerate(lanes):
        if (c.name, salt) not in want:
            want[c.name, salt] = Z.expect(c, salt)
        if d := Z.diff(got[i], want[c.name, salt]):
            bad.append((i, c.name, salt, d))
    assert not bad, f"{what}: {len(bad)}/{len(lanes)} lanes differ from the model; first: {bad[:4]}"


def _key(got):
    return [(g["status"], g["vector"], g["error"], g["addr"], g["rip"], g["icount"], g["gpr"], g["dirty"], g["mem"], g["vec"])
            for g in got]


def test_mixed_waves(eng):
    lanes = _mixed()
    load(eng, lanes)
    eng.run(0, len(lanes))
    got = collect(eng, lanes, views=True)
    check(got, lanes, "mixed waves")
    cov, ovf = eng.coverage(0, len(lanes))
    assert not ovf
    for i, (c, _) in enumerate(lanes):
        for rip in CODE_ON_LEAF.get(c.name, ()):
            assert rip in cov.get(i, set()), (c.name, hex(rip))
    # restore: nothing dirty, the edited mappings are the snapshot's again, and the same run gives the same results
    eng.restore(0, len(lanes))
    assert not eng.dirty_counts(0, len(lanes)).any()
    sp, _, f = Z.zoo()
    edited = [i for i, (c, _) in enumerate(lanes) if c.family in ("edit", "link")]
    for i in edited[:8]:
        assert eng.translate(i, Z.KDATA + 0x20) == (f["kd", 0] << 12) + 0x20
        assert eng.read_virt(i, Z.KLEAF + 0x3000, 8) == bytes(sp.pages[f["kleaf_x"]][:8])
    # a plain guest load of each edited case's X on its own lane: the snapshot's mapping again
    # (or its fault: KLINK has no mapping in the snapshot)
    plain = [(Z.Case("x-" + c.name, "edit", 0, 1, (("ld8", c.ops[-1][1], None),), False), 0) if i in edited else (c, s)
             for i, (c, s) in enumerate(lanes)]
    assert len(edited) >= 70
    eng.write_regs([Z.lane_regs(c, salt) for c, salt in plain])
    eng.run(0, len(lanes))
    check(collect(eng, plain), plain, "plain loads after restore")
    eng.restore(0, len(lanes))
    eng.write_regs([Z.lane_regs(c, salt) for c, salt in lanes])
    eng.run(0, len(lanes))
    again = collect(eng, lanes)
    assert _key(again) == _key(got)


def test_uniform_waves(eng):
    """One case per wave, all 64 lanes at the same instruction with their own
    store values: the whole wave misses together and copies together."""
    lanes = [(c, lane if c.salted else 0) for c in UNIFORM for lane in range(64)]
    assert len(UNIFORM) >= 150 and {c.name for c in UNIFORM} >= {"t-2m-st8-last", "t-out-st16-present", "t-ign-1g-st",
                                                                  "r-cmpxchg-ro-wp0", "r-two-page-second-ro-cpl0-wp0"}
    assert {c.family for c in UNIFORM} >= {"alias", "edit", "link", "rights", "translation"}
    load(eng, lanes)
    eng.run(0, len(lanes))
    check(collect(eng, lanes), lanes, "uniform waves")


@pytest.mark.parametrize("shape", ["regroup-64", "lpw-16"])
def test_launch_shapes(shape, monkeypatch):
    lanes = _mixed()

    def make_engine(_w):
        e, r0 = _new_engine()
        e.alloc_lanes(len(lanes), overlay_pages=K, cov_entries=64)
        e.set_initial_state(r0)
        e.set_limit(LIMIT)
        load(e, lanes)
        return e

    monkeypatch.setattr(shared, "make_engine", make_engine)
    e, retired = shared.SHAPES[shape](None, monkeypatch)
    try:
        got = collect(e, lanes)
        check(got, lanes, shape)
        assert retired == sum(g["icount"] for g in got)
    finally:
        e.close()


# ---------------------------------------------------------------- host accesses
def test_host_translate_and_read(eng):
    sp, _, _ = Z.zoo()
    eng.restore(0, 64)
    bad = []
    for va in Z.host_addresses():
        want = M.host_translate(sp.pages, sp.cr3, va)
        if eng.translate(0, va) != want:
            bad.append((hex(va), eng.translate(0, va), want))
    assert not bad, bad[:5]
    mem = M.Memory(sp.pages)
    for va in (Z.U1G + Z.GIB - 16, Z.L2 + 0xFFC, Z.L2_IGN + Z.MIB2 - 4, Z.U1G_IGN + 0x1FFA, Z.L2_U0 + 0x10, Z.L2 + Z.MIB2 // 2):
        parts = [(M.host_translate(sp.pages, sp.cr3, a), 1) for a in range(va, va + 16)]
        assert eng.read_virt(0, va, 16) == mem.read(parts), hex(va)
    with pytest.raises(Exception):
        eng.read_virt(0, Z.L2_B + Z.MIB2 - 4, 8)   # out of the leaf into a hole


def _after_host_write(eng, lane):
    d = sorted(eng.dirty(lane))
    return d, {g: eng.read_phys(lane, g, 4096) for g in d}


@pytest.mark.parametrize("block", [False, True], ids=["write_virt", "apply_writes"])
def test_host_writes(eng, block):
    """k_lane_mem's single-lane write and k_apply_writes' 64-thread block form.
    A write that fails half way is compared with the oracle for what it left."""
    sp, r0, _ = Z.zoo()
    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    n = len(Z.HOST_WRITES)
    eng.restore(0, 64)
    if block:   # every write on 8 lanes at once: lane 8 * w + j
        recs = [(8 * w + j, va, bytes(range(0xC1 + j, 0xC1 + j + k))) for w, (_, va, k, _) in enumerate(Z.HOST_WRITES)
                for j in range(8)]
        st = eng.apply_writes(recs, check=False)
        assert [s == 0 for s in st] == [Z.HOST_WRITES[r[0] // 8][3] for r in recs]
    for w, (name, va, k, lands) in enumerate(Z.HOST_WRITES):
        for j in range(8 if block else 1):
            lane = 8 * w + j
            data = bytes(range(0xC1 + j, 0xC1 + j + k))
            if not block:
                if lands:
                    eng.write_virt(lane, va, data)
                else:
                    with pytest.raises(Exception):
                        eng.write_virt(lane, va, data)
            o.restore(r0)
            try:
                o.write_virt(va, data)
                assert lands, name
            except ValueError:
                assert not lands, name
            od = sorted(o.dirty())
            assert _after_host_write(eng, lane) == (od, {g: o.read_phys(g, 4096) for g in od}), name
            if lands:
                parts = [(M.host_translate(sp.pages, sp.cr3, a), 1) for a in range(va, va + k)]
                mem = M.Memory(sp.pages)
                mem.write(parts, data)
                assert [g >> 12 for g in od] == sorted(mem.dirty) and eng.read_virt(lane, va, k) == data, name
    assert n * 8 <= 64


def test_host_edit_of_a_table_is_seen_after_resume(eng):
    """Lanes stop at a breakpoint between two loads of one page; the host
    repoints the page's PTE (write_virt on one lane, apply_writes on the
    others); resumed, the second load reads the other frame."""
    sp, _, f = Z.zoo()
    case = next(c for c in Z.ASSERTED if c.name == "h-two-loads")
    lanes = [(case, 0)] * 64
    bp = Z.entry_rip(case) + 3
    eng.set_breakpoints([bp])
    try:
        load(eng, lanes)
        eng.run(0, 64)
        ex = eng.exits_np(0, 64)
        assert set(ex["status"]) == {abi.EXIT_BREAKPOINT} and set(ex["rip"]) == {bp}
        entry = struct.pack("<Q", f["kd", 4] << 12 | Z.P | Z.RW)
        eng.write_virt(0, Z.PTWIN, entry)
        eng.apply_writes([(lane, Z.PTWIN, entry) for lane in range(1, 64)])
        eng.resume(list(range(64)), [1] * 64)
        eng.run(0, 64)
        got = eng.read_gprs(0, 64)
        ex = eng.exits_np(0, 64)
        assert set(ex["status"]) == {abi.EXIT_INT3}
        first, second = (int.from_bytes(sp.pages[f["kd", i]][0x20:0x28], "little") for i in (0, 4))
        assert set(got[:, Z.DEST[0]]) == {first} and set(got[:, Z.DEST[1]]) == {second}
        assert all(sorted(eng.dirty(lane)) == [f["table", 1] << 12] for lane in (0, 1, 63))
    finally:
        eng.set_breakpoints([])


def test_translate_matches_the_reference_lines():
    """Engine.translate on the large-page dump against kdmp-parser's own lines."""
    from wtf_amd.abi import regs_from_state
    from wtf_amd.engine import Engine
    from wtf_amd.tools.snapshot import user_state

    sp, want = M.reference_lines()
    e = Engine(0)
    try:
        pfns, blob = sp.phys()
        e.load_pool(pfns, blob)
        e.alloc_lanes(64, overlay_pages=2, cov_entries=64)
        e.set_initial_state(regs_from_state(user_state(0x140000000, 0x7F8000000100, sp.cr3)))
        e.restore()
        bad = [(hex(g), e.translate(0, g), gpa) for g, gpa in want.items() if e.translate(0, g) != gpa]
        assert not bad, bad
    finally:
        e.close()


def test_device_feed_into_a_table_is_seen_at_once(eng):
    """A Feed action (the device's own copy of a testcase chunk into guest
    memory) whose chunk is a PTE: the page it remaps was read just before, and
    the table's frame is the lane's own already, so nothing but the Feed copy's
    own page-table check drops the cached translation."""
    import ctypes as C

    sp, _, f = Z.zoo()
    case = next(c for c in Z.ASSERTED if c.name == "h-two-loads")
    lanes = [(case, 0)] * 64
    bp = Z.entry_rip(case) + 3
    entry = struct.pack("<Q", f["kd", 4] << 12 | Z.P | Z.RW)
    eng.set_breakpoints([bp])
    acts = (abi.BpAction * 1)()
    acts[0].gva, acts[0].kind, acts[0].value = bp, abi.BPACT_FEED, 2 * len(entry)   # (a chunk is shorter than its window)
    acts[0].gprs[0], acts[0].gprs[1] = 15, 14   # the buffer in r15, the size to r14
    assert eng.L.wtfgpu_set_breakpoint_actions(eng.ctx, acts, 1) == 0
    try:
        load(eng, lanes)
        eng.apply_writes([(lane, Z.PTWIN + 0x800, bytes(8)) for lane in range(64)])
        g = eng.read_gprs(0, 64)
        g[:, 15] = Z.PTWIN - len(entry)   # the chunk lands at the window's end
        eng.write_gprs(g)
        blob = (len(entry).to_bytes(4, "little") + entry) * 64
        offs = (C.c_uint64 * 65)(*[12 * i for i in range(65)])
        assert eng.L.wtfgpu_set_feed(eng.ctx, 0, 64, offs, None, blob, len(blob)) == 0
        eng.run(0, 64)
        ex = eng.exits_np(0, 64)
        got = eng.read_gprs(0, 64)
        assert set(ex["status"]) == {abi.EXIT_INT3}, set(ex["status"])
        first, second = (int.from_bytes(sp.pages[f["kd", i]][0x20:0x28], "little") for i in (0, 4))
        assert set(got[:, Z.DEST[0]]) == {first} and set(got[:, Z.DEST[1]]) == {second}
        assert set(got[:, 15]) == {Z.PTWIN} and set(got[:, 14]) == {len(entry)}
    finally:
        assert eng.L.wtfgpu_set_breakpoint_actions(eng.ctx, acts, 0) == 0
        eng.set_breakpoints([])
