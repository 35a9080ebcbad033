"""The page walk on large pages, inherited rights, ignored bits, aliases and
guest edits of page tables: every case of tests/paging_cases.py on the oracle
and on the engine's device code built for the host (tests/native/sim_lane.cc,
slow step and fast forms), each compared with tests/paging_model.py, a plain
restatement of SDM vol. 3 sections 4.5 - 4.7. Nothing here is expected because
one of the three engines does it.

Compared per case: exit status, vector, error code and fault address, rip and
retired count, every loaded value, the probed bytes read back by the host
through every address the case touched, and the dirty frames (as a list: a
frame entered twice shows) with all their bytes.

The host build gets its page-table bitmap from the engine's own marking
(wtf_amd/csrc/engine_ptmark.h), so the T_PT -> flush sites run here too."""
import ctypes as C
import struct

import pytest

from tests import paging_cases as Z
from tests import paging_model as M
from tests import simlane
from tests.oracle_lib import Oracle

LIMIT = 1000
ASSERTED, HOST_WRITES, diff = Z.ASSERTED, Z.HOST_WRITES, Z.diff


# ---------------------------------------------------------------- the three engines
def _vecs(r):
    return {i: struct.pack("<QQQQ", r.xmm[i][0], r.xmm[i][1], r.ymmh[i][0], r.ymmh[i][1]) for i in range(16)}


@pytest.fixture(scope="module")
def oracle():
    sp, _, _ = Z.zoo()
    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    o.set_limit(LIMIT)
    return o


def run_oracle(o, case, salt=0):
    o.restore(Z.lane_regs(case, salt))
    e = o.run()
    r = o.regs()
    dirty = sorted(g >> 12 for g in o.dirty())
    views = {}
    for _, va, _ in case.ops:
        try:
            views[va] = o.read_virt(va, 8)
        except ValueError:
            views[va] = None
    return {"status": e.status, "vector": e.vector, "error": e.error, "addr": e.addr, "rip": e.rip,
            "icount": o.icount(), "gpr": list(r.gpr), "vec": _vecs(r), "dirty": dirty,
            "mem": {p: o.read_phys(p << 12, 4096) for p in dirty}, "views": views}


@pytest.fixture(scope="module")
def sim():
    sp, _, _ = Z.zoo()
    return simlane.image(sp)


def run_sim(sim, case, fast, salt=0):
    pages = simlane.page_buffer()
    r = Z.lane_regs(case, salt)
    win = case.ops[-1][1]
    res, fin, cnt = simlane.run(sim, r, limit=LIMIT, fast=fast, win_va=win, pages=pages)
    k = min(res.ovn, 64)
    dirty = [int(res.dirty[i]) >> 12 for i in range(k)]
    return {"status": res.status, "vector": res.vector, "error": res.error, "addr": res.addr, "rip": res.rip,
            "icount": res.icount, "gpr": list(res.gpr), "vec": _vecs(fin), "dirty": sorted(dirty),
            "mem": {p: pages.raw[i * 4096:(i + 1) * 4096] for i, p in enumerate(dirty)},
            "views": {win: bytes(res.win[:8])}, "fast": cnt}


def _report(bad):
    return f"{len(bad)} cases differ from the model; first: " + "; ".join(f"{n}: {d}" for n, d in bad[:6])


# ---------------------------------------------------------------- the table itself
def test_table_shape():
    """The table cannot silently shrink, and its cases are about what they say."""
    cs = Z.cases()
    count = {}
    for c in cs:
        count[c.family] = count.get(c.family, 0) + 1
    assert count == Z.FAMILIES
    want = {c.name: Z.expect(c) for c in cs}
    # every rights placement and every large leaf is both entered and refused
    for key in [f"r-{bit.lower()}-l{level}-" for bit, level in Z.PLACE] + [f"r-{s}-{b}-" for s in ("2m", "1g")
                                                                           for b in ("w0", "u0", "nx")]:
        got = {want[c.name].completes for c in cs if c.name.startswith(key)}
        assert got == {True, False}, key
    # every large leaf is reached by a load, a store and a fetch
    leaves = {"1g": Z.U1G, "1g-ign": Z.U1G_IGN, "1g-w0": Z.U1G_W0, "1g-u0": Z.U1G_U0, "1g-nx": Z.U1G_NX, "2m": Z.L2,
              "2m-ign": Z.L2_IGN, "2m-b": Z.L2_B, "2m-w0": Z.L2_W0, "2m-u0": Z.L2_U0, "2m-nx": Z.L2_NX}
    for name, base in leaves.items():
        size = Z.GIB if name.startswith("1g") else Z.MIB2
        kinds = {k[:2] for c in cs for k, va, _ in c.ops if base <= va < base + size}
        if name == "2m-b":
            assert "jm" in kinds, name   # (the plain alias: there for the fetch that runs off its end)
        else:
            assert {"ld", "st", "jm"} <= kinds, (name, kinds)
    # the error codes of section 4.7 all occur (P alone cannot: no SMAP, a supervisor read is never refused)
    codes = {w.error for w in want.values() if w.vector == 14}
    assert codes == {0x00, 0x02, 0x04, 0x06, 0x14, 0x10, 0x03, 0x05, 0x07, 0x11, 0x15}, sorted(codes)
    assert any(w.vector == 13 for w in want.values())
    # a permitted CR0.WP = 0 store to a read-only page dirties exactly that frame
    _, _, f = Z.zoo()
    for level in (4, 3, 2, 1):
        assert want[f"r-w0-l{level}-sst-wp0"].dirty == [f["W0", level]]
    assert want["r-2m-w0-sst-wp0"].dirty == [Z.G2_W0 >> 12] and want["r-1g-w0-sst-wp0"].dirty == [Z.G1 >> 12]
    for c in cs:   # the refused two-page stores move nothing
        if c.name.startswith("r-two-page") and not c.name.endswith("wp0"):
            assert not want[c.name].completes and want[c.name].dirty == [], c.name
    assert len(want["r-two-page-second-ro-cpl0-wp0"].dirty) == 2
    # aliases: one frame per page stored to, once
    for c in cs:
        if c.family == "alias":
            w = want[c.name]
            assert w.completes and len(w.dirty) == (2 if "straddle" in c.name else 1) == len(set(w.dirty)), c.name
    # the frames any case can reach are frames of the dump or read as zeros:
    # every gpa a case's accesses translate to lies below the pfn map's end
    sp, _, _ = Z.zoo()
    assert max(sp.pages) == (Z.G1 + Z.GIB - 1) >> 12
    reach = set().union(*(w.reach for w in want.values()))
    assert all(p <= max(sp.pages) for p in reach) and len(reach - set(sp.pages)) == 3   # (three read as the zero page)


def test_model_is_not_the_walks_restated():
    """A few hand-computed translations (SDM figures 4-8 to 4-10) pin the model
    itself: 4 KiB, 2 MiB and 1 GiB address formation, PAT, rights."""
    sp, _, f = Z.zoo()
    t = lambda va, acc, cpl, wp=1: M.translate(sp.pages, sp.cr3, va, acc, cpl, wp, True)  # noqa: E731
    assert t(Z.U1G + 0x3FFFFFFF, M.R, 3) == ("ok", 0x7FFFFFFF)
    assert t(Z.U1G_IGN + 0x12345678, M.R, 3) == ("ok", 0x52345678)   # bit 12 of the entry is PAT, not address
    assert t(Z.L2 + 0x1FFFFF, M.W, 3) == ("ok", 0x3FFFFF) and t(Z.L2_IGN + 0x1234, M.R, 3) == ("ok", 0x201234)
    assert t(Z.IGN4 + 0xABC, M.X, 3) == ("ok", (f["ign4"] << 12) + 0xABC)
    assert t(Z.PLACE["W0", 4] + 8, M.W, 0, 1) == ("pf", 3) and t(Z.PLACE["W0", 4] + 8, M.W, 0, 0)[0] == "ok"
    assert t(Z.PLACE["W0", 4] + 8, M.W, 3, 0) == ("pf", 7) and t(Z.PLACE["U0", 3], M.R, 3) == ("pf", 5)
    assert t(Z.PLACE["NX", 2], M.X, 0) == ("pf", 0x11) and t(Z.PLACE["NX", 2], M.X, 3) == ("pf", 0x15)
    assert t(Z.HOLE, M.X, 3) == ("pf", 0x14) and t(Z.HOLE, M.W, 0) == ("pf", 2)
    assert t(0x800000000000, M.R, 3) == ("gp",)
    assert M.translate(sp.pages, sp.cr3, Z.PLACE["NX", 1], M.X, 3, 1, False)[0] == "ok"   # XD is ignored without NXE
    assert M.access(sp.pages, sp.cr3, Z.HOLE - 4, 8, M.W, 3, 1, True) == ("pf", 6, Z.HOLE)
    assert M.access(sp.pages, sp.cr3, Z.LASTU + 0xFFC, 8, M.R, 3, 1, True) == ("gp",)
    assert M.host_translate(sp.pages, sp.cr3, Z.PLACE["U0", 4] + 5) == (f["U0", 4] << 12) + 5


# ---------------------------------------------------------------- every case, three engines
def test_oracle_matches_the_model(oracle):
    bad = [(c.name, d) for c in ASSERTED if (d := diff(run_oracle(oracle, c), Z.expect(c)))]
    assert not bad, _report(bad)


def test_host_build_slow_step_matches_the_model(sim):
    bad = [(c.name, d) for c in ASSERTED if (d := diff(run_sim(sim, c, 0), Z.expect(c)))]
    assert not bad, _report(bad)


def test_host_build_fast_forms_match_the_model(sim):
    bad, fast = [], {}
    for c in ASSERTED:
        got = run_sim(sim, c, 1)
        fast[c.family] = fast.get(c.family, 0) + got["fast"]
        if d := diff(got, Z.expect(c)):
            bad.append((c.name, d))
    assert not bad, _report(bad)
    # the fast forms did retire instructions where the cases mean them to
    assert fast["alias"] >= 60 and fast["translation"] >= 60, fast
    leaf = [c for c in ASSERTED if c.name.startswith(("t-1g-", "t-2m-"))]
    assert sum(run_sim(sim, c, 1)["fast"] for c in leaf) >= len(leaf)


def test_per_lane_store_values(oracle, sim):
    """The salted form of a case (tests/test_gpu_paging.py gives every lane of
    a wave its own store values) is the same case: a few salts, every engine."""
    bad = []
    for c in ASSERTED:
        if c.salted and c.family == "alias":
            for salt in (1, 0x7F):
                w = Z.expect(c, salt)
                bad += [(c.name, salt, d) for d in (diff(run_oracle(oracle, c, salt), w), diff(run_sim(sim, c, 1, salt), w)) if d]
    assert not bad, bad[:4]


def test_runtime_linked_table_without_invlpg_is_recorded(oracle, sim):
    """A data page linked in as a page table at run time and then edited, no
    invlpg: the snapshot's marking does not know the frame, so the engine may
    keep the translation it cached, as hardware and bochs may; the oracle has
    no TLB. What each does is printed (DESIGN.md U50 records it) and only the
    two possible outcomes are asserted: the second load reads the old frame or
    the new one, and everything else is as the model says."""
    _, _, f = Z.zoo()
    case = next(c for c in Z.cases() if c.family == "link-unasserted")
    want = Z.expect(case)
    old, new = ((f["kd", i] << 12) + 0x20 for i in (1, 2))
    last = Z.DEST[len(case.ops) - 1]
    assert want.gpr[last] == new
    for name, got in (("oracle", run_oracle(oracle, case)), ("host build, slow step", run_sim(sim, case, 0)),
                      ("host build, fast forms", run_sim(sim, case, 1))):
        print(f"{name}: the load after the edit reads {'the new' if got['gpr'][last] == new else 'the old'} frame")
        assert got["gpr"][last] in (old, new), name
        want.gpr[last] = got["gpr"][last]
        assert not diff(got, want), name


# ---------------------------------------------------------------- host accesses
def test_host_translate_is_present_bits_only(oracle):
    sp, r0, _ = Z.zoo()
    oracle.restore(r0)
    bad = [(hex(va), oracle.translate(va), M.host_translate(sp.pages, sp.cr3, va)) for va in Z.host_addresses()
           if oracle.translate(va) != M.host_translate(sp.pages, sp.cr3, va)]
    assert not bad, bad[:5]
    assert sum(M.host_translate(sp.pages, sp.cr3, va) is None for va in Z.host_addresses()) >= 4


@pytest.mark.parametrize("name,va,n,lands", HOST_WRITES, ids=[w[0] for w in HOST_WRITES])
def test_host_write_virt(oracle, name, va, n, lands):
    """VirtWrite by present bits: a read-only or supervisor page takes it, and
    the frame the model names becomes dirty."""
    sp, r0, _ = Z.zoo()
    oracle.restore(r0)
    data = bytes(range(0xC1, 0xC1 + n))
    parts = [(M.host_translate(sp.pages, sp.cr3, a), 1) for a in range(va, va + n)]
    assert all(g is not None for g, _ in parts) == lands
    if not lands:
        with pytest.raises(ValueError):
            oracle.write_virt(va, data)
        return
    oracle.write_virt(va, data)
    mem = M.Memory(sp.pages)
    mem.write(parts, data)
    assert sorted(g >> 12 for g in oracle.dirty()) == sorted(mem.dirty)
    assert all(oracle.read_phys(p << 12, 4096) == bytes(mem.own[p]) for p in mem.dirty)
    assert oracle.read_virt(va, n) == data


# ---------------------------------------------------------------- the reference's own walk
def test_walks_match_the_reference_lines(sim):
    from wtf_amd.abi import regs_from_state
    from wtf_amd.tools.snapshot import user_state

    sp, want = M.reference_lines()
    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    o.restore(regs_from_state(user_state(0x140000000, 0x7F8000000100, sp.cr3)))
    arr = (C.c_uint64 * len(pfns))(*pfns)
    for g, gpa in want.items():
        assert o.translate(g) == gpa, hex(g)
        out = C.c_uint64()
        rc = simlane.lib().sim_translate(arr, blob, len(pfns), sp.cr3, g, C.byref(out))
        if M.canonical(g):   # (the device walk refuses a non-canonical address; the host's takes its low 48 bits)
            assert (None if rc else out.value) == gpa, hex(g)
