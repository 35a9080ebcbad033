"""wtfgpu_attribute_coverage against its model (tests/cov_attrib_model.py).

The SYN loop with one trip and a per-lane start: a lane that starts at
instruction k logs k .. ret and the exit, so the sets nest; lane 0 alone
starts at the first instruction (a value with one owner), every seventh lane
is stopped before the run (an empty set), and the tail of the loop is shared
by every running lane. The raw sets are read with Engine.coverage(), which
leaves them in place; the expectation is the model's walk over them."""
import ctypes as C
import random

import numpy as np
import pytest

from tests.cov_attrib_model import attribute
from wtf_amd import abi
from wtf_amd.abi import regs_from_state
from wtf_amd.tools import syn

pytestmark = pytest.mark.gpu

STARTS = (0, 3, 9, 13, 16, 19, 22, 27, 34, 38, 41, 43)  # the loop's instruction starts
ENTRY = tuple(s for s in STARTS if s != 41)  # (a start at the jnz would take it: the flags say "not zero")


class Rig:
    """An engine over the SYN snapshot whose lanes end with differing sets."""

    def __init__(self, n, cov_entries=256, edges=False, code_pages=(syn.CODE_VA >> 12, syn.EXIT_VA >> 12)):
        from wtf_amd.engine import Engine

        sp, st, _ = syn.build()
        self.n = n
        self.eng = eng = Engine(0)
        pfns, blob = sp.phys()
        eng.load_pool(pfns, blob)
        eng.alloc_lanes(n, overlay_pages=4, cov_entries=cov_entries)
        eng.set_initial_state(regs_from_state(st))
        eng.set_limit(1000)
        eng.set_breakpoints([syn.EXIT_VA])
        if edges:
            eng.set_edges(True)
        eng.set_code_pages(list(code_pages))
        rng = random.Random(n)
        self.start = [0] + [rng.choice(ENTRY[1:]) for _ in range(n - 1)]
        self.idle = [l for l in range(n) if l % 7 == 3]
        self.run()

    def run(self):
        """Every lane back to the snapshot, run again: the sets as at first
        (the aggregate keeps what was committed)."""
        eng = self.eng
        eng.restore()
        g = eng.read_gprs()
        g[:, 1] = 1  # one trip
        g[:, 16] = np.array([syn.CODE_VA + s for s in self.start], dtype=np.uint64)
        eng.write_gprs(g)
        if self.idle:
            eng.stop(self.idle)
        eng.run()

    def sets(self):
        cov, ovf = self.eng.coverage()
        return [cov.get(l, set()) for l in range(self.n)]

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(n, **kw):
        key = (n, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Rig(n, **kw)
        else:
            made[key].run()
        return made[key]

    yield get
    for r in made.values():
        r.close()


def owners(sets):
    own = {}
    for l, s in enumerate(sets):
        for v in s:
            own.setdefault(v, []).append(l)
    return own


def check(rig, lanes, revoke=None, aggregate=(), full=False):
    """One attribution of `lanes` against the model; returns (pos, vals)."""
    eng = rig.eng
    sets = rig.sets()
    listed = [sets[l] for l in lanes]
    want = attribute(listed, revoke, aggregate, full)
    want_ovf = any(eng.coverage(l, 1)[1] for l in lanes)
    pos, vals, entries, ovf = eng.attribute_coverage(lanes, revoke, full)
    got = list(zip(pos.tolist(), vals.tolist()))
    assert got == want
    assert entries == sum(len(s) for s in listed)
    assert ovf == want_ovf
    after = rig.sets()
    for l in range(rig.n):
        assert after[l] == (set() if l in set(lanes) else sets[l]), l
    return pos, vals


def test_rig_has_the_shapes_the_cases_need(rigs):
    for n in (63, 64, 65, 256):
        sets = rigs(n).sets()
        shared = [len(o) for o in owners(sets).values()]
        assert max(shared) >= 3 and min(shared) == 1
        assert any(not s for s in sets) and sets[0] and syn.CODE_VA in sets[0]
        assert len({frozenset(s) for s in sets}) >= 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_identity_order(rigs, n):
    pos, vals = check(rigs(n), list(range(n)))
    # nothing revoked: every value once, at its first owner
    assert len(set(vals.tolist())) == len(vals) > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_reversed_order(rigs, n):
    check(rigs(n), list(range(n))[::-1])


@pytest.mark.parametrize("n", [63, 64, 65, 256])
def test_shuffled_strict_subset(rigs, n):
    lanes = random.Random(5 * n).sample(range(n), n // 2)
    assert lanes != sorted(lanes)
    check(rigs(n), lanes)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("how", ["all", "first_owner", "half"])
def test_revoke(rigs, n, how):
    rig = rigs(n)
    lanes = list(range(n))
    if how == "all":
        revoke = [1] * n
    elif how == "first_owner":  # of the value most lanes share
        own = owners(rig.sets())
        v = max(own, key=lambda k: (len(own[k]), k))
        revoke = [1 if l == own[v][0] else 0 for l in lanes]
    else:
        rng = random.Random(n + 1)
        revoke = [rng.randrange(2) for _ in lanes]
    pos, vals = check(rig, lanes, revoke)
    if how == "all" and n >= 63:  # shared values come back for every owner
        assert len(vals) > len(set(vals.tolist()))


@pytest.mark.parametrize("n", [63, 256])
@pytest.mark.parametrize("one_page", [False, True])
def test_aggregate_grown_after_the_run(n, one_page):
    # an engine of its own: the aggregate stays changed
    kw = {"code_pages": (syn.CODE_VA >> 12,)} if one_page else {}
    rig = Rig(n, **kw)
    try:
        union = sorted(set().union(*rig.sets()))
        half = set(random.Random(3).sample(union, len(union) // 2))
        if one_page:
            half.add(syn.EXIT_VA)  # not a byte of a registered page: the extra set
        rig.eng.commit_coverage(half)
        rng = random.Random(n)
        pos, vals = check(rig, list(range(n)), [rng.randrange(2) for _ in range(n)], aggregate=half)
        assert not (set(vals.tolist()) & half) and len(vals)
    finally:
        rig.close()


@pytest.mark.parametrize("n", [65, 256])
def test_edges(n):
    rig = Rig(n, edges=True)
    try:
        sets = rig.sets()
        rips = {syn.CODE_VA + s for s in STARTS} | {syn.EXIT_VA}
        edge_values = set().union(*sets) - rips
        assert edge_values  # the jnz of every running lane
        rig.eng.commit_coverage({min(edge_values)})
        rng = random.Random(n)
        lanes = rng.sample(range(n), n)
        check(rig, lanes, [rng.randrange(2) for _ in lanes], aggregate={min(edge_values)})
    finally:
        rig.close()


@pytest.mark.parametrize("n", [1, 65, 256])
def test_full_is_each_sorted_set(rigs, n):
    rig = rigs(n)
    sets = rig.sets()
    lanes = list(range(n))[::-1]
    pos, vals = check(rig, lanes, [1] * n, full=True)
    want = [(i, v) for i, l in enumerate(lanes) for v in sorted(sets[l])]
    assert list(zip(pos.tolist(), vals.tolist())) == want


def collect_lanes(eng, lanes):
    """The overflow flag wtfgpu_collect_coverage_lanes reports for `lanes` (it empties their sets)."""
    la = np.ascontiguousarray(lanes, dtype=np.uint32)
    cap = 1 << 16
    ol, orr = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
    total, ovf = C.c_uint64(), C.c_uint32()
    rc = eng.L.wtfgpu_collect_coverage_lanes(eng.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), len(la),
                                             ol.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             orr.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(total),
                                             C.byref(ovf))
    assert rc == 0 and total.value <= cap
    return ovf.value


@pytest.mark.parametrize("n", [64, 65])
def test_overflow_flag_with_small_sets(n):
    # 16 entries hold 12: lane 0 (13 values) overflows, a lane that starts at the tail does not
    a, b = Rig(n, cov_entries=16), Rig(n, cov_entries=16)
    try:
        tail = [l for l in range(1, n) if a.start[l] >= 38 and l not in a.idle]
        assert tail
        for lanes in ([0] + tail, tail, list(range(n))[::-1]):
            a.run()
            b.run()
            want = collect_lanes(b.eng, lanes)
            sets = a.sets()
            pos, vals, entries, ovf = a.eng.attribute_coverage(lanes)
            assert int(ovf) == want == (1 if 0 in lanes else 0)
            assert list(zip(pos.tolist(), vals.tolist())) == attribute([sets[l] for l in lanes])
    finally:
        a.close()
        b.close()


def raw_call(eng, lanes, cap, flags=0):
    la = np.ascontiguousarray(lanes, dtype=np.uint32)
    pos, vals = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64)
    total, entries, ovf = C.c_uint64(77), C.c_uint64(77), C.c_uint32(77)
    rc = eng.L.wtfgpu_attribute_coverage(eng.ctx, la.ctypes.data_as(C.POINTER(C.c_uint32)), None, len(la), flags,
                                         pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         vals.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(total),
                                         C.byref(entries), C.byref(ovf))
    return rc, pos, vals, total.value, entries.value, ovf.value


@pytest.mark.parametrize("flags", [0, abi.ATTRIB_ALL])
def test_cap_smaller_than_total(rigs, flags):
    rig = rigs(65)
    sets = rig.sets()
    lanes = list(range(65))
    want = attribute(sets, full=bool(flags))
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, lanes, len(want) - 1, flags)
    assert rc == 0 and total == len(want)
    assert rig.sets() == sets  # nothing emptied
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, lanes, len(want) + 5, flags)
    assert rc == 0 and total == len(want)
    assert list(zip(pos[:total].tolist(), vals[:total].tolist())) == want
    assert entries == sum(len(s) for s in sets) and ovf == 0
    assert not any(rig.sets())
    # the sets are empty now: nothing to report
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, lanes, 4, flags)
    assert (rc, total, entries, ovf) == (0, 0, 0, 0)


def test_trivial_and_invalid_calls(rigs):
    rig = rigs(64)
    sets = rig.sets()
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, [], 4)
    assert (rc, total, entries, ovf) == (0, 0, 0, 0)
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, [1, 64], 4)
    assert rc == abi_err_invalid()
    rc, pos, vals, total, entries, ovf = raw_call(rig.eng, [1, 2], 4, flags=2)
    assert rc == abi_err_invalid()
    total = C.c_uint64()
    la = (C.c_uint32 * 2)(1, 2)
    assert rig.eng.L.wtfgpu_attribute_coverage(rig.eng.ctx, la, None, 2, 0, None, None, 4, C.byref(total), None,
                                               None) == abi_err_invalid()
    assert rig.eng.L.wtfgpu_attribute_coverage(rig.eng.ctx, la, None, 2, 0, None, None, 0, None, None,
                                               None) == abi_err_invalid()
    assert rig.eng.L.wtfgpu_attribute_coverage(None, la, None, 2, 0, None, None, 0, C.byref(total), None,
                                               None) == abi_err_invalid()
    assert rig.sets() == sets  # a refused call touches nothing


def abi_err_invalid():
    return -1  # WTFGPU_ERR_INVALID


def test_coverage_off_reports_nothing():
    from wtf_amd.engine import Engine

    sp, st, _ = syn.build()
    eng = Engine(0)
    try:
        pfns, blob = sp.phys()
        eng.load_pool(pfns, blob)
        eng.alloc_lanes(64, overlay_pages=4, cov_entries=0)
        rc, pos, vals, total, entries, ovf = raw_call(eng, [0, 5], 4)
        assert (rc, total, entries, ovf) == (0, 0, 0, 0)
    finally:
        eng.close()
