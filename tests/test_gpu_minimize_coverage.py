"""Keeping coverage on the GPU: k_cov_contains against tests/covkeep_model.py
through the C ABI, on sets that k_run filled, and `wtfgpu minimize
--keep-coverage` against `wtf_twin minimize --keep-coverage` byte for byte.

The context has 320 lanes and 64-slot coverage tables (48 values at most), so
probe chains wrap and the longer paths overflow. The guest is four runs of
one-byte nops joined by two branches on rcx's low bits, ending at an int3: a
lane's set is decided by where it starts and by rcx, every seventh lane is
stopped before the run (an empty set), and a lane that starts near the top
walks more than 48 instructions (an overflowed set). The reference is each
lane's set as Engine.coverage() reads it before the call, and the model's
missing(S, T) over it. k_cov_contains takes four lanes a block, so lists of 1,
63, 64, 65 and 257 lanes give partial blocks, full ones, and both."""
import functools
import random

import numpy as np
import pytest

from tests import covkeep_model as M
from tests import tlv_harness as H
from tests.test_minimize_coverage import CASES, hevd_inputs, keep_coverage, tlv_inputs
from wtf_amd import abi
from wtf_amd.abi import regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

pytestmark = pytest.mark.gpu

NL = 320
COV_ENTRIES = 64
CODE_VA, STACK_VA = 0x140000000, 0x7FF000000000
TARGET_SIZES = (0, 1, 63, 64, 65, 200)
LIST_SIZES = (1, 63, 64, 65, 257)
RCX, RIP = 1, 16  # columns of Engine.read_gprs()


def _code() -> bytes:
    c = bytearray()
    c += b"\x90" * 40                  # 0: run A
    c += b"\xf6\xc1\x01\x75\x1e"       # 40: test cl, 1 ; 43: jnz 75 (past run B)
    c += b"\x90" * 30                  # 45: run B
    c += b"\xf6\xc1\x02\x75\x14"       # 75: test cl, 2 ; 78: jnz 100 (past run C)
    c += b"\x90" * 20                  # 80: run C
    c += b"\x90" * 20                  # 100: run D
    c += b"\xcc"                       # 120: int3
    assert len(c) == 121
    return bytes(c)


# where a lane may start: anywhere in run A (long paths: most overflow), the
# second branch, runs C and D (short paths)
STARTS = list(range(0, 40, 3)) + [75] + list(range(80, 120))


@functools.lru_cache(maxsize=None)
def space():
    sp = AddressSpace()
    sp.map_range(CODE_VA, _code() + b"\xcc" * 64, write=False)
    sp.map(STACK_VA, b"")
    return sp, regs_from_state(user_state(CODE_VA, STACK_VA + 0x800, sp.cr3))


class Rig:
    def __init__(self, cov_entries=COV_ENTRIES, lanes=NL):
        from wtf_amd.engine import Engine

        sp, regs = space()
        self.eng = eng = Engine(0)
        pfns, blob = sp.phys()
        eng.load_pool(pfns, blob)
        if lanes:
            eng.alloc_lanes(lanes, overlay_pages=2, cov_entries=cov_entries)
            eng.set_initial_state(regs)
            eng.set_limit(1000)
        self.idle = [l for l in range(lanes) if l % 7 == 3]

    def run(self, salt):
        """Every lane back to the snapshot and run from its start of this salt."""
        eng = self.eng
        rng = random.Random(1000 + salt)
        eng.restore()
        g = eng.read_gprs()
        g[:, RIP] = np.array([CODE_VA + rng.choice(STARTS) for _ in range(NL)], dtype=np.uint64)
        g[:, RCX] = np.array([rng.randrange(4) for _ in range(NL)], dtype=np.uint64)
        eng.write_gprs(g)
        eng.stop(self.idle)
        eng.run()

    def state(self):
        """([set of each lane], [overflow flag of each lane]) as the existing calls read them."""
        cov, _ = self.eng.coverage()
        sets = [cov.get(l, set()) for l in range(NL)]
        # only a set holding all a table can may have overflowed: ask for those lanes alone
        ovf = [len(s) >= M.cap(COV_ENTRIES) and self.eng.coverage(l, 1)[1] for l, s in enumerate(sets)]
        return sets, ovf

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def lane_lists(n):
    return {"ascending": np.arange(n), "sparse": np.random.default_rng(n).permutation(NL)[:n]}


def check(eng, lanes, sets, ovf, target):
    """One call against the model; returns the missing counts."""
    missing, size, overflow = eng.coverage_contains(lanes)
    want = [M.missing(sets[l], target) for l in lanes]
    assert missing.tolist() == want
    assert size.tolist() == [len(sets[l]) for l in lanes]
    assert overflow.tolist() == [int(ovf[l]) for l in lanes]
    return want


def test_kernel_matches_the_model(rig):
    eng = rig.eng
    rig.run(0)
    sets, ovf = rig.state()
    # the shapes the cases need
    assert len({frozenset(s) for s in sets}) >= 8
    assert all(not sets[l] for l in rig.idle) and any(ovf) and not all(ovf)
    assert all(len(s) <= M.cap(COV_ENTRIES) for s in sets) and any(0 < len(s) < M.cap(COV_ENTRIES) for s in sets)
    union = sorted(set().union(*sets))
    rng = random.Random(0xC0FFEE)
    targets = M.targets(union, [], rng, TARGET_SIZES)
    # targets inside one lane's set: every lane whose set holds that one lacks nothing
    small = min((s for s in sets if s), key=len)
    targets += [sorted(small), sorted(small)[::2]]
    assert [len(t) for t in targets[:6]] == list(TARGET_SIZES)
    zero = more = 0
    for t in targets:
        eng.coverage_target(t)
        for n in LIST_SIZES:
            for style, lanes in lane_lists(n).items():
                got = check(eng, lanes, sets, ovf, t)
                if t:
                    zero += sum(1 for m, l in zip(got, lanes) if m == 0 and sets[l])
                    more += sum(1 for m in got if m > 0)
    assert zero > 0 and more > 0
    after, _ = rig.state()
    assert after == sets  # the call reads the sets and leaves them


def test_values_of_the_run_before_do_not_count(rig):
    """Run, restore, run other paths: the tables still hold the first run's
    values under the old generation, in and next to the new chains."""
    eng = rig.eng
    rig.run(1)
    first, _ = rig.state()
    rig.run(2)
    sets, ovf = rig.state()
    gone = [(l, v) for l in range(NL) for v in first[l] - sets[l]]
    assert len(gone) > NL // 2  # lanes lost values they had
    target = sorted(set().union(*first))
    eng.coverage_target(target)
    lanes = np.arange(NL)
    got = check(eng, lanes, sets, ovf, target)
    assert any(m > 0 for m in got)
    # the same after the sets were emptied without a restore
    some = [l for l in range(NL) if sets[l]][:70]
    eng.clear_coverage_lanes(some)
    emptied = [set() if l in set(some) else sets[l] for l in range(NL)]
    check(eng, lanes, emptied, [False if l in set(some) else ovf[l] for l in range(NL)], target)


def test_twice_and_on_both_queues_the_same(rig):
    eng = rig.eng
    rig.run(3)
    sets, ovf = rig.state()
    target = sorted(set().union(*sets))[::2]
    eng.coverage_target(target)
    lanes = lane_lists(257)["sparse"]
    a = [x.tolist() for x in eng.coverage_contains(lanes)]
    b = [x.tolist() for x in eng.coverage_contains(lanes)]
    eng.select_queue(1)
    try:
        c = [x.tolist() for x in eng.coverage_contains(lanes)]
    finally:
        eng.select_queue(0)
    assert a == b == c
    check(eng, lanes, sets, ovf, target)


def test_argument_errors_return_their_codes():
    r = Rig()
    try:
        eng = r.eng
        r.run(4)
        sets, ovf = r.state()
        assert eng.coverage_contains_rc([1, 2])[0] == abi.ERR_STATE  # no target yet
        assert eng.coverage_target_rc(None) == abi.ERR_INVALID
        assert eng.coverage_contains_rc([1, 2])[0] == abi.ERR_STATE  # a refused target sets none
        target = sorted(sets[0] | {5})
        eng.coverage_target(target)
        assert eng.coverage_contains_rc(None)[0] == abi.ERR_INVALID
        assert eng.coverage_contains_rc([1, 2], want_out=False)[0] == abi.ERR_INVALID
        assert eng.coverage_contains_rc([1, NL])[0] == abi.ERR_INVALID
        assert eng.coverage_contains_rc([])[0] == 0
        check(eng, np.array([0, 1, 2, NL - 1]), sets, ovf, target)  # a valid call still works
        eng.coverage_target([])  # the empty target replaces it: nothing is missing anywhere
        assert eng.coverage_contains(np.arange(NL))[0].tolist() == [0] * NL
        after, _ = r.state()
        assert after == sets
    finally:
        r.close()
    for kw in ({"cov_entries": 0}, {"lanes": 0}):  # coverage off; no lanes
        r = Rig(**kw)
        try:
            r.eng.coverage_target([1, 2, 3])
            assert r.eng.coverage_contains_rc([0])[0] == abi.ERR_STATE, kw
        finally:
            r.close()


# ---- `wtfgpu minimize --keep-coverage` against `wtf_twin minimize --keep-coverage`

KEYS = ("mode", "values", "output_values", "input_bytes", "output_bytes", "rounds", "remove_rounds", "zero_rounds",
        "candidates", "skipped", "ok_but_missing", "overflowed", "crash", "stopped_by_rounds")
FEW = [(64, "device", "device", False), (4096, "device", "device", False), (4096, "host", "device", True),
       (4096, "device", "host", False)]
ALL = [(lanes, cov, cand, attrib) for lanes in (64, 4096) for cov in ("device", "host") for cand in ("device", "host")
       for attrib in (False, True)]
SESSIONS = [("hevd", "www_ok_pad", False, *c) for c in ALL] + \
           [(t, n, False, *c) for t, n in CASES if n != "www_ok_pad" for c in FEW] + \
           [("hevd", "integer_big", True, 4096, "device", "device", False),
            ("tlv_server", "multi", True, 4096, "host", "device", False)]


@pytest.fixture(scope="module")
def targets(tmp_path_factory):
    d = tmp_path_factory.mktemp("keepcov_gpu")
    out = {"hevd": (H.build_hevd_target(str(d / "hevd")), {}), "tlv_server": (H.build_target(str(d / "tlv")), {})}
    for tname, inputs in (("hevd", hevd_inputs()), ("tlv_server", tlv_inputs())):
        for name, data in inputs.items():
            p = str(d / name)
            with open(p, "wb") as f:
                f.write(data)
            out[tname][1][name] = p
    return out


@pytest.fixture(scope="module")
def twin(targets, tmp_path_factory):
    """The twin's session, once an (input, edges) asked for."""
    d = tmp_path_factory.mktemp("keepcov_twin")
    done = {}

    def get(tname, name, edges):
        if (name, edges) not in done:
            target, paths = targets[tname]
            o = str(d / f"{name}{int(edges)}.min")
            st = keep_coverage(H.TWIN, target, tname, paths[name], o, extra=("--edges",) if edges else ())
            done[(name, edges)] = (st, open(o, "rb").read())
        return done[(name, edges)]

    return get


@pytest.mark.parametrize("tname,name,edges,lanes,cov,cand,attrib", SESSIONS)
def test_wtfgpu_keeps_coverage_as_the_twin_does(targets, twin, tmp_path, tname, name, edges, lanes, cov, cand, attrib):
    target, paths = targets[tname]
    want_st, want = twin(tname, name, edges)
    assert want_st["cov_on_device"] is False and len(want) < want_st["input_bytes"] and want_st["ok_but_missing"] >= 1
    env = {"WTFGPU_COVKEEP_HOST": "1" if cov == "host" else "0",
           "WTFGPU_MINIMIZE_HOST": "1" if cand == "host" else "0"}
    extra = (("--edges",) if edges else ()) + (("--device-attrib",) if attrib else ())
    out = str(tmp_path / "gpu.min")
    st = keep_coverage(H.WTFGPU, target, tname, paths[name], out, lanes=lanes, extra=extra, env=env)
    print({k: st[k] for k in KEYS}, "seconds", st["seconds"], "cov_readback_values", st["cov_readback_values"],
          "covlog_ms", st["executor"]["covlog_ms"], "attrib_ms", st["executor"]["attrib_ms"])
    assert open(out, "rb").read() == want
    assert {k: st[k] for k in KEYS} == {k: want_st[k] for k in KEYS}
    assert st["cov_on_device"] is (cov == "device") and st["on_device"] is (cand == "device")
    if cov == "device":
        assert st["cov_readback_values"] == st["values"]  # only the input's own set came back
    else:
        assert st["cov_readback_values"] > st["values"]
