"""The spill pool's bookkeeping on the CPU: several lanes of the engine's slow
step, built for the host (tests/native/sim_spill.cc), run one after another
over one shared pool, each compared with the oracle, which has no page limit.

K = 2 private pages, X = 6 pool pages per lane. The guest loop
(tests/spill_lib.py) dirties M pages: M = 0, 1, K, K + 1 and K + X must match
the oracle in registers, retired count, dirty set and memory; M = K + X + 1
must end as EXIT_OVERLAY_FULL exactly at the store to page K + X. Restoring
every lane empties the pool. Without a pool the harness gives the engine's
behaviour as it has always been: EXIT_OVERLAY_FULL at page K + 1."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from wtf_amd.abi import Regs

from tests import spill_lib as S

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
K, X = S.K, S.X
MS = [0, 1, K, K + 1, K + X, K + X + 1]
DEPS = [os.path.join(NATIVE, "sim_spill.cc"), os.path.join(NATIVE, "host_sim_shim.h")]


class LaneOut(C.Structure):
    _fields_ = [("gpr", C.c_uint64 * 16), ("rip", C.c_uint64), ("rflags", C.c_uint64), ("icount", C.c_uint64),
                ("status", C.c_uint32), ("ovn", C.c_uint32)]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """libsimspill.so, built as tests/native/Makefile builds libsimlane.so."""
    so = str(tmp_path_factory.mktemp("simspill") / "libsimspill.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fPIC",
                           "-shared", "-o", so, DEPS[0]])
    L = C.CDLL(so)
    P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.spill_sim_create.argtypes = [C.POINTER(U64), C.c_char_p, U64, C.POINTER(Regs), U32, U32, U64, U32]
    L.spill_sim_create.restype = P
    L.spill_sim_destroy.argtypes = [P]
    L.spill_sim_restore.argtypes = [P, U32]
    L.spill_sim_run.argtypes = [P, U32, U64, U64, U64, C.POINTER(LaneOut)]
    L.spill_sim_dirty.argtypes = [P, U32, C.POINTER(U64), U32]
    L.spill_sim_dirty.restype = U32
    L.spill_sim_page.argtypes = [P, U32, U64, C.c_char_p]
    L.spill_sim_stats.argtypes = [P, C.POINTER(U64)]
    L.spill_sim_stats.restype = U64
    return L


def _create(L, lanes, pool, k=K, x=X):
    sp, r0, _ = S.space()
    pfns, blob = sp.phys()
    arr = (C.c_uint64 * len(pfns))(*pfns)
    return L.spill_sim_create(arr, blob, len(pfns), C.byref(r0), lanes, k, pool, x)


def _stats(L, h):
    st = (C.c_uint64 * 5)()
    owned = L.spill_sim_stats(h, st)
    return dict(zip(("in_use", "peak", "lanes", "empty", "claims"), st)), owned


def _lane(L, h, lane, m, seed):
    o = LaneOut()
    L.spill_sim_run(h, lane, S.BASE, m, seed, C.byref(o))
    d = (C.c_uint64 * 16)()
    n = L.spill_sim_dirty(h, lane, d, 16)
    pages = {}
    for g in d[:n]:
        b = C.create_string_buffer(4096)
        L.spill_sim_page(h, lane, g, b)
        pages[g] = b.raw
    return {"status": o.status, "rip": o.rip, "gpr": tuple(o.gpr), "rflags": o.rflags, "icount": o.icount,
            "dirty": tuple(sorted(d[:n])), "pages": pages}


def _check_full(got, cap, seed, m):
    w = S.want_full(cap, seed, m)
    assert (got["status"], got["rip"], got["icount"]) == (w["status"], w["rip"], w["icount"])
    assert got["gpr"][2] == w["rdx"] and got["gpr"][8] == w["r8"]
    assert got["dirty"] == w["dirty"] and got["pages"] == w["pages"]


def test_lanes_over_one_pool_match_the_oracle(sim):
    h = _create(sim, len(MS), pool=16)
    try:
        for rnd in range(2):  # the second round takes the pages the first gave back
            for lane, m in enumerate(MS):
                seed = 0x1000 * rnd + 0x10 * lane + 1
                got = _lane(sim, h, lane, m, seed)
                if m <= K + X:
                    assert got == S.want(m, seed), (rnd, m)
                    assert got["status"] == S.EXIT_INT3 and len(got["dirty"]) == m
                else:
                    _check_full(got, K + X, seed, m)
            demand = sum(min(m, K + X) - K for m in MS if m > K)
            st, owned = _stats(sim, h)
            assert owned == demand and st["in_use"] == demand and st["peak"] == demand and st["empty"] == 0
            assert st["lanes"] == (rnd + 1) * sum(m > K for m in MS) and st["claims"] == (rnd + 1) * demand
            for lane in range(len(MS)):
                sim.spill_sim_restore(h, lane)
            st, owned = _stats(sim, h)
            assert owned == 0 and st["in_use"] == 0
    finally:
        sim.spill_sim_destroy(h)


def test_empty_pool_ends_the_lane_and_is_counted(sim):
    """A pool of 4 pages and two lanes that want 6 each: the first takes all
    four and stops at the store to page K + 4 with one pool-empty failure; the
    second stops at page K. Neither was at its cap."""
    h = _create(sim, 2, pool=4)
    try:
        _check_full(_lane(sim, h, 0, K + X, 5), K + 4, 5, K + X)
        _check_full(_lane(sim, h, 1, K + X, 6), K, 6, K + X)
        st, owned = _stats(sim, h)
        assert owned == 4 and st == {"in_use": 4, "peak": 4, "lanes": 1, "empty": 2, "claims": 4}
        sim.spill_sim_restore(h, 0)
        sim.spill_sim_restore(h, 1)
        assert _stats(sim, h)[1] == 0
        assert _lane(sim, h, 1, K + 4, 7) == S.want(K + 4, 7)
    finally:
        sim.spill_sim_destroy(h)


def test_without_a_pool_the_overlay_is_full_at_page_k_plus_1(sim):
    h = _create(sim, 2, pool=0)
    try:
        assert _lane(sim, h, 0, K, 3) == S.want(K, 3)
        _check_full(_lane(sim, h, 1, K + 1, 4), K, 4, K + 1)
        assert _stats(sim, h) == ({"in_use": 0, "peak": 0, "lanes": 0, "empty": 0, "claims": 0}, 0)
    finally:
        sim.spill_sim_destroy(h)


def test_scenario_runs_clean_under_the_sanitizers(tmp_path):
    """The same scenario as a program of its own (tests/native/sim_spill_main.cc)
    with AddressSanitizer and UndefinedBehaviorSanitizer on the host."""
    exe = str(tmp_path / "sim_spill_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(NATIVE, "sim_spill_main.cc")])
    sp, r0, _ = S.space()
    pfns, blob = sp.phys()
    snap = tmp_path / "snapshot.bin"
    snap.write_bytes(struct.pack("<Q", len(pfns)) + struct.pack(f"<{len(pfns)}Q", *pfns) + blob + bytes(r0))
    r = subprocess.run([exe, str(snap), hex(S.BASE), hex(S.STORE_RIP), hex(S.DONE_RIP)], capture_output=True,
                       text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
