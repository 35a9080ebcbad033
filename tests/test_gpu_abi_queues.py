"""The C ABI's argument contract for the lane-list calls, and a direct queue switch.

Nothing else pins either: the engine's Python handle never passes a null list
or a lane out of range, and the streaming node is the only user of the second
queue. Both are host plumbing of wtf_amd/csrc/engine.hip.

test_argument_contract      CONTRACT is the literal table of return codes,
    read from the source of every exported call that takes a lane list: a null
    list with n = 0 and with n = 1, a list holding a lane equal to the lane
    count, each invalid-argument case the call's own body checks, and one valid
    call. Every invalid case returns before any device work. The lanes of the
    128-lane engine are restored and never run.
test_check_order_without_coverage   the same calls on an engine without
    coverage sets: wtfgpu_attribute_coverage checks the lane range before it
    looks for the sets, wtfgpu_collect_coverage_lanes and
    wtfgpu_clear_coverage_lanes after (so a lane out of range is accepted
    there). An accident of history that callers may depend on by now.
test_two_queues_match_synchronous_run   256 lanes of the shared-program set
    of tests/progfuzz.py (seed 31: the CPU oracle ends every one of the 256
    lanes with a fault, the final int3 or the instruction limit, none with
    UNIMPLEMENTED), two halves of 128 lanes, the smallest count at which an
    asynchronous run regroups. Reference: a synchronous run to completion.
    Test run, on a fresh engine: each half on its own queue in slices of 64
    wave-steps, and once, while the other queue's slice is in flight, a few
    finished lanes of queue 0 are restored (wtfgpu_restore_lanes), given their
    first registers again and resumed, so they run a second time to the same
    end. Exits, registers, retired counts and dirty counts of every lane equal
    the reference; wtfgpu_run_wait on an idle queue returns zeroed statistics.
"""
import ctypes as C

import numpy as np
import pytest

from tests import progfuzz
from wtf_amd.abi import EXIT_STOPPED, EXIT_UNIMPLEMENTED, RUNNING, Exit, regs_from_state

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1  # WTFGPU_OK, WTFGPU_ERR_INVALID
NL, K = 128, 16      # lanes and overlay pages of the contract engine
SEED, N_PROGRAMS, LIMIT = 31, 16, 2000

P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
U8P, U32P, U64P = C.POINTER(C.c_uint8), C.POINTER(U32), C.POINTER(U64)

# the lane-list calls wtf_amd.abi leaves undeclared (the C++ host is their user)
SIGS = {
    "wtfgpu_restore_lanes": [P, U32P, U32],
    "wtfgpu_set_feed_lanes": [P, U32P, U32, U64P, U8P, U8P, U64],
    "wtfgpu_collect_coverage_lanes": [P, U32P, U32, U32P, U64P, U64, U64P, U32P],
    "wtfgpu_read_gprs_list": [P, U32P, U32, U64P],
    "wtfgpu_write_gprs_list": [P, U32P, U32, U64P],
    "wtfgpu_read_dirty_list": [P, U32P, U32, U32P],
    "wtfgpu_gather_bytes": [P, U32P, U64P, U32, U32, U8P],
}


def declare(lib):
    for name, args in SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    return lib


def u32(*v):
    return (U32 * len(v))(*v)


def u64(*v):
    return (U64 * len(v))(*v)


@pytest.fixture(scope="module")
def programs():
    """(AddressSpace, base state, [(code va, registers, flags)]) of 256 lanes."""
    return progfuzz.build_shared(256, N_PROGRAMS, SEED)


def make_engine(programs, nlanes, cov_entries=1024):
    from wtf_amd.engine import Engine

    sp, st, _ = programs
    eng = Engine(0)
    declare(eng.L)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(nlanes, overlay_pages=K, cov_entries=cov_entries)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(LIMIT)
    eng.restore()
    return eng


# ---------------------------------------------------------------------------
# 1. argument contract
# ---------------------------------------------------------------------------
# (entry point, case, return code). "range": the list (0, nlanes) with every
# other argument valid.
CONTRACT = [
    ("wtfgpu_resume", "n0_null", OK),
    ("wtfgpu_resume", "n1_null", INVALID),
    ("wtfgpu_resume", "range", INVALID),
    ("wtfgpu_resume", "valid", OK),
    ("wtfgpu_resume", "valid_no_skip", OK),
    ("wtfgpu_stop", "n0_null", OK),
    ("wtfgpu_stop", "n1_null", INVALID),
    ("wtfgpu_stop", "range", INVALID),
    ("wtfgpu_stop", "valid", OK),
    ("wtfgpu_restore_lanes", "n0_null", OK),
    ("wtfgpu_restore_lanes", "n1_null", INVALID),
    ("wtfgpu_restore_lanes", "range", INVALID),
    ("wtfgpu_restore_lanes", "valid", OK),
    ("wtfgpu_clear_coverage_lanes", "n0_null", OK),
    ("wtfgpu_clear_coverage_lanes", "n1_null", INVALID),
    ("wtfgpu_clear_coverage_lanes", "range", INVALID),
    ("wtfgpu_clear_coverage_lanes", "valid", OK),
    ("wtfgpu_lane_seeds", "n0_null", OK),
    ("wtfgpu_lane_seeds", "n1_null", INVALID),
    ("wtfgpu_lane_seeds", "null_seeds", INVALID),
    ("wtfgpu_lane_seeds", "range", INVALID),
    ("wtfgpu_lane_seeds", "valid", OK),
    ("wtfgpu_lane_seeds", "valid_write", OK),
    ("wtfgpu_read_stop_args", "n0_null", OK),
    ("wtfgpu_read_stop_args", "n1_null", INVALID),
    ("wtfgpu_read_stop_args", "null_out", INVALID),
    ("wtfgpu_read_stop_args", "range", INVALID),
    ("wtfgpu_read_stop_args", "valid", OK),
    ("wtfgpu_read_gprs_list", "n0_null", OK),
    ("wtfgpu_read_gprs_list", "n1_null", INVALID),
    ("wtfgpu_read_gprs_list", "range", INVALID),
    ("wtfgpu_read_gprs_list", "valid", OK),
    ("wtfgpu_write_gprs_list", "n0_null", OK),
    ("wtfgpu_write_gprs_list", "n1_null", INVALID),
    ("wtfgpu_write_gprs_list", "range", INVALID),
    ("wtfgpu_write_gprs_list", "valid", OK),
    ("wtfgpu_read_dirty_list", "n0_null", OK),
    ("wtfgpu_read_dirty_list", "n1_null", INVALID),
    ("wtfgpu_read_dirty_list", "range", INVALID),
    ("wtfgpu_read_dirty_list", "valid", OK),
    ("wtfgpu_gather_pages", "n0_null", OK),
    ("wtfgpu_gather_pages", "n0_all_null", OK),      # n = 0 returns before the other arguments are looked at
    ("wtfgpu_gather_pages", "n1_null", INVALID),
    ("wtfgpu_gather_pages", "range", INVALID),
    ("wtfgpu_gather_pages", "null_gpas", INVALID),
    ("wtfgpu_gather_pages", "null_out", INVALID),
    ("wtfgpu_gather_pages", "valid", OK),
    ("wtfgpu_inject_fault", "n0_null", OK),
    ("wtfgpu_inject_fault", "n0_vector_32", OK),     # as above
    ("wtfgpu_inject_fault", "n1_null", INVALID),
    ("wtfgpu_inject_fault", "range", INVALID),
    ("wtfgpu_inject_fault", "null_addrs", INVALID),
    ("wtfgpu_inject_fault", "null_delivered", INVALID),
    ("wtfgpu_inject_fault", "vector_32", INVALID),
    ("wtfgpu_inject_fault", "valid", OK),
    ("wtfgpu_gather_bytes", "n0_null", OK),
    ("wtfgpu_gather_bytes", "n0_len_0", OK),         # as above
    ("wtfgpu_gather_bytes", "n1_null", INVALID),
    ("wtfgpu_gather_bytes", "range", INVALID),
    ("wtfgpu_gather_bytes", "null_gpas", INVALID),
    ("wtfgpu_gather_bytes", "null_out", INVALID),
    ("wtfgpu_gather_bytes", "len_0", INVALID),
    ("wtfgpu_gather_bytes", "len_257", INVALID),
    ("wtfgpu_gather_bytes", "crosses_page", INVALID),
    ("wtfgpu_gather_bytes", "valid", OK),
    ("wtfgpu_gather_bytes", "valid_len_256_page_end", OK),
    ("wtfgpu_collect_coverage_lanes", "n0_null", OK),
    ("wtfgpu_collect_coverage_lanes", "n1_null", INVALID),
    ("wtfgpu_collect_coverage_lanes", "null_total", INVALID),
    ("wtfgpu_collect_coverage_lanes", "cap_null_out", INVALID),
    ("wtfgpu_collect_coverage_lanes", "range", INVALID),
    ("wtfgpu_collect_coverage_lanes", "valid", OK),
    ("wtfgpu_collect_coverage_lanes", "valid_cap_0", OK),
    ("wtfgpu_attribute_coverage", "n0_null", OK),
    ("wtfgpu_attribute_coverage", "n1_null", INVALID),
    ("wtfgpu_attribute_coverage", "null_total", INVALID),
    ("wtfgpu_attribute_coverage", "cap_null_out", INVALID),
    ("wtfgpu_attribute_coverage", "flags_2", INVALID),
    ("wtfgpu_attribute_coverage", "range", INVALID),
    ("wtfgpu_attribute_coverage", "valid", OK),
    ("wtfgpu_attribute_coverage", "valid_all_revoke", OK),
    ("wtfgpu_set_feed_lanes", "n0_null", OK),
    ("wtfgpu_set_feed_lanes", "n1_null", INVALID),
    ("wtfgpu_set_feed_lanes", "null_offsets", INVALID),
    ("wtfgpu_set_feed_lanes", "null_bytes", INVALID),
    ("wtfgpu_set_feed_lanes", "range", INVALID),
    ("wtfgpu_set_feed_lanes", "descending_offsets", INVALID),
    ("wtfgpu_set_feed_lanes", "offsets_past_bytes", INVALID),
    ("wtfgpu_set_feed_lanes", "valid", OK),
    ("wtfgpu_set_feed_lanes", "valid_has_feed", OK),
]


def contract_calls(L, ctx, gpa):
    """(entry point, case) -> a call with that case's arguments. The buffers
    live as long as the returned dict: an asynchronous upload may read them
    after the call."""
    one, two, bad = u32(3), u32(5, 9), u32(0, NL)
    skip = (C.c_uint8 * 2)(0, 1)
    seeds, out6, g18 = u64(7, 7), u64(*[0] * 12), u64(*[0] * 36)
    dirty = u32(*[0] * (2 * (K + 1)))
    gpas, pages = u64(gpa, gpa), (C.c_uint8 * 8192)()
    addrs, delivered = u64(progfuzz.WIN_VA, progfuzz.WIN_VA), (C.c_int32 * 2)()
    at_end, crossing = u64(gpa + 0xF00, gpa + 0xF00), u64(gpa, gpa + 0xFF0)
    olanes, ovals, total, entries, ovf = u32(*[0] * 16), u64(*[0] * 16), U64(), U64(), U32()
    feed = (C.c_uint8 * 8)(*range(8))
    asc, desc, past = u64(0, 4, 8), u64(0, 4, 2), u64(0, 4, 12)
    tot = C.byref(total)
    f = {}
    for name, fn in (("wtfgpu_resume", lambda la, n, s=skip: L.wtfgpu_resume(ctx, la, n, s)),
                     ("wtfgpu_stop", lambda la, n: L.wtfgpu_stop(ctx, la, n, EXIT_STOPPED)),
                     ("wtfgpu_restore_lanes", lambda la, n: L.wtfgpu_restore_lanes(ctx, la, n)),
                     ("wtfgpu_clear_coverage_lanes", lambda la, n: L.wtfgpu_clear_coverage_lanes(ctx, la, n)),
                     ("wtfgpu_lane_seeds", lambda la, n, s=seeds, w=0: L.wtfgpu_lane_seeds(ctx, la, n, s, w)),
                     ("wtfgpu_read_stop_args", lambda la, n, o=out6: L.wtfgpu_read_stop_args(ctx, la, n, o)),
                     ("wtfgpu_read_gprs_list", lambda la, n: L.wtfgpu_read_gprs_list(ctx, la, n, g18)),
                     ("wtfgpu_write_gprs_list", lambda la, n: L.wtfgpu_write_gprs_list(ctx, la, n, g18)),
                     ("wtfgpu_read_dirty_list", lambda la, n: L.wtfgpu_read_dirty_list(ctx, la, n, dirty)),
                     ("wtfgpu_gather_pages",
                      lambda la, n, g=gpas, o=pages: L.wtfgpu_gather_pages(ctx, la, g, n, o)),
                     ("wtfgpu_inject_fault",
                      lambda la, n, v=14, a=addrs, d=delivered: L.wtfgpu_inject_fault(ctx, la, n, v, 2, a, d)),
                     ("wtfgpu_gather_bytes",
                      lambda la, n, g=gpas, ln=32, o=pages: L.wtfgpu_gather_bytes(ctx, la, g, n, ln, o)),
                     ("wtfgpu_collect_coverage_lanes",
                      lambda la, n, ol=olanes, cap=16, t=tot: L.wtfgpu_collect_coverage_lanes(
                          ctx, la, n, ol, ovals, cap, t, C.byref(ovf))),
                     ("wtfgpu_attribute_coverage",
                      lambda la, n, rv=None, fl=0, op=olanes, cap=16, t=tot: L.wtfgpu_attribute_coverage(
                          ctx, la, rv, n, fl, op, ovals, cap, t, C.byref(entries), C.byref(ovf))),
                     ("wtfgpu_set_feed_lanes",
                      lambda la, n, off=asc, has=None, b=feed, nb=8: L.wtfgpu_set_feed_lanes(
                          ctx, la, n, off, has, b, nb))):
        f[name, "n0_null"] = lambda fn=fn: fn(None, 0)
        f[name, "n1_null"] = lambda fn=fn: fn(None, 1)
        f[name, "range"] = lambda fn=fn: fn(bad, 2)
        f[name, "valid"] = lambda fn=fn: fn(two, 2)
        f[name, "call"] = fn
    call = lambda name: f[name, "call"]  # noqa: E731
    f["wtfgpu_resume", "valid_no_skip"] = lambda: call("wtfgpu_resume")(one, 1, None)
    f["wtfgpu_lane_seeds", "null_seeds"] = lambda: call("wtfgpu_lane_seeds")(one, 1, None)
    f["wtfgpu_lane_seeds", "valid_write"] = lambda: call("wtfgpu_lane_seeds")(two, 2, seeds, 1)
    f["wtfgpu_read_stop_args", "null_out"] = lambda: call("wtfgpu_read_stop_args")(one, 1, None)
    f["wtfgpu_gather_pages", "n0_all_null"] = lambda: call("wtfgpu_gather_pages")(None, 0, None, None)
    f["wtfgpu_gather_pages", "null_gpas"] = lambda: call("wtfgpu_gather_pages")(one, 1, None)
    f["wtfgpu_gather_pages", "null_out"] = lambda: call("wtfgpu_gather_pages")(one, 1, gpas, None)
    f["wtfgpu_inject_fault", "n0_vector_32"] = lambda: call("wtfgpu_inject_fault")(None, 0, 32)
    f["wtfgpu_inject_fault", "null_addrs"] = lambda: call("wtfgpu_inject_fault")(one, 1, 14, None)
    f["wtfgpu_inject_fault", "null_delivered"] = lambda: call("wtfgpu_inject_fault")(one, 1, 14, addrs, None)
    f["wtfgpu_inject_fault", "vector_32"] = lambda: call("wtfgpu_inject_fault")(one, 1, 32)
    f["wtfgpu_gather_bytes", "n0_len_0"] = lambda: call("wtfgpu_gather_bytes")(None, 0, gpas, 0)
    f["wtfgpu_gather_bytes", "null_gpas"] = lambda: call("wtfgpu_gather_bytes")(one, 1, None)
    f["wtfgpu_gather_bytes", "null_out"] = lambda: call("wtfgpu_gather_bytes")(one, 1, gpas, 32, None)
    f["wtfgpu_gather_bytes", "len_0"] = lambda: call("wtfgpu_gather_bytes")(one, 1, gpas, 0)
    f["wtfgpu_gather_bytes", "len_257"] = lambda: call("wtfgpu_gather_bytes")(one, 1, gpas, 257)
    f["wtfgpu_gather_bytes", "crosses_page"] = lambda: call("wtfgpu_gather_bytes")(two, 2, crossing, 32)
    f["wtfgpu_gather_bytes", "valid_len_256_page_end"] = lambda: call("wtfgpu_gather_bytes")(two, 2, at_end, 256)
    for name in ("wtfgpu_collect_coverage_lanes", "wtfgpu_attribute_coverage"):
        f[name, "null_total"] = lambda name=name: call(name)(one, 1, t=None)
    f["wtfgpu_collect_coverage_lanes", "cap_null_out"] = lambda: call("wtfgpu_collect_coverage_lanes")(one, 1, ol=None)
    f["wtfgpu_collect_coverage_lanes", "valid_cap_0"] = lambda: call("wtfgpu_collect_coverage_lanes")(
        two, 2, ol=None, cap=0)
    f["wtfgpu_attribute_coverage", "cap_null_out"] = lambda: call("wtfgpu_attribute_coverage")(one, 1, op=None)
    f["wtfgpu_attribute_coverage", "flags_2"] = lambda: call("wtfgpu_attribute_coverage")(one, 1, fl=2)
    f["wtfgpu_attribute_coverage", "valid_all_revoke"] = lambda: call("wtfgpu_attribute_coverage")(
        two, 2, rv=skip, fl=1)
    f["wtfgpu_set_feed_lanes", "null_offsets"] = lambda: call("wtfgpu_set_feed_lanes")(one, 1, off=None)
    f["wtfgpu_set_feed_lanes", "null_bytes"] = lambda: call("wtfgpu_set_feed_lanes")(one, 1, b=None)
    f["wtfgpu_set_feed_lanes", "descending_offsets"] = lambda: call("wtfgpu_set_feed_lanes")(two, 2, off=desc)
    f["wtfgpu_set_feed_lanes", "offsets_past_bytes"] = lambda: call("wtfgpu_set_feed_lanes")(two, 2, off=past)
    f["wtfgpu_set_feed_lanes", "valid_has_feed"] = lambda: call("wtfgpu_set_feed_lanes")(two, 2, has=skip)
    return f


def first_gpa(programs):
    """A guest-physical page of the pool (the lowest one)."""
    sp = programs[0]
    return sorted(sp.phys()[0])[0] << 12


@pytest.fixture(scope="module")
def contract_engine(programs):
    eng = make_engine(programs, NL)
    yield eng, contract_calls(eng.L, eng.ctx, first_gpa(programs))
    eng.read_gprs()  # the queue drained: the asynchronous uploads have read their buffers
    eng.close()


@pytest.mark.parametrize("entry,case,code", CONTRACT, ids=[f"{e[7:]}-{c}" for e, c, _ in CONTRACT])
def test_argument_contract(contract_engine, entry, case, code):
    _, calls = contract_engine
    assert calls[entry, case]() == code


def test_contract_covers_every_case(contract_engine):
    _, calls = contract_engine
    assert {k for k in calls if k[1] != "call"} == {(e, c) for e, c, _ in CONTRACT}


def test_valid_calls_took_effect(contract_engine):
    """After the table: the valid calls did their work (lanes 5 and 9)."""
    eng, calls = contract_engine
    L, two = eng.L, u32(5, 9)
    g = np.arange(36, dtype=np.uint64) + 100
    assert L.wtfgpu_write_gprs_list(eng.ctx, two, 2, g.ctypes.data_as(U64P)) == OK
    back = np.zeros(36, dtype=np.uint64)
    assert L.wtfgpu_read_gprs_list(eng.ctx, two, 2, back.ctypes.data_as(U64P)) == OK
    assert np.array_equal(back, g)
    assert np.array_equal(eng.read_gprs(5, 1)[0], g[:18]) and np.array_equal(eng.read_gprs(9, 1)[0], g[18:])
    seeds = u64(11, 12)
    assert L.wtfgpu_lane_seeds(eng.ctx, two, 2, seeds, 1) == OK
    seeds[0] = seeds[1] = 0
    assert L.wtfgpu_lane_seeds(eng.ctx, two, 2, seeds, 0) == OK
    assert list(seeds) == [11, 12]
    assert L.wtfgpu_stop(eng.ctx, two, 2, EXIT_STOPPED) == OK
    assert [e.status for e in eng.exits(5, 1) + eng.exits(9, 1)] == [EXIT_STOPPED] * 2
    assert L.wtfgpu_restore_lanes(eng.ctx, two, 2) == OK
    assert [e.status for e in eng.exits(5, 1) + eng.exits(9, 1)] == [RUNNING] * 2
    assert np.array_equal(eng.read_gprs(5, 1), eng.read_gprs(0, 1))  # the initial state again


def test_check_order_without_coverage(programs):
    eng = make_engine(programs, NL, cov_entries=0)
    calls = contract_calls(eng.L, eng.ctx, first_gpa(programs))
    assert calls["wtfgpu_attribute_coverage", "range"]() == INVALID
    assert calls["wtfgpu_collect_coverage_lanes", "range"]() == OK
    assert calls["wtfgpu_clear_coverage_lanes", "range"]() == OK
    for name in ("wtfgpu_attribute_coverage", "wtfgpu_collect_coverage_lanes", "wtfgpu_clear_coverage_lanes"):
        assert calls[name, "n1_null"]() == INVALID
        assert calls[name, "valid"]() == OK
    eng.close()


# ---------------------------------------------------------------------------
# 2. queue switch
# ---------------------------------------------------------------------------
N, HALF, SLICE = 256, 128, 64


def first_registers(programs):
    """[N, 18] u64: the 16 GPRs, rip and rflags each lane starts with."""
    return np.array([list(g) + [va, flags] for va, g, flags in programs[2]], dtype=np.uint64)


def final_state(eng):
    ex = eng.exits_np()
    assert not (ex["status"] == RUNNING).any() and not (ex["status"] == EXIT_UNIMPLEMENTED).any()
    return ex, eng.read_gprs(), eng.dirty_counts()


def test_two_queues_match_synchronous_run(programs):
    g0 = first_registers(programs)
    ref = make_engine(programs, N)
    ref.write_gprs(g0)
    ref_stats = ref.run()
    want_ex, want_g, want_dirty = final_state(ref)
    assert ref_stats.lane_retired == int(want_ex["icount"].sum())
    ref.close()

    eng = make_engine(programs, N)
    L = eng.L
    assert L.wtfgpu_select_queue(eng.ctx, 2) == INVALID
    eng.write_gprs(g0)
    halves = [(0, HALF), (HALF, HALF)]
    for q, (first, count) in enumerate(halves):
        eng.select_queue(q)
        eng.run_async(first, count, SLICE)
    in_flight, slices, retired, again = [True, True], [0, 0], 0, []
    # a wave of 64 lanes at LIMIT instructions each cannot take more wave-steps, run twice
    for _ in range(2 * (64 * (LIMIT + 1) // SLICE + 2)):
        for q, (first, count) in enumerate(halves):
            if not in_flight[q]:
                continue
            eng.select_queue(q)
            st = eng.run_wait()
            assert st.kernel_launches >= 1
            slices[q] += 1
            retired += st.lane_retired
            status = eng.exits_np(first, count)["status"]
            if q == 0 and not again and in_flight[1] and (status != RUNNING).any():
                # queue 1's slice is queued and not waited for: plumbing on queue 0 meanwhile
                again = [first + int(i) for i in np.flatnonzero(status != RUNNING)[:4]]
                la = u32(*again)
                assert L.wtfgpu_restore_lanes(eng.ctx, la, len(again)) == OK
                regs = np.ascontiguousarray(g0[again])
                assert L.wtfgpu_write_gprs_list(eng.ctx, la, len(again), regs.ctypes.data_as(U64P)) == OK
                eng.resume(again, [0] * len(again))
                status = eng.exits_np(first, count)["status"]
                assert (status[np.array(again) - first] == RUNNING).all()
            if (status == RUNNING).any():
                eng.run_async(first, count, SLICE)
            else:
                in_flight[q] = False
        if not any(in_flight):
            break
    else:
        raise AssertionError("lanes still running after every possible wave-step")
    assert again, "no lane of queue 0 finished while queue 1 was still running"
    assert min(slices) > 4, slices  # lanes lived across several slices
    for q in (1, 0, 1, 0):
        eng.select_queue(q)
        st = eng.run_wait()  # idle queue
        assert (st.kernel_launches, st.group_steps, st.lane_retired, st.kernel_ms) == (0, 0, 0, 0.0)
    got_ex, got_g, got_dirty = final_state(eng)
    for name in Exit._fields_:
        diff = np.flatnonzero(got_ex[name[0]] != want_ex[name[0]])
        assert diff.size == 0, f"exit.{name[0]} differs in lanes {diff[:8]}"
    diff = np.flatnonzero((got_g != want_g).any(axis=1))
    assert diff.size == 0, f"registers differ in lanes {diff[:8]}"
    diff = np.flatnonzero(got_dirty != want_dirty)
    assert diff.size == 0, f"dirty counts differ in lanes {diff[:8]}"
    assert retired == ref_stats.lane_retired + int(want_ex["icount"][again].sum())
    eng.close()
