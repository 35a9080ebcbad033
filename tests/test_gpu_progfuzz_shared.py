"""Grouped execution in k_run vs the CPU oracle: many lanes on few programs.

tests/test_gpu_progfuzz.py gives every lane a program of its own, so a wave
never holds two lanes at one rip and every group of the wave-level interpreter
has one lane. Here 512 lanes share 16 programs (progfuzz.build_shared: lane i
runs program (i // 4) % 16, registers / flags / XMM state per lane), and the
programs derive per-lane effective addresses from that state. Per lane, bit
exact against the oracle: exit status / vector / error / address, rip, retired
count, the 16 GPRs, RFLAGS, the coverage set, the dirty set, the byte counter,
with sse the XMM / YMM-high / MXCSR state, with evex zmm0-31 and k0-7 as well,
and for every 8th lane the contents of the data window and the stack. tests/test_progfuzz_shared.py holds the
generator to the divergence this needs.

Which group hazards each test reaches (engine_run.h, k_run):

  test_grouped_run_matches_oracle        default launch. Min-rip selection with
      several groups in a wave; the ingm mask (lanes of a group on different
      code-page copies); the round-based fast path with some lanes of a group
      missing (TLB miss, first write) while the others retire; fast_fault in a
      part of a group (#PF on the read-only page, #GP of a misaligned SSE
      operand, #XM, #DE) while the rest goes on; page-crossing operands in a
      part of a group (slow step for those lanes); the wave-cooperative
      copy-on-write with several lanes making their first write at once, to
      the same guest page or to different ones; per-position `logged` bits
      (lanes of a group reaching a rip the others have logged already); the
      regrouping permutation between launches (default schedule of a run to
      completion). Asserts that groups really formed: more than 2 lanes
      retired per wave-step.
  test_launch_shapes_match_oracle        the same under every launch shape:
      fixed lane order (one launch, no permutation); regrouping forced every
      64 wave-steps (store_lane / load_lane and the permutation many times,
      lanes of a group change wave and position); host-sliced runs of 5 and 64
      wave-steps (launch boundaries inside loops, rep strings and groups; the
      warm LDS image carried from launch to launch); async slices; 32 and 16
      lanes per wave (the lane / position mapping, waves with idle positions);
      a cold LDS uop cache at every launch; no shared uop cache (every decode
      by the wave itself); hot caches (a second pass over warm LDS images and
      a filled shared cache); a coverage map over the code pages (the
      covered-flag lookups, nothing committed); and forced regrouping +
      slices + 16 lanes per wave together on the floating-point seed.
  test_slice_length_is_path_independent  the U44 claim of k_run: what a lane
      has done after each 64 wave-step slice does not depend on which path
      served a group (warm or cold LDS cache, shared cache or own decode,
      covered or uncovered rips: the `logged` / UC_COVERED paths).
  test_breakpoints_with_mixed_skip_groups  host breakpoints at block heads,
      also inside counted loops and at jcc targets; lanes stop, are checked
      against the oracle's stop list and resumed with skip, every other one a
      round later, so that resumed and freshly arriving lanes meet at one
      breakpoint rip in one group (`ingm & ~__ballot(skip)`): asserted to have
      happened. Once in fixed order, once with forced regrouping (lflags
      travel with the lane through the permutation).

Observed on MI355X, lanes retired per wave-step with default settings (the
test asserts > 2.0, the non-degeneracy bound; with a program per lane the
figure cannot exceed 1.0): seed 31: 30.4, seed 32: 29.6, seed 35 (sse): 24.2,
seed 34 (sse, fp): 30.2, each in 4 launches. The default run to completion
regroups, which brings the 32 lanes of a program side by side, and the
programs that run into the instruction limit do so in lockstep; both push the
figure far above the 4 lanes of a program that a wave holds in lane order.
Stops of a fresh lane in one group with a resumed (skip) lane, fixed order:
668 (seed 31) and 670 (seed 34). The 61 tests of the module before the
evex case took 19 s; with it and the reduced rep stos case there are 76.
"""
import numpy as np
import pytest

from tests import progfuzz
from tests.launch_shapes import (CASES, EVEX, FP, INT_A, LIMIT, N, N_PROGRAMS, SHAPES, Totals, Workload, case_id, check,
                                 load_lanes, make_engine, shape_combined)
from wtf_amd.abi import EXIT_BREAKPOINT, EXIT_FAULT, RUNNING, regs_from_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workloads():
    """case -> Workload; the oracle runs once per case, its results are shared
    and never modified."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Workload(case)
        return cache[case]

    return get


# ---------------------------------------------------------------------------
# 2. grouped execution, default settings
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_grouped_run_matches_oracle(case, workloads):
    w = workloads(case)
    eng = make_engine(w)
    stats = eng.run()
    check(eng, w, w.want, "default", retired=stats.lane_retired)
    per_step = stats.lane_retired / stats.group_steps
    print(f"{case_id(case)}: {per_step:.2f} lanes retired per wave-step, {stats.kernel_launches} launches")
    # non-degeneracy: with a program per lane this cannot exceed 1.0
    assert per_step > 2.0
    eng.close()


# ---------------------------------------------------------------------------
# 3. the same workload under every launch shape
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_launch_shapes_match_oracle(case, shape, workloads, monkeypatch):
    w = workloads(case)
    eng, retired = SHAPES[shape](w, monkeypatch)
    check(eng, w, w.want, shape, retired=retired)
    eng.close()


def test_regroup_sliced_lpw16_matches_oracle(workloads, monkeypatch):
    w = workloads(FP)
    eng, retired = shape_combined(w, monkeypatch)
    check(eng, w, w.want, "regroup-64 + sliced-64 + lpw-16", retired=retired)
    eng.close()


# ---------------------------------------------------------------------------
# 4. slice length does not depend on the path (U44)
# ---------------------------------------------------------------------------
def slice_records(eng):
    """(status, rip, icount) of every lane after each 64 wave-step slice."""
    recs = []
    for _ in range(64 * (LIMIT + 1) // 64 + 2):
        eng.run(max_steps=64)
        ex = eng.exits_np()
        recs.append(np.stack([ex["status"].astype(np.uint64), ex["rip"], ex["icount"]]))
        if not (ex["status"] == RUNNING).any():
            return recs
    raise AssertionError("lanes still running after every possible wave-step")


_BASELINE = {}


def baseline_records(w):
    """Variant (a): default caches. Fixed lane order, 64 lanes per wave."""
    if w.case not in _BASELINE:
        eng = make_engine(w)
        _BASELINE[w.case] = slice_records(eng)
        check(eng, w, w.want, "U44 baseline")
        eng.close()
    return _BASELINE[w.case]


def assert_same_slices(got, base, what):
    for k, (g, b) in enumerate(zip(got, base)):
        if not np.array_equal(g, b):
            lane = int(np.flatnonzero((g != b).any(axis=0))[0])
            raise AssertionError(f"{what}: slice {k}, lane {lane} (program {progfuzz.lane_program(lane, N_PROGRAMS)}): "
                                 f"(status, rip, icount) {[hex(int(v)) for v in g[:, lane]]}, "
                                 f"default {[hex(int(v)) for v in b[:, lane]]}")
    assert len(got) == len(base), f"{what}: {len(got)} slices, default {len(base)}"


@pytest.mark.parametrize("variant", ["cold-lds", "no-guc", "second-pass", "coverage-committed"])
@pytest.mark.parametrize("case", [INT_A, FP], ids=case_id)
def test_slice_length_is_path_independent(case, variant, workloads, monkeypatch):
    w = workloads(case)
    monkeypatch.setenv("WTFGPU_REGROUP_STEPS", "0")
    base = baseline_records(w)
    cov = True
    if variant == "cold-lds":
        monkeypatch.setenv("WTFGPU_WARM", "0")
    if variant == "no-guc":
        monkeypatch.setenv("WTFGPU_GUC", "0")
    eng = make_engine(w, code_pages=variant == "coverage-committed")
    if variant == "second-pass":
        assert_same_slices(slice_records(eng), base, "first pass")
        load_lanes(eng, w)
    if variant == "coverage-committed":
        eng.commit_coverage(set().union(*(x["cov"] for x in w.want)))
        load_lanes(eng, w)
        cov = False  # committing empties the per-lane new-coverage sets by design
    assert_same_slices(slice_records(eng), base, variant)
    check(eng, w, w.want, f"U44 {variant}", cov=cov)
    eng.close()


# ---------------------------------------------------------------------------
# 5. breakpoints, resume and mixed skip groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("regroup", [False, True], ids=["fixed-order", "regroup-64"])
@pytest.mark.parametrize("case", [INT_A, FP, EVEX], ids=case_id)
def test_breakpoints_with_mixed_skip_groups(case, regroup, workloads, monkeypatch):
    w = workloads(case)
    want = w.want_bp()
    assert sum(len(x["stops"]) for x in want) > N  # the breakpoints are hit
    if regroup:
        monkeypatch.setenv("WTFGPU_REGROUP_AUTO", "0")
    else:
        monkeypatch.setenv("WTFGPU_REGROUP_STEPS", "0")
    eng = make_engine(w, breakpoints=w.breakpoints())
    if regroup:
        eng.set_regroup(64)
    pos = [0] * N        # stops seen per lane
    held = []            # stopped lanes left alone for one more round
    tot = Totals()
    mixed = 0            # a fresh lane met a resumed (skip) lane at its breakpoint: see below
    before = eng.exits_np()
    skip_at = set()      # (wave, rip) of the lanes resumed with skip before the last slice
    bad = []
    for _ in range(64 * (LIMIT + 1) // 64 + 2 * N):
        tot.add(eng.run(max_steps=64))
        ex = eng.exits_np()
        stopped = [int(i) for i in np.flatnonzero(ex["status"] == EXIT_BREAKPOINT)]
        if not stopped and not (ex["status"] == RUNNING).any():
            break
        new = [i for i in stopped if i not in held]
        g = eng.read_gprs()
        for i in new:
            stops = want[i]["stops"]
            got = (int(ex["rip"][i]), int(ex["icount"][i]), [int(v) for v in g[i, :16]])
            if pos[i] >= len(stops) or got != stops[pos[i]]:
                bad.append((i, progfuzz.lane_program(i, N_PROGRAMS), pos[i], got,
                            stops[pos[i]] if pos[i] < len(stops) else None))
            pos[i] += 1
            # Fixed order, 64 lanes per wave: a group runs only when its rip is
            # the lowest of the wave's running lanes. A lane that was behind a
            # skip lane of its wave (lower rip, same program) when the slice
            # began and now stops at that lane's breakpoint reached it while
            # the skip lane still stood there: one group, skip set in a part.
            if not regroup:
                mixed += (i // 64, got[0]) in skip_at and int(before["rip"][i]) < got[0]
        assert not bad, f"{case_id(case)}: (lane, program, stop number, got, expected): {bad[:3]}"
        go = held + new[::2]   # every other new stop goes on now, the rest a round later
        held = new[1::2]
        eng.resume(go, [1] * len(go))
        skip_at = {(i // 64, int(ex["rip"][i])) for i in go}
        before = ex
    else:
        raise AssertionError("lanes still running or stopped after every possible round")
    assert pos == [len(x["stops"]) for x in want]
    check(eng, w, want, "breakpoints " + ("regroup-64" if regroup else "fixed-order"), retired=tot.retired)
    if not regroup:
        print(f"{case_id(case)}: {mixed} stops in a group with a skip lane")
        assert mixed > 0
    eng.close()


# ---------------------------------------------------------------------------
# 6. the finding of the evex case, reduced
# ---------------------------------------------------------------------------
def test_rep_stos_first_write_across_a_page_in_part_of_a_group():
    """rep stosq, 5 qwords, the first across a page edge, on the 64 lanes of one
    wave at one rip. Of every four lanes, two have written the first page only
    (the second page's copy-on-write sends them round the slow step's retry),
    one has written both (it finishes in its first attempt) and one crosses
    into the read-only page (#PF, nothing written). The evex case met this in
    program 10 and the retrying lanes lost their first qword (engine_ops.h,
    string_op). Every lane against the oracle, the window's bytes included."""
    from wtf_amd.engine import Engine
    from wtf_amd.tools.snapshot import AddressSpace, user_state

    n = 64
    code = bytes.fromhex("8803" "8802" "f348ab" "cc")  # mov [rbx], al; mov [rdx], al; rep stosq; int3
    sp = AddressSpace()
    sp.map_range(progfuzz.CODE_VA, code + b"\xcc" * (0x1000 - len(code)), write=False)
    sp.map_range(progfuzz.WIN_VA, bytes((7 * i + 1) & 0xFF for i in range(0x2000)), nx=True)
    sp.map(progfuzz.RO_VA, bytes(0x1000), write=False, nx=True)
    sp.map_range(progfuzz.STACK_VA, bytes(0x2000), nx=True)
    st = user_state(progfuzz.CODE_VA, progfuzz.STACK_TOP, sp.cr3)
    lanes = []
    for i in range(n):
        g = [0x0101010101010101 * (i + 1)] * 16
        g[4] = progfuzz.STACK_TOP
        g[1] = 5                                   # rcx
        g[3] = progfuzz.WIN_VA + 0x10 + i          # rbx: the first page
        g[2] = progfuzz.WIN_VA + (0x1010 if i % 4 == 3 else 0x20) + i   # rdx: the second page for every fourth lane
        g[7] = progfuzz.WIN_VA + (0x1FFC if i % 4 == 0 else 0xFFC)      # rdi: into the read-only page / across RW|RW
        lanes.append((progfuzz.CODE_VA, g, 0x202))
    want = progfuzz.oracle_run(sp, st, lanes, limit=LIMIT)
    assert {w["status"] for w in want} == {EXIT_FAULT, 3}
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=16, cov_entries=64)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(LIMIT)
    eng.restore()
    regs = eng.read_regs(0, n)
    for i, (va, g, flags) in enumerate(lanes):
        for k in range(16):
            regs[i].gpr[k] = g[k]
        regs[i].rip, regs[i].rflags = va, flags
    eng.write_regs(regs)
    eng.run()
    ex = eng.exits()
    out = eng.read_regs(0, n)
    bad = []
    for i, x in enumerate(want):
        e, r = ex[i], out[i]
        f = x["status"] == EXIT_FAULT
        if (e.status, r.rip, e.icount) != (x["status"], x["rip"], x["icount"]) or \
                (f and (e.vector, e.error, e.addr) != (x["vector"], x["error"], x["addr"])):
            bad.append((i, "exit", e.status, hex(r.rip), e.icount))
        elif [r.gpr[k] for k in range(16)] != x["gpr"]:
            bad.append((i, "regs"))
        elif set(eng.dirty(i)) != x["dirty"]:
            bad.append((i, "dirty"))
        elif eng.read_virt(i, progfuzz.WIN_VA, 0x2000) != x["win"]:
            got = eng.read_virt(i, progfuzz.WIN_VA, 0x2000)
            bad.append((i, "memory", [j for j in range(0x2000) if got[j] != x["win"][j]][:10]))
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:4]}"
    eng.close()
