"""The shared-program generator (progfuzz.build_shared) on the CPU oracle alone.

tests/test_gpu_progfuzz_shared.py compares the engine's grouped execution with
the oracle on these programs. That comparison only reaches the group hazards
(partial misses, partial faults, partial page crossings, lanes of one group
dirtying different pages) if the lanes of a program really diverge in path, in
effective address and in how they end. The conditions below say so; they are
requirements on the generator, asserted for every (seed, sse, fp) the GPU
tests use, and the generator's constants and seeds were chosen to meet them.
"""
from collections import defaultdict

import pytest

from tests import progfuzz
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, EXIT_TIMEOUT, RUNNING, regs_from_state

N_LANES, N_PROGRAMS, LIMIT = 512, 16, 2000


def lane_trace(sp, st, lanes, i, kw, limit=LIMIT):
    """[(rip, status, vector, error after the step)] of lane i, by Oracle.step()."""
    from tests.oracle_lib import Oracle

    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    va, regs, flags = lanes[i]
    r = regs_from_state(st)
    for k in range(16):
        r.gpr[k] = regs[k]
        if kw:
            r.xmm[k][0], r.xmm[k][1] = kw["xmm"][i][2 * k], kw["xmm"][i][2 * k + 1]
            r.ymmh[k][0], r.ymmh[k][1] = kw["ymmh"][i][2 * k], kw["ymmh"][i][2 * k + 1]
    if kw:
        r.mxcsr = kw["mxcsr"][i]
    r.rip, r.rflags = va, flags
    o.restore(regs_from_state(st))
    o.set_regs(r)
    o.set_limit(limit)
    out = []
    for _ in range(limit + 1):
        rip = o.regs().rip
        ex = o.step()
        out.append((rip, ex.status, ex.vector, ex.error))
        if ex.status != RUNNING:
            break
    return out


def partial_write_fault(sp, st, lanes, kw, want, members):
    """A (faulting lane, passing lane, rip) of one program: the first takes #PF
    on a write at rip, the second retires the instruction at the same rip.
    Both read from step() traces. None if the program has no such pair."""
    for a in members:
        w = want[a]
        if not (w["status"] == EXIT_FAULT and w["vector"] == 14 and w["error"] & 2):
            continue
        ta = lane_trace(sp, st, lanes, a, kw)
        rip, status, vector, error = ta[-1]
        assert (status, vector, error & 2) == (EXIT_FAULT, 14, 2) and rip == w["rip"]
        for b in members:
            if b == a or rip not in want[b]["cov"]:
                continue
            if want[b]["status"] == EXIT_FAULT and want[b]["rip"] == rip:
                continue  # it may have passed in an earlier loop iteration; lanes that end elsewhere suffice
            if any(r == rip and s == RUNNING for r, s, _, _ in lane_trace(sp, st, lanes, b, kw)):
                return a, b, rip
    return None


def shared_figures(seed, sse, fp):
    sp, st, lanes, progs = progfuzz.build_shared_info(N_LANES, N_PROGRAMS, seed, sse=sse, fp=fp)
    kw = {}
    if sse:
        kw = dict(xmm=progfuzz.lane_xmm(N_LANES, seed), ymmh=progfuzz.lane_xmm(N_LANES, seed, 0x4E4),
                  mxcsr=progfuzz.lane_mxcsr(N_LANES, seed))
    want = progfuzz.oracle_run(sp, st, lanes, limit=LIMIT, **kw)
    members = defaultdict(list)
    for i in range(N_LANES):
        members[progfuzz.lane_program(i, N_PROGRAMS)].append(i)
    ends = {p["va"]: p["end"] for p in progs}
    fig = {
        "int3": sum(w["status"] == EXIT_INT3 and w["rip"] == ends[lanes[i][0]] for i, w in enumerate(want)),
        "timeout": sum(w["status"] == EXIT_TIMEOUT for w in want),
        "retired": 0, "dirty": 0, "ends": 0, "partial_pf": [],
    }
    for p, ms in sorted(members.items()):
        fig["retired"] += len({want[i]["icount"] for i in ms}) >= 2
        fig["dirty"] += len({frozenset(want[i]["dirty"]) for i in ms}) >= 2
        faults = {want[i]["rip"] for i in ms if want[i]["status"] == EXIT_FAULT}
        clean = any(want[i]["status"] != EXIT_FAULT for i in ms)
        fig["ends"] += (bool(faults) and clean) or len(faults) >= 2
        hit = partial_write_fault(sp, st, lanes, kw, want, ms)
        if hit:
            fig["partial_pf"].append((p,) + hit)
    return fig, (sp, st, lanes, want, members)


@pytest.mark.parametrize("seed,sse,fp", progfuzz.SHARED_CASES)
def test_shared_programs_diverge_inside_their_groups(seed, sse, fp):
    fig, _ = shared_figures(seed, sse, fp)
    print(f"seed {seed} sse {sse} fp {fp}: {fig}")
    assert 3 * fig["int3"] >= N_LANES, "at least one third of the lanes end at the final int3"
    assert 4 * fig["timeout"] <= N_LANES, "at most one quarter end in the timeout"
    assert 2 * fig["retired"] >= N_PROGRAMS, "half of the programs: lanes with different retired counts"
    assert 4 * fig["dirty"] >= N_PROGRAMS, "a quarter of the programs: lanes with different dirty-page sets"
    assert 4 * fig["ends"] >= N_PROGRAMS, "a quarter of the programs: lanes that end differently"
    assert fig["partial_pf"], "a program where one lane takes #PF on a write and another passes the same rip"


def test_shared_layout():
    """Lane i runs program (i // 4) % n_programs: every 16 consecutive lanes
    (the smallest wave) hold 4 programs, 4 lanes of each, with registers of
    their own; build_shared returns what build returns."""
    sp, st, lanes, progs = progfuzz.build_shared_info(N_LANES, N_PROGRAMS, 1)
    sp2, st2, lanes2 = progfuzz.build_shared(N_LANES, N_PROGRAMS, 1)
    assert lanes2 == lanes and st2 == st and sp2.phys() == sp.phys()
    assert len(progs) == N_PROGRAMS and all(p["blocks"] for p in progs)
    for w in range(0, N_LANES, 16):
        vas = [lanes[i][0] for i in range(w, w + 16)]
        assert len(set(vas)) == 4 and all(vas.count(v) == 4 for v in set(vas))
    assert len({tuple(l[1]) for l in lanes}) == N_LANES  # registers stay per lane
