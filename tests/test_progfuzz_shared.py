"""The shared-program generator (progfuzz.build_shared) on the CPU oracle alone.

tests/test_gpu_progfuzz_shared.py compares the engine's grouped execution with
the oracle on these programs. That comparison only reaches the group hazards
(partial misses, partial faults, partial page crossings, lanes of one group
dirtying different pages) if the lanes of a program really diverge in path, in
effective address and in how they end. The conditions below say so; they are
requirements on the generator, asserted for every (seed, sse, fp, evex) the GPU
tests use, and the generator's constants and seeds were chosen to meet them.
The evex case has conditions of its own on top (evex_figures): the AVX-512
forms must really be retired, family by family, with different masks in the
lanes of a group, and a masked store must fault, be suppressed and cross a
page edge in three lanes at one rip.
"""
import functools
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
    progfuzz.set_lane_state(r, i, **kw)
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


@functools.lru_cache(maxsize=None)
def shared_figures(seed, sse, fp, evex=False):
    sp, st, lanes, progs = progfuzz.build_shared_info(N_LANES, N_PROGRAMS, seed, sse=sse, fp=fp, evex=evex)
    kw = progfuzz.lane_state(N_LANES, seed, sse, evex)
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
    return fig, (sp, st, lanes, want, members, progs, kw)


def _case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}" + ("-evex" if c[3] else "")


@pytest.mark.parametrize("seed,sse,fp,evex", progfuzz.SHARED_CASES, ids=[_case_id(c) for c in progfuzz.SHARED_CASES])
def test_shared_programs_diverge_inside_their_groups(seed, sse, fp, evex):
    fig, _ = shared_figures(seed, sse, fp, evex)
    print(f"seed {seed} sse {sse} fp {fp} evex {evex}: {fig}")
    assert 3 * fig["int3"] >= N_LANES, "at least one third of the lanes end at the final int3"
    assert 4 * fig["timeout"] <= N_LANES, "at most one quarter end in the timeout"
    assert 2 * fig["retired"] >= N_PROGRAMS, "half of the programs: lanes with different retired counts"
    assert 4 * fig["dirty"] >= N_PROGRAMS, "a quarter of the programs: lanes with different dirty-page sets"
    assert 4 * fig["ends"] >= N_PROGRAMS, "a quarter of the programs: lanes that end differently"
    assert fig["partial_pf"], "a program where one lane takes #PF on a write and another passes the same rip"


# ---------------------------------------------------------------------------
# the EVEX case
# ---------------------------------------------------------------------------
_RO_PAGE = progfuzz.RO_VA >> 12
_RW_EDGES = (progfuzz.WIN_VA + 0x1000, progfuzz.WIN2_VA + 0x1000)  # a writable page on either side
_MAPPED = set(range(progfuzz.WIN_VA >> 12, (progfuzz.WIN2_VA + progfuzz.WIN2_LEN) >> 12))


def evex_figures(sp, st, lanes, members, progs, kw):
    """Every lane stepped through the oracle, each step at an EVEX-pool rip
    (progs[p]["evex"]) judged from the registers before it and its status:
      unimplemented  lanes that end UNIMPLEMENTED
      ten            lanes that retire 10 or more EVEX-encoded instructions
      families       per family of progfuzz.EVEX_FAMILIES, the programs with a lane that retires it
      masks          programs where two lanes reach one masked instruction with different mask values
      triples        (program, rip, faulting lane, suppressed lane, crossing lane) of a masked store:
                     #PF with a selected element on the read-only or an absent page; retired with every
                     element on such a page masked off; retired with selected elements on both sides
                     of an RW|RW edge.
    """
    from tests.oracle_lib import Oracle
    from wtf_amd.abi import EXIT_UNIMPLEMENTED

    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    o.set_limit(LIMIT)
    fig = {"unimplemented": 0, "ten": 0, "families": {f: set() for f in progfuzz.EVEX_FAMILIES}, "masks": 0,
           "triples": []}
    for p, ms in sorted(members.items()):
        meta = progs[p]["evex"]
        seen = defaultdict(lambda: defaultdict(set))      # rip -> mask value -> lanes
        roles = defaultdict(lambda: defaultdict(list))    # rip -> "pf" / "suppressed" / "crossing" -> lanes
        for i in ms:
            va, regs, flags = lanes[i]
            r = regs_from_state(st)
            for k in range(16):
                r.gpr[k] = regs[k]
            progfuzz.set_lane_state(r, i, **kw)
            r.rip, r.rflags = va, flags
            o.restore(regs_from_state(st))
            o.set_regs(r)
            retired = 0
            for _ in range(LIMIT + 1):
                before = o.regs()
                m = meta.get(before.rip)
                ex = o.step()
                if m is not None:
                    ok = ex.status == RUNNING
                    retired += ok and m["fam"] != "vex" and m["fam"] != "U47.k"
                    if ok and m["fam"] in fig["families"]:
                        fig["families"][m["fam"]].add(p)
                    if m["aaa"]:
                        kv = before.k[m["aaa"]] & ((1 << m["n"]) - 1)
                        seen[before.rip][kv].add(i)
                        if m["store"]:
                            base, index, ss, disp = m["ea"]
                            ea = (before.gpr[base] + ((before.gpr[index] << ss) if index is not None else 0) + disp) \
                                & 0xFFFFFFFFFFFFFFFF
                            es = m["es"]
                            sel = [ea + j * es + b for j in range(m["n"]) if (kv >> j) & 1 for b in (0, es - 1)]
                            off = [ea + j * es + b for j in range(m["n"]) if not (kv >> j) & 1 for b in (0, es - 1)]
                            bad = lambda a: (a >> 12) == _RO_PAGE or (a >> 12) not in _MAPPED  # noqa: E731
                            if ex.status == EXIT_FAULT and ex.vector == 14 and ex.error & 2 and any(bad(a) for a in sel):
                                roles[before.rip]["pf"].append(i)
                            elif ok and any(bad(a) for a in off) and not any(bad(a) for a in sel):
                                roles[before.rip]["suppressed"].append(i)
                            elif ok and any(min(sel, default=e) < e <= max(sel, default=0) for e in _RW_EDGES):
                                roles[before.rip]["crossing"].append(i)
                if ex.status != RUNNING:
                    fig["unimplemented"] += ex.status == EXIT_UNIMPLEMENTED
                    break
            fig["ten"] += retired >= 10
        fig["masks"] += any(len(v) >= 2 and len(set().union(*v.values())) >= 2 for v in seen.values())
        for rip, rl in sorted(roles.items()):
            if rl["pf"] and rl["suppressed"] and rl["crossing"]:
                fig["triples"].append((p, rip, rl["pf"][0], rl["suppressed"][0], rl["crossing"][0]))
    return fig


@pytest.mark.parametrize("seed,sse,fp,evex", [c for c in progfuzz.SHARED_CASES if c[3]],
                         ids=[_case_id(c) for c in progfuzz.SHARED_CASES if c[3]])
def test_evex_programs_reach_the_masked_hazards(seed, sse, fp, evex):
    _, (sp, st, lanes, want, members, progs, kw) = shared_figures(seed, sse, fp, evex)
    fig = evex_figures(sp, st, lanes, members, progs, kw)
    print(f"seed {seed}: unimplemented {fig['unimplemented']}, lanes with 10 or more EVEX instructions {fig['ten']}, "
          f"programs per family { {f: len(v) for f, v in fig['families'].items()} }, "
          f"programs with differing masks {fig['masks']}, triples {fig['triples']}")
    assert fig["unimplemented"] == 0, "no lane ends UNIMPLEMENTED"
    assert 2 * fig["ten"] >= N_LANES, "half of the lanes retire 10 or more EVEX instructions"
    for fam, ps in fig["families"].items():
        assert len(ps) >= 2, f"family {fam} is retired by lanes of at least two programs"
    assert fig["triples"], "a masked store that faults, is suppressed and crosses an RW|RW edge in three lanes at one rip"
    assert 4 * fig["masks"] >= N_PROGRAMS, "a quarter of the programs: one masked instruction, different mask values"


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
