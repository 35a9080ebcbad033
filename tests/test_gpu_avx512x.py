"""The AVX-512 integer forms of convention U49 on the GPU: the native vectors
of tests/test_avx512x.py one lane each, and the multi-instruction routines of
tests/golden/gen_avx512x_programs.py through k_run (uop cache, fast loop <->
generic step, the cold zmm state shared by both)."""
import pytest

from tests import vector_replay as V
from tests.avx512x_programs import PROGS, program_case, program_check, program_space
from tests.insn_cases import CODE_VA
from wtf_amd.abi import EXIT_INT3, EXIT_UNIMPLEMENTED, regs_from_state
from wtf_amd.tools.snapshot import user_state

pytestmark = pytest.mark.gpu


def test_gpu_matches_native_avx512x_vectors():
    """Every case one lane with GPRs, RFLAGS, zmm0-31, k0-7 and the 512-byte
    window across a page boundary; the guard cases (one of the two pages
    absent) in their own address spaces, one engine per guard value, as
    test_gpu_matches_native_avx512_vectors does."""
    cases = V.AVX512X.doc["cases"]
    fails = V.run_family(V.AVX512X, V.replay_gpu, cases)
    total = len(cases)
    assert total == len(V.AVX512X.doc["cases"])
    assert not fails, f"{len(fails)}/{total} mismatches, first: {fails[:6]}"


def test_gpu_runs_avx512x_programs():
    """320 lanes — one full 256-thread block and a partial one — each running one
    of the four routines at one of its 8 lengths, the lengths interleaved within
    every wave so its lanes leave their loops at different steps. Per lane: the
    int3 exit, the retired count the native run implies, both destination areas
    and the GPRs; no lane UNIMPLEMENTED."""
    from wtf_amd.engine import Engine

    n = 320
    lay = PROGS["layout"]
    buf_va = int(PROGS["buf_va"], 16)
    sp = program_space()
    eng = Engine(0)
    pfns, pblob = sp.phys()
    eng.load_pool(pfns, pblob)
    eng.alloc_lanes(n, overlay_pages=8, cov_entries=64)
    init = regs_from_state(user_state(CODE_VA, 0, sp.cr3))
    init.xcr0 = V.XCR0
    eng.set_initial_state(init)
    eng.set_limit(0)
    eng.restore()
    regs = eng.read_regs(0, n)
    names = list(PROGS["routines"])
    lanes, writes = [], []
    for i in range(n):
        routine = names[(i // 8) % len(names)]
        c = [c for c in PROGS["cases"] if c["routine"] == routine][i % 8]
        lanes.append(c)
        src = program_case(c, regs[i])
        writes.append((i, buf_va + lay["src"], src))
    # every wave holds all 8 lengths of each routine it runs
    assert all(len({(c["routine"], c["len"]) for c in lanes[w: w + 64]}) == 32 for w in range(0, n, 64))
    eng.write_regs(regs)
    eng.apply_writes(writes)
    eng.run()
    ex = eng.exits()
    out = eng.read_regs(0, n)
    assert sum(e.status == EXIT_UNIMPLEMENTED for e in ex[:n]) == 0
    fails = []
    for i, c in enumerate(lanes):
        e = ex[i]
        if e.status != EXIT_INT3:
            fails.append((i, c["routine"], c["len"], "exit", e.status, e.vector, hex(out[i].rip)))
            continue
        bad = program_check(c, e.icount, list(out[i].gpr), eng.read_virt(i, buf_va + lay["dst"], lay["area"]),
                            eng.read_virt(i, buf_va + lay["dst2"], lay["area"]))
        if bad:
            fails.append((i, c["routine"], c["len"]) + bad)
    assert not fails, f"{len(fails)}/{n} lanes, first: {fails[:6]}"
