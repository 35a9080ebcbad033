"""k_run on the native golden vectors with their memory operand on a page edge
(tests/test_page_edge.py explains the placements and what each is held to).

One test per family: every placed case is one lane, its window written at its
own place with apply_writes, in two address spaces: both pages present (the
straddle placements) and the second page absent (absent and flush). Judged as
on the CPU: the moved native result through the family's check(), the derived
#PF, equality with the oracle for the exempt cases, and the byte count
against the oracle's. One more test runs the gathers with their elements on
two pages (registers, memory, byte count), and the gather of eight elements
that each cross a page edge of their own.
"""
import pytest

from tests import vector_replay as V
from tests.insn_cases import get_ymm, oracle_of
from wtf_amd.abi import EXIT_INT3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fam", V.PLACED, ids=[f.name for f in V.PLACED])
def test_gpu_matches_native_on_the_page_edge(fam):
    cases = [c for kind in V.KINDS for c in V.placed_cases(fam, kind)]
    refs = list(V.replay_oracle(fam, cases))
    fails = V.run_placed(fam, V.replay_gpu, cases, refs)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:6]}"


def test_gpu_gathers_across_the_edge_count_every_element():
    from wtf_amd.engine import Engine

    cases = V.gather_cut_cases()
    assert len(cases) == 1569
    refs = list(V.replay_oracle(V.AVX2X, cases))
    fails = V.run_placed(V.AVX2X, V.replay_gpu, cases, refs)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:6]}"
    # eight elements, each across a page edge of its own (16 serviced misses)
    sp, regs, want = V.gather8_case(V.GPU_CODE_VA, nx=True)
    o = oracle_of(sp)
    o.restore(regs)
    assert o.run().status == EXIT_INT3
    eng = Engine(0)
    try:
        eng.load_pool(*sp.phys())
        eng.alloc_lanes(64, overlay_pages=4, cov_entries=64)
        eng.set_initial_state(regs)
        eng.set_limit(0)
        eng.restore()
        eng.run()
        ex, out, nb = eng.exits(), eng.read_regs(0, 64), eng.nbytes()
    finally:
        eng.close()
    for i in range(64):
        assert (ex[i].status, ex[i].icount, int(nb[i])) == (EXIT_INT3, 1, o.nbytes()), (i, ex[i].status, ex[i].vector)
        assert get_ymm(out[i])[:12] == get_ymm(o.regs())[:12], i
    assert get_ymm(out[0])[0:4] == [want[2 * q] | want[2 * q + 1] << 32 for q in range(4)]
