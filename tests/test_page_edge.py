"""The native golden vectors with their memory operand on a page edge
(tests/vector_replay.py, "placements").

Ten families keep their window in the middle of one page, so their 13,110
cases with a memory operand of 2 to 32 bytes were never replayed where the
engine's memory path differs most from a flat model: vread / vwrite's two-page
branch, wide operands assembled from pieces, a miss on the second page that
restarts the whole instruction, a store that must probe both pages before it
writes either. Here each such case is replayed three more times, on the
oracle and on the engine's lane code built for the host (generic and through
the fast loop's forms); tests/test_gpu_page_edge.py does the same on the GPU:

  straddle  the operand's first `split` bytes end the first page; expected:
            the native result with its pointers moved (the family's check());
  absent    the same place, the second page not present: #PF at the page's
            first byte, error 4 (| 2 for a write), nothing retired, the mapped
            window unchanged, every register as the oracle leaves it;
  flush     the operand's last byte is the page's last byte, the second page
            absent; expected: the native result on the mapped bytes.

Every executor's byte count is compared with the oracle's for the same placed
case (native execution has none). The exemptions are tables in the harness,
none computed by the code under test: the aligned forms (#GP(0) at a
misaligned place: flush only), the address-dependent cases
(ADDRESS_DEPENDENT) and the byte-masked stores are judged equal to the oracle.

The avx2x gathers that load two or more elements run with their window 64,
128 and 192 bytes before the edge, so that their elements lie on two pages:
an attempt that misses the TLB restarts, and the attempt that retires must
still count the bytes and log the Tenet accesses of the elements earlier
attempts finished (U46).
"""
import collections
import functools

import pytest

from tests import simlane
from tests import vector_replay as V
from tests.insn_cases import get_ymm, layout, oracle_of, set_ymm
from tests.test_avx2x import GATHER_DD_L0
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, RUNNING

# placed cases per family: (straddle, absent, flush)
COUNTS = {
    "native": (1586, 1420, 1420), "sse": (804, 306, 804), "mmx": (660, 648, 660), "avx": (875, 805, 875),
    "fp": (2016, 1602, 2016), "sse4": (913, 614, 806), "ext": (704, 544, 704), "avx2x": (1452, 929, 929),
    "x87": (2721, 2721, 2721), "x87_directed": (1379, 1379, 1379),
}
# of the straddle placements: aligned forms, which end in #GP(0)
ALIGNED = {"native": 6, "sse": 498, "mmx": 12, "avx": 70, "fp": 414, "sse4": 192, "ext": 160, "avx2x": 0, "x87": 0,
           "x87_directed": 0}
# judged equal to the oracle because the result depends on the address: (straddle, flush)
ADDRESS = {"native": (30, 6), "ext": (21, 24)}
MASKED = {"mmx": 36}    # maskmovq at `absent`
FAM_KINDS = [(f, k) for f in V.PLACED for k in V.KINDS]


@functools.lru_cache(maxsize=2)
def placed(fam, kind):
    """(the family's placed cases of one kind, the oracle's Outcome of each)."""
    cases = V.placed_cases(fam, kind)
    return cases, list(V.replay_oracle(fam, cases))


def ids(fk):
    return f"{fk[0].name}-{fk[1]}"


@pytest.mark.parametrize("fk", FAM_KINDS, ids=ids)
def test_oracle_matches_native_on_the_page_edge(fk):
    fam, kind = fk
    cases, refs = placed(fam, kind)
    assert len(cases) == COUNTS[fam.name][V.KINDS.index(kind)]
    fails = [(c.get("name", fam.name), c["code"], c["at"].split) + bad
             for c, o in zip(cases, refs) if (bad := V.judge(fam, c, o, o))]
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"
    # the exemptions are exactly the tables: #GP(0) on the aligned forms and nowhere else
    gp = {c["index"] for c, o in zip(cases, refs) if (o.status, o.vector) == (EXIT_FAULT, 13)}
    aligned = {c["index"] for c in cases if c["at"].why == "aligned"}
    assert gp == aligned and len(aligned) == (ALIGNED[fam.name] if kind == "straddle" else 0)
    for c, o in zip(cases, refs):
        if c["at"].why == "aligned":
            assert (o.error, o.icount, o.rip) == (0, 0, o.entry), (c["name"], c["code"])
            assert V.reg_state(o.regs) == V.reg_state(o.initial) and o.mem in (None, o.window)
    why = collections.Counter(c["at"].why for c in cases)
    assert why["address"] == (0 if kind == "absent" else ADDRESS.get(fam.name, (0, 0))[kind == "flush"])
    assert why["masked"] == (MASKED.get(fam.name, 0) if kind == "absent" else 0)
    # an absent second page is what faults, wherever the derived expectation is not used either
    if kind == "absent":
        assert all(o.status == EXIT_FAULT and o.vector == 14 for c, o in zip(cases, refs) if c["at"].rule == "fault")
    else:
        assert all(o.status == RUNNING for c, o in zip(cases, refs) if c["at"].rule == "native" and
                   "trap_mx" not in c)


def test_the_exemption_tables_are_no_larger_than_stated():
    assert sum(a for a, _ in ADDRESS.values()) == 51 and sum(b for _, b in ADDRESS.values()) == 30
    assert sum(ALIGNED.values()) == 1352
    assert sum(s for s, _, _ in COUNTS.values()) == 13110
    assert len(V.ADDRESS_DEPENDENT) == 8 and all(why for why, _ in V.ADDRESS_DEPENDENT.values())


@pytest.mark.parametrize("fam", V.PLACED, ids=[f.name for f in V.PLACED])
def test_every_split_of_an_operand_length_occurs(fam):
    """Per (name prefix, access length) with enough placeable cases, the
    straddle placements take every split of the length."""
    seen, count = collections.defaultdict(set), collections.Counter()
    for c in V.placed_cases(fam, "straddle"):
        key = (c.get("name", c["code"]).split(".")[0], c["at"].access[2])
        seen[key].add(c["at"].split)
        count[key] += 1
        assert c["at"].split in V.splits(key[1]) and 0 < c["at"].split < key[1]
        assert c["at"].access[0] + c["at"].split == fam.page + 0x1000
    missing = {k: sorted(set(V.splits(k[1])) - s) for k, s in seen.items()
               if count[k] >= len(V.splits(k[1])) and s != set(V.splits(k[1]))}
    assert not missing, missing


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
@pytest.mark.parametrize("fk", FAM_KINDS, ids=ids)
def test_engine_code_matches_native_on_the_page_edge(fk, fast):
    fam, kind = fk
    cases, refs = placed(fam, kind)
    fails = V.run_placed(fam, V.replay_sim, cases, refs, fast=fast)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


# ---------------------------------------------------------------- gathers
@functools.lru_cache(maxsize=None)
def gather_cuts():
    cases = V.gather_cut_cases()
    return cases, list(V.replay_oracle(V.AVX2X, cases, tenet=True))


def test_gather_placements_are_the_ones_counted():
    cases, refs = gather_cuts()
    assert len(cases) == 1569
    assert sum(V.elements_on_both_pages(V.AVX2X, c) for c in cases) == 918


def test_oracle_gathers_match_native_across_the_edge():
    cases, refs = gather_cuts()
    fails = [(c["name"], c["code"], c["at"].split) + bad
             for c, o in zip(cases, refs) if (bad := V.judge(V.AVX2X, c, o, o))]
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"
    # a retired gather counts its instruction bytes once and every loaded element
    for c, o in zip(cases, refs):
        if "trap_mx" not in c:
            acc = V.tenet_accesses(o.tenet)
            assert o.nbytes == len(c["code"]) // 2 + sum(len(data) for _, _, data in acc), (c["name"], c["code"])


def test_engine_gathers_across_the_edge_count_every_element():
    """Registers, mask and destination against native; the byte count and the
    Tenet access list against the oracle's, however many attempts it took."""
    cases, refs = gather_cuts()
    fails = []
    for c, o, ref in zip(cases, V.replay_sim(V.AVX2X, cases, tenet=True), refs, strict=True):
        bad = V.judge(V.AVX2X, c, o, ref)
        if not bad and V.tenet_accesses(o.tenet) != V.tenet_accesses(ref.tenet):
            bad = ("tenet", len(V.tenet_accesses(o.tenet)), len(V.tenet_accesses(ref.tenet)))
        if bad:
            fails.append((c["name"], c["code"], c["at"].split) + bad)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


def test_gather_of_eight_straddling_elements_completes():
    """vpgatherdd ymm with each element across a page edge of its own: 16
    pages, 16 serviced misses (exec_retry's limit), one retired instruction."""
    sp, regs, want = V.gather8_case()
    o = oracle_of(sp)
    o.restore(regs)
    o.set_tenet(True)
    ex = o.run()
    assert (ex.status, o.icount()) == (EXIT_INT3, 1)
    simlane.lib().sim_set_tenet(V.TENET_CAP)
    out, fin, _ = simlane.run(sp, regs)
    buf = V.C.create_string_buffer(V.TENET_CAP)
    stream = buf.raw[:n] if (n := simlane.lib().sim_tenet(buf, V.TENET_CAP)) else b""
    simlane.lib().sim_set_tenet(0)
    assert (out.status, out.icount) == (EXIT_INT3, 1), (out.status, out.vector, out.error, hex(out.addr))
    for r in (o.regs(), fin):
        y = get_ymm(r)
        assert y[0:4] == [want[2 * q] | want[2 * q + 1] << 32 for q in range(4)]
        assert y[4:8] == [0] * 4
    assert out.nbytes == o.nbytes() == len(V.GATHER8_CODE) + 32
    assert stream == o.tenet()
    assert len(V.tenet_accesses(stream)) == 8


def test_gather_fault_keeps_the_done_elements_bytes_and_tenet():
    """tests/test_avx2x.py's test_gather_fault_keeps_the_done_elements layout
    (element 2 of 4 on an unmapped page, no IDT): the two finished elements'
    register writes stay, no bytes are counted, and the Tenet stream is the
    oracle's (the finished elements' accesses, then the registers)."""
    buf_va = 0x10000
    win = bytes(range(256))

    def setup(regs):
        regs.gpr[0] = buf_va
        y = [0] * 64
        y[0], y[1] = 0x1111111122222222, 0x3333333344444444
        y[4], y[5] = 0x8000000080000000, 0x8000000080000000
        y[8], y[9] = (1 << 32) | 0, (3 << 32) | 0x40000
        set_ymm(regs, y)
        return regs
    sp, regs = layout(GATHER_DD_L0, buf_va, win)
    o = oracle_of(sp)
    o.restore(setup(regs))
    o.set_tenet(True)
    ex = o.run()
    simlane.lib().sim_set_tenet(V.TENET_CAP)
    out, fin, _ = simlane.run(sp, regs)
    buf = V.C.create_string_buffer(V.TENET_CAP)
    stream = buf.raw[:n] if (n := simlane.lib().sim_tenet(buf, V.TENET_CAP)) else b""
    simlane.lib().sim_set_tenet(0)
    assert (ex.status, ex.vector, out.status, out.vector) == (EXIT_FAULT, 14, EXIT_FAULT, 14)
    assert get_ymm(fin)[:12] == get_ymm(o.regs())[:12]
    assert out.nbytes == o.nbytes() == 0
    assert stream == o.tenet()
    assert [(va, len(data)) for va, _, data in V.tenet_accesses(stream)] == [(buf_va, 4), (buf_va + 4, 4)]
