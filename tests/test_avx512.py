"""The AVX-512 subset (convention U47; engine_avx512.h, oracle/x86_oracle_avx512.inc).

Native-execution vectors (tests/golden/gen_avx512_vectors.py, run on an
AVX512F / BW / VL / DQ host) pin the oracle and the engine's device code built
for the host: GPRs, RFLAGS, zmm0-31, k0-7 and a 512-byte window across a page
boundary, and for the faulting cases the vector, the page-fault error code and
CR2 (memory fault suppression: "guard" cases whose second page is absent).
The GPU runs the same vectors in tests/test_gpu_sse.py.
"""
import pytest

from tests import simlane
from tests.insn_cases import CODE_VA, oracle_of
from tests.vector_replay import AVX512, XCR0, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

DOC = AVX512.doc


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_native_avx512(chunk):
    cases = DOC["cases"][chunk::2]
    fails = run_family(AVX512, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


@pytest.mark.parametrize("fast", [False, True], ids=["exec", "fast"])
def test_engine_avx512_code_matches_native_vectors(fast):
    """The engine's decode / exec built for the host (tests/native/sim_lane.cc);
    fast=True goes through k_run's fast-loop digest first (EVEX stays generic)."""
    fails = run_family(AVX512, replay_sim, DOC["cases"], fast=fast)
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:5]}"


def test_avx512_vector_file_is_substantial():
    cases = DOC["cases"]
    names = {c["name"].split(".")[0] for c in cases}
    assert len(cases) > 2500
    for n in ("vmovdqu8", "vmovdqu16", "vmovdqu32", "vmovdqu64", "vmovdqa32", "vmovdqa64", "vmovups", "vmovapd",
              "vpternlogd", "vpternlogq", "vpcmpub", "vpcmpq", "vptestnmb", "vpbroadcastq", "vpminuw", "vpcmpeqb",
              "kmovq", "kortestd", "ktestb", "kshiftlq", "kxnorw", "knotb"):
        assert n in names, n
    # memory fault suppression was exercised both ways: guard cases that fault and that complete
    guard = [c for c in cases if c["guard"]]
    assert sum("fault" in c for c in guard) > 20 and sum("fault" not in c for c in guard) > 20
    # the #UD rules and the aligned forms' #GP were met natively
    assert sum(c.get("fault", {}).get("vec") == 6 for c in cases) > 100
    assert sum(c.get("fault", {}).get("vec") == 13 for c in cases) > 20
    # every vector length and zmm16-31 appear
    assert {c["name"].split(".")[1] for c in cases if c["name"].startswith("vp")} >= {"L0", "L1", "L2"}


def _cpuid(leaf, sub, xcr0=XCR0):
    sp = AddressSpace()
    sp.map_range(CODE_VA, bytes([0x0F, 0xA2, 0xCC]), write=False)
    regs = regs_from_state(user_state(CODE_VA, 0, sp.cr3))
    regs.gpr[0], regs.gpr[1] = leaf, sub
    regs.xcr0 = xcr0
    o = oracle_of(sp)
    o.restore(regs)
    o.step()
    return list(o.regs().gpr)


def test_avx512_disabled_by_xcr0_is_ud():
    """With XCR0[7:5] clear (a guest that never enabled the AVX-512 state) every
    EVEX form and the opmask instructions are #UD, engine and oracle."""
    c = next(c for c in DOC["cases"] if c["name"].startswith("vpaddd") and "fault" not in c)
    k = next(c for c in DOC["cases"] if c["name"].startswith("kandw") and "fault" not in c)
    for case in (c, k):
        for xcr0 in (0x7, 0x1F, 0x67):
            regs = regs_from_state(user_state(CODE_VA, 0, AddressSpace().cr3))
            win = AVX512.setup(case, regs)
            regs.xcr0 = xcr0
            sp = AVX512.space(bytes.fromhex(case["code"]) + b"\xcc", CODE_VA, win, 0)
            o = oracle_of(sp)
            o.restore(regs)
            ex = o.step()
            assert (ex.status, ex.vector) == (EXIT_FAULT, 6), (case["name"], xcr0)
            out, _, _ = simlane.run(sp, regs)
            assert (out.status, out.vector) == (EXIT_FAULT, 6), (case["name"], xcr0)


def test_cpuid_enumerates_avx512_f_bw_vl():
    g = _cpuid(7, 0)
    ebx = g[3]
    assert ebx & (1 << 16) and ebx & (1 << 30) and ebx & (1 << 31)
