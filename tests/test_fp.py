"""SSE / AVX floating point (conventions U39 / U40; engine_ssefp.h / engine_fp.h,
oracle/x86_oracle_fp.inc).

Native-execution vectors (tests/golden/gen_fp_vectors.py: legacy and VEX
forms, special values, every rounding mode, DAZ / FTZ, sticky flags, unmasked
exceptions that trap) pin the oracle (which runs the instruction on the host
CPU in register form, around its own decode, checks and memory access) and
the engine's own device code built for the host (tests/native/sim_lane.cc,
the integer arithmetic of engine_fp.h). The GPU runs the same vectors in
tests/test_gpu_sse.py. The #UD / #NM / #GP rules native execution cannot show
are hand-checked below.
"""
import pytest

from tests.insn_cases import norm, run_case
from tests.vector_replay import FP, VEC_XM, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, RUNNING

DOC = FP.doc


@pytest.mark.parametrize("chunk", range(4))
def test_oracle_matches_native_fp(chunk):
    cases = DOC["cases"][chunk::4]
    fails = run_family(FP, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


def test_engine_fp_code_matches_native_vectors():
    fails = run_family(FP, replay_sim, DOC["cases"])
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:5]}"


def test_fp_vector_file_is_substantial():
    cases = DOC["cases"]
    assert len(cases) > 5000
    assert sum("trap_mx" in c for c in cases) > 100  # unmasked exceptions
    names = {c["name"].split(".")[0] for c in cases}
    for n in ("addps", "sqrtsd", "divss", "minpd", "cmpps", "comiss", "ucomisd", "cvtsd2ss", "cvttps2dq", "cvtsi2sd",
              "cvtss2si", "haddps", "addsubpd", "movddup", "roundsd", "blendvps", "vaddps", "vcmpsd", "vcvtpd2ps",
              "vroundps", "vblendvpd", "vtcvtsd2si"):
        assert n in names, n


# ---- hand-checked: what native execution cannot show
FP_FAULT_CASES = [
    # legacy packed operands need 16-byte alignment, scalar ones do not
    ([0x0F, 0x58, 0x06], EXIT_FAULT, 13),                    # addps xmm0, [rsi] (misaligned)
    ([0xF3, 0x0F, 0x58, 0x06], RUNNING, None),               # addss xmm0, [rsi]
    ([0x66, 0x0F, 0x5A, 0x06], EXIT_FAULT, 13),              # cvtpd2ps xmm0, [rsi]
    ([0x0F, 0x5A, 0x06], RUNNING, None),                     # cvtps2pd xmm0, [rsi] (m64)
    ([0xF2, 0x0F, 0x12, 0x06], RUNNING, None),               # movddup xmm0, [rsi] (m64)
    ([0xF3, 0x0F, 0x12, 0x06], EXIT_FAULT, 13),              # movsldup xmm0, [rsi] (m128)
    ([0xF2, 0x0F, 0xF0, 0x06], RUNNING, None),               # lddqu xmm0, [rsi]
    ([0xF2, 0x0F, 0xF0, 0xC1], EXIT_FAULT, 6),               # lddqu xmm0, xmm1: memory only
    ([0xC5, 0xFC, 0x58, 0x06], RUNNING, None),               # vaddps ymm0, ymm0, [rsi]: VEX needs no alignment
    ([0xC5, 0xF8, 0x51, 0xC1], RUNNING, None),               # vsqrtps xmm0, xmm1
    ([0xC5, 0xF0, 0x51, 0xC1], EXIT_FAULT, 6),               # vsqrtps with vvvv != 1111
    ([0xC5, 0xF0, 0x2F, 0xC1], EXIT_FAULT, 6),               # vcomiss with vvvv != 1111
    ([0xC5, 0xF2, 0x58, 0xC1], RUNNING, None),               # vaddss xmm0, xmm1, xmm1
    ([0xC4, 0xE3, 0xF1, 0x4A, 0xC2, 0x30], EXIT_FAULT, 6),   # vblendvps with VEX.W = 1
    ([0xC4, 0xE3, 0x71, 0x4A, 0xC2, 0x30], RUNNING, None),   # vblendvps xmm0, xmm1, xmm2, xmm3
    ([0x66, 0xC5, 0xF8, 0x58, 0xC1], EXIT_FAULT, 6),         # 66 before VEX
    ([0x66, 0x0F, 0x3A, 0x40, 0xC1, 0xFF], RUNNING, None),   # dpps
    ([0x66, 0x0F, 0x3A, 0x41, 0x06, 0x33], EXIT_FAULT, 13),  # dppd xmm0, [rsi]: legacy needs alignment
    ([0xC4, 0xE3, 0x7D, 0x40, 0x06, 0xFF], RUNNING, None),   # vdpps ymm0, ymm0, [rsi]
    ([0x0F, 0x53, 0xC1], RUNNING, None),                     # rcpps
    ([0x0F, 0x52, 0x06], EXIT_FAULT, 13),                    # rsqrtps xmm0, [rsi]: legacy needs alignment
    ([0xC5, 0xF0, 0x53, 0xC1], EXIT_FAULT, 6),               # vrcpps with vvvv != 1111
    ([0xC5, 0xF2, 0x52, 0x06], RUNNING, None),               # vrsqrtss xmm0, xmm1, [rsi]
    ([0x0F, 0x2A, 0xC1], RUNNING, None),                     # cvtpi2ps xmm0, mm1 (tests/test_mmx.py)
    ([0x0F, 0x2D, 0xC1], RUNNING, None),                     # cvtps2pi mm0, xmm1
    ([0xC5, 0xF8, 0x2A, 0xC1], EXIT_FAULT, 6),               # no VEX form
]


@pytest.mark.parametrize("code,status,vector", FP_FAULT_CASES)
def test_fp_faults_oracle_and_engine(code, status, vector):
    for got in (run_case(code), run_case(code, sim=True)):
        assert norm(got[0]) == status, (bytes(code).hex(), got[:2])
        if vector is not None:
            assert got[1] == vector


def test_fp_gating_and_unmasked_exceptions():
    """#UD (CR0.EM / !CR4.OSFXSR), #NM (CR0.TS), and an unmasked exception:
    #XM with CR4.OSXMMEXCPT, #UD without it; the flags land in MXCSR, the
    destination keeps its value."""
    divps = [0x0F, 0x5E, 0xC1]  # divps xmm0, xmm1: 1 / 0 raises ZE
    one, zero = (0x3F8000003F800000, 0x3F8000003F800000), (0, 0)
    for sim in (False, True):
        assert run_case(divps, sim, cr0=0x80050037)[:2] == (EXIT_FAULT, 6)   # EM
        assert run_case(divps, sim, cr4=0x370478)[:2] == (EXIT_FAULT, 6)     # !OSFXSR
        assert run_case(divps, sim, cr0=0x8005003B)[:2] == (EXIT_FAULT, 7)   # TS
        st, vec, mx, x = run_case(divps, sim, mx=0x1F80 & ~0x200, xmm={0: one, 1: zero})
        assert (st, vec, mx, x[0]) == (EXIT_FAULT, VEC_XM, 0x1D84, one)
        st, vec, mx, x = run_case(divps, sim, cr4=0x370278, mx=0x1F80 & ~0x200, xmm={0: one, 1: zero})
        assert (st, vec, mx) == (EXIT_FAULT, 6, 0x1D84)
        st, vec, mx, x = run_case(divps, sim, xmm={0: one, 1: zero})  # masked: infinities, ZE set
        assert norm(st) == RUNNING and mx == 0x1F84 and x[0] == (0x7F8000007F800000, 0x7F8000007F800000)
