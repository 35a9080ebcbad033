"""MMX (U37): the oracle and the engine's code built for the host
(tests/native/sim_lane.cc) against native-execution vectors
(tests/golden/gen_mmx_vectors.py: GPRs, RFLAGS, XMM, mm0-7, FSW and the
abridged tag byte after the instruction, the memory window), then the rules
native execution cannot show: #UD / #NM / #MF and the TOS rotation. The GPU
runs the same vectors in tests/test_gpu_sse.py."""
import pytest

from tests import simlane
from tests.insn_cases import layout, oracle_of
from tests.vector_replay import MMX, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, RUNNING

DOC = MMX.doc
BUF = MMX.buf_va


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_native_mmx(chunk):
    cases = DOC["cases"][chunk::2]
    fails = run_family(MMX, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:6]}"


def test_mmx_vector_file_is_substantial():
    assert len(DOC["cases"]) > 1500
    names = {c["name"].split(".")[0] for c in DOC["cases"]}
    for n in ("m60", "m6f", "mfe", "pshufw", "shimm", "movq", "movntq", "movd", "pextrw", "pinsrw", "pmovmskb",
              "movq2dq", "movdq2q", "emms"):
        assert n in names, n


def test_engine_mmx_code_matches_native_vectors():
    fails = run_family(MMX, replay_sim, DOC["cases"])
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:6]}"


# ---- hand-checked: the rules native execution cannot show
FAULT_CASES = [
    ([0x0F, 0xFC, 0xC1], dict(cr0=0x80050031 | 4), EXIT_FAULT, 6),    # CR0.EM: #UD
    ([0x0F, 0xFC, 0xC1], dict(cr0=0x80050031 | 8), EXIT_FAULT, 7),    # CR0.TS: #NM
    ([0x0F, 0xFC, 0xC1], dict(fsw=0x8081, fcw=0x37E), EXIT_FAULT, 16),  # an unmasked flag pending: #MF
    ([0x0F, 0x77], dict(fsw=0x8081, fcw=0x37E), EXIT_FAULT, 16),      # emms too
    ([0x0F, 0x77], dict(fsw=0x0001, fcw=0x37E), EXIT_FAULT, 16),      # the host's rule: ES not needed
    ([0x0F, 0x77], dict(fsw=0x0080, fcw=0x37F), RUNNING, None),       # ES with every flag masked: none
    ([0x0F, 0x73, 0xD9, 0x01], {}, EXIT_FAULT, 6),                    # psrldq has no MMX form
    ([0x0F, 0x71, 0xC1, 0x01], {}, EXIT_FAULT, 6),                    # 71 /0
    ([0x0F, 0x71, 0x16, 0x01], {}, EXIT_FAULT, 6),                    # shift-by-imm of memory
    ([0x0F, 0xD7, 0x06], {}, EXIT_FAULT, 6),                          # pmovmskb of memory
    ([0x0F, 0xE7, 0xC1], {}, EXIT_FAULT, 6),                          # movntq to a register
    ([0x0F, 0xD6, 0xC1], {}, EXIT_FAULT, 6),                          # 0f d6 without a prefix
    ([0x0F, 0xF7, 0xC1], {}, RUNNING, None),                          # maskmovq, no byte selected (U37)
    ([0x0F, 0xF7, 0x06], {}, EXIT_FAULT, 6),                          # maskmovq with a memory operand
    ([0x0F, 0x2A, 0xC1], {}, RUNNING, None),                          # cvtpi2ps xmm0, mm1
    ([0x0F, 0x2A, 0xC1], dict(fsw=0x8081, fcw=0x37E), EXIT_FAULT, 16),  # an mm source: #MF first
    ([0x0F, 0x2A, 0x06], dict(fsw=0x8081, fcw=0x37E), RUNNING, None),   # an m64 source: no x87 state touched
    ([0x0F, 0x2D, 0xC1], dict(fsw=0x8081, fcw=0x37E), EXIT_FAULT, 16),  # cvtps2pi: an mm destination
    ([0x66, 0x0F, 0x2D, 0x06], {}, EXIT_FAULT, 13),                   # cvtpd2pi mm0, [rsi]: m128 needs alignment
    ([0x0F, 0x38, 0x01, 0xC1], {}, RUNNING, None),                    # phaddw mm (SSSE3 on mm registers, U41)
    ([0x0F, 0x38, 0x01, 0xC1], dict(fsw=0x8081, fcw=0x37E), EXIT_FAULT, 16),  # ... #MF first
    ([0x0F, 0x38, 0x0C, 0xC1], {}, EXIT_FAULT, 6),                    # 0f 38 0c without 66: no instruction (U36)
]


def run_one(code, sim=False, cr0=None, fsw=0, tos=0, fptw=0xFFFF, mm=None, fcw=0x37F):
    sp, regs = layout(bytes(code), BUF, bytes(range(256)), cr0=cr0)
    regs.gpr[6] = BUF + 0x13
    regs.fpcw = fcw
    regs.fpsw = fsw | (tos << 11)
    regs.fptw = fptw
    for i in range(8):
        regs.fpst[i] = mm[i] if mm else 0x1111111111111111 * (i + 1)
    o = oracle_of(sp)
    o.restore(regs)
    ex = o.step()
    return ex, o.regs(), simlane.run(sp, regs)[:2] if sim else None


@pytest.mark.parametrize("code,kw,status,vector", FAULT_CASES)
def test_mmx_faults_oracle_and_engine(code, kw, status, vector):
    ex, _, (out, _) = run_one(code, True, **kw)
    assert (ex.status, ex.vector if vector else None) == (status, vector), bytes(code).hex()
    want = 3 if status == RUNNING else status
    assert (out.status, out.vector if vector else None) == (want, vector)


def test_tos_rotation_and_tags():
    """paddb mm1, mm2 with TOS = 3: mm i is ST((i - 3) & 7) = fpst[(i - 3) & 7]
    before; after, TOS = 0, fpst is in R order and every tag valid; emms
    then empties the tags and keeps the values."""
    mm = [0x0101010101010101 * (i + 1) for i in range(8)]
    ex, r, (out, f) = run_one([0x0F, 0xFC, 0xCA, 0x0F, 0x77], True, tos=3, fptw=0x5555, mm=mm)
    phys = [mm[(i - 3) & 7] for i in range(8)]
    want = list(phys)
    want[1] = sum((((phys[1] >> (8 * k)) + (phys[2] >> (8 * k))) & 0xFF) << (8 * k) for k in range(8))
    assert ex.status == RUNNING
    assert list(r.fpst) == want and (r.fpsw >> 11) & 7 == 0 and r.fptw == 0
    assert out.status == 3 and list(f.fpst) == want and f.fptw == 0xFFFF and (f.fpsw >> 11) & 7 == 0
