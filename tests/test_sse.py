"""SSE / SSE2 subset (convention U22).

The CPU oracle is pinned by native-execution vectors (tests/golden/
gen_sse_vectors.py: 16 GPRs, RFLAGS, 16 XMM registers, MXCSR and a 256-byte
memory window, run natively on the x86-64 host). Behaviour native execution
cannot show without crashing (misaligned 16-byte operands, CR0/CR4 gating,
register-only / memory-only encodings) is checked by hand here; the GPU engine
is compared with the oracle on all of it in test_gpu_sse.py.
"""
import pytest

from tests import simlane
from tests.insn_cases import BUF, SSE_FAULT_CASES, build, layout
from tests.vector_replay import SSE, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, RUNNING, regs_from_state

DOC = SSE.doc


@pytest.mark.parametrize("chunk", range(4))
def test_oracle_matches_native_sse(chunk):
    cases = DOC["cases"][chunk::4]
    fails = run_family(SSE, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:6]}"


def test_sse_vector_file_is_substantial():
    assert len(DOC["cases"]) > 2500
    names = {c["name"].split(".")[0] for c in DOC["cases"]}
    for n in ("movaps", "movdqu", "pef", "pmovmskb", "pshufd", "movd", "movq", "ldmxcsr", "shimm"):
        assert n in names, n


# ---- hand-checked faults and encodings (what native execution cannot show)
def run1(code, regs_fn=None, cr0=None, cr4=None):
    o, regs = build(bytes(code), BUF, bytes(range(256)), cr0=cr0, cr4=cr4)
    regs.gpr[3] = BUF + 0x10  # rbx -> window + 16 (16-byte aligned)
    regs.gpr[6] = BUF + 0x13  # rsi -> misaligned
    if regs_fn:
        regs_fn(regs)
    o.restore(regs)
    return o, o.step()


@pytest.mark.parametrize("code,status,vector", SSE_FAULT_CASES)
def test_oracle_sse_faults(code, status, vector):
    _, ex = run1(code)
    assert ex.status == status, (bytes(code).hex(), ex.status, ex.vector)
    if vector is not None:
        assert ex.vector == vector


def test_oracle_sse_control_register_gating():
    # CR4.OSFXSR = 0 -> #UD; CR0.EM -> #UD; CR0.TS -> #NM (7); fences are not gated
    _, ex = run1([0x66, 0x0F, 0xEF, 0xC1], cr4=0x370678 & ~0x200)
    assert (ex.status, ex.vector) == (EXIT_FAULT, 6)
    _, ex = run1([0x66, 0x0F, 0xEF, 0xC1], cr0=0x80050031 | 4)
    assert (ex.status, ex.vector) == (EXIT_FAULT, 6)
    _, ex = run1([0x66, 0x0F, 0xEF, 0xC1], cr0=0x80050031 | 8)
    assert (ex.status, ex.vector) == (EXIT_FAULT, 7)
    _, ex = run1([0x0F, 0xAE, 0xF0], cr0=0x80050031 | 8)
    assert ex.status == RUNNING


def test_oracle_ldmxcsr_reserved_bits_gp():
    o, regs = build(bytes([0x0F, 0xAE, 0x13]), BUF, (0x10000).to_bytes(4, "little") * 64)
    regs.gpr[3] = BUF + 0x10
    o.restore(regs)
    ex = o.step()
    assert (ex.status, ex.vector) == (EXIT_FAULT, 13)
    assert o.regs().mxcsr == 0x1F80


def test_oracle_page_crossing_movdqu_store_faults_whole():
    # movdqu [rsi], xmm0 with rsi 8 bytes before an unmapped page: #PF, nothing written
    def put(regs):
        regs.gpr[6] = (BUF & ~0xFFF) + 0x2000 - 8
        regs.xmm[0][0], regs.xmm[0][1] = 0x1111111111111111, 0x2222222222222222

    o, ex = run1([0xF3, 0x0F, 0x7F, 0x06], put)
    assert (ex.status, ex.vector) == (EXIT_FAULT, 14)
    assert o.read_virt((BUF & ~0xFFF) + 0x2000 - 8, 8) == bytes(8)


# ---- the engine's own SSE code (engine_sse.h), built for the host
# (tests/native/sim_lane.cc: one lane of k_run's decode / exec / retry loop)
# against the native vectors and the oracle, so the device semantics are
# checked on CPU before any GPU run.
def test_engine_sse_code_matches_native_vectors():
    fails = run_family(SSE, replay_sim, DOC["cases"])
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:6]}"


@pytest.mark.parametrize("code,status,vector", SSE_FAULT_CASES)
def test_engine_sse_code_faults(code, status, vector):
    sp, regs = layout(bytes(code), BUF, bytes(range(256)))
    regs.gpr[3] = BUF + 0x10
    regs.gpr[6] = BUF + 0x13
    out, _, _ = simlane.run(sp, regs)
    want = 3 if status == RUNNING else status  # a clean run stops at the int3
    assert out.status == want, (bytes(code).hex(), out.status, out.vector)
    if vector is not None:
        assert out.vector == vector


@pytest.mark.parametrize("fast,fp", [(False, False), (True, False), (True, True)])
def test_engine_sse_code_matches_oracle_on_random_programs(fast, fp):
    """fp: with the floating-point and SSE4 / AVX2 forms and a random MXCSR per lane."""
    from tests import progfuzz

    n = 160
    seed = 33 if fp else 31
    sp, st, lanes = progfuzz.build(n, seed=seed, sse=True, fp=fp)
    xmm = progfuzz.lane_xmm(n, seed)
    ymmh = progfuzz.lane_xmm(n, seed, 0x4E4)
    mx = progfuzz.lane_mxcsr(n, seed) if fp else None
    want = progfuzz.oracle_run(sp, st, lanes, xmm=xmm, ymmh=ymmh, mxcsr=mx)
    img = simlane.image(sp)
    bad = []
    for i, ((va, g, flags), w) in enumerate(zip(lanes, want)):
        regs = regs_from_state(st)
        for k in range(16):
            regs.gpr[k] = g[k]
            regs.xmm[k][0], regs.xmm[k][1] = xmm[i][2 * k], xmm[i][2 * k + 1]
            regs.ymmh[k][0], regs.ymmh[k][1] = ymmh[i][2 * k], ymmh[i][2 * k + 1]
        regs.rip, regs.rflags = va, flags
        if mx is not None:
            regs.mxcsr = mx[i]
        out, _, _ = simlane.run(img, regs, limit=20000, fast=fast)
        got = (out.status, out.vector if out.status == EXIT_FAULT else 0, out.rip, out.icount)
        exp = (w["status"], w["vector"] if w["status"] == EXIT_FAULT else 0, w["rip"], w["icount"])
        if got != exp:
            bad.append((i, "exit", got, exp))
        elif list(out.gpr) != w["gpr"] or out.rflags != w["rflags"]:
            bad.append((i, "regs"))
        elif list(out.xmm) != w["xmm"] or out.mxcsr != w["mxcsr"]:
            bad.append((i, "xmm"))
        elif list(out.ymmh) != w["ymmh"]:
            bad.append((i, "ymm"))
        elif out.nbytes != w["bytes"]:
            bad.append((i, "bytes", out.nbytes, w["bytes"]))
        elif {out.dirty[k] for k in range(min(out.ovn, 64))} != w["dirty"]:
            bad.append((i, "dirty"))
    sse_ran = sum(1 for i, w in enumerate(want) if w["xmm"] != xmm[i])
    assert sse_ran > n // 4, sse_ran
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:4]}"
