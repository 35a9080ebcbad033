"""GPU engine on the SSE / SSE2 subset, MMX (U37) and the
vector families after them.

1. Every native vector of each family's golden file as one lane, replayed and
   judged by tests/vector_replay.py (what each family compares is declared
   there).
2. The fault / encoding cases of tests/test_sse.py, GPU vs oracle.
3. Random programs mixing SSE and integer forms, GPU vs oracle lane by lane
   (exit, registers, XMM, coverage, dirty pages, bytes, memory).
"""
import numpy as np
import pytest

from tests import progfuzz
from tests import vector_replay as V
from tests.insn_cases import BUF, SSE_FAULT_CASES, get_xmm, get_zmm, layout, move_case, set_xmm, widening_program
from tests.insn_cases import CODE_VA as CVA
from tests.oracle_lib import Oracle
from wtf_amd.abi import EXIT_INT3, regs_from_state

pytestmark = pytest.mark.gpu


def _replay(fam):
    """Every case of the family's golden file as one lane, judged by the
    family's check() (tests/vector_replay.py)."""
    cases = fam.doc["cases"]
    fails = V.run_family(fam, V.replay_gpu, cases)
    total = len(cases)
    assert total == len(fam.doc["cases"])
    assert not fails, f"{len(fails)}/{total} mismatches, first: {fails[:6]}"


def test_gpu_matches_native_sse_vectors():
    _replay(V.SSE)


def test_gpu_matches_native_mmx_vectors():
    _replay(V.MMX)


def test_gpu_sse_faults_match_oracle():
    """Misaligned operands, register-only / memory-only forms, MMX / FP /
    SSE3 encodings and CR0 / CR4 gating: GPU exits equal the oracle's."""
    from wtf_amd.engine import Engine

    variants = [(code, None, None) for code, _, _ in SSE_FAULT_CASES]
    pxor = [0x66, 0x0F, 0xEF, 0xC1]
    variants += [(pxor, None, 0x370678 & ~0x200), (pxor, 0x80050031 | 4, None), (pxor, 0x80050031 | 8, None),
                 ([0x0F, 0xAE, 0xF0], 0x80050031 | 8, None)]
    for code, cr0, cr4 in variants:
        sp, regs = layout(bytes(code), BUF, bytes(range(256)), cr0=cr0, cr4=cr4)
        regs.gpr[3] = BUF + 0x10
        regs.gpr[6] = BUF + 0x13
        pfns, blob = sp.phys()
        o = Oracle(pfns=pfns, blob=blob)
        o.restore(regs)
        want = o.run()
        eng = Engine(0)
        eng.load_pool(pfns, blob)
        eng.alloc_lanes(64, overlay_pages=4, cov_entries=64)
        eng.set_initial_state(regs)
        eng.set_limit(0)
        eng.restore()
        eng.run()
        e = eng.exits(0, 1)[0]
        got = (e.status, e.vector if e.status == 5 else 0, e.rip, e.icount)
        exp = (want.status, want.vector if want.status == 5 else 0, want.rip, want.icount)
        assert got == exp, (bytes(code).hex(), cr0, cr4, got, exp)
        eng.close()


@pytest.mark.parametrize("seed,fp", [(21, False), (22, False), (23, True), (24, True)])
def test_gpu_matches_oracle_on_random_sse_programs(seed, fp):
    """fp: with the floating-point and SSE4 / AVX2 forms and a random MXCSR per lane."""
    from wtf_amd.engine import Engine

    n = 512
    sp, st, lanes = progfuzz.build(n, seed=seed, sse=True, fp=fp)
    xmm = progfuzz.lane_xmm(n, seed)
    ymmh = progfuzz.lane_xmm(n, seed, 0x4E4)
    mx = progfuzz.lane_mxcsr(n, seed) if fp else None
    want = progfuzz.oracle_run(sp, st, lanes, xmm=xmm, ymmh=ymmh, mxcsr=mx)
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=8, cov_entries=4096)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(20000)
    eng.restore()
    regs = eng.read_regs(0, n)
    for i, (va, g, flags) in enumerate(lanes):
        for k in range(16):
            regs[i].gpr[k] = g[k]
        regs[i].rip = va
        regs[i].rflags = flags
        set_xmm(regs[i], xmm[i])
        for k in range(16):
            regs[i].ymmh[k][0], regs[i].ymmh[k][1] = ymmh[i][2 * k], ymmh[i][2 * k + 1]
        if mx is not None:
            regs[i].mxcsr = mx[i]
    eng.write_regs(regs)
    stats = eng.run()
    ex = eng.exits()
    out = eng.read_regs(0, n)
    cov, ovf = eng.coverage()
    nb = eng.nbytes()
    bad = []
    for i, w in enumerate(want):
        e, r = ex[i], out[i]
        got = (e.status, e.vector if e.status == 5 else 0, e.addr if e.status == 5 else 0, r.rip, e.icount)
        exp = (w["status"], w["vector"] if w["status"] == 5 else 0, w["addr"] if w["status"] == 5 else 0,
               w["rip"], w["icount"])
        if got != exp:
            bad.append((i, "exit", got, exp))
        elif [r.gpr[k] for k in range(16)] != w["gpr"] or r.rflags != w["rflags"]:
            bad.append((i, "regs"))
        elif get_xmm(r) != w["xmm"] or r.mxcsr != w["mxcsr"]:
            bad.append((i, "xmm"))
        elif [r.ymmh[k][h] for k in range(16) for h in range(2)] != w["ymmh"]:
            bad.append((i, "ymm"))
        elif cov.get(i, set()) != w["cov"]:
            bad.append((i, "cov"))
        elif set(eng.dirty(i)) != w["dirty"]:
            bad.append((i, "dirty"))
        elif int(nb[i]) != w["bytes"]:
            bad.append((i, "bytes", int(nb[i]), w["bytes"]))
        elif i % 8 == 0 and (eng.read_virt(i, progfuzz.WIN_VA, 0x2000) != w["win"] or
                             eng.read_virt(i, progfuzz.STACK_VA, 0x2000) != w["stack"]):
            bad.append((i, "memory"))
    assert not ovf
    assert stats.lane_retired == sum(w["icount"] for w in want)
    statuses = np.bincount([w["status"] for w in want], minlength=13)
    assert statuses[EXIT_INT3] > n // 8, statuses  # most programs run to the end
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:4]}"


def test_gpu_matches_native_avx_vectors():
    """Every AVX / AVX2 vector (tests/golden/avx_vectors.json.gz) as one lane:
    GPRs, RFLAGS, all 16 YMM registers and the memory window."""
    _replay(V.AVX)


def test_gpu_matches_native_fp_vectors():
    """SSE / AVX floating point (tests/golden/fp_vectors.json.gz, U39 / U40): GPRs,
    RFLAGS, all 16 YMM registers, MXCSR, and for the unmasked-exception cases
    the #XM exit with the trap's MXCSR."""
    _replay(V.FP)


def test_gpu_matches_native_sse4_vectors():
    """SSSE3 / SSE4.1 integer and AVX2 lane-crossing forms (tests/golden/sse4_vectors.json.gz, U41)."""
    _replay(V.SSE4)


def test_gpu_matches_x87_vectors():
    """x87 arithmetic (tests/golden/x87_vectors.json.gz, U42): every case one
    lane; its x87 state, status flags and 16-byte memory operand in, the
    host CPU's answer out (registers, sign / exponent words, FCW / FSW / tags,
    RFLAGS, the operand bytes, #MF / #UD / stack-fault outcomes)."""
    _replay(V.X87)


def test_gpu_matches_x87_directed_vectors():
    """The single-form x87 instructions by operand class (tests/golden/
    x87_directed_vectors.json.gz; tests/test_x87.py counts the classes): fsqrt,
    frndint, fscale, fprem / fprem1, fxtract, fxam and the integer stores at
    their rounding, range and exception edges, one case per lane."""
    _replay(V.X87D)


def test_gpu_matches_native_ext_vectors():
    """BMI1 / BMI2 / ADX / MOVBE / CRC32, SSE4.2, AES, PCLMULQDQ (tests/golden/ext_vectors.json.gz, U45)."""
    _replay(V.EXT)


def test_gpu_matches_native_avx2x_vectors():
    """FMA3, F16C and the AVX2 gathers (tests/golden/avx2x_vectors.json.gz, U46)."""
    _replay(V.AVX2X)


def test_gpu_matches_native_avx512_vectors():
    """The AVX-512 subset and the opmask instructions (tests/golden/avx512_vectors.json.gz, U47):
    every case one lane with GPRs, RFLAGS, zmm0-31, k0-7 and the 512-byte window
    across a page boundary; the guard cases (one of the two pages absent) in
    their own address spaces, with the #PF error code and CR2 of the faults
    (memory fault suppression)."""
    _replay(V.AVX512)


@pytest.mark.parametrize("vzu", [False, True], ids=["moves", "moves-vzeroupper"])
def test_gpu_vex_writes_zero_to_maxvl_before_xcr0_is_widened(vzu):
    """tests/test_fast_path.py's widening program on the 64 lanes of one wave:
    XCR0 = 7 and nonzero zmm0-15 uppers, a VEX.128 load, a VEX.256 register
    move (and vzeroupper), xsetbv to 0xe7, vmovdqu64 stores. The odd lanes'
    load crosses a page, which takes them to the generic step for that VEX
    write while the even lanes stay in the fast loop. Every lane against the
    oracle: exit, GPRs, zmm0-31, k0-7, XCR0 and the stored bytes."""
    from wtf_amd.engine import Engine

    n = 64
    page = BUF & ~0xFFF
    sp, init = move_case(widening_program(vzu).hex(), 0x40, 0x100, xcr0=7)
    init.cr4 &= ~(3 << 20)  # no SMEP / SMAP: the stub runs on the test's user code page
    init.lstar = CVA + 8
    for k in range(16):
        for h in range(4):
            init.zmmh[k][h] = 0xC0C0C0C0C0C0C0C0 + 16 * k + h
    srcs = (page + 0x40, page + 0x1000 - 8)   # even lanes: inside the page; odd lanes: across its end
    pfns, blob = sp.phys()
    want = []
    for src in srcs:
        o = Oracle(pfns=pfns, blob=blob)
        init.gpr[6] = src
        o.restore(init)
        ex = o.run()
        assert ex.status == EXIT_INT3
        r = o.regs()
        z = get_zmm(r)
        assert z[8 * 1 + 2: 8 * 1 + 8] == [0] * 6 and z[8 * 3 + 4: 8 * 3 + 8] == [0] * 4
        want.append((o.icount(), list(r.gpr), z, list(r.k), r.xcr0, o.read_virt(page + 0x100, 256)))
    eng = Engine(0)
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=4, cov_entries=64)
    eng.set_initial_state(init)
    eng.set_limit(0)
    eng.restore()
    regs = eng.read_regs(0, n)
    for i in range(n):
        regs[i].gpr[6] = srcs[i & 1]
    eng.write_regs(regs)
    eng.run()
    ex = eng.exits()
    out = eng.read_regs(0, n)
    bad = []
    for i in range(n):
        icount, gpr, z, kk, xcr0, mem = want[i & 1]
        r, e = out[i], ex[i]
        if (e.status, e.icount) != (EXIT_INT3, icount):
            bad.append((i, "exit", e.status, e.vector, e.icount))
        elif list(r.gpr) != gpr or r.xcr0 != xcr0:
            bad.append((i, "regs"))
        elif get_zmm(r) != z:
            g = get_zmm(r)
            bad.append((i, "zmm", [(j // 8, j % 8, hex(g[j]), hex(z[j])) for j in range(256) if g[j] != z[j]][:4]))
        elif list(r.k) != kk:
            bad.append((i, "k"))
        elif eng.read_virt(i, page + 0x100, 256) != mem:
            bad.append((i, "memory"))
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:4]}"
    eng.close()
