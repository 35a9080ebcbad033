"""Random x86-64 programs for GPU-vs-oracle differential tests.

A program is a chain of blocks; each block re-establishes the pointer
registers its instruction form needs (mov r64, imm64 into a data window) and
then runs one random form drawn from the native-vector generator's encodings
(tests/golden/gen_native_vectors.py). Some blocks are guarded by a forward
conditional jump, some jump backwards through a counted loop. Programs end in
int3. Faults (#DE, #PF on a read-only page, ...) end a lane early; both
engines must agree on that too. With sse=True the SSE / SSE2 forms of
tests/golden/gen_sse_vectors.py join the pool (aligned forms sometimes get a
misaligned window: #GP) and every lane starts from its own XMM registers.
"""
from __future__ import annotations

import random

from tests.golden.gen_native_vectors import RCX, RDI, RSI, RSP, gen_forms
from wtf_amd.abi import regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

CODE_VA = 0x100000000
SLOT = 0x2000
WIN_VA = 0x200000000     # two RW pages
RO_VA = 0x200002000      # one read-only page right after (writes fault)
STACK_VA = 0x300000000   # two pages
STACK_TOP = STACK_VA + 0x2000 - 0x100


def mov_imm64(r, v):
    return bytes([0x48 | (r >> 3), 0xB8 + (r & 7)]) + (v & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")


def make_program(rng: random.Random, forms, n_blocks=24) -> bytes:
    code = bytearray()
    for _ in range(n_blocks):
        f = rng.choice(forms)
        if f.cls == "div" and rng.random() < 0.7:
            continue
        setup = bytearray()
        base = WIN_VA + rng.choice([0x100, 0x800, 0xF00, 0xFF8 - 0x80])
        for r, off in f.ptrs.items():
            setup += mov_imm64(r, base + off)
        for r, (lo, hi) in f.smalls.items():
            setup += mov_imm64(r, rng.randint(lo, hi))
        if f.cls == "string":
            setup += mov_imm64(RSI, WIN_VA + rng.randrange(0x40, 0x1F00))
            setup += mov_imm64(RDI, rng.choice([WIN_VA + rng.randrange(0x40, 0x1F00), RO_VA - 4]))
            setup += mov_imm64(RCX, rng.randrange(0, 12))
        if f.cls in ("stack", "popf"):
            setup += mov_imm64(RSP, STACK_TOP - rng.randrange(0, 32) * 8)
        block = bytes(setup) + f.code
        r = rng.random()
        if r < 0.15 and len(block) < 120:
            code += bytes([0x70 + rng.randrange(16), len(block)])  # jcc over the block
        elif r < 0.2 and len(block) < 100:
            # a short counted loop around the block: mov ecx, k ; block ; dec ecx ; jnz
            k = rng.randrange(1, 4)
            code += bytes([0xB9]) + k.to_bytes(4, "little")
            body = block + bytes([0xFF, 0xC9])
            code += body + bytes([0x75, (-(len(body) + 2)) & 0xFF])
            continue
        code += block
        if len(code) > SLOT - 64:
            break
    code += b"\xcc"
    return bytes(code[:SLOT])


def build(n_programs: int, seed: int, sse: bool = False, fp: bool = False):
    """Returns (AddressSpace, base state, list of (code_va, regs dict)). fp:
    the SSE / AVX floating-point (U39 / U40) and SSE4 / AVX2 (U41) forms join
    the SSE pool."""
    rng = random.Random(seed)
    forms = gen_forms(random.Random(seed ^ 0xABCDEF))
    if fp:
        from tests.golden.gen_fp_vectors import gen_forms as gen_fp_forms
        from tests.golden.gen_sse4_vectors import gen_forms as gen_sse4_forms

        forms = forms + (gen_fp_forms(random.Random(seed ^ 0xF9)) + gen_sse4_forms(random.Random(seed ^ 0x54))) * 2
    if sse:
        from tests.golden.gen_sse_vectors import gen_forms as gen_sse_forms

        from tests.golden.gen_avx_vectors import gen_forms as gen_avx_forms

        sse_forms = gen_sse_forms(random.Random(seed ^ 0x55E)) + gen_avx_forms(random.Random(seed ^ 0xA0C))
        forms = forms + sse_forms * 3  # mostly SSE / AVX
    sp = AddressSpace()
    progs = []
    for i in range(n_programs):
        code = make_program(rng, forms)
        va = CODE_VA + i * SLOT
        sp.map_range(va, code + b"\xcc" * (SLOT - len(code)), write=False)
        progs.append(va)
    win = bytes(rng.getrandbits(8) for _ in range(0x2000))
    sp.map_range(WIN_VA, win, nx=True)
    sp.map(RO_VA, bytes(rng.getrandbits(8) for _ in range(0x1000)), write=False, nx=True)
    sp.map_range(STACK_VA, bytes(0x2000), nx=True)
    st = user_state(CODE_VA, STACK_TOP, sp.cr3)
    lanes = []
    for i, va in enumerate(progs):
        regs = [rng.getrandbits(64) for _ in range(16)]
        regs[RSP] = STACK_TOP
        flags = 0x202 | (rng.getrandbits(12) & 0x8D5)
        lanes.append((va, regs, flags))
    return sp, st, lanes


def _form_pool(seed: int, sse: bool, fp: bool):
    """The block pool of build(): same forms, same order, same seeds."""
    forms = gen_forms(random.Random(seed ^ 0xABCDEF))
    if fp:
        from tests.golden.gen_fp_vectors import gen_forms as gen_fp_forms
        from tests.golden.gen_sse4_vectors import gen_forms as gen_sse4_forms

        forms = forms + (gen_fp_forms(random.Random(seed ^ 0xF9)) + gen_sse4_forms(random.Random(seed ^ 0x54))) * 2
    if sse:
        from tests.golden.gen_sse_vectors import gen_forms as gen_sse_forms

        from tests.golden.gen_avx_vectors import gen_forms as gen_avx_forms

        sse_forms = gen_sse_forms(random.Random(seed ^ 0x55E)) + gen_avx_forms(random.Random(seed ^ 0xA0C))
        forms = forms + sse_forms * 3
    return forms


# ---------------------------------------------------------------------------
# Shared programs: few programs, many lanes (the lanes of a program sit at the
# same rip and form a group in the engine's wave-level interpreter).
#
# Data window of the shared layout: the two RW pages of build(), the read-only
# page, then two more RW pages, so that a pointer can be moved to another
# writable page, onto a page boundary (RW|RW, RW|RO, RO|RW) or into the
# read-only page.
# ---------------------------------------------------------------------------
WIN2_VA = RO_VA + 0x1000  # two more RW pages behind the read-only page
WIN2_LEN = 0x2000
LANES_PER_PROGRAM_RUN = 4  # lane i runs program (i // 4) % n_programs

# How often a block's pointer gets a flag-dependent displacement, and where the
# displaced pointer lands (weights). Tuned on the oracle alone so that the
# conditions of tests/test_progfuzz_shared.py hold; see that test.
P_DISP = 0.6
P_DISP_BT = 0.6
P_DISP_ALIGNED = 0.75
# make_program's unconditional ways to end a whole program (the string store
# into the read-only page, the misaligning window base) are kept but thinned:
# here one of them ends every lane of a program at once, and the displacement
# reaches the same faults lane by lane.
P_STRING_RO = 0.15
BASES = (0x100, 0x800, 0xF00) * 3 + (0xFF8 - 0x80,)
DISP_KINDS = (("page", 40), ("cross_rw", 24), ("cross_ro", 14), ("ro", 22))
_RW_PAGES = (WIN_VA, WIN_VA + 0x1000, WIN2_VA, WIN2_VA + 0x1000)


def _disp_target(rng: random.Random, p: int) -> int:
    """Where a pointer that points at p goes when its displacement is taken."""
    kind = rng.choices([k for k, _ in DISP_KINDS], [w for _, w in DISP_KINDS])[0]
    if kind == "page":  # the same offset in another writable page
        return rng.choice([pg for pg in _RW_PAGES if pg != p & ~0xFFF]) + (p & 0xFFF)
    if kind == "cross_rw":  # at the end of a writable page whose successor is writable
        t = rng.choice([WIN_VA + 0x1000, WIN2_VA + 0x1000]) - rng.randrange(1, 48)
    elif kind == "cross_ro":  # across the edge of the read-only page, from either side
        t = rng.choice([RO_VA, WIN2_VA]) - rng.randrange(1, 48)
    else:
        t = RO_VA + rng.randrange(0x40, 0xF00)
    if rng.random() < P_DISP_ALIGNED:  # keep the pointer's 16-byte phase: an aligned SSE form stays aligned
        t -= (t - p) % 16
    return t


def _flag_disp(rng: random.Random, reg: int, p: int, fresh) -> bytes:
    """jcc +7 ; add reg, imm32: lanes whose flags do not take the jump move the
    pointer (which holds p) elsewhere, the others keep it. Both rejoin at the
    next instruction. The flags are the previous form's, or (P_DISP_BT of the
    time, while the program has registers left that it never loaded a constant
    into: fresh) those of a bt on a random bit of such a register first: SSE
    forms leave the flags alone and the add itself sets them alike in every
    lane that runs it, so flags alone soon stop telling lanes apart."""
    delta = _disp_target(rng, p) - p
    add = bytes([0x48 | (reg >> 3), 0x81, 0xC0 | (reg & 7)]) + (delta & 0xFFFFFFFF).to_bytes(4, "little")
    if fresh and rng.random() < P_DISP_BT:
        t = rng.choice(fresh)
        bt = bytes([0x48 | (t >> 3), 0x0F, 0xBA, 0xE0 | (t & 7), rng.randrange(64)])  # bt t, imm8
        return bt + bytes([rng.choice([0x72, 0x73]), len(add)]) + add  # jc / jnc
    return bytes([0x70 + rng.randrange(16), len(add)]) + add


def make_shared_program(rng: random.Random, forms, n_blocks=24):
    """make_program with flag-dependent pointer displacements. Returns (code,
    blocks); blocks: (offset of the block's first instruction, inside a counted
    loop, target of a jcc) per block."""
    code = bytearray()
    blocks = []
    after_guard = False
    const = {RSP}  # registers the program has loaded a constant into so far

    def fresh():
        return [r for r in range(16) if r not in const]

    for _ in range(n_blocks):
        f = rng.choice(forms)
        if f.cls == "div" and rng.random() < 0.7:
            continue
        setup = bytearray()
        base = WIN_VA + rng.choice(BASES)
        disp_reg = rng.choice(sorted(f.ptrs)) if f.ptrs and rng.random() < P_DISP else None
        const.update(f.ptrs, f.smalls)
        for r, off in f.ptrs.items():
            setup += mov_imm64(r, base + off)
            if r == disp_reg and r != RSP:
                setup += _flag_disp(rng, r, base + off, fresh())
        for r, (lo, hi) in f.smalls.items():
            setup += mov_imm64(r, rng.randint(lo, hi))
        if f.cls == "string":
            const.update((RSI, RDI, RCX))
            src = WIN_VA + rng.randrange(0x40, 0x1F00)
            dst = RO_VA - 4 if rng.random() < P_STRING_RO else WIN_VA + rng.randrange(0x40, 0x1F00)
            setup += mov_imm64(RSI, src)
            if rng.random() < P_DISP / 2:
                setup += _flag_disp(rng, RSI, src, fresh())
            setup += mov_imm64(RDI, dst)
            if rng.random() < P_DISP / 2:
                setup += _flag_disp(rng, RDI, dst, fresh())
            setup += mov_imm64(RCX, rng.randrange(0, 12))
        if f.cls in ("stack", "popf"):
            setup += mov_imm64(RSP, STACK_TOP - rng.randrange(0, 32) * 8)
        block = bytes(setup) + f.code
        r = rng.random()
        if r < 0.15 and len(block) < 120:
            code += bytes([0x70 + rng.randrange(16), len(block)])  # jcc over the block
            blocks.append((len(code), False, after_guard))
            after_guard = True
        elif r < 0.2 and len(block) < 100:
            k = rng.randrange(1, 4)
            const.add(RCX)
            code += bytes([0xB9]) + k.to_bytes(4, "little")
            blocks.append((len(code), True, True))  # the jnz comes back here
            body = block + bytes([0xFF, 0xC9])
            code += body + bytes([0x75, (-(len(body) + 2)) & 0xFF])
            after_guard = False
            continue
        else:
            blocks.append((len(code), False, after_guard))
            after_guard = False
        code += block
        if len(code) > SLOT - 64:
            break
    code += b"\xcc"
    assert len(code) <= SLOT
    return bytes(code), blocks


def build_shared_info(n_lanes: int, n_programs: int, seed: int, sse: bool = False, fp: bool = False):
    """build_shared plus, per program, {"va", "end" (the final int3), "blocks":
    [(rip, in_loop, jcc_target)]}."""
    rng = random.Random(seed)
    forms = _form_pool(seed, sse, fp)
    sp = AddressSpace()
    progs = []
    for i in range(n_programs):
        code, blocks = make_shared_program(rng, forms)
        va = CODE_VA + i * SLOT
        sp.map_range(va, code + b"\xcc" * (SLOT - len(code)), write=False)
        progs.append({"va": va, "end": va + len(code) - 1, "blocks": [(va + o, lp, tg) for o, lp, tg in blocks]})
    sp.map_range(WIN_VA, bytes(rng.getrandbits(8) for _ in range(0x2000)), nx=True)
    sp.map(RO_VA, bytes(rng.getrandbits(8) for _ in range(0x1000)), write=False, nx=True)
    sp.map_range(WIN2_VA, bytes(rng.getrandbits(8) for _ in range(WIN2_LEN)), nx=True)
    sp.map_range(STACK_VA, bytes(0x2000), nx=True)
    st = user_state(CODE_VA, STACK_TOP, sp.cr3)
    lanes = []
    for i in range(n_lanes):
        regs = [rng.getrandbits(64) for _ in range(16)]
        regs[RSP] = STACK_TOP
        flags = 0x202 | (rng.getrandbits(12) & 0x8D5)
        lanes.append((progs[lane_program(i, n_programs)]["va"], regs, flags))
    return sp, st, lanes, progs


def lane_program(lane: int, n_programs: int) -> int:
    return (lane // LANES_PER_PROGRAM_RUN) % n_programs


def build_shared(n_lanes: int, n_programs: int, seed: int, sse: bool = False, fp: bool = False):
    """As build(), but n_lanes lanes share n_programs programs: lane i runs
    program (i // 4) % n_programs, so at 64, 32 and 16 lanes per wave every
    hardware wave holds at least 4 programs and 4 lanes of each. Registers and
    flags stay per-lane random; the programs derive per-lane effective
    addresses from them (see _flag_disp). Returns (AddressSpace, base state,
    list of (code_va, regs, flags)), as build()."""
    return build_shared_info(n_lanes, n_programs, seed, sse, fp)[:3]


def lane_xmm(n: int, seed: int, salt: int = 0x3E3):
    """Initial XMM registers per lane (32 u64 each); salt 0x4E4: the YMM upper halves."""
    rng = random.Random(seed ^ salt)
    return [[rng.getrandbits(64) for _ in range(32)] for _ in range(n)]


def lane_mxcsr(n: int, seed: int):
    """Initial MXCSR per lane: rounding control, DAZ, FTZ, sometimes unmasked exceptions."""
    rng = random.Random(seed ^ 0x3C5)
    out = []
    for _ in range(n):
        mx = 0x1F80 | (rng.randrange(4) << 13) | (0x40 if rng.random() < 0.3 else 0) | (0x8000 if rng.random() < 0.3 else 0)
        if rng.random() < 0.2:
            mx &= ~(rng.getrandbits(6) << 7)
        out.append(mx)
    return out


def oracle_run(sp: AddressSpace, st: dict, lanes, limit=20000, breakpoints=(), xmm=None, ymmh=None, mxcsr=None,
               more=(), follow_bps=False):
    """Runs every lane on the CPU oracle; returns per-lane result dicts. more:
    further (va, length) ranges to read back ("more"). follow_bps: resume over
    every breakpoint hit (run(skip_bp=True)) until another exit, recording the
    hits as "stops": [(rip, icount, gprs)]."""
    from tests.oracle_lib import Oracle

    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    base = regs_from_state(st)
    o.set_limit(limit)
    o.set_breakpoints(list(breakpoints))
    out = []
    for i, (va, regs, flags) in enumerate(lanes):
        r = regs_from_state(st)
        for k in range(16):
            r.gpr[k] = regs[k]
        if xmm is not None:
            for k in range(16):
                r.xmm[k][0], r.xmm[k][1] = xmm[i][2 * k], xmm[i][2 * k + 1]
        if ymmh is not None:
            for k in range(16):
                r.ymmh[k][0], r.ymmh[k][1] = ymmh[i][2 * k], ymmh[i][2 * k + 1]
        if mxcsr is not None:
            r.mxcsr = mxcsr[i]
        r.rip = va
        r.rflags = flags
        o.restore(base)
        o.set_regs(r)
        ex = o.run()
        stops = []
        while follow_bps and ex.status == 1:  # EXIT_BREAKPOINT
            rr = o.regs()
            stops.append((rr.rip, ex.icount, list(rr.gpr)))
            ex = o.run(skip_bp=True)
        rr = o.regs()
        out.append({
            "stops": stops, "more": [o.read_virt(va_, n_) for va_, n_ in more],
            "status": ex.status, "vector": ex.vector, "error": ex.error, "addr": ex.addr, "rip": rr.rip,
            "icount": ex.icount, "gpr": list(rr.gpr), "rflags": rr.rflags, "cov": set(o.coverage()),
            "dirty": set(o.dirty()), "bytes": o.nbytes(),
            "win": o.read_virt(WIN_VA, 0x2000), "stack": o.read_virt(STACK_VA, 0x2000),
            "xmm": [rr.xmm[k][h] for k in range(16) for h in range(2)], "mxcsr": rr.mxcsr,
            "ymmh": [rr.ymmh[k][h] for k in range(16) for h in range(2)],
        })
    return out


# (seed, sse, fp) of the shared-program tests: tests/test_progfuzz_shared.py
# holds the generator to its conditions for each, tests/test_gpu_progfuzz_shared.py
# runs them on the engine.
SHARED_CASES = [(31, False, False), (32, False, False), (35, True, False), (34, True, True)]
