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
With evex=True the AVX-512 forms the oracle executes (conventions U47 and U49,
gen_evex_forms below) join as well, under XCR0 = 0xe7, and every lane starts
from its own zmm0-31 and k0-7 (lane_zmm, lane_k).
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


def _extra(f) -> dict:
    return getattr(f, "extra", None) or {}


def make_program(rng: random.Random, forms, n_blocks=24) -> bytes:
    code = bytearray()
    for _ in range(n_blocks):
        f = rng.choice(forms)
        if f.cls == "div" and rng.random() < 0.7:
            continue
        setup = bytearray()
        base = WIN_VA + rng.choice([0x100, 0x800, 0xF00, 0xFF8 - 0x80])
        base = WIN_VA + _extra(f).get("base", base - WIN_VA)
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


def build(n_programs: int, seed: int, sse: bool = False, fp: bool = False, evex: bool = False):
    """Returns (AddressSpace, base state, list of (code_va, regs dict)). fp:
    the SSE / AVX floating-point (U39 / U40) and SSE4 / AVX2 (U41) forms join
    the SSE pool. evex: the AVX-512 forms (U47, U49: gen_evex_forms) join, the
    base state enables their state in XCR0, and every lane starts from
    lane_zmm / lane_k (lane_state)."""
    rng = random.Random(seed)
    forms = _form_pool(seed, sse, fp, evex)
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
    if evex:
        st["xcr0"] = XCR0_AVX512
    lanes = []
    for i, va in enumerate(progs):
        regs = [rng.getrandbits(64) for _ in range(16)]
        regs[RSP] = STACK_TOP
        flags = 0x202 | (rng.getrandbits(12) & 0x8D5)
        lanes.append((va, regs, flags))
    return sp, st, lanes


# ---------------------------------------------------------------------------
# The EVEX pool: the AVX-512 forms of conventions U47 (moves, logic, compares,
# broadcasts, opmask instructions) and U49 (families A-H), encoded by the
# native generators' own encoders and form tables. Memory operands go through
# the block's pointer registers like every other pool's.
# ---------------------------------------------------------------------------
XCR0_AVX512 = 0xE7
EVEX_SHARE = 1.8          # EVEX forms in a pool, relative to everything else in it
EVEX_PER_FAMILY = 48      # forms drawn per U49 family, and per U47 kind group
EVEX_EDGE_BASE = 0xF00    # window base of an "edge" store: its operand ends across the RW|RW page edge
EVEX_ALIGNED_BASE = 0x800  # window base of an aligned form
EVEX_FAMILIES = tuple("ABCDEFGH") + ("U47.st",)  # what tests/test_progfuzz_shared.py wants retired in two programs


def _evex_mem(rng, ptrs, smalls, toff, n_scale):
    """pick_mem with this pool's roles: the base in ptrs, the index a constant
    in smalls. rcx is left alone: a counted loop around the block counts in it.
    Returns (mem, (base, index, scale bits, displacement in bytes))."""
    from tests.golden.gen_avx512_vectors import pick_mem

    while True:
        p, s = {}, {}
        m = pick_mem(rng, None, p, s, toff, n_scale)
        if RCX not in p and RCX not in s:
            break
    ptrs.update(p)
    smalls.update({r: (v, v) for r, v in s.items()})
    base, index, ss, disp, dsz = m
    return m, (base, index, ss, disp * n_scale if dsz == 1 else disp)


def _evex_toff(rng, osz, edge=False):
    """The operand's offset from the block's window base. edge: the operand
    ends 1 .. osz - 1 bytes past offset 0x100, across the page edge when the
    base is EVEX_EDGE_BASE."""
    if edge and osz > 1:
        return 0x100 - rng.randrange(1, osz)
    return rng.randrange(0, 0x48)


def _evex_enc(code, name, ptrs, smalls, fam, aaa=0, store=False, es=0, n=0, ea=None, edge=False, base=None):
    from tests.golden.gen_native_vectors import Enc

    extra = {"fam": fam, "aaa": aaa, "store": store, "es": es, "n": n, "ea": ea}
    if edge:
        base = EVEX_EDGE_BASE
    if base is not None:
        extra["base"] = base
    return Enc(code, name, ptrs, smalls, cls="evex", extra=extra)


def _evex_u47(rng, form):
    from tests.golden.gen_avx512_vectors import evex

    nm, mp, pp, w0, opc, kind, es, ex = form
    w = w0 if w0 is not None else rng.randrange(2)
    ll = rng.randrange(3)
    vlb = 16 << ll
    nt = nm.startswith("vmovnt")
    mem = nt or (kind != "bcr" and rng.random() < (0.8 if kind == "st" else 0.5))
    aaa = 0 if nt or rng.random() < 0.25 else rng.randrange(1, 8)
    z = 1 if aaa and kind != "kd" and not (kind == "st" and mem) and rng.random() < 0.4 else 0
    b = 1 if mem and ex.get("bc") and rng.random() < 0.4 else 0
    reg, vvvv, rm = rng.randrange(32), rng.randrange(32), rng.randrange(32)
    if kind in ("ld", "st", "bcm", "bcr"):
        vvvv = 0
    elif rng.random() < 0.3:  # a write-masked destination that is also a source
        vvvv = reg
    if kind == "bcr":
        rm = rng.choice([r for r in range(16) if r != RSP])
    if kind == "kd":
        reg = rng.randrange(8)
    imm = rng.randrange(256) if kind == "tern" or ex.get("imm") else None
    ptrs, smalls, ea = {}, {}, None
    store = kind == "st" and mem
    edge = store and aaa != 0 and not ex.get("al") and rng.random() < 0.7
    if mem:
        osz = es if kind == "bcm" or b else vlb
        toff = _evex_toff(rng, osz, edge)
        if ex.get("al"):
            toff &= ~(vlb - 1)
        m, ea = _evex_mem(rng, ptrs, smalls, toff, osz)
        code = evex(mp, pp, w, ll, z, b, aaa, reg, vvvv, opc, mem=m, imm=imm)
    else:
        code = evex(mp, pp, w, ll, z, 0, aaa, reg, vvvv, opc, rm=rm, imm=imm)
    fam = "U47.st" if store and aaa else "U47"
    # an aligned form starts aligned: only a lane whose pointer was displaced can take its #GP
    return _evex_enc(code, nm, ptrs, smalls, fam, aaa, store, es, vlb // es, ea, edge,
                     base=EVEX_ALIGNED_BASE if ex.get("al") and mem else None)


def _evex_u49(rng, f):
    from tests.golden import gen_avx512x_vectors as X

    ll = rng.choice(list(X.lengths(f)))
    vlb = 16 << ll
    w = f["w"] if f["w"] is not None else rng.randrange(2)
    mem = (rng.random() < 0.5 or bool(f.get("memonly"))) and not f.get("regonly")
    aaa = 0 if (f.get("nomask") or rng.random() < 0.25) else rng.randrange(1, 8)
    z = 1 if aaa and rng.random() < 0.4 and not (f.get("ext") and mem) else 0
    b = 1 if mem and f.get("bc") and rng.random() < 0.45 else 0
    reg, vvvv, rm = X.pick_regs(rng, f)
    if not (f.get("regk") or f.get("rmk") or f.get("rmg")):
        x = rng.random()
        if x < 0.15:  # the destination aliasing each source
            vvvv = reg
        elif x < 0.3:
            rm = reg
        elif x < 0.35:
            vvvv = rm = reg
    imm = X.imm_of(rng, f)
    ptrs, smalls, ea = {}, {}, None
    store = mem and (bool(f.get("ext")) or f.get("tag") in ("s", "xs"))
    blk = X.msize(f, vlb)
    if mem:
        osz = f["bc"] if b else blk
        m, ea = _evex_mem(rng, ptrs, smalls, _evex_toff(rng, osz, store and aaa != 0), osz)
        code = X.encode(f, w, ll, z, b, aaa, reg, vvvv, mem=m, imm=imm)
    else:
        code = X.encode(f, w, ll, z, 0, aaa, reg, vvvv, rm=rm, imm=imm)
    n = (blk if f.get("ext") else vlb) // f["es"]
    return _evex_enc(code, f["nm"], ptrs, smalls, f["fam"], aaa, store, f["es"], n, ea, store and aaa != 0)


def _evex_kop(rng):
    """A few of the VEX opmask instructions: moves from GPRs (per-lane masks),
    logic between masks, kortest / ktest (per-lane flags)."""
    from tests.golden.gen_avx512_vectors import vex3

    k, k2, k3 = rng.randrange(8), rng.randrange(8), rng.randrange(8)
    g = rng.choice([r for r in range(16) if r != RSP])
    pp, w = rng.choice(((0, 0), (0, 1), (1, 0), (1, 1)))
    what = rng.randrange(6)
    if what == 0:
        code, nm = vex3(1, 3, rng.randrange(2), 0, k, 0, 0x92, rm=g), "kmov.fromr"
    elif what == 1:
        code, nm = vex3(1, 3, rng.randrange(2), 0, g, 0, 0x93, rm=k), "kmov.tor"
    elif what == 2:
        code, nm = vex3(1, pp, w, 1, k, k2, rng.choice((0x41, 0x42, 0x45, 0x46, 0x47, 0x4A)), rm=k3), "klogic"
    elif what == 3:
        code, nm = vex3(1, pp, w, 0, k, 0, rng.choice((0x44, 0x90)), rm=k2), "knot/kmov"
    elif what == 4:
        code, nm = vex3(1, pp, w, 0, k, 0, rng.choice((0x98, 0x99)), rm=k2), "kortest/ktest"
    else:
        code, nm = vex3(3, 1, w, 0, k, 0, rng.choice((0x30, 0x31, 0x32, 0x33)), rm=k2, imm=rng.randrange(70)), "kshift"
    return _evex_enc(code, nm, {}, {}, "U47.k")


def _evex_vexmove(rng):
    """vmovdqu xmm / ymm (VEX), register, load or store: a VEX write zeroes the
    destination's bits 511:128 / 511:256, between EVEX forms that read them."""
    from tests.golden.gen_avx512_vectors import vex3

    l, reg, rm = rng.randrange(2), rng.randrange(16), rng.randrange(16)
    kind = rng.randrange(3)
    ptrs, smalls, ea = {}, {}, None
    if kind == 0:
        code = vex3(1, 2, 0, l, reg, 0, 0x6F, rm=rm)
    else:
        m, ea = _evex_mem(rng, ptrs, smalls, _evex_toff(rng, 16 << l), 1)
        code = vex3(1, 2, 0, l, reg, 0, 0x6F if kind == 1 else 0x7F, mem=m)
    return _evex_enc(code, "vmovdqu.vex", ptrs, smalls, "vex", 0, kind == 2, 16 << l, 1, ea)


def gen_evex_forms(rng: random.Random):
    """The EVEX block forms, with the interface of the other pools' forms
    (code, cls, ptrs, smalls); cls is "evex" and extra says what the
    generator's tests need to know of an instruction: its family ("A" .. "H",
    "U47", "U47.st" a masked U47 store, "U47.k", "vex"), its mask register,
    whether it stores, element bytes and count of what the mask counts, and
    the memory operand (base, index, scale bits, displacement). Every family
    and every U47 kind gets the same number of draws, so that none is rare."""
    from tests.golden import gen_avx512x_vectors as X
    from tests.golden.gen_avx512_vectors import evex_forms

    out = []
    by_fam = {}
    for f in X.forms():
        by_fam.setdefault(f["fam"], []).append(f)
    for fam in "ABCDEFGH":
        out += [_evex_u49(rng, rng.choice(by_fam[fam])) for _ in range(EVEX_PER_FAMILY)]
    by_kind = {}
    for form in evex_forms():
        aligned = bool(form[7].get("al"))
        by_kind.setdefault("al" if aligned else "op" if form[5] in ("op", "tern") else form[5], []).append(form)
    for kind, share in (("st", 2.0), ("ld", 0.5), ("op", 0.5), ("kd", 0.25), ("bcm", 0.12), ("bcr", 0.12), ("al", 0.12)):
        out += [_evex_u47(rng, rng.choice(by_kind[kind])) for _ in range(int(EVEX_PER_FAMILY * share))]
    out += [_evex_kop(rng) for _ in range(EVEX_PER_FAMILY // 3)]
    out += [_evex_vexmove(rng) for _ in range(EVEX_PER_FAMILY // 3)]
    return out


def _form_pool(seed: int, sse: bool, fp: bool, evex: bool = False):
    """The block pool of build() and build_shared(): the forms, their order and
    their seeds."""
    forms = _form_pool_legacy(seed, sse, fp)
    if evex:
        ev = gen_evex_forms(random.Random(seed ^ 0xE7E8))
        forms = forms + ev * max(1, round(EVEX_SHARE * len(forms) / len(ev)))
    return forms


def _form_pool_legacy(seed: int, sse: bool, fp: bool):
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
    blocks, insns); blocks: (offset of the block's first instruction, inside a
    counted loop, target of a jcc) per block; insns: {offset of a block's form
    instruction: the form}."""
    code = bytearray()
    blocks = []
    insns = {}
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
        base = WIN_VA + _extra(f).get("base", base - WIN_VA)
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
            insns[len(code) + len(setup)] = f
            body = block + bytes([0xFF, 0xC9])
            code += body + bytes([0x75, (-(len(body) + 2)) & 0xFF])
            after_guard = False
            continue
        else:
            blocks.append((len(code), False, after_guard))
            after_guard = False
        insns[len(code) + len(setup)] = f
        code += block
        if len(code) > SLOT - 64:
            break
    code += b"\xcc"
    assert len(code) <= SLOT
    return bytes(code), blocks, insns


def build_shared_info(n_lanes: int, n_programs: int, seed: int, sse: bool = False, fp: bool = False,
                      evex: bool = False):
    """build_shared plus, per program, {"va", "end" (the final int3), "blocks":
    [(rip, in_loop, jcc_target)], "evex": {rip: what gen_evex_forms says of the
    EVEX-pool instruction there}}."""
    rng = random.Random(seed)
    forms = _form_pool(seed, sse, fp, evex)
    sp = AddressSpace()
    progs = []
    for i in range(n_programs):
        code, blocks, insns = make_shared_program(rng, forms)
        va = CODE_VA + i * SLOT
        sp.map_range(va, code + b"\xcc" * (SLOT - len(code)), write=False)
        progs.append({"va": va, "end": va + len(code) - 1, "blocks": [(va + o, lp, tg) for o, lp, tg in blocks],
                      "evex": {va + o: f.extra for o, f in insns.items() if f.cls == "evex"}})
    sp.map_range(WIN_VA, bytes(rng.getrandbits(8) for _ in range(0x2000)), nx=True)
    sp.map(RO_VA, bytes(rng.getrandbits(8) for _ in range(0x1000)), write=False, nx=True)
    sp.map_range(WIN2_VA, bytes(rng.getrandbits(8) for _ in range(WIN2_LEN)), nx=True)
    sp.map_range(STACK_VA, bytes(0x2000), nx=True)
    st = user_state(CODE_VA, STACK_TOP, sp.cr3)
    if evex:
        st["xcr0"] = XCR0_AVX512
    lanes = []
    for i in range(n_lanes):
        regs = [rng.getrandbits(64) for _ in range(16)]
        regs[RSP] = STACK_TOP
        flags = 0x202 | (rng.getrandbits(12) & 0x8D5)
        lanes.append((progs[lane_program(i, n_programs)]["va"], regs, flags))
    return sp, st, lanes, progs


def lane_program(lane: int, n_programs: int) -> int:
    return (lane // LANES_PER_PROGRAM_RUN) % n_programs


def build_shared(n_lanes: int, n_programs: int, seed: int, sse: bool = False, fp: bool = False, evex: bool = False):
    """As build(), but n_lanes lanes share n_programs programs: lane i runs
    program (i // 4) % n_programs, so at 64, 32 and 16 lanes per wave every
    hardware wave holds at least 4 programs and 4 lanes of each. Registers and
    flags stay per-lane random; the programs derive per-lane effective
    addresses from them (see _flag_disp). Returns (AddressSpace, base state,
    list of (code_va, regs, flags)), as build()."""
    return build_shared_info(n_lanes, n_programs, seed, sse, fp, evex)[:3]


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


def lane_zmm(n: int, seed: int):
    """Initial zmm0-31 per lane (256 u64 each, register by register): random
    qwords mixed with the values the saturating and signed forms turn on."""
    rng = random.Random(seed ^ 0x2E2)
    special = (0, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F,
               0x8000800080008000, 0x7FFF7FFF7FFF7FFF, 0x8000000080000000, 0x0001000100010001, 0x00FF00FF00FF00FF)
    return [[rng.choice(special) if rng.random() < 0.2 else rng.getrandbits(64) for _ in range(256)] for _ in range(n)]


def lane_k(n: int, seed: int):
    """Initial k0-7 per lane: zero, all-ones, sparse (one to three bits), dense
    (all but a few bits) and random masks, so that lanes at one rip select
    different elements."""
    rng = random.Random(seed ^ 0x6B6)
    full = 0xFFFFFFFFFFFFFFFF

    def bits(k):
        v = 0
        for _ in range(k):
            v |= 1 << (rng.randrange(64) if rng.random() < 0.5 else rng.randrange(16))
        return v

    def one():
        x = rng.random()
        if x < 0.12:
            return 0
        if x < 0.27:
            return full
        if x < 0.5:
            return bits(rng.randrange(1, 4))
        if x < 0.7:
            return full & ~bits(rng.randrange(1, 6))
        return rng.getrandbits(64)

    return [[one() for _ in range(8)] for _ in range(n)]


def lane_state(n: int, seed: int, sse: bool, evex: bool = False) -> dict:
    """The per-lane vector state of a workload, as keyword arguments of
    oracle_run: nothing without sse; xmm / ymmh / mxcsr with it; with evex
    zmm (all of zmm0-31, the xmm and ymm parts included) / k / mxcsr."""
    if evex:
        return dict(zmm=lane_zmm(n, seed), k=lane_k(n, seed), mxcsr=lane_mxcsr(n, seed))
    if sse:
        return dict(xmm=lane_xmm(n, seed), ymmh=lane_xmm(n, seed, 0x4E4), mxcsr=lane_mxcsr(n, seed))
    return {}


def set_lane_state(r, i: int, xmm=None, ymmh=None, mxcsr=None, zmm=None, k=None):
    """Lane i's vector state into the register file r (wtf_amd.abi.Regs)."""
    if xmm is not None:
        for j in range(16):
            r.xmm[j][0], r.xmm[j][1] = xmm[i][2 * j], xmm[i][2 * j + 1]
    if ymmh is not None:
        for j in range(16):
            r.ymmh[j][0], r.ymmh[j][1] = ymmh[i][2 * j], ymmh[i][2 * j + 1]
    if zmm is not None:
        for j in range(32):
            q = zmm[i][8 * j: 8 * j + 8]
            if j < 16:
                r.xmm[j][0], r.xmm[j][1], r.ymmh[j][0], r.ymmh[j][1] = q[:4]
                for h in range(4):
                    r.zmmh[j][h] = q[4 + h]
            else:
                for h in range(8):
                    r.zmm_hi[j - 16][h] = q[h]
    if k is not None:
        for j in range(8):
            r.k[j] = k[i][j]
    if mxcsr is not None:
        r.mxcsr = mxcsr[i]


def get_zmm(r):
    """zmm0-31 of a register file as 256 u64."""
    out = []
    for j in range(32):
        if j < 16:
            out += [r.xmm[j][0], r.xmm[j][1], r.ymmh[j][0], r.ymmh[j][1]] + [r.zmmh[j][h] for h in range(4)]
        else:
            out += [r.zmm_hi[j - 16][h] for h in range(8)]
    return out


def oracle_run(sp: AddressSpace, st: dict, lanes, limit=20000, breakpoints=(), xmm=None, ymmh=None, mxcsr=None,
               more=(), follow_bps=False, zmm=None, k=None, writes=None):
    """Runs every lane on the CPU oracle; returns per-lane result dicts. more:
    further (va, length) ranges to read back ("more"). follow_bps: resume over
    every breakpoint hit (run(skip_bp=True)) until another exit, recording the
    hits as "stops": [(rip, icount, gprs)]. zmm / k: the per-lane AVX-512
    state (lane_zmm, lane_k); "zmm" (256 u64) and "k" (8) come back per lane.
    writes: per lane, the (va, bytes) the host writes into the lane's memory
    before it runs (VirtWrite: present bits only, the frames become dirty)."""
    from tests.oracle_lib import Oracle

    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    base = regs_from_state(st)
    o.set_limit(limit)
    o.set_breakpoints(list(breakpoints))
    out = []
    for i, (va, regs, flags) in enumerate(lanes):
        r = regs_from_state(st)
        for j in range(16):
            r.gpr[j] = regs[j]
        set_lane_state(r, i, xmm=xmm, ymmh=ymmh, mxcsr=mxcsr, zmm=zmm, k=k)
        r.rip = va
        r.rflags = flags
        o.restore(base)
        o.set_regs(r)
        for va_, data in (writes[i] if writes else ()):
            o.write_virt(va_, data)
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
            "xmm": [rr.xmm[j][h] for j in range(16) for h in range(2)], "mxcsr": rr.mxcsr,
            "ymmh": [rr.ymmh[j][h] for j in range(16) for h in range(2)],
            "zmm": get_zmm(rr), "k": list(rr.k),
        })
    return out


# (seed, sse, fp, evex) of the shared-program tests: tests/test_progfuzz_shared.py
# holds the generator to its conditions for each, tests/test_gpu_progfuzz_shared.py
# runs them on the engine.
SHARED_CASES = [(31, False, False, False), (32, False, False, False), (35, True, False, False), (34, True, True, False),
                (36, True, False, True)]


def run_gpu(sp, st, lanes, limit=20000, overlay_pages=8):
    """The lanes of build() through k_run: (the engine, run()'s statistics)."""
    import numpy as np
    from wtf_amd.engine import Engine

    n = len(lanes)
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=overlay_pages, cov_entries=4096)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(limit)
    eng.restore()
    g = eng.read_gprs()
    for i, (va, regs, flags) in enumerate(lanes):
        g[i, :16] = np.array(regs, dtype=np.uint64)
        g[i, 16] = va
        g[i, 17] = flags
    eng.write_gprs(g)
    stats = eng.run()
    return eng, stats
