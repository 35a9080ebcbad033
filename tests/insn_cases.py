"""Hand-written single-instruction cases: the one-case address space, the
vector-register accessors and the case tables more than one test file runs."""
import struct

from tests import simlane
from tests.oracle_lib import Oracle
from wtf_amd.abi import EXIT_FAULT, RUNNING, regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

CODE_VA = 0x140001000
BUF = 0x7FF000100800  # any user address: the hand-written cases do not use the native window


def layout(code: bytes, buf_va, window: bytes, cr0=None, cr4=None):
    """The address space of one case (code page, window page + the next page)
    and its initial registers."""
    page_va = buf_va & ~0xFFF
    sp = AddressSpace()
    sp.map(CODE_VA, code + b"\xcc", write=False)
    first = bytearray(4096)
    off = buf_va - page_va
    first[off:off + len(window)] = window
    sp.map(page_va, bytes(first))
    sp.map(page_va + 0x1000, b"")
    regs = regs_from_state(user_state(CODE_VA, 0, sp.cr3))
    if cr0 is not None:
        regs.cr0 = cr0
    if cr4 is not None:
        regs.cr4 = cr4
    return sp, regs


def oracle_of(sp):
    pfns, blob = sp.phys()
    return Oracle(pfns=pfns, blob=blob)


def build(code: bytes, buf_va, window: bytes, cr0=None, cr4=None):
    sp, regs = layout(code, buf_va, window, cr0, cr4)
    return oracle_of(sp), regs


def set_xmm(r, xs):
    for k in range(16):
        r.xmm[k][0], r.xmm[k][1] = xs[2 * k], xs[2 * k + 1]


def _u64(arr):
    """A ctypes array (of arrays) of u64 as a flat list, in one copy."""
    raw = bytes(arr)
    return list(struct.unpack(f"<{len(raw) // 8}Q", raw))


def get_xmm(r):
    return _u64(r.xmm)


def set_ymm(regs, ys):
    for i in range(16):
        regs.xmm[i][0], regs.xmm[i][1] = ys[4 * i], ys[4 * i + 1]
        regs.ymmh[i][0], regs.ymmh[i][1] = ys[4 * i + 2], ys[4 * i + 3]


def get_ymm(r):
    """ymm0-15 as 64 u64 in native order."""
    lo, hi = _u64(r.xmm), _u64(r.ymmh)
    return [v for i in range(0, 32, 2) for v in (lo[i], lo[i + 1], hi[i], hi[i + 1])]


def set_zmm(r, z):
    """z: 256 u64 (zmm0-31, 8 each) into the state's xmm / ymmh / zmmh / zmm_hi."""
    for i in range(32):
        q = z[8 * i: 8 * i + 8]
        if i < 16:
            r.xmm[i][0], r.xmm[i][1] = q[0], q[1]
            r.ymmh[i][0], r.ymmh[i][1] = q[2], q[3]
            for j in range(4):
                r.zmmh[i][j] = q[4 + j]
        else:
            for j in range(8):
                r.zmm_hi[i - 16][j] = q[j]


def get_zmm(r):
    """zmm0-31 as 256 u64 in native order."""
    lo, hi, top = _u64(r.xmm), _u64(r.ymmh), _u64(r.zmmh)
    out = []
    for i in range(16):
        out += lo[2 * i: 2 * i + 2] + hi[2 * i: 2 * i + 2] + top[4 * i: 4 * i + 4]
    return out + _u64(r.zmm_hi)


SSE_FAULT_CASES = [
    # (bytes, expected status, vector)
    ([0x0F, 0x28, 0x06], EXIT_FAULT, 13),             # movaps xmm0, [rsi] misaligned -> #GP(0)
    ([0x66, 0x0F, 0xEF, 0x06], EXIT_FAULT, 13),       # pxor xmm0, [rsi] misaligned
    ([0x66, 0x0F, 0x7F, 0x06], EXIT_FAULT, 13),       # movdqa [rsi], xmm0 misaligned
    ([0xF3, 0x0F, 0x6F, 0x06], RUNNING, None),        # movdqu xmm0, [rsi]: fine
    ([0x0F, 0x11, 0x06], RUNNING, None),              # movups [rsi], xmm0: fine
    ([0x0F, 0x28, 0x03], RUNNING, None),              # movaps xmm0, [rbx] aligned
    ([0x66, 0x0F, 0xD7, 0x03], EXIT_FAULT, 6),        # pmovmskb eax, [rbx]: register-only -> #UD
    ([0x66, 0x0F, 0x73, 0x1B, 0x04], EXIT_FAULT, 6),  # psrldq [rbx], 4: register-only
    ([0x0F, 0x13, 0xC1], EXIT_FAULT, 6),              # movlps xmm1, xmm0 (0f 13 reg): #UD
    ([0x0F, 0x2B, 0xC1], EXIT_FAULT, 6),              # movntps reg form: #UD
    ([0x0F, 0xC3, 0xC1], EXIT_FAULT, 6),              # movnti reg form: #UD
    ([0x0F, 0xEF, 0xC1], RUNNING, None),              # MMX pxor mm0, mm1 (U37)
    ([0x0F, 0xF7, 0xC1], RUNNING, None),              # MMX maskmovq (no byte selected: nothing written)
    ([0x0F, 0x58, 0xC1], RUNNING, None),              # addps (floating point, U39)
    ([0xF2, 0x0F, 0xF0, 0x03], RUNNING, None),        # lddqu (SSE3, U39)
    ([0x0F, 0x53, 0xC1], RUNNING, None),              # rcpps (the host CPU's table, U40)
]


def run_case(code, sim=False, cr0=None, cr4=None, mx=0x1F80, xmm=None):
    """One instruction with rsi misaligned for 16-byte operands, on the oracle
    or (sim) the engine's host build: (status, vector, mxcsr, xmm0-15)."""
    sp, regs = layout(bytes(code), BUF, b"\0" * 256, cr0, cr4)
    regs.gpr[6] = BUF + 4
    regs.mxcsr = mx
    for i, v in (xmm or {}).items():
        regs.xmm[i][0], regs.xmm[i][1] = v
    if sim:
        ex, r, _ = simlane.run(sp, regs)
    else:
        o = oracle_of(sp)
        o.restore(regs)
        ex = o.step()
        r = o.regs()
    return ex.status, ex.vector, r.mxcsr, [(r.xmm[i][0], r.xmm[i][1]) for i in range(16)]


def norm(status):
    """A clean step: RUNNING from the oracle, the int3 behind the instruction from the engine."""
    return RUNNING if status == 3 else status


def move_case(code_hex, off_src, off_dst, cr0=None, cr4=None, xcr0=None):
    """A vector move over a patterned page: rsi / rdi at the two offsets,
    distinct xmm / ymm-high values in every register."""
    code = bytes.fromhex(code_hex)
    page = BUF & ~0xFFF
    sp, regs = layout(code, page, bytes((i * 7 + 3) & 0xFF for i in range(4096)), cr0=cr0, cr4=cr4)
    regs.gpr[6] = page + off_src  # rsi
    regs.gpr[7] = page + off_dst  # rdi
    for k in range(16):
        regs.xmm[k][0], regs.xmm[k][1] = 0x1111111111111111 * (k + 1), 0x0101010101010101 * (k + 3)
        regs.ymmh[k][0], regs.ymmh[k][1] = 0xA0A0A0A0A0A0A0A0 + k, 0xB0B0B0B0B0B0B0B0 + k
    if xcr0 is not None:
        regs.xcr0 = xcr0
    return sp, regs


def widening_program(vzu):
    """A kernel stub that writes vector registers through VEX while XCR0 = 7,
    then widens XCR0 to 0xe7 and stores zmm0 / 1 / 3 / 5 with vmovdqu64. A VEX
    write zeroes the destination up to MAXVL (bits 511:128 / 511:256; SDM vol. 1
    15.5) whatever XCR0 enables, so the stores show zeros there."""
    from tests.golden.gen_avx512_vectors import evex

    code = bytes.fromhex(
        "0f05" "cccccccccccc"   # 0  syscall -> lstar = 8 (ring 0: xsetbv is privileged)
        "c5fa6f0e"              # 8  vmovdqu xmm1, [rsi]    VEX.128 load
        "c5fe6fda"              #    vmovdqu ymm3, ymm2     VEX.256 register move
        + ("c5f877" if vzu else "") +  # vzeroupper
        "b900000000" "b8e7000000" "ba00000000"  # mov ecx, 0; mov eax, 0xe7; mov edx, 0
        "0f01d1")               #    xsetbv
    for slot, reg in enumerate((0, 1, 3, 5)):
        code += bytes(evex(1, 2, 1, 2, 0, 0, 0, reg, 0, 0x7F, mem=(7, None, 0, slot, 1)))  # vmovdqu64 [rdi + 64 * slot], zmm
    return code
