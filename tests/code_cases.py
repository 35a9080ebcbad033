"""Code the uop cache cannot serve: instructions that cross a page edge and
instructions on a page the lane has written (k_run's slow_step,
wtf_amd/csrc/engine_run.h). TEST INFRASTRUCTURE ONLY: the case tables and the
runners of the oracle and of the host lane build; tests/test_code_cases.py and
tests/test_gpu_code_cases.py run them. Nothing here is expected because an
engine does it: every expectation is the oracle's run of the same lane.

The split table: one instruction, then int3, with k bytes at the end of a page
(every k from 1 to its length; at k = length the int3 starts the next page), for
instructions whose every decode field meets the edge (SPLIT_INSNS), and for
every kind of second page (SPLIT_KINDS). The programs (PROGRAMS): short
self-modifying programs whose patch comes from a per-lane register, so that
lanes at one rip run different bytes.

A lane is (name, Regs, writes): `writes` are the host's writes into the lane's
memory before it runs, (address, bytes, physical)."""
import functools
import random
import struct
from collections import namedtuple

from tests import progfuzz
from wtf_amd.abi import EXIT_BREAKPOINT, EXIT_FAULT, Regs, regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

LIMIT = 1000
DATA_VA = 0x200000000    # two RW pages
STACK_VA = 0x300000000   # two RW pages
STACK_TOP = STACK_VA + 0x2000 - 0x100
STUB_VA = 0x400000000    # a read-only page: the stores of the guest-written kinds, then jmp rsi
SMC_VA = 0x500000000     # the programs, 0x10000 apart
ALIAS_VA = 0x580000000   # program c's writable, non-executable view of its read-only page
FRESH_VA = 0x5C0000000   # program g's empty RW+X page
VIEW_VA = {"pp": 0x1000000000, "absent": 0x1100000000, "nx": 0x1200000000, "u0": 0x1300000000}
# k_run runs the group at the lowest rip first (engine_run.h, the fast loop's group choice), so the lanes that
# start in the stub reach a split point's instruction while the lanes that start there still wait
assert STUB_VA < min(VIEW_VA.values())
PAIR = 0x4000            # a split pair's two pages, then two unmapped ones
XCR0_AVX512 = progfuzz.XCR0_AVX512
RAX, RCX, RDX, RBX, RSP, RBP, RSI, RDI, R8, R9, R12, R13 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13

Lane = namedtuple("Lane", "name regs writes")


def u32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


def u64(v):
    return struct.pack("<Q", v & 0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------- the split table
MOV64 = b"\x48\xb8" + u64(0x1122334455667788)
# name: (bytes, rflags). Each field kind of decode() that can run out of bytes:
# opcode / ModRM (inc), the immediate (mov), prefixes up to and past the limit,
# SIB + disp32 + imm32, the two-byte opcode's disp32 (nop), rel32 of a branch
# taken and not, a call's return address, a VEX prefix with a rip-relative
# disp32, EVEX's four bytes with a disp32, VEX with a vector SIB.
SPLIT_INSNS = {
    "inc": (b"\xff\xc0", 0x202),
    "mov64": (MOV64, 0x202),
    "mov64-p5": (b"\x2e" * 5 + MOV64, 0x202),      # 15 bytes
    "mov64-p6": (b"\x2e" * 6 + MOV64, 0x202),      # 16 bytes: #GP, unless the fetch faults first (U52)
    "alu-sib": (b"\x81\x84\x8b" + u32(0x40) + u32(0x12345678), 0x202),   # add dword [rbx+rcx*4+0x40], imm32
    "nop10": (b"\x66\x2e\x0f\x1f\x84\x00\x00\x00\x00\x00", 0x202),
    "jz-taken": (b"\x0f\x84" + u32(0x20), 0x242),
    "jz-not": (b"\x0f\x84" + u32(0x20), 0x202),
    "call": (b"\xe8" + u32(0x40), 0x202),
    "vmovdqu-rip": (None, 0x202),                  # vmovdqu ymm0, [rip+disp32]: the first page's offset 0x100
    "evex-disp32": (b"\x62\xf1\xfe\x48\x6f\x83" + u32(0x80), 0x202),     # vmovdqu64 zmm0, [rbx+0x80]
    "gather": (b"\xc4\xe2\x65\x90\x8c\x93" + u32(0x20), 0x202),          # vpgatherdd ymm1, [rbx+ymm2*4+0x20], ymm3
}
SPLIT_KINDS = ("pool", "host2", "guest2", "absent", "nx", "u0", "priv1", "priv12")


def split_bytes(name, k):
    code = SPLIT_INSNS[name][0]
    if code is None:   # the load's address does not move with k: rip-relative from the end of the instruction
        code = b"\xc5\xfe\x6f\x05" + u32(0x100 - (0x1000 - k + 8))
    return code


def split_len(name):
    return len(split_bytes(name, 1))


def split_points():
    """[(instruction, k)] in table order: the pair index of each."""
    return [(name, k) for name in SPLIT_INSNS for k in range(1, split_len(name) + 1)]


# ---------------------------------------------------------------- a small assembler for the programs
class Asm:
    def __init__(self, va):
        self.va, self.b, self.labels, self.fix = va, bytearray(), {}, []

    def __call__(self, *parts):
        for p in parts:
            self.b += bytes([p]) if isinstance(p, int) else bytes(p)
        return self

    def here(self):
        return self.va + len(self.b)

    def label(self, name):
        self.labels[name] = self.here()
        return self

    def rel(self, op, name, n):
        """op, then the n-byte displacement of `name` from the next instruction."""
        self(op)
        self.fix.append((len(self.b), n, name, None))
        self.b += bytes(n)
        return self

    def lea_rdi(self, name):
        return self.rel(b"\x48\x8d\x3d", name, 4)

    def mov_abs(self, reg, name, add=0, base=None):
        """mov reg, imm64: the address of `name` (+ add), seen from `base` instead of the program's own view."""
        self(progfuzz.mov_imm64(reg, 0)[:2])
        self.fix.append((len(self.b), 8, name, (add, base)))
        self.b += bytes(8)
        return self

    def done(self):
        for at, n, name, absolute in self.fix:
            t = self.labels[name]
            if absolute is None:
                v = t - (self.va + at + n)
                assert -(1 << (8 * n - 1)) <= v < 1 << (8 * n - 1), name
            else:
                add, base = absolute
                v = t + add if base is None else base + (t - (self.va & ~0xFFF)) + add
            self.b[at:at + n] = (v & ((1 << (8 * n)) - 1)).to_bytes(n, "little")
        return bytes(self.b)


NOP = 0x90
ST_R12D = b"\x44\x89\x27"    # mov [rdi], r12d
ST_R12 = b"\x4c\x89\x27"     # mov [rdi], r12
TAIL = b"\x48\x83\xc0\x01\xcc"   # add rax, 1 ; int3
RUN = (b"\xb8\x01\x00\x00\x00" b"\x83\xc0\x02" b"\x6b\xc0\x03" b"\x4c\x01\xe0" b"\x48\xc1\xc0\x03" b"\x48\x31\xdb"
       b"\x48\x01\xc3" + SPLIT_INSNS["nop10"][0])   # mov eax,1; add eax,2; imul eax,eax,3; add rax,r12; rol rax,3;
#                                                     xor rbx,rbx; add rbx,rax; nop
LOOP = b"\x4c\x01\xe0" b"\x48\xc1\xc0\x03" b"\xff\xc9"   # add rax, r12 ; rol rax, 3 ; dec ecx


def _prog_a(va):
    a = Asm(va)
    a.lea_rdi("imm")(ST_R12D).label("patched")(0xB8).label("imm")(u32(0x11111111))(TAIL)
    return a


def _prog_b(va):
    a = Asm(va)
    a(b"\xb9\x03\x00\x00\x00", b"\x31\xc0").label("patched")(0x05).label("imm")(u32(0x10))
    a(b"\x4d\x85\xed").rel(0x74, "skip", 1).lea_rdi("imm")(ST_R12D).label("skip")(b"\xff\xc9").rel(0x75, "patched", 1)
    a.label("end")(0xCC)
    return a


def _prog_c(va):
    a = Asm(va)
    a.mov_abs(RDI, "imm", base=ALIAS_VA)(ST_R12D).label("patched")(0xB8).label("imm")(u32(0x22222222))(TAIL)
    return a


def _prog_d1(va):   # rep stosb over the immediate ahead
    a = Asm(va)
    a(b"\x44\x89\xe0").lea_rdi("imm")(b"\xb9\x04\x00\x00\x00", b"\xf3\xaa").label("patched")(0xBB).label("imm")
    a(u32(0x33333333), 0xCC)
    return a


def _prog_d2(va):   # movdqu: sixteen nops become a ten-byte mov and six nops
    a = Asm(va)
    a.lea_rdi("patched")(b"\xf3\x0f\x7f\x07").label("patched")(bytes([NOP] * 16), 0xCC)
    return a


def _prog_d3(va):   # vmovdqu ymm: two ten-byte movs, or ud2
    a = Asm(va)
    a.lea_rdi("patched")(b"\xc5\xfe\x7f\x0f").label("patched")(bytes([NOP] * 32), 0xCC)
    return a


def _prog_d4(va):   # lock cmpxchg: four nops become int3, ud2, inc eax or stay
    a = Asm(va)
    a(0xB8, u32(0x90909090), b"\x44\x89\xe2").lea_rdi("patched")(b"\xf0\x0f\xb1\x17").label("patched")
    a(bytes([NOP] * 4), 0xCC)
    return a


def _prog_d5(va):   # push onto the code ahead
    a = Asm(va)
    a.mov_abs(RSP, "patched", add=8)(b"\x41\x54").label("patched")(bytes([NOP] * 8), 0xCC)
    return a


def _prog_f(va, first=b""):
    a = Asm(va)
    a(first).lea_rdi("data")(ST_R12).label("patched")(RUN, b"\x44\x89\xe9").label("loop")(LOOP).rel(0x75, "loop", 1)
    a.label("end")(0xCC)
    a.labels["data"] = va + 0x800
    return a


def _prog_i(va):    # f behind two data stores: with one overlay page the code page's copy is the third
    return _prog_f(va, b"\x4c\x89\x23" b"\x4c\x89\xa3\x00\x10\x00\x00")   # mov [rbx], r12 ; mov [rbx+0x1000], r12


def _prog_g(va):
    a = Asm(va)
    a.mov_abs(RSI, "tmpl")(progfuzz.mov_imm64(RDI, FRESH_VA), b"\xb9\x09\x00\x00\x00", b"\xf3\xa4")
    a(progfuzz.mov_imm64(RDI, FRESH_VA + 1), ST_R12D, progfuzz.mov_imm64(RSI, FRESH_VA), b"\xff\xd6").label("end")(0xCC)
    a.label("tmpl")(0xB8, u32(0x55555555), b"\x44\x01\xe0", 0xC3)   # mov eax, imm32 ; add eax, r12d ; ret
    a.labels["patched"] = FRESH_VA
    return a


def _prog_e(va):
    """Pages: data, the target (four nops, then int3s), the program (read-only)."""
    a = Asm(va + 0x2000)
    a(progfuzz.mov_imm64(RDI, va + 0x1000 - 4), ST_R12, progfuzz.mov_imm64(RSI, va + 0x1000), b"\xff\xe6")
    a.labels["patched"] = va + 0x1000
    return a


def _prog_h(va):
    """The patched mov rax, imm64 has five bytes on the first page; lanes with
    r13 = 0 leave it alone."""
    a = Asm(va + 0xFFB - 18)
    a(b"\x4d\x85\xed").rel(0x74, "patched", 1).mov_abs(RDI, "patched", add=2)(ST_R12).label("patched")
    a(b"\x48\xb8", u64(0x4444444444444444), 0xCC)
    assert a.labels["patched"] == va + 0xFFB
    return a


PROGRAMS = {"a": _prog_a, "b": _prog_b, "c": _prog_c, "d1": _prog_d1, "d2": _prog_d2, "d3": _prog_d3, "d4": _prog_d4,
            "d5": _prog_d5, "e": _prog_e, "f": _prog_f, "g": _prog_g, "h": _prog_h, "i": _prog_i}
VARIANTS = 8   # per-lane parameter sets of a program


def _mov_rax(v):
    return b"\x48\xb8" + u64(v)


def prog_params(name, j, plain=False):
    """Lane variant j of a program: ({gpr: value}, xmm0 or None, ymm1 or None).
    plain: the variant that patches nothing, or patches in the bytes that are
    there already."""
    v = 0x0101010101010101 * (j + 1) ^ 0x00F0E0D0C0B0A090
    g, x0, y1 = {R12: v, R13: j & 1, RBX: DATA_VA + 0x200}, None, None
    if plain:
        g[R13] = 0
    if name in ("f", "i"):
        g[R13] = 2 + j
    elif name == "a" and plain:
        g[R12] = 0x11111111
    elif name == "c" and plain:
        g[R12] = 0x22222222
    elif name == "d1":
        g[R12] = 0x33 if plain else 0x40 + j
    elif name == "d2":
        x0 = bytes([NOP] * 16) if plain else _mov_rax(v) + bytes([NOP] * 6)
    elif name == "d3":
        y1 = (bytes([NOP] * 32) if plain else (b"\x0f\x0b" if j % 4 == 3 else b"") + _mov_rax(v) +
              progfuzz.mov_imm64(RBX, ~v))
        y1 = y1 + bytes([NOP] * (32 - len(y1)))
    elif name == "d4":
        g[R12] = 0x90909090 if plain else (0x909090CC, 0x90900B0F, 0x9090C0FF, 0x90909090)[j % 4]
    elif name == "d5":
        g[R12] = int.from_bytes(bytes([NOP] * 8) if plain else b"\x48\xc7\xc3" + u32(v) + b"\x90", "little")
    elif name == "e":
        tail = b"\x90\x90\x90\x90" if plain else (b"\xff\xc0\xff\xc0", b"\xff\xc8\x90\x90", b"\x48\xff\xc0\x90",
                                                    b"\x90\x90\x90\xcc")[j % 4]
        g[R12] = int.from_bytes(u32(v) + tail, "little")
    elif name == "g" and plain:
        g[R12] = 0x55555555
    return g, x0, y1


# ---------------------------------------------------------------- the address space
def _pattern(seed, n):
    rng = random.Random(seed)
    return bytes(rng.getrandbits(8) for _ in range(n))


@functools.lru_cache(maxsize=None)
def space():
    """(AddressSpace, base state, info): info["split"][(insn, k)] = the pair's
    index; info["prog"][name] = {"entry", "labels", "pages" (its code pages' vas)}."""
    sp = AddressSpace()
    sp.map_range(DATA_VA, _pattern(1, 0x2000), nx=True)
    sp.map_range(STACK_VA, bytes(0x2000), nx=True)
    stub = Asm(STUB_VA)
    stub.label("one")(b"\x41\x88\x10", b"\xff\xe6")                     # mov [r8], dl ; jmp rsi
    stub.label("two")(b"\x41\x88\x10", b"\x41\x88\x11", b"\xff\xe6")    # mov [r8], dl ; mov [r9], dl ; jmp rsi
    sp.map(STUB_VA, stub.done() + b"\xcc" * 64, write=False)
    info = {"stub": dict(stub.labels), "split": {}, "prog": {}, "frames": {}}
    for p, (name, k) in enumerate(split_points()):
        code = split_bytes(name, k)
        a = bytearray(b"\xcc" * 0x1000)
        a[0x100:0x140] = _pattern(2, 0x40)
        a[0x1000 - k:] = code[:k]
        b = bytearray(b"\xcc" * 0x1000)
        b[:len(code) - k] = code[k:]
        info["split"][name, k] = p
        # one pair of frames behind all four views: the same code frame runs at four addresses (the uop
        # cache is keyed by the frame)
        fa, fb = sp.alloc(bytes(a)), sp.alloc(bytes(b))
        info["frames"][p] = (fa, fb)
        for view, base in VIEW_VA.items():
            sp.map_pfn(base + p * PAIR, fa)
            if view != "absent":
                sp.map_pfn(base + p * PAIR + 0x1000, fb, user=view != "u0", nx=view == "nx")
    for n, (name, make) in enumerate(PROGRAMS.items()):
        va = SMC_VA + n * 0x10000
        a = make(va)
        code = a.done()
        start = a.va
        img = bytearray(b"\xcc" * 0x3000)
        img[start - va:start - va + len(code)] = code
        if name == "e":
            img[:0x1000] = _pattern(3, 0x1000)
            img[0x1000:0x1004] = bytes([NOP] * 4)
            sp.map(va, bytes(img[:0x1000]), nx=True)
            sp.map(va + 0x1000, bytes(img[0x1000:0x2000]))
            sp.map(va + 0x2000, bytes(img[0x2000:]), write=False)
            pages = [va + 0x1000, va + 0x2000]
        elif name == "c":
            pfn = sp.map(va, bytes(img[:0x1000]), write=False)
            sp.map_pfn(ALIAS_VA, pfn, nx=True)
            pages = [va]
        elif name == "g":
            sp.map(va, bytes(img[:0x1000]), write=False)
            sp.map(FRESH_VA, bytes(0x1000))
            pages = [va]   # (the fresh page is not among the code pages: its coverage goes to the extra set)
        elif name == "h":
            sp.map_range(va, bytes(img[:0x2000]))
            pages = [va, va + 0x1000]
        else:
            sp.map(va, bytes(img[:0x1000]))
            pages = [va]
        info["prog"][name] = {"entry": start, "labels": dict(a.labels), "pages": pages}
    st = user_state(STUB_VA, STACK_TOP, sp.cr3)
    st["xcr0"] = XCR0_AVX512
    return sp, st, info


def _regs(rip, flags, gprs, salt, xmm0=None, ymm1=None):
    _, st, _ = space()
    r = Regs.from_buffer_copy(regs_from_state(st))
    rng = random.Random(0xC0DE ^ salt)
    for i in range(16):
        r.gpr[i] = rng.getrandbits(64)
    z = progfuzz.lane_zmm(1, 0x51 ^ salt)
    progfuzz.set_lane_state(r, 0, zmm=z)
    r.gpr[RSP] = STACK_TOP
    r.gpr[RBX] = DATA_VA + 0x100
    r.gpr[RCX] = salt & 3
    for k, v in gprs.items():
        r.gpr[k] = v & 0xFFFFFFFFFFFFFFFF
    # the gather's dword indices (ymm2) and its mask (ymm3: every element)
    idx = struct.unpack("<4Q", b"".join(u32((3 * i + salt) % 24) for i in range(8)))
    r.xmm[2][0], r.xmm[2][1], r.ymmh[2][0], r.ymmh[2][1] = idx
    r.xmm[3][0] = r.xmm[3][1] = r.ymmh[3][0] = r.ymmh[3][1] = 0xFFFFFFFFFFFFFFFF
    if xmm0 is not None:
        r.xmm[0][0], r.xmm[0][1] = struct.unpack("<2Q", xmm0)
    if ymm1 is not None:
        r.xmm[1][0], r.xmm[1][1], r.ymmh[1][0], r.ymmh[1][1] = struct.unpack("<4Q", ymm1)
    r.rip, r.rflags = rip, flags
    return r


def split_va(name, k, view="pp"):
    """(the first page's va, the instruction's va) of a split point in a view."""
    _, _, info = space()
    a = VIEW_VA[view] + info["split"][name, k] * PAIR
    return a, a + 0x1000 - k


def split_lane(name, k, kind, salt=0):
    """One lane of the split table. The faulting kinds start at the instruction
    itself (the fault leaves icount 0 and rip where it was); the guest-written
    kinds start in the stub, whose stores (the lane's own dl) make the first,
    the second or both pages private before it jumps to the instruction."""
    sp, _, info = space()
    view = kind if kind in ("absent", "nx", "u0") else "pp"
    a, va = split_va(name, k, view)
    g = {RDX: 0x5A ^ salt, RSI: va}
    rip, writes = va, ()
    if kind == "host2":   # the bytes it has already: only the page pointer changes
        fb = info["frames"][info["split"][name, k]][1]
        writes = ((a + 0x1000, bytes(sp.pages[fb][:16]), False),)
    elif kind == "guest2":
        rip, g[R8] = info["stub"]["one"], a + 0x1800
    elif kind == "priv1":
        rip, g[R8] = info["stub"]["one"], a + 0x800
    elif kind == "priv12":
        rip, g[R8], g[R9] = info["stub"]["two"], a + 0x800, a + 0x1800
    return Lane(f"{name}/{k}/{kind}" + (f"/{salt}" if salt else ""), _regs(rip, SPLIT_INSNS[name][1], g, salt), writes)


def split_lanes(kinds=SPLIT_KINDS, salt=0):
    return [split_lane(name, k, kind, salt) for name, k in split_points() for kind in kinds]


def pte_gpa(va):
    """The guest-physical address of va's leaf entry."""
    sp, _, _ = space()
    table = sp.cr3 >> 12
    for level in (3, 2, 1):
        table = (sp._entry(table, (va >> (12 + 9 * level)) & 0x1FF) & 0x000FFFFFFFFFF000) >> 12
    return (table << 12) + ((va >> 12) & 0x1FF) * 8


def split_lane_unmapped(name, k, salt=0):
    """The pool kind with the second page's entry cleared for this lane alone
    (a physical host write): absent, in the view every other lane has present."""
    a, _ = split_va(name, k)
    lane = split_lane(name, k, "pool", salt)
    return Lane(lane.name.replace("pool", "edit"), lane.regs, ((pte_gpa(a + 0x1000), bytes(8), True),))


def prog_lane(name, j, plain=False):
    _, _, info = space()
    g, x0, y1 = prog_params(name, j, plain)
    rip = info["prog"][name]["entry"]
    return Lane(f"{name}/{j}" + ("/plain" if plain else ""), _regs(rip, 0x202, g, 0x100 + j, x0, y1), ())


def prog_lanes(names=None, plain=False, swap=False):
    """Every variant of every program, program by program (the VARIANTS lanes
    of one program are neighbours: one group at its first rip). swap: the
    variants in reverse order, so that a lane gets another lane's patch."""
    order = range(VARIANTS - 1, -1, -1) if swap else range(VARIANTS)
    return [prog_lane(n, j, plain) for n in (names or PROGRAMS) for j in order]


def prog_breakpoints(names=None):
    """The patched instruction of every program, and f's / i's loop head and
    b's: instructions on private pages."""
    _, _, info = space()
    out = set()
    for n in names or PROGRAMS:
        lab = info["prog"][n]["labels"]
        out.add(lab["patched"])
        if "loop" in lab:
            out.add(lab["loop"])
    return sorted(out)


def split_breakpoints(names, views=tuple(VIEW_VA)):
    """The instruction of every split point of `names`, at its address in each of `views`."""
    return sorted({split_va(name, k, view)[1] for name, k in split_points() if name in names for view in views})


def code_vpns(fresh=False):
    """The vpns of every page code is meant to run from (set_code_pages);
    program g's fresh page only on request."""
    _, _, info = space()
    out = {STUB_VA >> 12}
    for base in VIEW_VA.values():
        for p in info["frames"]:
            out |= {(base + p * PAIR) >> 12, (base + p * PAIR + 0x1000) >> 12}
    for d in info["prog"].values():
        out |= {va >> 12 for va in d["pages"]}
    if fresh:
        out.add(FRESH_VA >> 12)
    return sorted(out)


# ---------------------------------------------------------------- the executors
def new_oracle():
    from tests.oracle_lib import Oracle
    sp, _, _ = space()
    pfns, blob = sp.phys()
    return Oracle(pfns=pfns, blob=blob)


def _zmm(r):
    return progfuzz.get_zmm(r)


def start_oracle(o, lane, limit=LIMIT, bps=(), edges=False):
    o.set_limit(limit)
    o.set_breakpoints(list(bps))
    o.set_edges(edges)
    o.restore(lane.regs)
    for addr, data, phys in lane.writes:
        if phys:
            o.write_phys(addr, bytes(data))
        else:
            o.write_virt(addr, bytes(data))


def run_oracle(o, lane, limit=LIMIT, bps=(), edges=False):
    """The lane's result on the oracle, breakpoints followed ("stops")."""
    start_oracle(o, lane, limit, bps, edges)
    ex = o.run()
    stops = []
    while ex.status == EXIT_BREAKPOINT:
        rr = o.regs()
        stops.append((rr.rip, ex.icount, list(rr.gpr)))
        ex = o.run(skip_bp=True)
    r = o.regs()
    dirty = sorted(g >> 12 for g in o.dirty())
    return {"status": ex.status, "vector": ex.vector, "error": ex.error, "addr": ex.addr, "rip": r.rip,
            "icount": ex.icount, "gpr": list(r.gpr), "rflags": r.rflags, "zmm": _zmm(r), "dirty": dirty,
            "mem": {p: o.read_phys(p << 12, 4096) for p in dirty}, "cov": set(o.coverage()), "stops": stops,
            "bytes": o.nbytes()}


def run_sim(image, lane, fast, limit=LIMIT):
    """The lane on the host lane build (tests/native/sim_lane.cc): no coverage,
    no breakpoints, no physical writes."""
    from tests import simlane
    assert not any(phys for _, _, phys in lane.writes)
    pages = simlane.page_buffer()
    res, fin, cnt = simlane.run(image, lane.regs, limit=limit, fast=fast, pages=pages,
                                writes=[(va, d) for va, d, _ in lane.writes])
    k = min(res.ovn, 64)
    dirty = [int(res.dirty[i]) >> 12 for i in range(k)]
    return {"status": res.status, "vector": res.vector, "error": res.error, "addr": res.addr, "rip": res.rip,
            "icount": res.icount, "gpr": list(res.gpr), "rflags": res.rflags, "zmm": _zmm(fin), "dirty": sorted(dirty),
            "mem": {p: pages.raw[i * 4096:(i + 1) * 4096] for i, p in enumerate(dirty)}, "bytes": res.nbytes,
            "fast": cnt}


FAULT_KEYS = ("vector", "error", "addr")
KEYS = ("status", "rip", "icount", "gpr", "rflags", "zmm", "dirty", "mem", "bytes", "cov", "stops")


def diff(got, want, keys=KEYS):
    """The first field in which a result differs from the oracle's (bit-exact;
    a field an executor does not report is not in `got`), or None."""
    for k in keys + (FAULT_KEYS if want["status"] == EXIT_FAULT else ()):
        if k in got and got[k] != want[k]:
            if k in ("gpr", "zmm"):
                return k, [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:4]
            if k == "mem":
                return k, [(hex(p), next(i for i in range(4096) if got[k].get(p, b"")[i:i + 1] != want[k][p][i:i + 1]))
                           for p in want[k] if got[k].get(p) != want[k][p]][:4]
            if k == "cov":
                return k, sorted(hex(v) for v in got[k] ^ want[k])[:8]
            return k, got[k], want[k]
    return None
