"""One address space ("the zoo") with every kind of mapping the page walk has a
branch for, and a table of cases over it. A case is a few memory accesses made
by a short guest program (up to three warm-ups, an optional invlpg, one probed
access) at CPL 3 or 0 with CR0.WP set or clear; what it must do comes from
tests/paging_model.py alone (expect()). tests/test_paging.py runs the table on
the oracle and on the engine's host build, tests/test_gpu_paging.py on the GPU.

Programs are assembled from the kinds of a case's accesses, so cases with the
same kinds share one program and differ in their registers: access i takes
its address from r8 + slot and a store's value from r12 + slot (xmm / ymm
4 + slot), a load lands in rbx, rbp, rsi, rdx, rcx (xmm / ymm 0 ..) by position.
Every program ends in int3, which exits the lane before retiring (U12); the
IDT has no gates, so a fault ends the lane with its vector, error code and
address (U11)."""
from __future__ import annotations

import dataclasses
import functools
import struct

from wtf_amd.abi import regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, seg, user_state

from tests import paging_model as M
from tests import sysprog2 as S2

P, RW, US, PS, XD = M.P, M.RW, M.US, M.PS, M.XD
MASK64 = 2**64 - 1
EXIT_INT3, EXIT_FAULT = 3, 5
TLB_N = 4  # the lane TLB's entries, filled round-robin (engine_device.h)

# bits a walk must ignore: G, A, D, the software bits 9-11 and 52-62 (Windows
# keeps its working-set index there); PAT is bit 12 of a large leaf, bit 7 of a PTE
IGN = 0x100 | 0x20 | 0x40 | 0xE00 | (0x7FF << 52)
IGN_LARGE, IGN_4K = IGN | 0x1000, IGN | 0x80

# ---------------------------------------------------------------- the zoo's addresses
U1G = 0x7F8000000000            # 1 GiB leaf -> G1
U1G_IGN, U1G_W0, U1G_U0, U1G_NX = (U1G + (i << 30) for i in (2, 3, 4, 5))
U2 = U1G + (1 << 30)            # a page directory
L2, AFTER, L2_IGN, AFTER_NX, L2_B, HOLE, L2_W0, L2_U0, L2_NX = (U2 + (i << 21) for i in range(3, 12))
G1, G2, G2_W0, G2_U0, G2_NX = 0x40000000, 0x200000, 0x400000, 0x600000, 0x800000
GIB, MIB2 = 1 << 30, 1 << 21
PLACE = {(bit, level): ((0x10 + 4 * b + (4 - level)) << 39) | 0x1000
         for b, bit in enumerate(("W0", "U0", "NX")) for level in (4, 3, 2, 1)}
CLEAN4, IGN4 = 0x20 << 39, (0x20 << 39) | 0x1000
AL = 0x21 << 39
A1, B1, B2, A3 = AL, AL + 0x10000, AL + 0x20000, AL + 0x30000
A2 = L2 + 0x1000
CODE, KCODE = 0x140000000, 0xFFFFF80000600000
LASTU = 0x7FFFFFFFF000          # the last page below the canonical hole
KSTACK, KDATA = 0xFFFFF80000300000, 0xFFFFF80000800000
PRE = 0xFFFFF80000A00000        # a data page, then the windows on KDATA's tables
PTWIN, PDWIN, PDPTWIN = PRE + 0x1000, PRE + 0x2000, PRE + 0x3000
KLEAF = 0xFFFFF80000C00000      # a 2 MiB leaf whose first frame holds a page table
KLINK = 0xFFFFF80000E00000      # an empty PDE: a table is linked in at run time
LWIN = 0xFFFFF80001000000       # a 2 MiB leaf over the frames the tables live in
B3 = 0xFFFFF80001200000
GKLEAF, GLWIN = 0xA00000, 0x1000000
TARGET = b"\xb8\xde\xc0\x0d\x60\xcc"   # mov eax, 0x600dc0de; int3
TGT = 0x800                     # where a page that can be jumped into holds TARGET
MAGIC = 0x600DC0DE


def put(sp, va, level, entry, upper=None):
    """Write va's entry of `level` (4 = PML4E .. 1 = PTE); tables on the way are
    made as needed, entered with upper.get(level, P|RW|US). Returns the pfn of
    the table that holds the entry."""
    table = sp.cr3 >> 12
    for lv in (4, 3, 2, 1):
        idx = (va >> (12 + 9 * (lv - 1))) & 0x1FF
        if lv == level:
            sp._set_entry(table, idx, entry)
            return table
        e = sp._entry(table, idx)
        if not e & P:
            e = (sp.alloc() << 12) | (upper or {}).get(lv, P | RW | US)
            sp._set_entry(table, idx, e)
        assert not e & PS
        table = (e & M.ADDR) >> 12


def own(pfn: int) -> bytearray:
    """A frame in which every qword holds its own physical address."""
    return bytearray(b"".join(struct.pack("<Q", (pfn << 12) + 8 * i) for i in range(512)))


def _frame(sp, pfn=None, code_at=None):
    if pfn is None:
        pfn = sp.alloc()
    sp.pages[pfn] = own(pfn)
    if code_at is not None:
        sp.pages[pfn][code_at:code_at + len(TARGET)] = TARGET
    return pfn


def _build(blob: bytes):
    sp = AddressSpace()
    f = {}
    put(sp, CODE, 1, 0)   # the code's tables first, so that no frame number below depends on the programs
    put(sp, KCODE, 1, 0)
    # ---- large leaves
    for va, flags in ((U1G, 7), (U1G_IGN, 7 | IGN_LARGE), (U1G_W0, 5), (U1G_U0, 3), (U1G_NX, 7 | XD)):
        put(sp, va, 3, G1 | PS | flags)
    for va, gpa, flags in ((L2, G2, 7), (L2_IGN, G2, 7 | IGN_LARGE), (L2_B, G2, 7), (L2_W0, G2_W0, 5),
                           (L2_U0, G2_U0, 3), (L2_NX, G2_NX, 7 | XD)):
        put(sp, va, 2, gpa | PS | flags)
    for gpa in (G1, G1 + 0x1000, G1 + GIB - 0x1000, G2, G2 + 0x1000, G2 + MIB2 - 0x1000, G2_W0, G2_U0, G2_NX):
        _frame(sp, gpa >> 12, TGT if gpa & 0xFFFFF == 0 else None)  # (first frames: a jump target)
    # code across two 4 KiB frames inside the 2 MiB leaf, and across its end
    for gpa in (G2 + 0xFFD, G2 + MIB2 - 3):
        for i, b in enumerate(TARGET):
            if (gpa + i) >> 12 in sp.pages and gpa + i < G2 + MIB2:
                sp.pages[(gpa + i) >> 12][(gpa + i) & 0xFFF] = b
    f["after"] = _frame(sp)
    sp.pages[f["after"]][:3] = TARGET[3:]
    put(sp, AFTER, 1, f["after"] << 12 | 7)
    f["after_nx"] = _frame(sp)
    sp.pages[f["after_nx"]][:3] = TARGET[3:]
    put(sp, AFTER_NX, 1, f["after_nx"] << 12 | 7 | XD)
    # ---- W = 0, U = 0, NX at exactly one level of a 4 KiB mapping, each under its own PML4E
    bits = {"W0": lambda e: e & ~RW, "U0": lambda e: e & ~US, "NX": lambda e: e | XD}
    for (bit, level), va in PLACE.items():
        fl = {lv: bits[bit](7) if lv == level else 7 for lv in (4, 3, 2, 1)}
        f[bit, level] = _frame(sp, code_at=TGT)
        put(sp, va, 1, f[bit, level] << 12 | fl[1], upper=fl)
        f[bit, level, "before"] = _frame(sp)
        put(sp, va - 0x1000, 1, f[bit, level, "before"] << 12 | 7, upper=fl)
    f["ign4"] = _frame(sp, code_at=TGT)
    put(sp, CLEAN4, 1, f["ign4"] << 12 | 7)
    put(sp, IGN4, 1, f["ign4"] << 12 | 7 | IGN_4K)
    # ---- aliases: two pages each, so a store can straddle
    for i in range(2):
        f["a1", i] = _frame(sp)
        put(sp, A1 + 0x1000 * i, 1, f["a1", i] << 12 | 7)
        put(sp, B1 + 0x1000 * i, 1, f["a1", i] << 12 | 7)
        put(sp, B2 + 0x1000 * i, 1, ((G2 >> 12) + 1 + i) << 12 | 7)   # (the second of them: absent from the dump)
        f["a3", i] = _frame(sp)
        put(sp, A3 + 0x1000 * i, 1, f["a3", i] << 12 | P | US)
        put(sp, B3 + 0x1000 * i, 1, f["a3", i] << 12 | P | RW)
    sp.map(LASTU, bytes(own(0)))
    # ---- ring 0: GDT, IDT without gates, TSS, stack (tests/test_gpu_spill.py::_kspace)
    sp.map(S2.IDT, bytes(0x1000), user=False, write=False, nx=True)
    sp.map(S2.GDT, S2.gdt_page(), user=False, nx=True)
    sp.map(S2.TSS, bytes(0x1000), user=False, nx=True)
    for i in range(2):
        sp.map(KSTACK + 0x1000 * i, b"", user=False, nx=True)
    for i in range(6):
        f["kd", i] = _frame(sp, code_at=TGT)
        put(sp, KDATA + 0x1000 * i, 1, f["kd", i] << 12 | P | RW)
    # KDATA page 5 doubles as the table linked in at run time: its entry 0 -> page 1
    struct.pack_into("<Q", sp.pages[f["kd", 5]], 0, f["kd", 1] << 12 | P | RW)
    f["pre"] = _frame(sp)
    put(sp, PRE, 1, f["pre"] << 12 | P | RW | XD)
    table = sp.cr3 >> 12
    for lv, win in ((4, PDPTWIN), (3, PDWIN), (2, PTWIN)):
        table = (sp._entry(table, (KDATA >> (12 + 9 * (lv - 1))) & 0x1FF) & M.ADDR) >> 12
        f["table", lv - 1] = table
        put(sp, win, 1, table << 12 | P | RW | XD)
    put(sp, LWIN, 2, GLWIN | PS | P | RW | XD)
    put(sp, KLEAF, 2, GKLEAF | PS | P | RW)
    f["kleaf_pt"] = _frame(sp, GKLEAF >> 12)
    f["kleaf_x"] = _frame(sp, (GKLEAF >> 12) + 3)
    f["kleaf_4k"] = _frame(sp)
    struct.pack_into("<Q", sp.pages[f["kleaf_pt"]], 3 * 8, f["kleaf_4k"] << 12 | P | RW)
    # ---- code, last: one frame per page of programs, seen from both rings
    for i in range(0, len(blob), 4096):
        pfn = sp.alloc(blob[i:i + 4096])
        put(sp, CODE + i, 1, pfn << 12 | P | US)
        put(sp, KCODE + i, 1, pfn << 12 | P)
    assert max(sp.pages) < 1 << 20 and sp.next_pfn <= (GLWIN + MIB2) >> 12  # below 4 GiB; LWIN covers every table
    st = user_state(KCODE, KSTACK + 0x1800, sp.cr3)
    st.update({"cs": seg(0x10, 0, 0, 0x209B), "ss": seg(0x18, 0, 0xFFFFFFFF, 0xC93), "rflags": 0x202,
               "gdtr": {"base": S2.GDT, "limit": S2.GDT_LIMIT}, "idtr": {"base": S2.IDT, "limit": 0xFFF},
               "tr": seg(0x40, S2.TSS, 0x67, 0x8B)})
    return sp, regs_from_state(st), f


@functools.lru_cache(maxsize=None)
def zoo():
    """-> (AddressSpace, base Regs (ring 0, WP = 1), {name: pfn})"""
    return _build(programs_blob())


@functools.lru_cache(maxsize=None)
def zoo_frames_only():
    """The zoo before its code pages, which are placed last: cases() takes
    frame numbers and table entries from here, the programs come from cases()."""
    return _build(b"")


# ---------------------------------------------------------------- programs
DEST = (3, 5, 6, 2, 1, 7)   # rbx rbp rsi rdx rcx rdi: where the load at position p lands
SIZE = {"ld1": 1, "ld8": 8, "ld16": 16, "ld32": 32, "st1": 1, "st8": 8, "st16": 16, "st32": 32}
SLOT = 0x60              # bytes per program


def _asm(kind, p, s):
    """The instructions of one access: [(bytes, what)]; what names the memory
    access of that instruction (None: registers only)."""
    m = lambda reg: bytes([(reg << 3) | s])  # noqa: E731  modrm [r8 + s], reg
    if kind == "ld8":
        return [(b"\x49\x8b" + m(DEST[p]), "ld")]
    if kind == "ld1":
        return [(b"\x41\x0f\xb6" + m(DEST[p]), "ld")]
    if kind == "ld16":
        return [(b"\xf3\x41\x0f\x6f" + m(p), "ld")]
    if kind == "ld32":
        return [(b"\xc4\xc1\x7e\x6f" + m(p), "ld")]
    if kind == "st8":
        return [(b"\x4d\x89" + m(4 + s), "st")]
    if kind == "st1":
        return [(b"\x45\x88" + m(4 + s), "st")]
    if kind == "st16":
        return [(b"\xf3\x41\x0f\x7f" + m(4 + s), "st")]
    if kind == "st32":
        return [(b"\xc4\xc1\x7e\x7f" + m(4 + s), "st")]
    if kind in ("stosq1", "stosq2"):
        return [(bytes([0x4C, 0x89, 0xC7 | s << 3]), None), (bytes([0x4C, 0x89, 0xC0 | (4 + s) << 3]), None),
                (b"\xb9" + struct.pack("<I", int(kind[-1])), None), (b"\xf3\x48\xab", "stos")]
    if kind == "cmpxchg":
        return [(b"\x49\x8b" + m(0), "ldrax"), (b"\xf0\x4d\x0f\xb1" + m(4 + s), "rmw")]
    if kind == "push":
        return [(bytes([0x4C, 0x89, 0xC4 | s << 3]), None), (bytes([0x41, 0x54 + s]), "push")]
    if kind == "jmp":
        return [(bytes([0x41, 0xFF, 0xE0 | s]), "jmp")]
    if kind == "invlpg":
        return [(bytes([0x41, 0x0F, 0x01, 0x38 | s]), None)]
    raise KeyError(kind)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str
    cpl: int
    wp: int
    ops: tuple          # ((kind, va, value), ...): value an int (1 / 8 bytes, stos, cmpxchg, push) or bytes (16 / 32)
    salted: bool = True  # a store's value may vary by lane (not a page-table entry)

    @property
    def shape(self):
        """((kind, slot), ...): the program. Slots name the distinct addresses."""
        vas = []
        for _, va, _ in self.ops:
            if va not in vas:
                vas.append(va)
        assert len(vas) <= 4 and len(self.ops) <= 6, self.name
        return tuple((k, vas.index(va)) for k, va, _ in self.ops)


_SHAPES: list = []


def _program(shape) -> bytes:
    out = b""
    for p, (kind, s) in enumerate(shape):
        out += b"".join(b for b, _ in _asm(kind, p, s))
    assert len(out) < SLOT, shape
    return out + b"\xcc"


def programs_blob() -> bytes:
    """Every case's program, one SLOT each, in first-use order."""
    _SHAPES[:] = []
    for c in cases():
        if c.shape not in _SHAPES:
            _SHAPES.append(c.shape)
    blob = b"".join(_program(s).ljust(SLOT, b"\xcc") for s in _SHAPES)
    return blob + b"\xcc" * (-len(blob) % 4096)


def entry_rip(case) -> int:
    zoo()
    return (CODE if case.cpl == 3 else KCODE) + SLOT * _SHAPES.index(case.shape)


def _bytes(case, value, n, salt) -> bytes:
    b = value if isinstance(value, bytes) else (value & (256**n - 1)).to_bytes(n, "little")
    assert len(b) == n
    return bytes(x ^ (salt & 0xFF) for x in b) if case.salted else b


def lane_regs(case, salt=0):
    """The lane's starting registers (a full Regs: the ring and CR0.WP are per lane)."""
    _, r0, _ = zoo()
    r = type(r0).from_buffer_copy(r0)
    r.rip = entry_rip(case)
    if case.cpl == 3:
        r.seg[1].selector, r.seg[2].selector = 0x33, 0x2B  # cs, ss (wtfgpu.h order: es cs ss ds fs gs)
    if not case.wp:
        r.cr0 &= ~(1 << 16)
    for (kind, s), (_, va, value) in zip(case.shape, case.ops):
        r.gpr[8 + s] = va
        if value is None:
            continue
        n = SIZE.get(kind, 8)
        b = _bytes(case, value, n, salt)
        if n <= 8:
            r.gpr[12 + s] = int.from_bytes(b, "little")
        else:
            r.xmm[4 + s][0], r.xmm[4 + s][1] = struct.unpack("<QQ", b[:16])
            if n == 32:
                r.ymmh[4 + s][0], r.ymmh[4 + s][1] = struct.unpack("<QQ", b[16:])
    return r


# ---------------------------------------------------------------- what a case must do (the model)
@dataclasses.dataclass
class Want:
    status: int
    vector: int
    error: int
    addr: int | None       # CR2 of a #PF (None: not compared)
    rip: int
    icount: int
    gpr: dict              # {register index: value} of the registers the model knows
    vec: dict              # {xmm / ymm index: bytes} loaded
    dirty: list            # sorted pfns
    mem: dict              # {pfn: bytes} of the dirty frames
    views: dict            # {va: 8 bytes the host reads there afterwards, None where it does not translate}
    probe: tuple           # the model's verdict of the last access: ("ok", ..) / ("pf", ..) / ("gp",)
    reach: set             # every frame a walk of the case read an entry from or an access translated to

    @property
    def completes(self):
        return self.status == EXIT_INT3


def expect(case: Case, salt=0) -> Want:
    sp, r0, _ = zoo()
    mem = M.Memory(sp.pages)
    cr3, nxe = sp.cr3, True
    reach = set()
    view = _View(mem, reach)

    def acc(va, n, a):
        v = M.access(view, cr3, va, n, a, case.cpl, case.wp, nxe)
        if v[0] == "ok":
            reach.update(g >> 12 for g, _ in v[1])
        return v

    rip, icount = entry_rip(case), 0
    assert acc(rip, SLOT, M.X)[0] == "ok"
    gpr, vec, verdict = {}, {}, None

    def done(status, v=None, at=None):
        views = {}
        for _, va, _ in case.ops:
            parts, ok = [], True
            for a in range(va, va + 8):
                g = M.host_translate(view, cr3, a)
                ok = ok and g is not None
                parts.append((g, 1))
            views[va] = mem.read(parts) if ok else None
        pf = v is not None and v[0] == "pf"
        return Want(status, 0 if v is None else 14 if pf else 13, v[1] if pf else 0, v[2] if pf else None,
                    rip if at is None else at, icount, gpr, vec, sorted(mem.dirty),
                    {p: bytes(mem.own[p]) for p in mem.dirty}, views, verdict, reach)

    for p, ((kind, s), (_, va, value)) in enumerate(zip(case.shape, case.ops)):
        for code, what in _asm(kind, p, s):
            n = SIZE.get(kind, 8)
            if what == "ld" or what == "ldrax":
                verdict = v = acc(va, n, M.R)
                if v[0] != "ok":
                    return done(EXIT_FAULT, v)
                data = mem.read(v[1])
                if n <= 8:
                    gpr[0 if what == "ldrax" else DEST[p]] = int.from_bytes(data, "little")
                else:
                    vec[p] = data
            elif what in ("st", "rmw", "push"):
                at = (va - 8) & MASK64 if what == "push" else va
                verdict = v = acc(at, n, M.W)
                if v[0] != "ok":
                    return done(EXIT_FAULT, v)
                mem.write(v[1], _bytes(case, value, n, salt))
            elif what == "stos":
                for i in range(int(kind[-1])):
                    verdict = v = acc(va + 8 * i, 8, M.W)
                    if v[0] != "ok":
                        return done(EXIT_FAULT, v)
                    mem.write(v[1], _bytes(case, value, 8, salt))
            elif what == "jmp":
                if not M.canonical(va) and not M.BRANCH_GP_AT_TARGET:   # (the SDM's JMP: #GP(0) at the jump)
                    verdict = ("gp",)
                    return done(EXIT_FAULT, verdict)
                icount += 1
                rip = va
                for length in (5, 1):   # TARGET: mov eax, imm32; int3
                    verdict = v = acc(rip, length, M.X)
                    if v[0] != "ok":
                        return done(EXIT_FAULT, v)
                    assert mem.read(v[1]) == (TARGET[:5] if length == 5 else TARGET[5:]), case.name
                    if length == 5:
                        gpr[0] = MAGIC
                        icount += 1
                        rip += 5
                return done(EXIT_INT3)
            rip += len(code)
            icount += 1
    return done(EXIT_INT3)


class _View:
    """The model's memory as the {pfn: frame} mapping translate() reads."""

    def __init__(self, mem, reach):
        self.mem, self.reach = mem, reach

    def get(self, pfn):
        self.reach.add(pfn)   # a table frame some walk went through, edited entries included
        return self.mem.get(pfn)


# ---------------------------------------------------------------- the table
def _v(i):  # a store's value: no byte of it occurs in a frame that holds its own addresses
    return (0xA5C3E1F00D5A7B91 * (2 * i + 1)) & MASK64 | 0x8080808080808080


def _vb(i, n):
    return b"".join(struct.pack("<Q", _v(i + k)) for k in range(n // 8))


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, family, cpl, wp, *ops, salted=True):
        out.append(Case(name, family, cpl, wp, tuple(ops), salted))

    # ---- translation: sizes and places in a 1 GiB and a 2 MiB leaf
    for leaf, base, size in (("1g", U1G, GIB), ("2m", L2, MIB2)):
        for n in (1, 8, 16, 32):
            spots = {"first": 0, "last": size - n}
            if n > 1:
                spots["cross4k"] = 0x1000 - n // 2
            for spot, off in spots.items():
                add(f"t-{leaf}-ld{n}-{spot}", "translation", 3, 1, (f"ld{n}", base + off, None))
                add(f"t-{leaf}-st{n}-{spot}", "translation", 3, 1, (f"st{n}", base + off, _v(n) if n <= 8 else _vb(n, n)),
                    (f"ld{n}", base + off, None))
        # the frame in the middle that the dump does not hold: zeros, and a store makes it the lane's own
        add(f"t-{leaf}-ld8-absent", "translation", 3, 1, ("ld8", base + size // 2 + 0x18, None))
        add(f"t-{leaf}-st8-absent", "translation", 3, 1, ("st8", base + size // 2 + 0x18, _v(40)),
            ("ld8", base + size // 2 + 0x18, None))
    # out of a leaf's end: into a present page, into a hole
    for n in (8, 16, 32):
        val = _v(n) if n <= 8 else _vb(n, n)
        for name, end in (("present", AFTER), ("hole", HOLE), ("1g-hole", U1G + GIB)):
            add(f"t-out-ld{n}-{name}", "translation", 3, 1, (f"ld{n}", end - n // 2, None))
            add(f"t-out-st{n}-{name}", "translation", 3, 1, (f"st{n}", end - n // 2, val), (f"ld{n}", end - n, None))
    # ignored bits: the same frames as the clean twin
    for name, va in (("1g", U1G_IGN), ("2m", L2_IGN), ("4k", IGN4)):
        add(f"t-ign-{name}-ld", "translation", 3, 1, ("ld8", va + 0x28, None), ("ld16", va + 0xFF8 if name != "4k" else va + 0x30, None))
        add(f"t-ign-{name}-st", "translation", 3, 1, ("st8", va + 0x28, _v(50)),
            ("ld8", {"1g": U1G, "2m": L2, "4k": CLEAN4}[name] + 0x28, None))
        add(f"t-ign-{name}-x", "translation", 3, 1, ("jmp", va + TGT, None))
    # canonical addresses
    add("t-canon-ld-straddle", "translation", 3, 1, ("ld8", LASTU + 0xFFC, None))
    add("t-canon-st-straddle", "translation", 3, 1, ("st8", LASTU + 0xFFC, _v(60)), ("ld8", LASTU + 0xFF0, None))
    add("t-canon-ld-plain", "translation", 3, 1, ("ld8", 0x0000800000000000, None))
    add("t-canon-st-plain", "translation", 0, 1, ("st8", 0xFFFF7FFFFFFFFFF8, _v(61)))
    add("t-canon-x-plain", "translation", 3, 1, ("jmp", 0x0000800000000000, None))   # U51: faults at the target
    add("t-canon-x-plain-ring0", "translation", 0, 1, ("jmp", 0xFFFF7FFFFFFFF000, None))
    add("t-canon-last-byte", "translation", 3, 1, ("ld1", LASTU + 0xFFF, None))
    # code on large leaves
    add("t-x-2m-cross4k", "translation", 3, 1, ("jmp", L2 + 0xFFD, None))
    add("t-x-2m-out-present", "translation", 3, 1, ("jmp", L2 + MIB2 - 3, None))
    add("t-x-2m-out-nx", "translation", 3, 1, ("jmp", L2_IGN + MIB2 - 3, None))
    add("t-x-2m-out-hole", "translation", 3, 1, ("jmp", L2_B + MIB2 - 3, None))
    add("t-x-1g", "translation", 0, 1, ("jmp", U1G + TGT, None))

    # ---- rights: every placement and every large leaf, by every kind of access
    targets = {f"{bit.lower()}-l{level}": va for (bit, level), va in PLACE.items()}
    targets.update({"2m-w0": L2_W0, "2m-u0": L2_U0, "2m-nx": L2_NX, "1g-w0": U1G_W0, "1g-u0": U1G_U0,
                    "1g-nx": U1G_NX, "2m-clean": L2, "1g-clean": U1G, "4k-clean": CLEAN4})
    for name, va in targets.items():
        for acc, cpl, wp, op in (("uld", 3, 1, ("ld8", va + 0x10, None)), ("ust", 3, 1, ("st8", va + 0x10, _v(1))),
                                 ("sld", 0, 1, ("ld8", va + 0x10, None)), ("sst-wp1", 0, 1, ("st8", va + 0x10, _v(2))),
                                 ("sst-wp0", 0, 0, ("st8", va + 0x10, _v(3))), ("ux", 3, 1, ("jmp", va + TGT, None)),
                                 ("sx", 0, 1, ("jmp", va + TGT, None))):
            ops = (op, ("ld8", va + 0x10, None)) if op[0] == "st8" and cpl == 0 else (op,)
            add(f"r-{name}-{acc}", "rights", cpl, wp, *ops)
    # a two-page store whose second page is read-only: nothing moves
    for cpl, wp in ((3, 1), (0, 1), (0, 0)):
        add(f"r-two-page-second-ro-cpl{cpl}-wp{wp}", "rights", cpl, wp, ("st8", PLACE["W0", 1] - 4, _v(4)),
            ("ld8", PLACE["W0", 1] - 8, None))
    add("r-two-page-movdqu-second-ro", "rights", 3, 1, ("st16", PLACE["W0", 1] - 8, _vb(5, 16)))
    # nothing mapped, seen from ring 0 (ring 3 meets holes in the translation family)
    add("r-hole-sld", "rights", 0, 1, ("ld8", HOLE + 8, None))
    add("r-hole-sst", "rights", 0, 1, ("st8", HOLE + 8, _v(15)))
    add("r-hole-sx", "rights", 0, 1, ("jmp", HOLE + TGT, None))
    add("r-push-ro", "rights", 3, 1, ("push", PLACE["W0", 2] + 0x40, _v(6)))
    add("r-push-ok", "rights", 3, 1, ("push", CLEAN4 + 0x40, _v(7)), ("ld8", CLEAN4 + 0x38, None))
    add("r-cmpxchg-ro", "rights", 3, 1, ("cmpxchg", PLACE["W0", 3] + 0x40, _v(8)))
    add("r-cmpxchg-ro-wp0", "rights", 0, 0, ("cmpxchg", PLACE["W0", 3] + 0x40, _v(9)), ("ld8", PLACE["W0", 3] + 0x40, None))

    # ---- aliases: read one view, store through the other, read the first again
    for pair, a, b, cpl, wps in (("4k", A1, B1, 3, (1, 1)), ("leaf", A2, B2, 3, (1, 1)), ("ro-rw", B3, A3, 0, (1, 0))):
        for order, (w, r), wp in (("ab", (a, b), wps[0]), ("ba", (b, a), wps[1])):
            for kind, off, val in (("st8", 0x108, _v(10)), ("st16", 0x108, _vb(11, 16)), ("stosq2", 0x108, _v(12)),
                                   ("st8", 0xFFC, _v(13)), ("cmpxchg", 0x108, _v(14))):
                tag = kind + ("-straddle" if off == 0xFFC else "")
                add(f"a-{pair}-{order}-{tag}", "alias", cpl, wp, ("ld8", r + off, None), (kind, w + off, val),
                    ("ld8", r + off, None), ("ld8", r + off + 8 if kind in ("st16", "stosq2") else w + off, None))

    # ---- guest edits of page tables (ring 0)
    _, _, f = zoo_frames_only()
    pt, pd = f["table", 1], f["table", 2]

    def table_edit(tag, win, table_pfn, idx, new, warm, probe, kinds, x):
        old = [struct.unpack_from("<Q", own_or_table(table_pfn), 8 * (idx + k))[0] for k in range(4)]
        pre_tail = struct.unpack_from("<I", own(f["pre"]), 0xFFC)[0]
        stores = {"mov": ("st8", win + 8 * idx, new),
                  "movdqu": ("st16", win + 8 * idx, struct.pack("<QQ", new, old[1])),
                  "vmovdqu": ("st32", win + 8 * idx, struct.pack("<QQQQ", new, *old[1:])),
                  "stosq": ("stosq1", win + 8 * idx, new),
                  "cmpxchg": ("cmpxchg", win + 8 * idx, new),
                  # from the data page below the window into the entry's low half
                  "straddle": ("st8", win - 4, (new & 0xFFFFFFFF) << 32 | pre_tail)}
        for k in kinds:
            if k == "straddle" and (idx != 0 or win != PTWIN or (new ^ old[0]) >> 32):
                continue
            for inv in (False, True):
                # the table's frame is the lane's own before the warm-up: the edit is then no first
                # write, whose copy would drop every cached translation by itself
                # (so is the data page a straddling store starts on)
                ops = [("st8", win + 0x800, 0)] + ([("st8", PRE + 0x800, 0)] if k == "straddle" else []) + [warm, stores[k]] + ([("invlpg", warm[1], None)] if inv else []) + [probe]
                add(f"e-{tag}-{k}" + ("-invlpg" if inv else ""), "edit", 0, 1, *ops, salted=False)

    x = KDATA
    e0 = f["kd", 0] << 12 | P | RW
    every = ("mov", "straddle", "movdqu", "vmovdqu", "stosq", "cmpxchg")
    ld, st = ("ld8", x + 0x20, None), ("st8", x + 0x20, _v(20))
    table_edit("repoint", PTWIN, pt, 0, f["kd", 4] << 12 | P | RW, ld, ld, every, x)
    table_edit("repoint-after-store", PTWIN, pt, 0, f["kd", 4] << 12 | P | RW, st, ld, ("mov", "straddle"), x)
    table_edit("clear-p", PTWIN, pt, 0, e0 & ~P, ld, ld, every, x)
    table_edit("clear-w", PTWIN, pt, 0, e0 & ~RW, st, st, every, x)
    table_edit("set-nx", PTWIN, pt, 0, e0 | XD, ld, ("jmp", x + TGT, None), ("mov", "movdqu", "vmovdqu", "stosq", "cmpxchg"), x)
    pde = struct.unpack_from("<Q", own_or_table(pd), 8 * ((KDATA >> 21) & 0x1FF))[0]
    ld3 = ("ld8", KDATA + 0x3020, None)
    table_edit("set-ps", PDWIN, pd, (KDATA >> 21) & 0x1FF, pde | PS, ld3, ld3, ("mov", "movdqu", "stosq", "cmpxchg"), KDATA + 0x3000)
    ldk = ("ld8", KLEAF + 0x3020, None)
    table_edit("clear-ps", PDWIN, pd, (KLEAF >> 21) & 0x1FF, GKLEAF | P | RW, ldk, ldk, ("mov", "movdqu", "stosq", "cmpxchg"),
               KLEAF + 0x3000)
    # the same leaf table reached through a 2 MiB leaf
    lw = LWIN + (pt << 12) - GLWIN
    for inv in (False, True):
        add("e-repoint-through-leaf" + ("-invlpg" if inv else ""), "edit", 0, 1, ("st8", lw + 0x800, 0), ld,
            ("st8", lw, f["kd", 4] << 12 | P | RW),
            *((("invlpg", ld[1], None),) if inv else ()), ld, salted=False)
    # a control: no edit, the jump target runs
    add("e-control-x", "edit", 0, 1, ld, ("jmp", x + TGT, None), salted=False)
    # a data page linked in as a page table at run time, then edited (only the invlpg twin is a requirement)
    link = ("st8", PDWIN + 8 * ((KLINK >> 21) & 0x1FF), f["kd", 5] << 12 | P | RW)
    edit = ("st8", KDATA + 0x5000, f["kd", 2] << 12 | P | RW)
    own5 = ("st8", KDATA + 0x5800, 0)   # (the frame is the lane's own before the warm-up, as above)
    add("l-link-edit-invlpg", "link", 0, 1, link, own5, ("ld8", KLINK + 0x20, None), edit, ("invlpg", KLINK + 0x20, None),
        ("ld8", KLINK + 0x20, None), salted=False)
    add("l-link-edit", "link-unasserted", 0, 1, link, own5, ("ld8", KLINK + 0x20, None), edit, ("ld8", KLINK + 0x20, None),
        salted=False)
    # two loads of one page: the host edits its mapping between them (tests/test_gpu_paging.py)
    add("h-two-loads", "host", 0, 1, ld, ld, salted=False)
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    for c in out:
        _check_tlb_budget(c)
    return tuple(out)


def _check_tlb_budget(c):
    """A staleness case proves something only while the entry an access left
    in the lane's TLB is still there when the page is touched again: at most
    TLB_N - 2 other data pages in between (a straddling access takes two)."""
    if c.family not in ("alias", "edit", "link"):
        return
    span = []
    for kind, va, _ in c.ops:
        n = 8 * int(kind[-1]) if kind.startswith("stosq") else SIZE.get(kind, 8)
        span.append(set() if kind == "invlpg" else {va >> 12, (va + n - 1) >> 12})
    for i, pages in enumerate(span):
        for pg in pages:
            before = [j for j in range(i) if pg in span[j]]
            if before:
                other = set().union(*span[before[-1] + 1:i]) - {pg}
                assert len(other) <= TLB_N - 2, (c.name, i, sorted(other))


def own_or_table(pfn):
    return zoo_frames_only()[0].pages[pfn]


FAMILIES = {"translation": 87, "rights": 158, "alias": 30, "edit": 69, "link": 1, "link-unasserted": 1, "host": 1}


# ---------------------------------------------------------------- shared by the CPU and the GPU tests
ASSERTED = [c for c in cases() if c.family != "link-unasserted"]


def diff(got, want):
    """The fields in which an engine's result differs from the model's."""
    bad = []
    if got["status"] != want.status:
        bad.append(("status", got["status"], want.status))
    elif want.status == EXIT_FAULT:
        if (got["vector"], got["error"]) != (want.vector, want.error):
            bad.append(("fault", got["vector"], got["error"], want.vector, want.error))
        if want.addr is not None and got["addr"] != want.addr:
            bad.append(("addr", hex(got["addr"]), hex(want.addr)))
    for k in ("rip", "icount"):
        if got[k] != getattr(want, k):
            bad.append((k, got[k], getattr(want, k)))
    bad += [("gpr", r, hex(got["gpr"][r]), hex(v)) for r, v in want.gpr.items() if got["gpr"][r] != v]
    bad += [("vec", i) for i, b in want.vec.items() if got["vec"][i][:len(b)] != b]
    if got["dirty"] != want.dirty:
        bad.append(("dirty", [hex(p) for p in got["dirty"]], [hex(p) for p in want.dirty]))
    elif got["mem"] != want.mem:
        bad.append(("mem", [hex(p) for p in want.dirty if got["mem"][p] != want.mem[p]]))
    for va, b in got["views"].items():
        # (the host build's window is the guest's walk from ring 0, byte by byte: compared where all 8 bytes translate)
        if b != want.views[va] and not ("fast" in got and (want.views[va] is None or not M.canonical(va))):
            bad.append(("view", hex(va), b, want.views[va]))
    return bad


def host_addresses():
    vas = {va for c in cases() for _, va, _ in c.ops}
    vas |= {U1G + GIB - 1, L2 + MIB2 - 1, L2 + MIB2, HOLE, HOLE - 1, L2_U0, L2_NX + 0x1234, L2_W0 + 7,
            U1G_U0 + 0x2FFFFFFF, PTWIN, LWIN + 0x1FFFFF, KLEAF + 0x3000, KLINK, 0, 0xFFFF800000000000}
    return sorted(vas)


HOST_WRITES = [  # (name, va, bytes written, lands)
    ("ro-2m-leaf", L2_W0 + 0x1FFC, 8, True), ("ro-1g-leaf", U1G_W0 + GIB - 8, 8, True),
    ("supervisor-nx-4k", PLACE["U0", 1] + 0xFF0, 16, True), ("absent-frame", L2 + MIB2 // 2 + 4, 8, True),
    ("out-of-leaf-into-hole", L2_B + MIB2 - 4, 8, False), ("hole", HOLE + 8, 8, False),
]
