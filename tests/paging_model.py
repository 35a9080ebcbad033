"""IA-32e paging as the SDM states it (vol. 3 sections 4.5 - 4.7), in plain
Python: the reference the page-walk tests compare the oracle, the engine's
host build and the GPU engine with. Written from the manual, not from either
walk.

  4.5    4-level paging: CR3 -> PML4E -> PDPTE -> PDE -> PTE; a PDPTE or a PDE
         with PS = 1 maps a 1 GiB / 2 MiB page, whose physical address takes
         bits 51:30 / 51:21 from the entry and the rest from the linear address
         (so PAT, bit 12 of such an entry, is no address bit); PS in a PML4E
         is reserved and in a PTE it is PAT: neither ends the walk.
  4.6    access rights: user-mode iff CPL = 3. A user-mode access needs U/S = 1
         in every entry of the walk; a write needs R/W = 1 in every entry,
         except a supervisor-mode write with CR0.WP = 0; a fetch needs XD = 0
         in every entry when EFER.NXE = 1.
  4.7    the #PF error code: P (bit 0) = the fault was a rights violation, not
         a missing entry; W/R (bit 1) = a write; U/S (bit 2) = user-mode;
         I/D (bit 4) = a fetch, reported only with NXE = 1 (no SMEP here).
  3.3.7.1 a non-canonical linear address is #GP(0) before any walk (a stack
         reference would be #SS(0); the cases use none).

What this project fixes on top (the paging row) enters as
the named switches below; they are facts about the engine and the oracle that
the tests document, not SDM behaviour."""
from __future__ import annotations

import os
import struct

P, RW, US, PS, XD = 1, 2, 4, 0x80, 1 << 63
ADDR = 0x000FFFFFFFFFF000
PAGE = 4096
R, W, X = "r", "w", "x"

# ---- conventions
AD_UPDATES = False        # U8: a walk sets no accessed / dirty bit
CHECK_RESERVED = False    # reserved bits of an entry are not checked (no RSVD faults)
SMEP = SMAP = PKE = False  # CR4.SMEP / SMAP / PKE are not read: supervisor code may run and touch user pages
BRANCH_GP_AT_TARGET = True  # U51: a near branch to a non-canonical target retires; #GP(0) at the fetch, rip = the target
HOST_RIGHTS = False       # VirtRead / VirtWrite / VirtTranslate of the host: present bits only, no canonical check


def canonical(va: int) -> bool:
    return va >> 47 in (0, 0x1FFFF)


def _entry(pages, table_pa: int, idx: int) -> int:
    frame = pages.get(table_pa >> 12)
    return struct.unpack_from("<Q", frame, idx * 8)[0] if frame is not None else 0


def _walk(pages, cr3: int, va: int):
    """The entries of the walk, top down, ending at the first one that is not
    present or maps a page: [(level, entry)], level 4 = PML4E .. 1 = PTE."""
    out = []
    table = cr3 & ADDR
    for level in (4, 3, 2, 1):
        e = _entry(pages, table, (va >> (12 + 9 * (level - 1))) & 0x1FF)
        out.append((level, e))
        if not e & P or (level in (3, 2) and e & PS) or level == 1:
            break
        table = e & ADDR
    return out


def _gpa(level: int, e: int, va: int) -> int:
    low = (1 << (12 + 9 * (level - 1))) - 1    # 4 KiB, 2 MiB, 1 GiB
    return (e & ADDR & ~low) | (va & low)


def translate(pages, cr3, va, acc, cpl, cr0_wp, efer_nxe):
    """One access of mode acc (R, W, X) at one linear address.
    pages: {pfn: 4096 bytes}; a frame it does not hold reads as zeros.
    -> ("ok", gpa) | ("pf", error_code) | ("gp",)"""
    assert not (AD_UPDATES or CHECK_RESERVED or SMEP or SMAP or PKE)
    if not canonical(va):
        return ("gp",)
    user = cpl == 3
    code = (2 if acc == W else 0) | (4 if user else 0) | (16 if acc == X and efer_nxe else 0)
    entries = _walk(pages, cr3, va)
    level, e = entries[-1]
    if not e & P:
        return ("pf", code)
    writable = all(x & RW for _, x in entries)
    usermode = all(x & US for _, x in entries)
    noexec = efer_nxe and any(x & XD for _, x in entries)
    if (user and not usermode) or (acc == W and not writable and (user or cr0_wp)) or (acc == X and noexec):
        return ("pf", code | 1)
    return ("ok", _gpa(level, e, va))


def host_translate(pages, cr3, va):
    """The host's VirtTranslate: present bits only (HOST_RIGHTS), the linear
    address taken by its low 48 bits. -> gpa | None"""
    assert not HOST_RIGHTS
    level, e = _walk(pages, cr3, va)[-1]
    return _gpa(level, e, va) if e & P else None


def access(pages, cr3, va, n, acc, cpl, cr0_wp, efer_nxe):
    """An access of n bytes at va, page by page in address order, as the engine
    documents it: every page is checked before a byte moves,
    and the first page that fails gives the fault, whose address is the operand
    start (first page) or the page boundary (a later one). A non-canonical
    byte anywhere in the operand is #GP(0) before any walk.
    -> ("ok", [(gpa, count)]) | ("pf", error_code, fault_va) | ("gp",)"""
    if not canonical(va) or not canonical((va + n - 1) & (2**64 - 1)) or va + n > 2**64:
        return ("gp",)
    parts, at = [], va
    while at < va + n:
        k = min(PAGE - (at & 0xFFF), va + n - at)
        t = translate(pages, cr3, at, acc, cpl, cr0_wp, efer_nxe)
        if t[0] != "ok":
            return t + (at,) if t[0] == "pf" else t
        parts.append((t[1], k))
        at += k
    return ("ok", parts)


class Memory:
    """Guest physical memory of one lane: the snapshot's frames, copied on the
    first write (the frame then counts as dirty); an absent frame is zeros."""

    def __init__(self, frames):
        self.base = frames
        self.own: dict[int, bytearray] = {}
        self.dirty: list[int] = []

    def get(self, pfn):
        return self.own.get(pfn, self.base.get(pfn))

    def read(self, parts) -> bytes:
        out = b""
        for gpa, k in parts:
            f = self.get(gpa >> 12)
            out += bytes(f[gpa & 0xFFF:(gpa & 0xFFF) + k]) if f is not None else bytes(k)
        return out

    def write(self, parts, data: bytes):
        for gpa, k in parts:
            pfn = gpa >> 12
            if pfn not in self.own:
                self.own[pfn] = bytearray(self.base.get(pfn, bytes(PAGE)))
                self.dirty.append(pfn)
            self.own[pfn][gpa & 0xFFF:(gpa & 0xFFF) + k] = data[:k]
            data = data[k:]


# ---------------------------------------------------------------- the reference's own walk
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kdmp_fixtures.json")
PAT_1G, PAT_2M = 6, 12   # the PDPT / PD slots of the PAT leaves


def in_pat_leaf(gva: int) -> bool:
    return 0x7F8000000000 + (PAT_1G << 30) <= gva < 0x7F8000000000 + (PAT_1G + 1 << 30) or \
        0x7F8040000000 + (PAT_2M << 21) <= gva < 0x7F8040000000 + (PAT_2M + 1 << 21)


def vt(out: list[str]) -> dict[int, int | None]:
    """{gva: gpa or None} of the VT lines."""
    return {int(a, 16): None if b == "-1" else int(b, 16) for a, b in (ln.split()[1:] for ln in out if ln.startswith("VT "))}


def large_page_space():
    """Page tables with a 1 GiB leaf (PDPTE.PS) and a 2 MiB leaf (PDE.PS),
    the kdmp-parser walk's large-page branches (kdmp-parser.h:300-330)."""
    from wtf_amd.tools.snapshot import AddressSpace

    sp = AddressSpace()
    sp.map(0x140000000, b"\x90" * 16)               # an ordinary 4 KiB page
    pml4 = sp.cr3 >> 12
    # 1 GiB leaf at 0x7f8000000000 -> gpa 0x40000000
    pdpt = sp.alloc()
    struct.pack_into("<Q", sp.pages[pml4], 0xFF * 8, (pdpt << 12) | 0x7)
    struct.pack_into("<Q", sp.pages[pdpt], 0, 0x40000000 | 0x87)
    # 2 MiB leaf at 0x7f8040000000 -> gpa 0x200000
    pd = sp.alloc()
    struct.pack_into("<Q", sp.pages[pdpt], 1 * 8, (pd << 12) | 0x7)
    struct.pack_into("<Q", sp.pages[pd], 3 * 8, 0x200000 | 0x87)
    # the same frames again through leaves that carry the bits a walk must ignore (G, A, D, the software
    # bits 9-11 and 52-62), through W = 0, U = 0 and NX leaves, and through leaves with PAT (bit 12 of a
    # large leaf) set
    ign = 0x100 | 0x20 | 0x40 | 0xE00 | (0x7FF << 52)
    for i, bits in ((2, 0x87 | ign), (3, 0x85), (4, 0x83), (5, 0x87 | 1 << 63), (PAT_1G, 0x87 | 0x1000)):
        struct.pack_into("<Q", sp.pages[pdpt], i * 8, 0x40000000 | bits)
    for i, bits in ((5, 0x87 | ign), (9, 0x85), (10, 0x83), (11, 0x87 | 1 << 63), (PAT_2M, 0x87 | 0x1000)):
        struct.pack_into("<Q", sp.pages[pd], i * 8, 0x200000 | bits)
    # a few pages inside both large mappings, so GetPhysicalPage sees them
    for gpa in (0x40000000, 0x40001000, 0x200000, 0x3FF000):
        sp.pages[gpa >> 12] = bytearray(struct.pack("<Q", gpa) * 512)
    gvas = [0x140000000, 0x140000FFF, 0x7F8000000000, 0x7F8000001234, 0x7F803FFFFFFF, 0x7F8040600000,
            0x7F80407FFFFF, 0x7F8040800000, 0x7F9000000000, 0x0, 0xFFFF800000000000, 0x800000000000]
    for base, size in [(0x7F8000000000 + (i << 30), 1 << 30) for i in (2, 3, 4, 5, PAT_1G)] + \
                      [(0x7F8040000000 + (i << 21), 1 << 21) for i in (5, 9, 10, 11, PAT_2M)]:
        gvas += [base, base + 0x1234, base + size - 1, base + size]   # first, inside, last byte, first byte past the end
    return sp, gvas


def reference_lines():
    """The large-page dump of tests/test_snapshot_format.py and what the
    reference's kdmp-parser translates its addresses to (the committed VT lines
    of tests/golden/kdmp_fixtures.json): (AddressSpace, {gva: gpa or None}).
    In a leaf with PAT set kdmp-parser adds bit 12 of the entry into the
    address; there the SDM's address (tables 4-15, 4-17) is what is wanted."""
    import json

    sp, gvas = large_page_space()
    ref = vt(json.load(open(FIXTURES))["large_full"])
    assert set(ref) == set(gvas) and len(ref) >= 40
    want = {}
    for g in gvas:
        model = host_translate(sp.pages, sp.cr3, g)
        assert model == (ref[g] - 0x1000 if in_pat_leaf(g) else ref[g]), hex(g)   # the model against the reference
        want[g] = model
    assert sum(v is None for v in want.values()) >= 6 and sum(map(in_pat_leaf, gvas)) == 8
    return sp, want
