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
