"""Shared by the spill-pool tests (test_spill_cpu.py, test_gpu_spill.py): a
hand-assembled guest loop that dirties M pages, its snapshot, and the oracle's
result for it. TEST INFRASTRUCTURE ONLY.

The loop stores one qword, rsi + the address, to each of rcx pages from rdi at
a 4 KB stride, then sums them back into rax and ends at an int3. The oracle
has no page limit, so it is the reference for every M."""
from __future__ import annotations

import functools

from wtf_amd.abi import regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

from tests.oracle_lib import Oracle

CODE_VA = 0x140000000
DATA_VA = 0x150000000
STACK_VA = 0x7FF000000000
STACK_TOP = STACK_VA + 0x800
K, X = 2, 6                 # private pages per lane, pool pages per lane
NDATA = K + X + 2           # data pages mapped: one more than any lane may dirty, and a spare
STORE_OFF = 0x18            # the stores' offset inside each page
EXIT_INT3, EXIT_OVERLAY_FULL = 3, 8


def _assemble():
    """(code bytes, offset of the store instruction)"""
    c = bytearray()
    c += b"\x31\xc0"                      # xor eax, eax
    c += b"\x48\x89\xfa"                  # mov rdx, rdi
    c += b"\x49\x89\xc8"                  # mov r8, rcx
    c += b"\x4d\x85\xc0"                  # test r8, r8
    jz = len(c)
    c += b"\x74\x00"                      # jz done
    loop1 = len(c)
    c += b"\x4c\x8d\x0c\x16"              # lea r9, [rsi + rdx]
    store = len(c)
    c += b"\x4c\x89\x0a"                  # mov [rdx], r9
    c += b"\x48\x81\xc2\x00\x10\x00\x00"  # add rdx, 0x1000
    c += b"\x49\xff\xc8"                  # dec r8
    c += b"\x75" + bytes([(loop1 - (len(c) + 2)) & 0xFF])  # jnz loop1
    c += b"\x48\x89\xfa"                  # mov rdx, rdi
    c += b"\x49\x89\xc8"                  # mov r8, rcx
    loop2 = len(c)
    c += b"\x48\x03\x02"                  # add rax, [rdx]
    c += b"\x48\x81\xc2\x00\x10\x00\x00"  # add rdx, 0x1000
    c += b"\x49\xff\xc8"                  # dec r8
    c += b"\x75" + bytes([(loop2 - (len(c) + 2)) & 0xFF])  # jnz loop2
    done = len(c)
    c += b"\xcc"                          # int3
    c[jz + 1] = done - (jz + 2)
    return bytes(c), store


_LOOP, STORE_AT = _assemble()
STORE_RIP = CODE_VA + STORE_AT
DONE_RIP = CODE_VA + len(_LOOP) - 1
# a call to a hook for breakpoint actions, as tests/test_gpu_action_memory.py has it
FEED_CALL, FEED_RET, FEED_HOOK = CODE_VA + 0x100, CODE_VA + 0x105, CODE_VA + 0x120
_page = bytearray(b"\xcc" * 0x140)
_page[:len(_LOOP)] = _LOOP
_page[0x100:0x105] = b"\xe8" + (FEED_HOOK - FEED_RET).to_bytes(4, "little")  # call hook
_page[0x105] = 0x90  # nop: the return address (a STOP_OK action)
_page[0x120] = 0x90  # hook: nop (the action's breakpoint)
_page[0x121] = 0xC3  # ret
CODE = bytes(_page)
BASE = DATA_VA + STORE_OFF  # rdi


def data_page(i: int) -> bytes:
    """Snapshot contents of data page i: every byte depends on the page and
    the offset, so a page that was not copied, or copied from elsewhere, shows."""
    return bytes(((i * 37 + 11) ^ (o * 7 + (o >> 8))) & 0xFF for o in range(4096))


@functools.lru_cache(maxsize=None)
def space():
    """(AddressSpace, initial Regs, gpa of each data page)"""
    sp = AddressSpace()
    sp.map_range(CODE_VA, CODE, write=False)
    sp.map(STACK_VA, b"")
    for i in range(NDATA):
        sp.map(DATA_VA + 0x1000 * i, data_page(i))
    regs = regs_from_state(user_state(CODE_VA, STACK_TOP, sp.cr3))
    gpas = tuple(sp.translate(DATA_VA + 0x1000 * i) for i in range(NDATA))
    return sp, regs, gpas


def lane_regs(m: int, seed: int):
    _, r0, _ = space()
    r = type(r0).from_buffer_copy(r0)
    r.gpr[7], r.gpr[1], r.gpr[6] = BASE, m, seed
    return r


@functools.lru_cache(maxsize=None)
def _oracle():
    sp, _, _ = space()
    pfns, blob = sp.phys()
    return Oracle(pfns=pfns, blob=blob)


@functools.lru_cache(maxsize=None)
def want(m: int, seed: int) -> dict:
    """The oracle's result of the loop over m pages: status, rip, the 16 GPRs,
    rflags, retired count, the dirty set and each dirty page's bytes."""
    o = _oracle()
    o.restore(lane_regs(m, seed))
    e = o.run()
    r = o.regs()
    dirty = sorted(o.dirty())
    return {"status": e.status, "rip": e.rip, "gpr": tuple(r.gpr[i] for i in range(16)), "rflags": r.rflags,
            "icount": o.icount(), "dirty": tuple(dirty), "pages": {g: o.read_phys(g, 4096) for g in dirty}}


def want_full(cap: int, seed: int, m: int) -> dict:
    """What a lane that may hold `cap` dirty pages leaves when the loop wants
    m > cap: it stops at the store to page cap (0-based), unretired, with
    the first cap pages written. Worked out from the program: 5 instructions
    before the loop, 5 per finished round, and the lea of the failing round."""
    _, _, gpas = space()
    pages = {}
    for i in range(cap):
        p = bytearray(data_page(i))
        va = BASE + 0x1000 * i
        p[STORE_OFF:STORE_OFF + 8] = ((seed + va) & (2**64 - 1)).to_bytes(8, "little")
        pages[gpas[i]] = bytes(p)
    return {"status": EXIT_OVERLAY_FULL, "rip": STORE_RIP, "icount": 5 + 5 * cap + 1,
            "rdx": BASE + 0x1000 * cap, "r8": m - cap, "dirty": tuple(sorted(gpas[:cap])), "pages": pages}
