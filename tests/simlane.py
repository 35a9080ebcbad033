"""The one binding of tests/native/libsimlane.so: the engine's lane code (one
lane of k_run's decode / exec / retry loop) built for the host."""
import ctypes as C
import functools
import os
import struct

from tests.cpu_bins import SIMLANE_SO, ensure
from wtf_amd.abi import Regs

U64P = C.POINTER(C.c_uint64)


class SimResult(C.Structure):
    """tests/native/sim_lane.cc's struct SimResult (lib() checks the size)."""
    _fields_ = [("gpr", C.c_uint64 * 16), ("rip", C.c_uint64), ("rflags", C.c_uint64), ("icount", C.c_uint64),
                ("nbytes", C.c_uint64), ("status", C.c_uint32), ("vector", C.c_uint32), ("error", C.c_uint32),
                ("ovn", C.c_uint32), ("addr", C.c_uint64), ("dirty", C.c_uint64 * 64), ("xmm", C.c_uint64 * 32),
                ("mxcsr", C.c_uint32), ("pad", C.c_uint32), ("ymmh", C.c_uint64 * 32), ("win", C.c_uint8 * 512)]


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(ensure(SIMLANE_SO, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")))
    space = [U64P, C.c_char_p, C.c_uint64]                       # gpfns, pages, npages
    run = space + [C.POINTER(Regs), C.c_uint64, C.POINTER(SimResult)]  # + r0, limit, out
    mode = run + [C.c_int, U64P, C.c_uint64]                     # + fast, fast_count, win_va
    for name, args, res in (
            ("sim_run", run, C.c_int),
            ("sim_run_mode", mode, C.c_int),
            ("sim_run_full", mode + [C.POINTER(Regs), C.c_void_p], C.c_int),   # + final, ovpages
            ("sim_digest", [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)], C.c_int),
            ("sim_translate", space + [C.c_uint64, C.c_uint64, U64P], C.c_int),
            ("sim_set_tenet", [C.c_uint64], None),
            ("sim_set_writes", [C.c_char_p, C.c_uint64], None),
            ("sim_tenet", [C.c_char_p, C.c_uint64], C.c_uint64),
            ("sim_result_size", [], C.c_uint64)):
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    assert C.sizeof(SimResult) == L.sim_result_size(), (C.sizeof(SimResult), L.sim_result_size())
    return L


def image(sp):
    """An address space as the sim_* entry points take it: (gpfns, pages, npages)."""
    pfns, blob = sp.phys()
    return (C.c_uint64 * len(pfns))(*pfns), blob, len(pfns)


def run(sp, regs, limit=0, fast=False, win_va=0, pages=None, writes=()):
    """One lane from `regs` until it stops: (SimResult, the merged final Regs,
    the instructions the fast loop's forms retired). sp: an AddressSpace, or
    its image() where many lanes share one. fast=True tries the fast loop's
    form of each instruction first (k_run's order); `win_va` selects the 512
    bytes returned in `win`; `pages` (a 64-page buffer) receives the dirty pages;
    `writes`: (va, bytes) the host writes into the lane's memory before it runs."""
    arr, blob, n = sp if isinstance(sp, tuple) else image(sp)
    if writes:
        recs = b"".join(struct.pack("<QQ", va, len(data)) + bytes(data) for va, data in writes)
        lib().sim_set_writes(recs, len(recs))
    out, fin, cnt = SimResult(), Regs(), C.c_uint64(0)
    lib().sim_run_full(arr, blob, n, C.byref(regs), limit, C.byref(out), 1 if fast else 0, C.byref(cnt), win_va,
                       C.byref(fin), pages)
    return out, fin, cnt.value


def page_buffer():
    """A buffer for run(..., pages=)."""
    return C.create_string_buffer(64 * 4096)


def dirty_pages(out, pages):
    """{gpa: bytes} of the dirty pages a run(..., pages=page_buffer()) left."""
    raw = pages.raw
    return {int(out.dirty[k]): raw[k * 4096:(k + 1) * 4096] for k in range(min(out.ovn, 64))}
