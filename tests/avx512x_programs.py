"""The natively recorded multi-instruction AVX-512 routines
(tests/golden/gen_avx512x_programs.py): their address space, a lane's
registers for one case and the comparison with the recorded outcome."""
import gzip
import json
import os

from tests.golden.gen_avx512x_programs import GPR_INDEX, source
from tests.insn_cases import CODE_VA
from tests.vector_replay import XCR0
from wtf_amd.tools.snapshot import AddressSpace

with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avx512x_programs.json.gz"),
               "rt") as _f:
    PROGS = json.load(_f)


def program_space():
    """The routines at CODE_VA; four pages at the native run's buffer address:
    source (per case), constants, and the two destination areas."""
    lay = PROGS["layout"]
    buf_va = int(PROGS["buf_va"], 16)
    sp = AddressSpace()
    sp.map_range(CODE_VA, bytes.fromhex(PROGS["code"]), write=False)
    for off in (lay["src"], lay["dst"], lay["dst2"]):
        sp.map(buf_va + off, b"")
    sp.map(buf_va + lay["consts"], bytes.fromhex(PROGS["consts"]))
    return sp


def program_case(c, regs):
    """Set a lane's registers for case c (the arguments the native harness
    passed; every other GPR a value no routine relies on); returns its source bytes."""
    lay = PROGS["layout"]
    buf_va = int(PROGS["buf_va"], 16)
    for i in range(16):
        if i != 4:
            regs.gpr[i] = 0x1111111111111111 * i
    regs.gpr[7], regs.gpr[6] = buf_va + lay["src"], buf_va + lay["dst"]
    regs.gpr[2], regs.gpr[1] = c["len"], buf_va + lay["consts"]
    regs.rip = CODE_VA + PROGS["routines"][c["routine"]]["entry"]
    regs.xcr0 = XCR0
    return source(c["routine"], c["seed"])


def program_check(c, icount, gpr, dst, dst2):
    if icount != c["icount"]:
        return ("icount", icount, c["icount"])
    want = {nm: int(v, 16) for nm, v in zip(PROGS["gprs"], c["gpr"])}
    got = {nm: gpr[GPR_INDEX[nm]] for nm in want}
    if got != want:
        return ("gpr", {nm: (hex(got[nm]), hex(want[nm])) for nm in want if got[nm] != want[nm]})
    if dst != bytes.fromhex(c["dst"]):
        return ("dst", [i for i in range(len(dst)) if dst[i] != bytes.fromhex(c["dst"])[i]][:8])
    if dst2 != bytes.fromhex(c["dst2"]):
        return ("dst2", [i for i in range(len(dst2)) if dst2[i] != bytes.fromhex(c["dst2"])[i]][:8])
    return None
