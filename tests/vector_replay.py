"""One replay harness for the native-execution golden vectors
(tests/golden/*_vectors.json.gz): each family is declared once (how a case is
set up, what is compared), and replayed on three executors: the oracle, the
engine's lane code built for the host (tests/simlane.py) and k_run on the GPU.
Every executor hands the family's one check() the same Outcome record.

Where a case's window sits is a property of the case: a placement (below,
"placements") moves it so that the memory operand meets a page edge, with the
second page present or absent; judge() holds a placed case to the moved native
result, to the #PF derived from the layout, or, for the tabled exemptions, to
the oracle (tests/test_page_edge.py, tests/test_gpu_page_edge.py)."""
import ctypes as C
import dataclasses
import functools
import gzip
import json
import os

from tests import simlane
from tests.golden.gen_avx512_vectors import BOUND, WIN
from tests.insn_cases import CODE_VA, get_xmm, get_ymm, get_zmm, oracle_of, set_xmm, set_ymm, set_zmm
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, RUNNING, Regs, regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

HERE = os.path.dirname(os.path.abspath(__file__))
GPU_CODE_VA = 0x140000000
XCR0 = 0xE7
VEC_XM = 19
CR3 = AddressSpace().cr3  # every AddressSpace puts its root table in the same frame
TENET_CAP = 1 << 12       # one instruction's stream: 17 registers twice and a few accesses


@functools.lru_cache(maxsize=None)
def load_doc(name):
    """tests/golden/<name>_vectors.json.gz"""
    with gzip.open(os.path.join(HERE, "golden", f"{name}_vectors.json.gz"), "rt") as f:
        return json.load(f)


@dataclasses.dataclass
class Outcome:
    """What one replayed case produced, whichever executor produced it."""
    executor: str        # "oracle" / "sim" / "gpu"
    clean: bool          # the instruction retired and nothing else ran
    status: int
    vector: int
    error: int
    addr: int
    icount: int
    rip: int
    entry: int           # where the case's code was placed
    regs: Regs           # the full final registers
    initial: Regs        # the registers the case started from
    window: bytes        # the window the case started from
    mem: bytes | None    # the window afterwards (zeros for an unmapped page); None: not read
    fast: int = 0        # sim only: the instructions the fast loop's forms retired
    nbytes: int = 0      # the executor's byte count (instruction bytes + bytes accessed) of the run
    mapped: int | None = None   # a placed case: the window's leading bytes that are mapped (None: all)
    tenet: bytes | None = None  # the run's Tenet stream, where the executor was asked for it


def abridged(ftw):
    return sum(1 << i for i in range(8) if (ftw >> (2 * i)) & 3 != 3)


def patched(data, diff):
    out = bytearray(data)
    for i, v in diff:
        out[i] = v
    return bytes(out)


def hexes(vals):
    return [int(v, 16) for v in vals]


class Family:
    """One golden file. `fields` names what check() compares (tests/
    test_vector_replay.py holds check() to it); `skip` switches a field off on
    one executor (a recorded finding, with its first failing case)."""
    win_len = 256
    gpu_code_va = GPU_CODE_VA
    vreg = "xmm"         # the Regs array that holds the family's vector registers
    skip = {}

    def __init__(self, name, fields, mem_sample):
        self.name, self.fields, self.mem_sample = name, fields, mem_sample

    @property
    def doc(self):
        return load_doc(self.name)

    @property
    def buf_va(self):
        return int(self.doc["buf_va"], 16)

    @property
    def page(self):
        return self.buf_va & ~0xFFF

    # ---- how a case is laid out
    def win_va(self, c):
        """Where the case's window sits: buf_va, or its placement's address."""
        return c["at"].va if "at" in c else self.buf_va

    def group(self, c):
        """Cases of one group share an address space on the GPU (placed cases:
        1 with both pages present, 2 with the second page absent)."""
        return 0 if "at" not in c else 1 if c["at"].present2 else 2

    def segments(self, group):
        """The window's pieces: (offset, length, mapped)."""
        return [(0, self.win_len, True)]

    def case_segments(self, c):
        """segments() of the case's group; a placed case's window ends where
        its absent second page begins."""
        n = self.mapped(c)
        if n is None:
            return self.segments(self.group(c))
        return [(0, n, True), (n, self.win_len - n, False)]

    def mapped(self, c):
        """The leading bytes of a placed case's window that are mapped (None: all)."""
        if "at" not in c or c["at"].present2:
            return None
        return max(0, min(self.win_len, self.page + 0x1000 - c["at"].va))

    def space_at(self, c):
        """space()'s keywords for the case's own place."""
        return {"va": c["at"].va} if "at" in c else {}

    def space(self, code, code_va, window, group, nx=False, va=None):
        """Code at code_va; the window's page and the page after it, the window
        at va (buf_va) wherever that puts it on the two; group 2: the second
        page is absent, and the window's bytes on it are dropped."""
        sp = AddressSpace()
        sp.map_range(code_va, code, write=False)
        off = (self.buf_va if va is None else va) - self.page
        assert 0 <= off and off + len(window) <= 0x2000
        both = bytearray(0x2000)
        both[off:off + len(window)] = window
        sp.map(self.page, bytes(both[:0x1000]), nx=nx)
        if group != 2:
            sp.map(self.page + 0x1000, bytes(both[0x1000:]), nx=nx)
        return sp

    def init(self, regs):
        """The tweak to the initial state every case of the family starts from."""

    def setup(self, c, regs):
        """Apply the case to regs (not rip); returns the window bytes."""
        raise NotImplementedError

    def gprs_in(self, c, regs):
        for i in range(16):
            regs.gpr[i] = int(c["in"][i], 16)
        regs.rflags = int(c["fl"], 16) | 0x200  # ring 3 cannot clear IF: the native run had IF = 1

    # ---- what is compared
    def flag_mask(self, c):
        return 0x8D5

    def fields_of(self, c):
        """What is compared for this case: a placed replay also compares the
        byte count, with the oracle's for the same placed case."""
        return self.fields + (("bytes",) if "at" in c else ())

    def on(self, o, field):
        return field in self.fields and field not in self.skip.get(o.executor, ())

    def check(self, c, o):
        """A mismatch tuple, or None."""
        raise NotImplementedError

    def check_exit(self, c, o):
        if not o.clean or (self.on(o, "icount") and o.icount != 1):
            return ("exit", o.status, o.vector, o.icount)
        return None

    def check_gpr(self, c, o, want, dst=None):
        got = list(o.regs.gpr)
        if dst is not None:
            got[dst] = want[dst]
        if self.on(o, "gpr") and got != want:
            return ("regs", [(i, hex(got[i]), hex(want[i])) for i in range(16) if got[i] != want[i]])
        if self.on(o, "flags") and (o.regs.rflags ^ int(c["flo"], 16)) & self.flag_mask(c):
            return ("flags", hex(o.regs.rflags), c["flo"])
        return None

    def check_vec(self, o, got, want, per):
        if self.on(o, "vec") and got != want:
            return ("vec", [(i // per, i % per, hex(got[i]), hex(want[i])) for i in range(len(want))
                            if got[i] != want[i]][:4])
        return None

    def check_tail(self, c, o, mem):
        """The window (where the executor read it) and rip, last as in every loop."""
        if self.on(o, "mem") and o.mem is not None and o.mem[:o.mapped] != mem[:o.mapped]:
            return ("mem", [(i, o.mem[i], mem[i]) for i in range(len(mem[:o.mapped])) if o.mem[i] != mem[i]][:6])
        if self.on(o, "rip") and o.rip != o.entry + len(c["code"]) // 2:
            return ("rip", hex(o.rip), hex(o.entry))
        return None


class Native(Family):
    """Integer forms: GPRs, the defined RFLAGS bits (fmask), rip, the window."""

    def setup(self, c, regs):
        from tests.golden.gen_native_vectors import splitmix_bytes
        self.gprs_in(c, regs)
        return splitmix_bytes(int(c["seed"], 16), 256)

    def flag_mask(self, c):
        return int(c["fmask"], 16)

    def check(self, c, o):
        # BSF / BSR leave the destination undefined for a zero source
        dst = c["dst"] if c["cls"] == "bsx" and int(c["flo"], 16) & 0x40 else None
        return self.check_exit(c, o) or self.check_gpr(c, o, hexes(c["out"]), dst) or \
            self.check_tail(c, o, patched(o.window, c["diff"]))


class Sse(Family):
    def setup(self, c, regs):
        from tests.golden.gen_sse_vectors import window_in
        self.gprs_in(c, regs)
        set_xmm(regs, hexes(c["xin"]))
        regs.mxcsr = int(c["mx"], 16)
        return window_in(int(c["seed"], 16), c["ldmx"])

    def check(self, c, o):
        bad = self.check_exit(c, o) or self.check_gpr(c, o, hexes(c["out"])) or \
            self.check_vec(o, get_xmm(o.regs), hexes(c["xout"]), 2)
        if not bad and self.on(o, "mxcsr") and o.regs.mxcsr != int(c["mxo"], 16):
            bad = ("mxcsr", hex(o.regs.mxcsr), c["mxo"])
        return bad or self.check_tail(c, o, patched(o.window, c["diff"]))


class Mmx(Family):
    vreg = "fpst"

    def setup(self, c, regs):
        from tests.golden.gen_native_vectors import splitmix_bytes
        self.gprs_in(c, regs)
        set_xmm(regs, hexes(c["xin"]))
        for i in range(8):
            regs.fpst[i] = int(c["mmin"][i], 16)
        regs.fpsw = 0       # the stub's movq loads leave TOS = 0
        regs.fptw = 0x0000  # and every tag valid
        return splitmix_bytes(int(c["seed"], 16), 256)

    def check(self, c, o):
        r = o.regs
        bad = self.check_exit(c, o) or self.check_gpr(c, o, hexes(c["out"])) or \
            self.check_vec(o, get_xmm(r), hexes(c["xout"]), 2) or \
            self.check_vec(o, list(r.fpst), hexes(c["mmout"]), 1)
        if not bad and self.on(o, "x87") and (r.fpsw != int(c["fsw"], 16) or abridged(r.fptw) != int(c["ftw"], 16)):
            bad = ("x87", hex(r.fpsw), hex(r.fptw), c["fsw"], c["ftw"])
        return bad or self.check_tail(c, o, patched(o.window, c["diff"]))


class Avx(Family):
    vreg = "ymmh"

    def setup(self, c, regs):
        from tests.golden.gen_native_vectors import splitmix_bytes
        self.gprs_in(c, regs)
        set_ymm(regs, hexes(c["yin"]))
        return splitmix_bytes(int(c["seed"], 16), 256)

    def check(self, c, o):
        return self.check_exit(c, o) or self.check_gpr(c, o, hexes(c["out"])) or \
            self.check_vec(o, get_ymm(o.regs), hexes(c["yout"]), 4) or \
            self.check_tail(c, o, patched(o.window, c["diff"]))


class FpFormat(Family):
    """gen_fp_vectors.run_native's document format: the inputs come from the
    generator's case_inputs, the expectations are differences (gdiff / ydiff /
    mdiff), and an unmasked exception traps (trap_mx)."""
    vreg = "ymmh"

    def __init__(self, name, fields, mem_sample, case_inputs):
        super().__init__(name, fields, mem_sample)
        self.case_inputs = case_inputs

    def inputs(self, c):
        """(ymm0-15 as 64 u64, the window)."""
        ymm, win = self.case_inputs(c)
        return [v for r in ymm for v in r], b"".join(v.to_bytes(8, "little") for v in win)

    def setup(self, c, regs):
        yin, win = self.inputs(c)
        self.gprs_in(c, regs)
        set_ymm(regs, yin)
        regs.mxcsr = int(c["mx"], 16)
        return win

    def flag_mask(self, c):
        return int(c.get("flm", "8d5"), 16)

    def check(self, c, o):
        if "trap_mx" in c:  # #XM with the trap's MXCSR; nothing else of it is compared
            if o.status != EXIT_FAULT or o.vector != VEC_XM:
                return ("trap expected", o.status, o.vector)
            if o.regs.mxcsr != int(c["trap_mx"], 16):
                return ("trap mxcsr", hex(o.regs.mxcsr), c["trap_mx"])
            return None
        g = hexes(c["in"])
        for i, v in c["gdiff"]:
            g[i] = int(v, 16)
        y = get_ymm(o.initial)
        for i, v in c["ydiff"]:
            y[i] = int(v, 16)
        bad = self.check_exit(c, o) or self.check_gpr(c, o, g) or self.check_vec(o, get_ymm(o.regs), y, 4)
        if not bad and self.on(o, "mxcsr") and o.regs.mxcsr != int(c["mxo"], 16):
            bad = ("mxcsr", hex(o.regs.mxcsr), c["mxo"])
        return bad or self.check_tail(c, o, patched(o.window, c.get("mdiff", [])))


class X87Stack(Family):
    """The x87 state and a 16-byte operand at rsi; the expected values are the
    case's "out" (tests/golden/gen_x87_vectors.py)."""
    win_len = 16
    vreg = "fpst"

    def setup(self, c, regs):
        from tests.golden.gen_x87_vectors import case_regs
        regs.gpr[6] = self.win_va(c)
        case_regs(c, regs)
        return bytes.fromhex(c["mem"])

    def check(self, c, o):
        w, r = c["out"], o.regs
        if w["status"] == EXIT_FAULT:
            if o.status != EXIT_FAULT or o.vector != w["vector"]:
                return ("fault", o.status, o.vector)
        elif bad := self.check_exit(c, o):
            return bad
        if self.on(o, "x87") and (r.fpcw, r.fpsw, r.fptw) != (w["fcw"], w["fsw"], w["ftw"]):
            return ("status", hex(r.fpcw), hex(r.fpsw), hex(r.fptw), hex(w["fcw"]), hex(w["fsw"]), hex(w["ftw"]))
        if self.on(o, "flags") and r.rflags & 0x8D5 != w["fl"]:
            return ("fl", hex(r.rflags), hex(w["fl"]))
        if self.on(o, "vec") and [(r.fpst[k], r.fpse[k]) for k in range(8)] != [tuple(x) for x in w["st"]]:
            return ("st",)
        if self.on(o, "mem") and o.mem is not None and o.mem[:o.mapped] != bytes.fromhex(w["mem"])[:o.mapped]:
            return ("mem", o.mem.hex(), w["mem"])
        if w["status"] != EXIT_FAULT and self.on(o, "rip") and o.rip != o.entry + len(c["code"]) // 2:
            return ("rip", hex(o.rip), hex(o.entry))
        return None


class Evex(Family):
    """zmm0-31, k0-7 and a 512-byte window across a page boundary; the guard
    cases (one of the two pages absent) run in their own address spaces; a
    fault case must fault as recorded and leave zmm and the window unchanged."""
    win_len = WIN
    gpu_code_va = CODE_VA
    vreg = "zmm_hi"

    def __init__(self, name, fields, mem_sample, inputs):
        super().__init__(name, fields, mem_sample)
        self.inputs = inputs   # (zmm0-31 as 256 u64, the window with the absent page zeroed)

    def group(self, c):
        return c["guard"]

    def segments(self, guard):
        return [(0, BOUND, guard != 2), (BOUND, WIN - BOUND, guard != 1)]

    def space(self, code, code_va, window, guard, nx=False):
        """The window's first 256 bytes end one page, the rest start the next
        (guard 1: the second page absent; guard 2: the first)."""
        sp = AddressSpace()
        sp.map_range(code_va, code, write=False)
        page = self.buf_va & ~0xFFF
        off = self.buf_va - page
        assert off + BOUND == 0x1000
        first = bytearray(4096)
        first[off:] = window[:BOUND]
        if guard != 2:
            sp.map(page, bytes(first))
        if guard != 1:
            sp.map(page + 0x1000, bytes(window[BOUND:]) + bytes(4096 - (WIN - BOUND)))
        return sp

    def init(self, regs):
        regs.xcr0 = XCR0

    def setup(self, c, regs):
        zin, win = self.inputs(c)
        self.gprs_in(c, regs)
        set_zmm(regs, zin)
        for i in range(8):
            regs.k[i] = int(c["k"][i], 16)
        return win

    def check(self, c, o):
        zin, zmm = get_zmm(o.initial), get_zmm(o.regs)
        if "fault" in c:
            f = c["fault"]
            if o.status != EXIT_FAULT or o.vector != f["vec"]:
                return ("fault", o.status, o.vector, f)
            if self.on(o, "icount") and o.icount != 0:
                return ("icount", o.icount, o.status, o.vector)
            if f["vec"] == 14 and (o.error != f["err"] or o.addr != int(f["addr"], 16)):
                return ("pf", hex(o.error), hex(o.addr), f)
            if (self.on(o, "vec") and zmm != zin) or (self.on(o, "mem") and o.mem is not None and o.mem != o.window):
                return ("fault state",)
            return None
        g = hexes(c["in"])
        for i, v in c["gdiff"]:
            g[i] = int(v, 16)
        z = list(zin)
        for i, v in c["zdiff"]:
            z[i] = int(v, 16)
        bad = self.check_exit(c, o) or self.check_gpr(c, o, g) or self.check_vec(o, zmm, z, 8)
        if not bad and self.on(o, "k") and list(o.regs.k) != hexes(c["ko"]):
            bad = ("k", [hex(x) for x in o.regs.k], c["ko"])
        return bad or self.check_tail(c, o, patched(o.window, c["mdiff"]))


def _fp_inputs(c):
    from tests.golden.gen_fp_vectors import case_inputs
    return case_inputs(int(c["seed"], 16), c["ew"], bool(c["ints"]))


def _sse4_inputs(c):
    from tests.golden.gen_sse4_vectors import case_inputs
    return case_inputs(int(c["seed"], 16))


def _ext_inputs(c):
    from tests.golden.gen_ext_vectors import case_inputs
    return case_inputs(int(c["seed"], 16), c["ints"])


def _avx2x_inputs(c):
    from tests.golden.gen_avx2x_vectors import case_inputs
    ymm, win = case_inputs(int(c["seed"], 16), c["ew"], c["kind"])
    for i, v in c.get("yset", []):
        ymm[i // 4][i % 4] = int(v, 16)
    return ymm, win


def _avx512_inputs(c):
    from tests.golden.gen_avx512_vectors import case_inputs, guard_window
    zmm, win = case_inputs(int(c["seed"], 16))
    return [v for r in zmm for v in r], guard_window(win, c["guard"])


def _avx512x_inputs(c):
    """case_inputs(seed), then the case's deliberate inputs (zov: whole
    registers, wov: window bytes), then the guard."""
    from tests.golden.gen_avx512_vectors import case_inputs, guard_window
    zmm, win = case_inputs(int(c["seed"], 16))
    zmm = [list(v) for v in zmm]
    for r, q in c.get("zov", []):
        zmm[r] = [int(v, 16) for v in q]
    win = bytearray(win)
    for off, hx in c.get("wov", []):
        bs = bytes.fromhex(hx)
        win[off: off + len(bs)] = bs
    return [v for r in zmm for v in r], guard_window(bytes(win), c["guard"])


# What each family compares (on every executor), and which lanes' windows the
# GPU executor reads back (i: the lane).
_CLEAN = ("status", "icount", "gpr", "flags", "rip")
_FP = _CLEAN + ("vec", "mxcsr", "fault")
_EVEX = _CLEAN + ("vec", "k", "mem", "fault")
_every = lambda i, c: True  # noqa: E731
NATIVE = Native("native", _CLEAN + ("mem",), lambda i, c: c["diff"] or i % 7 == 0)
SSE = Sse("sse", _CLEAN + ("vec", "mxcsr", "mem"), lambda i, c: c["diff"] or i % 5 == 0)
MMX = Mmx("mmx", _CLEAN + ("vec", "x87", "mem"), lambda i, c: bool(c["diff"]))
AVX = Avx("avx", _CLEAN + ("vec", "mem"), lambda i, c: c["diff"] or i % 5 == 0)
FP = FpFormat("fp", _FP, None, _fp_inputs)   # no loop ever compared fp's window
SSE4 = FpFormat("sse4", _FP + ("mem",), lambda i, c: bool(c.get("mdiff")), _sse4_inputs)
EXT = FpFormat("ext", _FP + ("mem",), lambda i, c: bool(c.get("mdiff")), _ext_inputs)
AVX2X = FpFormat("avx2x", _FP + ("mem",), lambda i, c: bool(c.get("mdiff")), _avx2x_inputs)
X87 = X87Stack("x87", ("status", "icount", "flags", "rip", "vec", "x87", "mem", "fault"), _every)
X87D = X87Stack("x87_directed", X87.fields, _every)   # the single-form instructions by operand class
AVX512 = Evex("avx512", _EVEX, _every, _avx512_inputs)
AVX512X = Evex("avx512x", _EVEX, _every, _avx512x_inputs)
FAMILIES = (NATIVE, SSE, MMX, AVX, FP, SSE4, EXT, AVX2X, X87, X87D, AVX512, AVX512X)


# ---------------------------------------------------------------- executors
def cpu_case(fam, c):
    """One case in its own address space: (space, registers, window)."""
    regs = regs_from_state(user_state(CODE_VA, 0, CR3))
    fam.init(regs)
    win = fam.setup(c, regs)
    sp = fam.space(bytes.fromhex(c["code"]) + b"\xcc", CODE_VA, win, fam.group(c), **fam.space_at(c))
    assert sp.cr3 == CR3
    return sp, regs, win


def replay_oracle(fam, cases, tenet=False):
    """One Outcome per case from one oracle step (tenet: with its Tenet stream)."""
    for c in cases:
        sp, regs, win = cpu_case(fam, c)
        o = oracle_of(sp)
        o.restore(regs)
        if tenet:
            o.set_tenet(True)
        ex = o.step()
        r = o.regs()
        mem = None
        if "mem" in fam.fields:
            mem = b"".join(o.read_virt(fam.win_va(c) + off, n) if mapped and n else bytes(n)
                           for off, n, mapped in fam.case_segments(c))
        yield Outcome("oracle", ex.status == RUNNING, ex.status, ex.vector, ex.error, ex.addr, o.icount(), r.rip,
                      CODE_VA, r, regs, win, mem, nbytes=o.nbytes(), mapped=fam.mapped(c),
                      tenet=o.tenet() if tenet else None)


def replay_sim(fam, cases, fast=False, tenet=False):
    """One Outcome per case from the engine's lane code built for the host;
    fast=True goes through k_run's fast-loop digest first (tenet: with the
    run's Tenet stream)."""
    for c in cases:
        win_va = fam.win_va(c) if "mem" in fam.fields else 0
        sp, regs, win = cpu_case(fam, c)
        stream = None
        if tenet:
            simlane.lib().sim_set_tenet(TENET_CAP)
        out, fin, cnt = simlane.run(sp, regs, fast=fast, win_va=win_va)
        if tenet:
            buf = C.create_string_buffer(TENET_CAP)
            stream = buf.raw[:n] if (n := simlane.lib().sim_tenet(buf, TENET_CAP)) else b""
            simlane.lib().sim_set_tenet(0)
        yield Outcome("sim", out.status == EXIT_INT3 and out.icount == 1, out.status, out.vector, out.error,
                      out.addr, out.icount, out.rip, CODE_VA, fin, regs, win,
                      bytes(out.win[:fam.win_len]) if win_va else None, cnt, out.nbytes, fam.mapped(c), stream)


def replay_gpu(fam, cases):
    """One Outcome per case from k_run: per address-space group one Engine,
    case i of the group on lane i, one 32-byte code slot (the code, then int3)
    per distinct code in sorted order, the lane count rounded up to 64 with the
    padding lanes on a lone int3, every lane's window written with apply_writes
    at the case's own place (win_va). A placed case's window is read back
    whenever its operand is written."""
    from wtf_amd.engine import Engine

    outcomes = [None] * len(cases)
    for group in sorted({fam.group(c) for c in cases}):
        idx = [j for j, c in enumerate(cases) if fam.group(c) == group]
        codes = sorted({cases[j]["code"] for j in idx})
        slot = {code: i for i, code in enumerate(codes)}
        blob = bytearray(32 * len(codes))
        for code, i in slot.items():
            b = bytes.fromhex(code) + b"\xcc"
            blob[32 * i: 32 * i + len(b)] = b
        cva = fam.gpu_code_va
        sp = fam.space(bytes(blob), cva, bytes(fam.win_len), group, nx=True)
        n = (len(idx) + 63) // 64 * 64
        eng = Engine(0)
        try:
            eng.load_pool(*sp.phys())
            eng.alloc_lanes(n, overlay_pages=4, cov_entries=64)
            init = regs_from_state(user_state(cva, 0, sp.cr3))
            fam.init(init)
            eng.set_initial_state(init)
            eng.set_limit(0)
            eng.restore()
            regs = eng.read_regs(0, n)
            writes, wins = [], []
            for i, j in enumerate(idx):
                c = cases[j]
                win = fam.setup(c, regs[i])
                wins.append(win)
                regs[i].rip = cva + 32 * slot[c["code"]]
                writes += [(i, fam.win_va(c) + off, win[off:off + ln]) for off, ln, mapped in fam.case_segments(c)
                           if mapped and ln]
            first = cases[idx[0]]["code"]
            for i in range(len(idx), n):  # padding lanes run a lone int3
                regs[i].rip = cva + 32 * slot[first] + len(first) // 2
            eng.write_regs(regs)
            eng.apply_writes(writes)
            eng.run()
            ex = eng.exits()
            out = eng.read_regs(0, n)
            nb = eng.nbytes()
            for i, j in enumerate(idx):
                c, e, mem = cases[j], ex[i], None
                if "mem" in fam.fields and (fam.mem_sample(i, c) or ("at" in c and c["at"].writes)):
                    mem = b"".join(eng.read_virt(i, fam.win_va(c) + off, ln) if mapped and ln else bytes(ln)
                                   for off, ln, mapped in fam.case_segments(c))
                outcomes[j] = Outcome("gpu", e.status == EXIT_INT3 and e.icount == 1, e.status, e.vector, e.error,
                                      e.addr, e.icount, out[i].rip, regs[i].rip, out[i], regs[i], wins[i], mem,
                                      nbytes=int(nb[i]), mapped=fam.mapped(c))
        finally:
            eng.close()
    assert all(o is not None for o in outcomes)
    return outcomes


def run_family(fam, executor, cases, **kw):
    """The failures of `cases` on one executor: (name, code) + the mismatch."""
    fails = []
    for c, o in zip(cases, executor(fam, cases, **kw), strict=True):
        bad = fam.check(c, o)
        if bad:
            fails.append((c.get("name", fam.name), c["code"]) + bad)
    return fails


# ---------------------------------------------------------------- placements
# A placement moves a case's window from buf_va to `va` on the same two pages,
# so that its memory operand meets the page edge; the case's pointer registers
# (inputs and expectations) move with it, every other expected value stays the
# native one. Where the operand is comes from one oracle run at the original
# place with Tenet on: the first access of 2 bytes or more.
TN_R, TN_W, TN_RW = 1, 2, 3
KINDS = ("straddle", "absent", "flush")
SPLITS = {2: (1,), 4: (1, 2, 3), 8: (1, 4, 7), 10: (1, 8, 9), 16: (1, 8, 12, 15), 32: (1, 8, 16, 20, 31)}
PLACED = (NATIVE, SSE, MMX, AVX, FP, SSE4, EXT, AVX2X, X87, X87D)   # the Evex families' window is on the edge already


def splits(n):
    """How many of an n-byte operand's bytes end the first page: cuts inside
    an 8-byte piece and between pieces."""
    return SPLITS.get(n) or (1, n // 2, n - 1)


@dataclasses.dataclass(frozen=True)
class Place:
    kind: str            # "straddle" / "absent" / "flush", or "cut": the whole window so many bytes before the edge
    va: int              # where the window sits
    access: tuple        # the operand at its new place: (va, type, length)
    split: int           # the operand's bytes on the first page
    rule: str            # "native": judged by check(); "fault": the derived #PF; "oracle": equal to the oracle
    why: str = ""        # rule "oracle": "aligned" (#GP(0)), "address" (ADDRESS_DEPENDENT) or "masked" (byte_masked)

    @property
    def present2(self):
        return self.kind in ("straddle", "cut")

    @property
    def writes(self):
        return self.access[1] != TN_R


def tenet_accesses(stream):
    from tests.test_tenet import parse
    return [e[1:] for e in parse(stream) if e[0] == "acc"]


@functools.lru_cache(maxsize=None)
def accesses(fam):
    """Per case of the family's file: its data accesses at the original place
    as ((va, type, length), ...), from the oracle's Tenet stream."""
    return tuple(tuple((va, ty, len(data)) for va, ty, data in tenet_accesses(o.tenet))
                 for o in replay_oracle(fam, fam.doc["cases"], tenet=True))


def opcode_of(code):
    """(vex, pp, map, opcode, modrm.reg, rex_w) of one instruction's bytes; pp: 0 none, 1 66, 2 f3, 3 f2."""
    i = pp = w = 0
    while code[i] in (0x66, 0xF2, 0xF3, 0x2E, 0x36, 0x3E, 0x26, 0x64, 0x65, 0x67, 0xF0):
        pp = {0x66: pp or 1, 0xF3: 2, 0xF2: 3}.get(code[i], pp)
        i += 1
    if code[i] in (0xC4, 0xC5):
        if code[i] == 0xC5:
            m, pp, i = 1, code[i + 1] & 3, i + 2
        else:
            m, pp, w, i = code[i + 1] & 0x1F, code[i + 2] & 3, code[i + 2] >> 7, i + 3
        return True, pp, m, code[i], (code[i + 1] >> 3) & 7, w
    if 0x40 <= code[i] <= 0x4F:
        w, i = (code[i] >> 3) & 1, i + 1
    m = 0
    if code[i] == 0x0F:
        m, i = 1, i + 1
        if code[i] in (0x38, 0x3A):
            m, i = 2 if code[i] == 0x38 else 3, i + 1
    return False, pp, m, code[i], (code[i + 1] >> 3) & 7 if i + 1 < len(code) else 0, w


# SDM vol. 1 table 14-22 / vol. 2 per instruction: a legacy-SSE 16-byte memory
# operand must be aligned except for the unaligned moves (and the string
# compares, which say so themselves); VEX forms need no alignment except the
# aligned and non-temporal moves; cmpxchg16b's operand is aligned. (pp, map, opcode):
LEGACY_UNALIGNED = {(0, 1, 0x10), (0, 1, 0x11),     # movups
                    (1, 1, 0x10), (1, 1, 0x11),     # movupd
                    (2, 1, 0x6F), (2, 1, 0x7F),     # movdqu
                    (3, 1, 0xF0),                   # lddqu
                    (1, 3, 0x60), (1, 3, 0x61), (1, 3, 0x62), (1, 3, 0x63)}   # pcmpestrm / estri / istrm / istri
VEX_ALIGNED = {(0, 1, 0x28), (0, 1, 0x29),          # vmovaps
               (1, 1, 0x28), (1, 1, 0x29),          # vmovapd
               (1, 1, 0x6F), (1, 1, 0x7F),          # vmovdqa
               (0, 1, 0x2B), (1, 1, 0x2B),          # vmovntps / vmovntpd
               (1, 1, 0xE7), (1, 2, 0x2A)}          # vmovntdq / vmovntdqa


def aligned_form(c, length):
    """The case's memory operand (of `length` bytes) must be aligned: a
    misaligned place is #GP(0)."""
    vex, pp, m, op, reg, w = opcode_of(bytes.fromhex(c["code"]))
    if vex:
        return length in (16, 32) and (pp, m, op) in VEX_ALIGNED
    if (m, op, reg, w) == (1, 0xC7, 1, 1):          # cmpxchg16b
        return True
    return m >= 1 and length == 16 and (pp, m, op) not in LEGACY_UNALIGNED


# Cases whose result depends on where the window is: a pointer register is also
# data, or a pointer is stored to memory. The native result holds at buf_va
# only, so these are judged equal to the oracle on every field.
# {(family, name, code): (why, m)}: the native result still holds where the
# window moved by a multiple of m (0: nowhere).
ADDRESS_DEPENDENT = {
    ("native", "enter.0", "c8180000"): ("enter 0x18, 0 pushes rbp, which points into the window", 0),
    ("native", "enter.1", "c8180001"): ("enter 0x18, 1 pushes rbp and the new frame pointer", 0),
    ("native", "enter.2", "c8180002"): ("enter 0x18, 2 pushes rbp and the new frame pointer", 0),
    ("native", "enter.3", "c8180003"): ("enter 0x18, 3 pushes rbp and the new frame pointer", 0),
    ("native", "enter.33", "c8000121"): ("enter 0x100, 33 (level 1) pushes rbp and the new frame pointer", 0),
    ("ext", "shlx.w0.m", "c4e249f75e08"): ("shlx ebx, [rsi + 8], esi: the count is the pointer's low five bits", 32),
    ("ext", "pdep.w0.m", "c4e243f52f"): ("pdep ebp, edi, [rdi]: the pointer is the source operand", 0),
    ("ext", "movbe64.st.m", "4d0f38f16d11"): ("movbe [r13 + 0x11], r13: the pointer is the stored value", 0),
}


def byte_masked(c):
    """maskmovq / maskmovdqu: which bytes are stored, and so whether the store
    faults, depends on the mask register."""
    vex, pp, m, op, reg, w = opcode_of(bytes.fromhex(c["code"]))
    return m == 1 and op == 0xF7


def rebase(fam, c, delta):
    """The case with its pointer values (input GPRs, expected GPRs) moved by delta."""
    lo, hi = fam.buf_va - 0x100, fam.buf_va + fam.win_len + 0x100

    def mv(h):
        v = int(h, 16)
        return format(v + delta, "x") if lo <= v < hi else h
    out = dict(c)
    if "in" in c:
        out["in"] = [mv(h) for h in c["in"]]
    if isinstance(c.get("out"), list):
        out["out"] = [mv(h) for h in c["out"]]
    if "gdiff" in c:
        out["gdiff"] = [[i, mv(h)] for i, h in c["gdiff"]]
    return out   # (the x87 families' one pointer, gpr[6], is set from win_va in setup)


def place(fam, i, kind):
    """Case i of the family's file at a placement of `kind`, or None where the
    kind does not apply to it."""
    c, acc = fam.doc["cases"][i], accesses(fam)[i]
    first = next((a for a in acc if a[2] >= 2), None)
    if first is None or (kind != "straddle" and len(acc) != 1):
        return None
    va, ty, ln = first
    if not (fam.buf_va <= va and va + ln <= fam.buf_va + fam.win_len):
        return None
    aligned = aligned_form(c, ln)
    if kind == "absent" and aligned:
        return None     # #GP(0) comes first
    sp = splits(ln)
    split = ln if kind == "flush" else sp[i % len(sp)]
    new_va = fam.page + 0x1000 - split - (va - fam.buf_va)
    delta = new_va - fam.buf_va
    _, m = ADDRESS_DEPENDENT.get((fam.name, c.get("name", ""), c["code"]), ("", None))
    if kind == "absent":
        rule, why = ("oracle", "masked") if byte_masked(c) else ("fault", "")
    elif kind == "straddle" and aligned:
        rule, why = "oracle", "aligned"
    elif m is not None and (m == 0 or delta % m):
        rule, why = "oracle", "address"
    else:
        rule, why = "native", ""
    return dict(rebase(fam, c, delta), at=Place(kind, new_va, (va + delta, ty, ln), split, rule, why), index=i)


def placed_cases(fam, kind):
    return [p for p in (place(fam, i, kind) for i in range(len(fam.doc["cases"]))) if p is not None]


def cut_case(fam, i, cut):
    """Case i with its whole window `cut` bytes before the page edge, both pages present."""
    c, acc = fam.doc["cases"][i], accesses(fam)[i]
    new_va = fam.page + 0x1000 - cut
    delta = new_va - fam.buf_va
    va, ty, ln = acc[0]
    return dict(rebase(fam, c, delta), at=Place("cut", new_va, (va + delta, ty, ln), cut, "native"), index=i)


def reg_state(r):
    """Every register an instruction of these families can change."""
    return (bytes(r.gpr), r.rflags, r.mxcsr, r.fpcw, r.fpsw, r.fptw, bytes(r.fpst), bytes(r.fpse), bytes(r.xmm),
            bytes(r.ymmh), bytes(r.zmmh), bytes(r.k))


def differs(o, ref):
    """Where o is not what the oracle made of the same placed case (ref)."""
    def exit_of(x):   # (a clean step: RUNNING from the oracle, the int3 behind the instruction from the engine)
        return (RUNNING, 0, 0, 0, 1) if x.clean else (x.status, x.vector, x.error, x.addr, x.icount)
    for name, a, b in (("exit", exit_of(o), exit_of(ref)), ("rip", o.rip - o.entry, ref.rip - ref.entry),
                       ("bytes", o.nbytes, ref.nbytes)):
        if a != b:
            return ("oracle " + name, a, b)
    if reg_state(o.regs) != reg_state(ref.regs):
        return ("oracle regs",)
    if o.mem is not None and ref.mem is not None and o.mem[:o.mapped] != ref.mem[:o.mapped]:
        return ("oracle mem",)
    return None


def bytes_differ(fam, c, o, ref):
    if "bytes" in fam.fields_of(c) and "bytes" not in fam.skip.get(o.executor, ()) and o.nbytes != ref.nbytes:
        return ("bytes", o.nbytes, ref.nbytes)
    return None


def judge(fam, c, o, ref):
    """A mismatch tuple, or None, for a placed case; ref: the oracle's Outcome
    of the same placed case (native execution has no byte count)."""
    at = c["at"]
    if at.rule == "oracle":
        return differs(o, ref)
    if at.rule == "fault":      # the operand's first byte on the absent page is the one that faults
        want = (EXIT_FAULT, 14, 4 | (2 if at.writes else 0), fam.page + 0x1000, 0, 0)
        got = (o.status, o.vector, o.error, o.addr, o.icount, o.rip - o.entry)
        if got != want:
            return ("pf", got, want)
        if o.mem is not None and o.mem[:o.mapped] != o.window[:o.mapped]:
            return ("pf mem",)
        if reg_state(o.regs) != reg_state(ref.regs):
            return ("pf regs",)
        return bytes_differ(fam, c, o, ref)
    return fam.check(c, o) or bytes_differ(fam, c, o, ref)


def run_placed(fam, executor, cases, refs, **kw):
    """The failures of placed `cases` on one executor: (name, code, kind, split) + the mismatch."""
    fails = []
    for c, o, ref in zip(cases, executor(fam, cases, **kw), refs, strict=True):
        bad = judge(fam, c, o, ref)
        if bad:
            fails.append((c.get("name", fam.name), c["code"], c["at"].kind, c["at"].split) + bad)
    return fails


# ---- gathers across the edge
GATHER_CUTS = (64, 128, 192)


def gather_cut_cases():
    """Every avx2x gather case that loads two or more elements, its window 64,
    128 and 192 bytes before the page edge."""
    fam = AVX2X
    return [cut_case(fam, i, cut) for i, c in enumerate(fam.doc["cases"])
            if c["kind"] == "gather" and len(accesses(fam)[i]) >= 2 for cut in GATHER_CUTS]


def elements_on_both_pages(fam, c):
    """The gather's loaded elements (at the case's place) begin on both pages."""
    edge, delta = fam.page + 0x1000, c["at"].va - fam.buf_va
    acc = [va + delta for va, ty, ln in accesses(fam)[c["index"]]]
    return any(va < edge for va in acc) and any(va >= edge for va in acc)


# vpgatherdd ymm0, [rax + ymm2 * 1], ymm1 with each of the eight elements across
# a page edge of its own: 16 data pages, one TLB miss each.
GATHER8_CODE = bytes([0xC4, 0xE2, 0x75, 0x90, 0x04, 0x10])
GATHER8_BASE = 0x7FF000200000


def gather8_case(code_va=CODE_VA, nx=False):
    """(space, registers, the eight expected elements): element j has 1 + j % 3
    of its four bytes at the end of data page 2j, the rest on page 2j + 1."""
    sp = AddressSpace()
    sp.map(code_va, GATHER8_CODE + b"\xcc", write=False)
    idx, want = [], []
    for j in range(8):
        a, b = bytearray(4096), bytearray(4096)
        n0 = 1 + j % 3
        el = bytes([0x10 * j + k + 1 for k in range(4)])
        a[4096 - n0:] = el[:n0]
        b[:4 - n0] = el[n0:]
        sp.map(GATHER8_BASE + 0x2000 * j, bytes(a), nx=nx)
        sp.map(GATHER8_BASE + 0x2000 * j + 0x1000, bytes(b), nx=nx)
        idx.append(0x2000 * j + 0x1000 - n0)
        want.append(int.from_bytes(el, "little"))
    regs = regs_from_state(user_state(code_va, 0, sp.cr3))
    regs.gpr[0] = GATHER8_BASE
    y = [0] * 64
    y[4:8] = [0x8000000080000000] * 4                                  # ymm1: all eight masked in
    y[8:12] = [idx[2 * q] | idx[2 * q + 1] << 32 for q in range(4)]    # ymm2: the indices
    set_ymm(regs, y)
    return sp, regs, want
