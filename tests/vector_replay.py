"""One replay harness for the native-execution golden vectors
(tests/golden/*_vectors.json.gz): each family is declared once (how a case is
set up, what is compared), and replayed on three executors: the oracle, the
engine's lane code built for the host (tests/simlane.py) and k_run on the GPU.
Every executor hands the family's one check() the same Outcome record."""
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

    # ---- how a case is laid out
    def group(self, c):
        """Cases of one group share an address space on the GPU."""
        return 0

    def segments(self, group):
        """The window's pieces: (offset, length, mapped)."""
        return [(0, self.win_len, True)]

    def space(self, code, code_va, window, group, nx=False):
        """Code at code_va; the window's page and the page after it."""
        sp = AddressSpace()
        sp.map_range(code_va, code, write=False)
        page = self.buf_va & ~0xFFF
        first = bytearray(4096)
        off = self.buf_va - page
        first[off:off + len(window)] = window
        sp.map(page, bytes(first), nx=nx)
        sp.map(page + 0x1000, b"", nx=nx)
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
        if self.on(o, "mem") and o.mem is not None and o.mem != mem:
            return ("mem", [(i, o.mem[i], mem[i]) for i in range(len(mem)) if o.mem[i] != mem[i]][:6])
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
        regs.gpr[6] = self.buf_va
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
        if self.on(o, "mem") and o.mem is not None and o.mem.hex() != w["mem"]:
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
    sp = fam.space(bytes.fromhex(c["code"]) + b"\xcc", CODE_VA, win, fam.group(c))
    assert sp.cr3 == CR3
    return sp, regs, win


def replay_oracle(fam, cases):
    """One Outcome per case from one oracle step."""
    for c in cases:
        sp, regs, win = cpu_case(fam, c)
        o = oracle_of(sp)
        o.restore(regs)
        ex = o.step()
        r = o.regs()
        mem = None
        if "mem" in fam.fields:
            mem = b"".join(o.read_virt(fam.buf_va + off, n) if mapped else bytes(n)
                           for off, n, mapped in fam.segments(fam.group(c)))
        yield Outcome("oracle", ex.status == RUNNING, ex.status, ex.vector, ex.error, ex.addr, o.icount(), r.rip,
                      CODE_VA, r, regs, win, mem)


def replay_sim(fam, cases, fast=False):
    """One Outcome per case from the engine's lane code built for the host;
    fast=True goes through k_run's fast-loop digest first."""
    win_va = fam.buf_va if "mem" in fam.fields else 0
    for c in cases:
        sp, regs, win = cpu_case(fam, c)
        out, fin, cnt = simlane.run(sp, regs, fast=fast, win_va=win_va)
        yield Outcome("sim", out.status == EXIT_INT3 and out.icount == 1, out.status, out.vector, out.error,
                      out.addr, out.icount, out.rip, CODE_VA, fin, regs, win,
                      bytes(out.win[:fam.win_len]) if win_va else None, cnt)


def replay_gpu(fam, cases):
    """One Outcome per case from k_run: per address-space group one Engine,
    case i of the group on lane i, one 32-byte code slot (the code, then int3)
    per distinct code in sorted order, the lane count rounded up to 64 with the
    padding lanes on a lone int3, every lane's window written with apply_writes."""
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
        segs = fam.segments(group)
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
                writes += [(i, fam.buf_va + off, win[off:off + ln]) for off, ln, mapped in segs if mapped]
            first = cases[idx[0]]["code"]
            for i in range(len(idx), n):  # padding lanes run a lone int3
                regs[i].rip = cva + 32 * slot[first] + len(first) // 2
            eng.write_regs(regs)
            eng.apply_writes(writes)
            eng.run()
            ex = eng.exits()
            out = eng.read_regs(0, n)
            for i, j in enumerate(idx):
                e, mem = ex[i], None
                if "mem" in fam.fields and fam.mem_sample(i, cases[j]):
                    mem = b"".join(eng.read_virt(i, fam.buf_va + off, ln) if mapped else bytes(ln)
                                   for off, ln, mapped in segs)
                outcomes[j] = Outcome("gpu", e.status == EXIT_INT3 and e.icount == 1, e.status, e.vector, e.error,
                                      e.addr, e.icount, out[i].rip, regs[i].rip, out[i], regs[i], wins[i], mem)
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
