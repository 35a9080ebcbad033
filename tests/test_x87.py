"""x87 arithmetic (convention U42; engine_x87.h, oracle/x86_oracle_x87.inc).

The golden vectors (tests/golden/gen_x87_vectors.py) hold random x87 states
under every non-control d8-df form with the host CPU's answer (the oracle
runs each form natively): they pin the oracle's native path (regression) and
the engine's integer extended-precision arithmetic built for the host; the
GPU runs the same vectors in tests/test_gpu_sse.py. A second file holds
directed cases for the instructions with a single encoding (fsqrt, frndint,
fscale, fprem / fprem1, fxtract, fxam, the integer stores): replayed the same
way, its operand classes counted from the inputs in exact arithmetic, and the
recorded values of its plain cases checked against an exact model. Hand-checked
here: #UD / #NM / #MF / UNIMPLEMENTED, stores that fault, FNINIT, the FSW that
a loaded image normalises, and the MMX exponent words.
"""
import collections
import math
from fractions import Fraction

import pytest

from tests import simlane
from tests.golden.gen_x87_vectors import case_regs, mem_forms, reg_forms, run_oracle
from tests.insn_cases import BUF, layout, oracle_of
from tests.vector_replay import X87, X87D, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, EXIT_UNIMPLEMENTED

DOC = X87.doc


def run_sim(c, buf_va):
    """One case through the engine's host build, in run_oracle's form."""
    sp, regs = layout(bytes.fromhex(c["code"]), buf_va, bytes.fromhex(c["mem"]))
    regs.gpr[6] = buf_va
    case_regs(c, regs)
    out, r, _ = simlane.run(sp, regs, win_va=buf_va)
    st = 0 if out.status == 3 else out.status
    return dict(status=st, vector=out.vector if st == EXIT_FAULT else 0, fcw=r.fpcw, fsw=r.fpsw, ftw=r.fptw,
                st=[(r.fpst[i], r.fpse[i]) for i in range(8)], fl=r.rflags & 0x8D5, mem=bytes(out.win[:16]).hex())


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_x87_vectors(chunk):
    cases = DOC["cases"][chunk::2]
    fails = run_family(X87, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


@pytest.mark.parametrize("chunk", range(2))
def test_engine_x87_code_matches_vectors(chunk):
    cases = DOC["cases"][chunk::2]
    fails = run_family(X87, replay_sim, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


def test_x87_vector_file_covers_every_form():
    codes = {c["code"] for c in DOC["cases"]}
    for f in reg_forms():
        assert f.hex() in codes, f.hex()
    for f, _ in mem_forms():
        assert f.hex() in codes, f.hex()
    assert len(DOC["cases"]) > 4000
    # every outcome class appears: faults (#MF), stack faults, unmasked exceptions, stores
    outs = [c["out"] for c in DOC["cases"]]
    assert any(o["status"] == EXIT_FAULT and o["vector"] == 16 for o in outs)
    assert sum(1 for o in outs if o["fsw"] & 0x40) > 200
    assert sum(1 for o in outs if o["fsw"] & 0x8000) > 500


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_x87_directed_vectors(chunk):
    cases = X87D.doc["cases"][chunk::2]
    fails = run_family(X87D, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


@pytest.mark.parametrize("chunk", range(2))
def test_engine_x87_code_matches_directed_vectors(chunk):
    cases = X87D.doc["cases"][chunk::2]
    fails = run_family(X87D, replay_sim, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


# ---- the directed file's operands, from the cases' inputs in exact arithmetic
J = 1 << 63
BIAS = 16383
FSQRT, FRNDINT, FSCALE, FPREM, FPREM1, FXTRACT, FXAM = "d9fa", "d9fc", "d9fd", "d9f8", "d9f5", "d9f4", "d9e5"
PREC = {0: 24, 2: 53, 3: 64}


def f80_class(v):
    m, e = v[0], v[1] & 0x7FFF
    if e == 0:
        return "zero" if m == 0 else "pseudo-denormal" if m & J else "denormal"
    if e == 0x7FFF:
        if not m & J:
            return "pseudo"            # pseudo-infinity / pseudo-NaN
        if m == J:
            return "inf"
        return "qnan" if m & (J >> 1) else "snan"
    return "normal" if m & J else "unnormal"


def f80_sign(v):
    return v[1] >> 15


def f80_mag(v):
    """|v| of a zero, denormal, pseudo-denormal or normal"""
    return Fraction(v[0]) * Fraction(2) ** (max(v[1] & 0x7FFF, 1) - BIAS - 63)


def ilog2(x):
    """floor(log2 x) of a positive Fraction"""
    n = x.numerator.bit_length() - x.denominator.bit_length()
    return n if Fraction(2) ** n <= x else n - 1


def st_of(c, i):
    """ST(i) of a case's input, or None where its register is empty"""
    top = (c["fsw"] >> 11) & 7
    return None if (c["ftw"] >> (2 * ((top + i) & 7))) & 3 == 3 else tuple(c["st"][i])


def runs(c):
    """no unmasked exception is pending: the instruction executes"""
    return not (c["fsw"] & ~c["fcw"] & 0x3F)


def of_code(code):
    return [c for c in X87D.doc["cases"] if c["code"] == code and runs(c)]


def sqrt_parts(v):
    """floor(sqrt(v) * 2^k) for a k that leaves more than 64 bits, whether that is exact, and k"""
    m, e = v[0], (v[1] & 0x7FFF or 1) - BIAS - 63
    if e & 1:
        m, e = m << 1, e - 1
    r = math.isqrt(m << 128)          # sqrt(v) = sqrt(m * 2^128) * 2^(e / 2 - 64)
    return r, r * r == m << 128, e // 2 - 64


def round_sig(r, sticky, prec, rc, s):
    """The integer r (+ a sticky fraction) to prec significant bits under RC
    for sign s: (q, shift) with the result q * 2^shift, q's top bit at prec - 1."""
    sh = r.bit_length() - prec
    if sh <= 0:
        q, rem, half = r << -sh, 0, 1
    else:
        q, rem, half = r >> sh, r & ((1 << sh) - 1), 1 << (sh - 1)
    if rc == 0:
        up = rem > half or (rem == half and (sticky or q & 1))
    else:
        up = (rem != 0 or sticky) and ((rc == 1 and s) or (rc == 2 and not s))
    q += up
    if q >> prec:
        q, sh = q >> 1, sh + 1
    return q, sh


def f80_of(s, q, shift):
    """(-1)^s * q * 2^shift as an extended value; q = 0 or exact in 64 bits, a denormal where it must be"""
    if q == 0:
        return 0, s << 15
    low = (q & -q).bit_length() - 1
    q, shift = q >> low, shift + low
    n = q.bit_length()
    e = BIAS + shift + n - 1
    assert 64 - n >= 0
    if e >= 1:
        assert e < 0x7FFF
        return q << (64 - n), (s << 15) | e
    m, rem = divmod(q << 64, 1 << (n + 1 - e))    # 2^(1 - BIAS - 63) is the denormals' ulp
    assert rem == 0 and m < J
    return m, s << 15


def test_x87_directed_file_has_every_class():
    """The operand classes the directed generator promises, counted from the
    inputs alone (integers and Fractions on (significand, exponent); no engine)."""
    assert 5000 < len(X87D.doc["cases"]) <= 9000
    # fsqrt
    inexact, squares, seen = collections.Counter(), 0, collections.Counter()
    for c in of_code(FSQRT):
        a = st_of(c, 0)
        seen[(a is not None and f80_class(a), a is not None and f80_sign(a))] += 1
        if a is None or f80_sign(a) or f80_class(a) not in ("normal", "denormal", "pseudo-denormal"):
            continue
        pc, rc = (c["fcw"] >> 8) & 3, (c["fcw"] >> 10) & 3
        r, exact, _ = sqrt_parts(a)
        low = (r & -r).bit_length() - 1               # trailing zeros: the root's own width
        squares += exact and r.bit_length() - low <= 64
        inexact[(pc, rc)] += not exact or r.bit_length() - low > PREC[pc]
        seen[("mant", a[0])] += 1
        seen[("odd", a[1] & 1)] += 1
    for pc in PREC:
        for rc in range(4):
            assert inexact[(pc, rc)] >= 40, (pc, rc, inexact)
    assert squares >= 100
    for k in [("mant", J), ("mant", 2 * J - 1), ("mant", J | 1), ("odd", 0), ("odd", 1), ("zero", 0), ("zero", 1),
        ("inf", 0),
              ("inf", 1), ("normal", 1), ("denormal", 0), ("pseudo-denormal", 0), ("unnormal", 0), ("qnan", 0),
                  ("snan", 0),
              (False, False)]:
        assert seen[k], k
    # frndint
    frac, ties, zeros, seen = collections.Counter(), 0, 0, collections.Counter()
    for c in of_code(FRNDINT):
        a = st_of(c, 0)
        if a is None or f80_class(a) not in ("normal", "denormal", "pseudo-denormal"):
            continue
        x, rc = f80_mag(a), (c["fcw"] >> 10) & 3
        f = x - int(x)
        frac[rc] += f != 0
        ties += f == Fraction(1, 2)
        zeros += f80_sign(a) and x < Fraction(1, 2)   # -0 under RC 0, 2 and 3
        seen[("exp", (a[1] & 0x7FFF) - BIAS)] += 1
        seen[("int", f == 0)] += 1
        seen[f80_class(a)] += 1
        if x < 1:
            seen[("small", (x > Fraction(1, 2)) - (x < Fraction(1, 2)), rc)] += 1
        elif f:
            seen[("k", int(x) & 1, f * 4 if f.denominator <= 4 else 0, rc)] += 1
    assert all(frac[rc] >= 50 for rc in range(4)), frac
    assert ties >= 40 and zeros >= 20
    for rc in range(4):
        for k in [("small", d, rc) for d in (-1, 0, 1)] + [("k", odd, f, rc) for odd in (0, 1) for f in (1, 2, 3)]:
            assert seen[k], k
    assert all(seen[("exp", e)] >= 4 for e in range(61, 66)) and seen[("int", True)] >= 40 and seen["denormal"] >= 8
    # fprem / fprem1
    for code in (FPREM, FPREM1):
        ds, low, ties, plus1, zero_rem, classes, im = set(), set(), 0, 0, set(), set(), set()
        beside = collections.Counter()   # a remainder within one ulp of ST0 of half of |ST1|, not on it
        for c in of_code(code):
            a, b = st_of(c, 0), st_of(c, 1)
            if a is None or b is None:
                continue
            classes |= {("st0", f80_class(a)), ("st1", f80_class(b))}
            im.add(c["fcw"] & 1)
            if f80_class(a) != "normal" or f80_class(b) != "normal":
                continue
            D = (a[1] & 0x7FFF) - (b[1] & 0x7FFF)
            ds.add(D)
            if not -1 <= D < 64:
                continue
            x = f80_mag(a) / f80_mag(b)
            q, f = int(x), x - int(x)
            half = Fraction(1, 2)
            near = q + (f > half or (f == half and q & 1))
            low.add((near if code == FPREM1 else q) & 7)
            ties += f == half
            plus1 += near == q + 1
            if f != half and abs(f - half) * f80_mag(b) <= Fraction(2) ** ((a[1] & 0x7FFF) - BIAS - 63):
                beside[f > half] += 1
            if f == 0:
                zero_rem.add(f80_sign(a))
            if D == -1:
                classes.add(("D-1", f > half))
            if f == half:
                classes.add(("tie", q & 1))
        assert ds >= set(range(-2, 71)) and max(ds) > 1000, sorted(set(range(-2, 71)) - ds)
        assert low == set(range(8)), low
        assert zero_rem == {0, 1} and im == {0, 1}
        for k in ("inf", "zero", "denormal", "unnormal", "qnan", "snan"):
            assert ("st0", k) in classes and ("st1", k) in classes, k
        if code == FPREM1:
            assert ties >= 40 and plus1 >= 100, (ties, plus1)
            assert beside[False] >= 40 and beside[True] >= 40, beside   # the quotient stays / the sign flips
            assert {("D-1", False), ("D-1", True), ("tie", 0), ("tie", 1)} <= classes
    # fscale: what the exact result a * 2^trunc(b) does
    quad, far, seen = collections.Counter(), collections.Counter(), collections.Counter()
    for c in of_code(FSCALE):
        a, b = st_of(c, 0), st_of(c, 1)
        if a is None or b is None:
            continue
        ca, cb = f80_class(a), f80_class(b)
        seen[("st0", ca)] += 1
        seen[("st1", cb)] += 1
        seen[(ca, cb, f80_sign(b))] += 1
        fin = ("normal", "denormal", "pseudo-denormal")
        if ca not in fin or cb not in fin + ("zero",):
            continue
        if "denormal" in (ca, cb) or "pseudo-denormal" in (ca, cb):
            if not c["fcw"] & 2:
                continue                                 # an unmasked DE: no result
        x = f80_mag(b)
        n = -int(x) if f80_sign(b) else int(x)
        seen[("n", "int" if x.denominator == 1 else "frac<1" if x < 1 else "frac", abs(n) <= 40000)] += 1
        if cb == "normal" and (b[1] & 0x7FFF) - BIAS >= 14:
            seen[("big", min((b[1] & 0x7FFF) - BIAS, 23), f80_sign(b))] += 1
        e = ilog2(f80_mag(a)) + n
        if ca == "normal":
            seen[("end", (a[1] & 0x7FFF) <= 70, (a[1] & 0x7FFF) >= 0x7FFE - 70)] += 1
        if e > BIAS:
            quad[("over", bool(c["fcw"] & 8))] += 1
            far["over"] += not c["fcw"] & 8 and e - 24576 > BIAS
        elif e < 1 - BIAS:
            quad[("under", bool(c["fcw"] & 16))] += 1
            far["under"] += not c["fcw"] & 16 and e + 24576 < 1 - BIAS
    for k in [(w, m) for w in ("over", "under") for m in (False, True)]:
        assert quad[k] >= 30, (k, quad)
    assert far["over"] >= 30 and far["under"] >= 30, far
    for k in ("normal", "denormal", "pseudo-denormal", "zero", "inf", "unnormal"):
        assert seen[("st0", k)], k
    for k in ("normal", "denormal", "zero", "inf", "qnan", "snan"):
        assert seen[("st1", k)], k
    for k in [("inf", "inf", 1), ("zero", "inf", 0), ("denormal", "inf", 0), ("denormal", "inf", 1),
              ("n", "int", True), ("n", "frac", True), ("n", "frac<1", True), ("n", "int", False),
              ("end", True, False), ("end", False, True), ("end", False, False)] + \
             [("big", E, s) for E in range(14, 24) for s in (0, 1)]:
        assert seen[k], k
    # fxtract: every class with ST7 free and full
    cells = {(f80_class(st_of(c, 0)), st_of(c, 7) is None) for c in of_code(FXTRACT) if st_of(c, 0) is not None}
    for k in ("zero", "denormal", "pseudo-denormal", "normal", "inf", "qnan", "snan", "unnormal", "pseudo"):
        assert (k, True) in cells and (k, False) in cells, k
    # fxam: class x sign x tag (the register's contents are judged even when it is empty)
    cells = {(f80_class(c["st"][0]), f80_sign(c["st"][0]), st_of(c, 0) is None) for c in of_code(FXAM)}
    for k in ("zero", "denormal", "pseudo-denormal", "normal", "inf", "qnan", "snan", "unnormal", "pseudo"):
        for s in (0, 1):
            assert (k, s, False) in cells and (k, s, True) in cells, (k, s)
    # the integer stores: each form at its own range end under every RC, IM masked and unmasked
    for code, bits in (("df16", 15), ("df1e", 15), ("df0e", 15), ("db16", 31), ("db1e", 31), ("db0e", 31), ("df3e", 63),
                       ("dd0e", 63)):
        cells = set()
        for c in of_code(code):
            a = st_of(c, 0)
            if a is not None and f80_class(a) == "normal":
                x = f80_mag(a)
                side = "at" if x == 2 ** bits else "below" if 2 ** bits - 1 <= x < 2 ** bits else \
                    "above" if 2 ** bits < x <= 2 ** bits + 2 else "far" if x >= 2 ** 63 else None
                cells.add((side, (c["fcw"] >> 10) & 3))
                cells.add(("im", c["fcw"] & 1))
        assert cells >= {("im", 0), ("im", 1)}
        for side in ("at", "below", "above", "far"):
            assert all((side, rc) in cells for rc in range(4)), (code, side)


def model_value(c):
    """The exact ST0 (and for fprem / fprem1 the C0 C3 C1 quotient bits) of a
    case whose operands are finite normals with every exception masked, or
    None where the model does not apply. The value only, never the flags."""
    code, a, b = c["code"], st_of(c, 0), st_of(c, 1)
    if not runs(c) or c["fcw"] & 0x3F != 0x3F or a is None or f80_class(a) != "normal":
        return None
    pc, rc, s = (c["fcw"] >> 8) & 3, (c["fcw"] >> 10) & 3, f80_sign(a)
    if code == FSQRT:
        if s or pc not in PREC:
            return None
        r, exact, k = sqrt_parts(a)
        q, sh = round_sig(r, not exact, PREC[pc], rc, 0)
        return f80_of(0, q, sh + k), None
    if code == FRNDINT:
        x = f80_mag(a)
        q, f = int(x), x - int(x)
        half = Fraction(1, 2)
        up = (f > half or (f == half and q & 1)) if rc == 0 else f != 0 and ((rc == 1 and s) or (rc == 2 and not s))
        return f80_of(s, q + up, 0) if (q + up).bit_length() <= 64 else a, None
    if b is None or f80_class(b) != "normal":
        return None
    if code == FSCALE:
        x = f80_mag(b)
        e = (a[1] & 0x7FFF) + (-int(x) if f80_sign(b) else int(x))
        return ((a[0], (s << 15) | e), None) if 0 < e < 0x7FFF else None
    if code in (FPREM, FPREM1):
        D = (a[1] & 0x7FFF) - (b[1] & 0x7FFF)
        if D >= 64:
            return None                                  # a partial reduction: how far is the CPU's choice
        x, y = f80_mag(a), f80_mag(b)
        q = int(x / y)
        f = x / y - q
        half = Fraction(1, 2)
        if code == FPREM1 and (f > half or (f == half and q & 1)):
            q += 1
        r = x - q * y
        if r < 0:
            r, s = -r, s ^ 1
        sh = -(r.denominator.bit_length() - 1)           # r = numerator * 2^sh (a power-of-two denominator)
        assert r.denominator == 1 << -sh
        cc = (0x100 if q & 4 else 0) | (0x4000 if q & 2 else 0) | (0x200 if q & 1 else 0)
        return f80_of(s, r.numerator, sh), cc
    return None


def test_x87_directed_recording_matches_the_exact_model():
    """The recording itself: the host's ST0 (fprem / fprem1: and C0 C3 C1, C2
    clear) equals exact arithmetic on every case with normal operands and all
    exceptions masked, and those are at least half of each form's cases."""
    for code in (FSQRT, FRNDINT, FSCALE, FPREM, FPREM1):
        cases = [c for c in X87D.doc["cases"] if c["code"] == code]
        n, bad = 0, []
        for c in cases:
            want = model_value(c)
            if want is None:
                continue
            n += 1
            out = c["out"]
            if tuple(out["st"][0]) != want[0] or (want[1] is not None and out["fsw"] & 0x4700 != want[1]):
                bad.append((c["fcw"], c["st"][:2], out["st"][0], hex(out["fsw"]), want))
        assert not bad, (code, len(bad), bad[:3])
        assert 2 * n >= len(cases), (code, n, len(cases))


def test_x87_directed_file_holds_the_fscale_saturation_case():
    """An unmasked overflow that is still out of range after the -24576
    adjust: the host delivers a signed infinity with C1 = 1 under every RC."""
    hits = collections.Counter()
    for c in of_code(FSCALE):
        o, top = c["out"], (c["fsw"] >> 11) & 7
        if not c["fcw"] & 8 and o["fsw"] & 8 and o["status"] == 0:
            r = tuple(o["st"][0])
            if r[1] & 0x7FFF == 0x7FFF:
                assert r[0] == J and r[1] >> 15 == f80_sign(c["st"][0]) and o["fsw"] & 0x200, (c["fcw"], c["st"][:2], r)
                hits[((c["fcw"] >> 10) & 3, r[1] >> 15)] += 1
            assert (o["fsw"] >> 11) & 7 == top
    assert all(hits[(rc, s)] for rc in range(4) for s in (0, 1)), hits


ONE = (0x8000000000000000, 0x3FFF)


def x87_case(code, **kw):
    c = dict(code=bytes(code).hex(), mem="00" * 16, fcw=0x37F, fsw=0, ftw=0xFFFF, st=[(0, 0)] * 8, fl=0)
    c.update(kw)
    return c


X87_FAULT_CASES = [
    ([0xD9, 0xD1], EXIT_FAULT, 6, {}),                        # reserved d9 d1
    ([0xDD, 0xF0], EXIT_FAULT, 6, {}),                        # reserved dd f0
    ([0xD9, 0x0E], EXIT_FAULT, 6, {}),                        # d9 /1 m: reserved
    ([0xDB, 0x26], EXIT_FAULT, 6, {}),                        # db /4 m: reserved
    ([0xD9, 0xFE], EXIT_UNIMPLEMENTED, None, {}),             # fsin: outside
    ([0xD9, 0xFF], EXIT_UNIMPLEMENTED, None, {}),             # fcos: outside
    ([0xDF, 0x26], 0, None, {}),                              # fbld m80bcd (runs)
    ([0xD8, 0xC1], EXIT_FAULT, 16, dict(fcw=0x37E, fsw=0x8081)),  # pending unmasked IE: #MF
    ([0xD8, 0xC1], EXIT_FAULT, 16, dict(fcw=0x37E, fsw=0x0001)),  # pending even with ES clear
    ([0xD8, 0xC1], 0, None, dict(fcw=0x37F, fsw=0x0080)),     # ES alone, every flag masked: runs
    ([0xDB, 0xE0], 0, None, dict(fcw=0x37E, fsw=0x8081)),     # fneni does not wait
    ([0xD9, 0xD0], EXIT_FAULT, 16, dict(fcw=0x37E, fsw=0x8081)),  # fnop waits
]


@pytest.mark.parametrize("code,status,vector,kw", X87_FAULT_CASES)
def test_x87_faults_oracle_and_engine(code, status, vector, kw):
    c = x87_case(code, **kw)
    for got in (run_oracle(c, BUF), run_sim(c, BUF)):
        assert got["status"] == status, (bytes(code).hex(), got["status"], got["vector"])
        if vector is not None:
            assert got["vector"] == vector


def test_x87_nm_when_cr0_ts():
    sp, regs = layout(bytes([0xD9, 0xE8]), BUF, bytes(256), cr0=0x80050033 | 8)
    out, _, _ = simlane.run(sp, regs)
    o = oracle_of(sp)
    o.restore(regs)
    ex = o.step()
    assert (out.status, out.vector) == (EXIT_FAULT, 7) and (ex.status, ex.vector) == (EXIT_FAULT, 7)


def prog_state(code, st0=ONE):
    """A short program over a clean x87 state; rsi = BUF, rdi = BUF + 0x40."""
    sp, regs = layout(bytes(code), BUF, bytes(256))
    regs.gpr[6], regs.gpr[7] = BUF, BUF + 0x40
    regs.fpcw, regs.fptw = 0x37F, 0xFFFF
    return sp, regs


def run_both(code):
    sp, regs = prog_state(code)
    out, fin, _ = simlane.run(sp, regs, win_va=BUF)
    o = oracle_of(sp)
    o.restore(regs)
    for _ in range(64):
        ex = o.step()
        if ex.status != 0:
            break
    return out, fin, ex, o


def test_fninit_keeps_register_contents_and_fxsave_shows_exponents():
    # fld1; fldpi; fninit; fxsave [rdi]; int3: the host keeps R7 = 1 and R6 = pi (TOP = 0)
    code = [0xD9, 0xE8, 0xD9, 0xEB, 0xDB, 0xE3, 0x0F, 0xAE, 0x07]
    out, fin, ex, o = run_both(code)
    img = bytes(out.win[0x40:0x40 + 0xA0])
    assert img == o.read_virt(BUF + 0x40, 0xA0)
    assert int.from_bytes(img[32 + 16 * 7:40 + 16 * 7], "little") == 0x8000000000000000
    assert int.from_bytes(img[40 + 16 * 7:42 + 16 * 7], "little") == 0x3FFF
    assert int.from_bytes(img[32 + 16 * 6:40 + 16 * 6], "little") == 0xC90FDAA22168C235
    assert img[4] == 0 and fin.fpsw == 0 and fin.fptw == 0xFFFF


def test_mmx_write_sets_exponent_word():
    # movq mm0, [rsi]; fxsave [rdi]: ST0 / MM0's sign + exponent read all ones
    code = [0x0F, 0x6F, 0x06, 0x0F, 0xAE, 0x07]
    out, fin, ex, o = run_both(code)
    img = bytes(out.win[0x40:0x40 + 0xA0])
    assert img == o.read_virt(BUF + 0x40, 0xA0)
    assert int.from_bytes(img[40:42], "little") == 0xFFFF and fin.fpse[0] == 0xFFFF


def test_fxrstor_normalises_es():
    # fxrstor [rsi] of fcw = 037e / fsw = 0001 -> fsw 8081; then fnstsw ax
    img = bytearray(512)
    img[0:2] = (0x37E).to_bytes(2, "little")
    img[2:4] = (0x0001).to_bytes(2, "little")
    img[24:28] = (0x1F80).to_bytes(4, "little")
    sp, regs = layout(bytes([0x0F, 0xAE, 0x0E, 0xDF, 0xE0]), BUF, bytes(img[:256]))
    regs.gpr[6] = BUF
    out, fin, _ = simlane.run(sp, regs)
    o = oracle_of(sp)
    o.restore(regs)
    o.step()
    o.step()
    assert fin.fpsw == 0x8081 and out.gpr[0] & 0xFFFF == 0x8081
    assert o.regs().gpr[0] & 0xFFFF == 0x8081


def _env_prog(code, data):
    sp, regs = layout(bytes(code), BUF, bytes(data) + bytes(256 - len(data)))
    regs.gpr[6], regs.gpr[7] = BUF, BUF + 0x80
    regs.fpcw, regs.fptw = 0x37F, 0xFFFF
    out, fin, _ = simlane.run(sp, regs, win_va=BUF)
    o = oracle_of(sp)
    o.restore(regs)
    for _ in range(16):
        if o.step().status != 0:
            break
    env = bytes(out.win[0x80:0x80 + 28])
    assert env == o.read_virt(BUF + 0x80, 28)
    return [int.from_bytes(env[i:i + 2], "little") for i in (0, 4, 8)]


def test_fldenv_frstor_normalise_fcw_and_retag():
    """FLDENV / FRSTOR load FCW as FLDCW does and recompute every non-empty
    tag from the register contents; the values are this host's (fnstenv after
    the load): fldz / fld1 / fldpi, fldenv of fcw 0 / ftw 0 -> 0040 / 4155;
    fcw ffff / ftw aaaa -> 1f7f / 4155; frstor of fcw ffff, ST0 = 1.0 -> 1f7f / 5554."""
    ld3 = [0xD9, 0xEE, 0xD9, 0xE8, 0xD9, 0xEB]           # fldz; fld1; fldpi
    fldenv_fnstenv = [0xD9, 0x26, 0xD9, 0x37, 0xCC]     # fldenv [rsi]; fnstenv [rdi]; int3
    assert _env_prog(ld3 + fldenv_fnstenv, bytes(28)) == [0x0040, 0, 0x4155]
    env = bytearray(28)
    env[0:2], env[8:10] = (0xFFFF).to_bytes(2, "little"), (0xAAAA).to_bytes(2, "little")
    assert _env_prog(ld3 + fldenv_fnstenv, env) == [0x1F7F, 0, 0x4155]
    img = bytearray(108)
    img[0:2] = (0xFFFF).to_bytes(2, "little")
    img[28:36], img[36:38] = (1 << 63).to_bytes(8, "little"), (0x3FFF).to_bytes(2, "little")
    assert _env_prog([0xDD, 0x26, 0xD9, 0x37, 0xCC], img) == [0x1F7F, 0, 0x5554]   # frstor [rsi]; fnstenv [rdi]


def test_x87_store_fault_leaves_the_stack():
    # fstp dword [rsi + 0x2000] (unmapped): #PF (write), TOP and ST0 unchanged
    c = x87_case([0xD9, 0x9E, 0x00, 0x20, 0x00, 0x00], fsw=0x3800, ftw=0x3FFF, st=[ONE] + [(0, 0)] * 7)
    for got in (run_oracle(c, BUF), run_sim(c, BUF)):
        assert (got["status"], got["vector"]) == (EXIT_FAULT, 14)
        assert got["fsw"] == 0x3800 and tuple(got["st"][0]) == ONE
