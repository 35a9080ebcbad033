"""x87 arithmetic vectors (convention U42): random x87 states (TOP, tags,
control word, sticky flags, register contents of every class the x87 knows:
normals, denormals, pseudo-denormals, zeros, infinities, QNaN / SNaN,
unnormals and pseudo-NaN / infinities) under every non-control d8-df form,
the register forms and the memory forms on [rsi].

The expected results come from the host CPU: the oracle runs each form
natively (oracle/x86_oracle_x87.inc: FXRSTOR, the instruction, FXSAVE), so
the committed file pins the engine's integer extended-precision arithmetic
(wtf_amd/csrc/engine_x87.h) to hardware on the CPU suite and on the GPU.

    python -m tests.golden.gen_x87_vectors   # writes tests/golden/x87_vectors.json.gz

A second file holds directed cases for the forms with one encoding each, which
the random states above reach a handful of times: fsqrt, frndint, fscale,
fprem / fprem1, fxtract, fxam and the integer stores, with ST0 / ST1 chosen by
class (make_directed_cases; tests/test_x87.py counts the classes):

    python -m tests.golden.gen_x87_vectors directed   # tests/golden/x87_directed_vectors.json.gz
"""
from __future__ import annotations

import gzip
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "x87_vectors.json.gz")
DIRECTED_OUT = os.path.join(HERE, "x87_directed_vectors.json.gz")

UD_REG = {
    0xD9: lambda m: (0xD1 <= m <= 0xD7) or m in (0xE2, 0xE3, 0xE6, 0xE7, 0xEF),
    0xDA: lambda m: m >= 0xE0 and m != 0xE9,
    0xDB: lambda m: (0xE5 <= m <= 0xE7) or m >= 0xF8,
    0xDD: lambda m: m >= 0xF0,
    0xDE: lambda m: 0xD8 <= m <= 0xDF and m != 0xD9,
    0xDF: lambda m: (0xE1 <= m <= 0xE7) or m >= 0xF8,
}
UNIMPL_D9 = {0xF0, 0xF1, 0xF2, 0xF3, 0xF9, 0xFB, 0xFE, 0xFF}
CONTROL_REG = {(0xDB, 0xE2), (0xDB, 0xE3), (0xDF, 0xE0)}


def reg_forms():
    out = []
    for op in range(0xD8, 0xE0):
        for m in range(0xC0, 0x100):
            if (op, m) in CONTROL_REG or (op == 0xD9 and m in UNIMPL_D9):
                continue
            if op in UD_REG and UD_REG[op](m):
                continue
            out.append(bytes([op, m]))
    return out


# (op, /r) -> memory operand kind
MEM_KIND = {}
for r in range(8):
    MEM_KIND[(0xD8, r)] = "f32"
    MEM_KIND[(0xDC, r)] = "f64"
    MEM_KIND[(0xDA, r)] = "i32"
    MEM_KIND[(0xDE, r)] = "i16"
for r in (0, 2, 3):
    MEM_KIND[(0xD9, r)] = "f32"
    MEM_KIND[(0xDD, r)] = "f64"
for r in (0, 1, 2, 3):
    MEM_KIND[(0xDB, r)] = "i32"
    MEM_KIND[(0xDF, r)] = "i16"
MEM_KIND[(0xDD, 1)] = "i64"
MEM_KIND[(0xDB, 5)] = MEM_KIND[(0xDB, 7)] = "f80"
MEM_KIND[(0xDF, 5)] = MEM_KIND[(0xDF, 7)] = "i64"


def mem_forms():
    return [(bytes([op, (r << 3) | 6]), k) for (op, r), k in sorted(MEM_KIND.items())]


def rand_f80(rng):
    k = rng.random()
    s = rng.getrandbits(1) << 15
    if k < 0.42:
        e = rng.choice([rng.randint(0x3FFF - 70, 0x3FFF + 70), rng.randint(1, 0x7FFE), rng.randint(1, 40),
                        rng.randint(0x7FFE - 40, 0x7FFE), rng.randint(0x3FFF - 16445, 0x3FFF - 16300) & 0x7FFF or 1])
        m = (1 << 63) | rng.getrandbits(63)
        if rng.random() < 0.4:
            m &= ~((1 << rng.randint(0, 62)) - 1)
        return m, s | e
    if k < 0.52:  # small integers and halves
        v = rng.randint(1, 1 << rng.randint(1, 20))
        sh = 63 - (v.bit_length() - 1)
        return v << sh, s | (0x3FFF + v.bit_length() - 1 - rng.choice([0, 0, 1]))
    if k < 0.58:
        return 0, s
    if k < 0.64:
        return 1 << 63, s | 0x7FFF
    if k < 0.70:
        return (3 << 62) | rng.getrandbits(62) * rng.getrandbits(1), s | 0x7FFF
    if k < 0.75:
        return (1 << 63) | (rng.getrandbits(62) or 1), s | 0x7FFF
    if k < 0.83:
        return rng.getrandbits(63) >> rng.randint(0, 62) or 1, s
    if k < 0.86:
        return (1 << 63) | rng.getrandbits(63), s
    if k < 0.93:  # unnormal
        return rng.getrandbits(63), s | rng.randint(1, 0x7FFE)
    return rng.getrandbits(63), s | 0x7FFF  # pseudo-infinity / pseudo-NaN


def rand_float(rng, w):
    F, E = (23, 0xFF) if w == 32 else (52, 0x7FF)
    s = rng.getrandbits(1) << (w - 1)
    k = rng.random()
    if k < 0.5:
        e = rng.choice([rng.randint(1, E - 1), rng.randint(E // 2 - 30, E // 2 + 30), 1, E - 1])
        f = rng.getrandbits(F)
        if rng.random() < 0.4:
            f &= ~((1 << rng.randint(0, F)) - 1)
        return s | (e << F) | f
    if k < 0.6:
        return s
    if k < 0.7:
        return s | (E << F)
    if k < 0.8:
        return s | (E << F) | (1 << (F - 1)) | rng.getrandbits(F - 1)
    if k < 0.88:
        return s | (E << F) | (rng.getrandbits(F - 1) or 1)
    return s | (rng.getrandbits(F) >> rng.randint(0, F - 1) or 1)


def rand_mem(rng, kind):
    if kind == "f32":
        return rand_float(rng, 32).to_bytes(4, "little")
    if kind == "f64":
        return rand_float(rng, 64).to_bytes(8, "little")
    if kind == "f80":
        m, se = rand_f80(rng)
        return m.to_bytes(8, "little") + se.to_bytes(2, "little")
    n = {"i16": 2, "i32": 4, "i64": 8}[kind]
    v = rng.choice([rng.getrandbits(8 * n), rng.randint(0, 1000), (1 << (8 * n)) - rng.randint(1, 1000),
                    1 << (8 * n - 1), 0])
    return v.to_bytes(n, "little")


def rand_state(rng, pending=False):
    top = rng.randrange(8)
    tw = 0
    full = rng.random()
    for p in range(8):
        empty = rng.random() > (0.85 if full < 0.7 else 0.4)
        tw |= (3 if empty else 0) << (2 * p)
    st = [rand_f80(rng) for _ in range(8)]
    masks = 0x3F if rng.random() < 0.65 else rng.getrandbits(6)
    pc = rng.choice([0, 2, 3, 3, 3, 1])
    rc = rng.randrange(4)
    fcw = 0x40 | masks | (pc << 8) | (rc << 10)
    flags = rng.getrandbits(7) & (masks if not pending else 0x7F)
    cbits = rng.choice([0, 0x4700, rng.getrandbits(16) & 0x4700])
    fsw = (top << 11) | cbits | flags
    if fsw & ~fcw & 0x3F:
        fsw |= 0x8080
    fl = rng.getrandbits(12) & 0x8D5
    return dict(fcw=fcw, fsw=fsw, ftw=tw, st=st, fl=fl)


def case_regs(c, regs):
    """Apply a case's x87 state (and rsi = the buffer) to a Regs."""
    regs.fpcw, regs.fpsw, regs.fptw = c["fcw"], c["fsw"], c["ftw"]
    for i, (m, se) in enumerate(c["st"]):
        regs.fpst[i], regs.fpse[i] = m, se
    regs.rflags = c["fl"] | 0x202
    return regs


def make_cases(seed=0x87, per_reg=5, per_mem=48):
    rng = random.Random(seed)
    cases = []
    for code in reg_forms():
        for _ in range(per_reg):
            cases.append(dict(code=code.hex(), mem="00" * 16, **rand_state(rng, pending=rng.random() < 0.03)))
    for code, kind in mem_forms():
        store = not ((code[0] in (0xD8, 0xDA, 0xDC, 0xDE)) or ((code[1] >> 3) & 7) in (0, 5))
        for _ in range(per_mem):
            m = rand_mem(rng, kind) if not store else bytes(rng.getrandbits(8) for _ in range(10))
            cases.append(dict(code=code.hex(), mem=m.ljust(16, b"\0").hex(), **rand_state(rng, rng.random() < 0.03)))
    # fbld / fbstp (own generator: the cases above keep their values)
    brng = random.Random(seed ^ 0xBCD)
    for code in (bytes([0xDF, 0x26]), bytes([0xDF, 0x36])):
        for _ in range(per_mem * 4):
            st = rand_state(brng, brng.random() < 0.03)
            if code[1] == 0x26:
                m = rand_bcd(brng)
            else:
                m = bytes(brng.getrandbits(8) for _ in range(10))
                if brng.random() < 0.7:  # ST0 in (or near) the packed-BCD range, and valid
                    st["st"][0] = bcd_range_f80(brng)
                    top = (st["fsw"] >> 11) & 7
                    st["ftw"] &= ~(3 << (2 * top))
            cases.append(dict(code=code.hex(), mem=m.ljust(16, b"\0").hex(), **st))
    return cases


def rand_bcd(rng):
    """18 packed digits (a nibble above 9 now and then) and a sign byte."""
    k = rng.random()
    if k < 0.05:
        return bytes(9) + bytes([rng.choice([0, 0x80])])
    if k < 0.1:
        return bytes([0x99] * 9) + bytes([rng.choice([0, 0x80])])
    if k < 0.15:
        return bytes([0, 0, 0, 0, 0, 0, 0, 0xC0, 0xFF, 0xFF])  # the BCD indefinite
    n = rng.randint(1, 18)
    digits = [rng.randrange(10) if i < n else 0 for i in range(18)]
    if rng.random() < 0.15:
        digits[rng.randrange(18)] = rng.randint(10, 15)
    b = bytes(digits[2 * i] | (digits[2 * i + 1] << 4) for i in range(9))
    return b + bytes([rng.choice([0, 0x80, 0x80, rng.getrandbits(8)])])


def bcd_range_f80(rng):
    """An extended value around the packed-BCD range: integers, fractions, halves, 10^18 +- 1."""
    k = rng.random()
    if k < 0.1:
        v, frac = 10**18 + rng.choice([-1, 0, 1]), 0
    else:
        v = rng.randint(0, 10**rng.randint(0, 18))
        frac = rng.choice([0, 0, 1, 2, 3])  # none, a quarter, a half, three quarters
    s = rng.getrandbits(1)
    num = v * 4 + frac
    if num == 0:
        return 0, s << 15
    e = num.bit_length() - 1  # num = 1.f * 2^e, value = num / 4
    m = (num << (63 - e)) & ((1 << 64) - 1) if e <= 63 else num >> (e - 63)
    return m, (s << 15) | (0x3FFF + e - 2)


# ---------------------------------------------------------------- directed cases
J = 1 << 63
M64 = (1 << 64) - 1
INF = (J, 0x7FFF)
ZERO = (0, 0)


def neg(v):
    return v[0], v[1] ^ 0x8000


def sgn(rng, v):
    return neg(v) if rng.getrandbits(1) else v


def f80_int(v, s=0, scale=0):
    """(-1)^s * v * 2^scale for an integer 0 < v < 2^64, normalised."""
    n = v.bit_length()
    assert 0 < n <= 64 and 0 < 0x3FFF + n - 1 + scale < 0x7FFF, (v, scale)
    return v << (64 - n), (s << 15) | (0x3FFF + n - 1 + scale)


def rand_mant(rng):
    m = J | rng.getrandbits(63)
    k = rng.random()
    if k < 0.3:
        m &= ~((1 << rng.randint(1, 62)) - 1)
    elif k < 0.4:
        m |= (1 << rng.randint(1, 62)) - 1
    return m


def rand_normal(rng, lo=1, hi=0x7FFE):
    return rand_mant(rng), (rng.getrandbits(1) << 15) | rng.randint(lo, hi)


def rand_denormal(rng):
    return rng.getrandbits(63) >> rng.randint(0, 62) or 1, rng.getrandbits(1) << 15


def rand_pseudo_denormal(rng):
    return J | rng.getrandbits(63), rng.getrandbits(1) << 15


def rand_unnormal(rng):
    return rng.getrandbits(63), (rng.getrandbits(1) << 15) | rng.randint(1, 0x7FFE)


def rand_qnan(rng):
    return (3 << 62) | rng.getrandbits(62), (rng.getrandbits(1) << 15) | 0x7FFF


def rand_snan(rng):
    return J | (rng.getrandbits(62) or 1), (rng.getrandbits(1) << 15) | 0x7FFF


def rand_pseudo(rng):
    """pseudo-NaN / pseudo-infinity: exponent all ones, J clear"""
    return rng.getrandbits(63) * rng.getrandbits(1), (rng.getrandbits(1) << 15) | 0x7FFF


def rand_special(rng):
    """one value of a class other than the normals"""
    return rng.choice([lambda: sgn(rng, ZERO), lambda: sgn(rng, INF), lambda: rand_denormal(rng),
                       lambda: rand_pseudo_denormal(rng), lambda: rand_unnormal(rng), lambda: rand_qnan(rng),
                       lambda: rand_snan(rng), lambda: rand_pseudo(rng)])()


EMPTY = "empty"


def directed_state(rng, st0=None, st1=None, st7=None, masks=None, pc=None, rc=None, keep=0.1):
    """A rand_state with ST0 / ST1 / ST7 set on purpose ((m, se), EMPTY, or
    None: as drawn) and FCW's fields overridden; one state in ten (`keep`)
    keeps its random registers, half of those with ST0 or ST1 empty."""
    st = rand_state(rng)
    top = (st["fsw"] >> 11) & 7
    fcw = st["fcw"]
    if masks is None and rng.random() < 0.6:
        masks = 0x3F
    if masks is not None:
        fcw = (fcw & ~0x3F) | masks
    if pc is not None:
        fcw = (fcw & ~0x300) | (pc << 8)
    if rc is not None:
        fcw = (fcw & ~0xC00) | (rc << 10)
    st["fcw"] = fcw
    fsw = st["fsw"] & ~0x8080 & ~(~fcw & 0x3F)   # no exception is pending
    st["fsw"] = fsw
    regs = [(0, st0), (1, st1), (7, st7)]
    if rng.random() < keep:
        regs = [(rng.randrange(2), EMPTY)] if rng.getrandbits(1) else []
    for i, v in regs:
        if v is None:
            continue
        p = 2 * ((top + i) & 7)
        if v == EMPTY:
            st["ftw"] |= 3 << p
        else:
            st["ftw"] &= ~(3 << p)
            st["st"][i] = (v[0], v[1])
    return st


def sqrt_operand(rng):
    k = rng.random()
    if k < 0.3:    # the square of a 32-bit integer, or 1 ulp beside it; an odd scale: no square
        n = rng.getrandbits(rng.randint(1, 32)) | 1 << rng.randint(0, 31)
        m, se = f80_int(n * n, 0, 2 * rng.randint(-300, 300) + (rng.random() < 0.15))
        d = rng.choice([0, 0, 0, 1, -1])
        if d and m + d >= J:
            m += d
        return m, se
    if k < 0.62:
        return rand_mant(rng), rng.choice([rng.randint(1, 0x7FFE), rng.randint(0x3FFF - 40, 0x3FFF + 40)])
    if k < 0.72:
        return rng.choice([J, M64, J | 1, M64 - 1]), rng.randint(1, 0x7FFE)
    if k < 0.78:
        return rand_denormal(rng)[0], 0
    if k < 0.82:
        return rand_pseudo_denormal(rng)[0], 0
    if k < 0.85:
        return rand_unnormal(rng)
    if k < 0.88:
        return sgn(rng, ZERO)
    if k < 0.90:
        return INF
    if k < 0.94:   # negative: IE
        return rng.choice([neg(INF), (rand_mant(rng), 0x8000 | rng.randint(1, 0x7FFE)),
                           (rand_denormal(rng)[0], 0x8000)])
    return rng.choice([rand_qnan, rand_snan, rand_pseudo])(rng)


def rndint_operands(rng):
    """a batch of frndint operands; each runs under all four RC"""
    out = []
    for _ in range(30):          # k + 1/4, 1/2, 3/4 for even and odd k up to 2^62
        k = rng.getrandbits(rng.randint(1, 62))
        for f in (1, 2, 2, 3):
            out.append(f80_int(4 * k + f, rng.getrandbits(1), -2))
            k ^= 1
    for _ in range(8):           # |x| < 1: below, at and above a half, and tiny
        e = rng.choice([0x3FFE, 0x3FFD, 0x3FFC, rng.randint(1, 0x3FFB)])
        out += [sgn(rng, (J, 0x3FFE)), sgn(rng, (J | rng.getrandbits(63) or J | 1, 0x3FFE)), sgn(rng, (J | 1, 0x3FFE)),
                sgn(rng, (M64, 0x3FFD)), sgn(rng, (rand_mant(rng), e))]
    for _ in range(6):           # negative values that round to -0 (and to -1)
        out += [(rand_mant(rng), 0x8000 | rng.randint(0x3FF0, 0x3FFD)), (J, 0xBFFE), (J | rng.getrandbits(40), 0xBFFE)]
    for e in range(61, 66):      # around "already an integer"
        for _ in range(5):
            out.append((rng.choice([rand_mant(rng), J | rng.getrandbits(63), M64, J | 1, J | 2, J | 3]),
                        (rng.getrandbits(1) << 15) | (0x3FFF + e)))
    for _ in range(16):          # exact integers
        out.append(f80_int(rng.getrandbits(rng.randint(1, 63)) or 1, rng.getrandbits(1)))
    for _ in range(6):
        out += [rand_denormal(rng), rand_pseudo_denormal(rng)]
    for _ in range(12):
        out.append(rand_special(rng))
    return out


def scale_by(rng, n):
    """ST1 that truncates to n: n itself, or n and a fraction"""
    s = 1 if n < 0 else 0
    a = abs(n)
    if a == 0:
        below_one = (rand_mant(rng), (s << 15) | rng.randint(0x3FFF - 70, 0x3FFE))
        return rng.choice([sgn(rng, ZERO), below_one, rand_denormal(rng)])
    if rng.random() < 0.7 or a.bit_length() > 40:
        return f80_int(a, s)
    k = rng.randint(1, 63 - a.bit_length())
    return f80_int((a << k) | rng.getrandbits(k), s, -k)


def scale_pair(rng, kind):
    """(ST0, ST1) for fscale by what the exact result does; e + n is the result's biased exponent"""
    a = rand_normal(rng)
    if rng.random() < 0.5:   # within 70 of either end, or around 1
        e = rng.choice([rng.randint(1, 70), rng.randint(0x7FFE - 70, 0x7FFE), rng.randint(0x3FFF - 70, 0x3FFF + 70)])
        a = (rand_mant(rng), (rng.getrandbits(1) << 15) | e)
    e = a[1] & 0x7FFF
    if kind == "in":
        n = rng.randint(1, 0x7FFE) - e
    elif kind == "over":
        n = 0x7FFF - e + rng.choice([0, 1, rng.randint(0, 200), rng.randint(0, 24575)])
    elif kind == "over_far":   # beyond the unmasked response's -24576
        n = 0x7FFF + 24576 - e + rng.choice([0, 1, rng.randint(0, 3000), 1 << rng.randint(16, 30), 1 << 62])
    elif kind == "under":
        n = -e - rng.choice([0, 1, rng.randint(0, 70), rng.randint(0, 24575)])
    else:                      # under_far: beyond +24576
        n = -e - 24576 - rng.choice([0, 1, rng.randint(0, 3000), 1 << rng.randint(16, 30), 1 << 62])
    return a, scale_by(rng, n)


def scale_specials(rng):
    den, pden = rand_denormal(rng), rand_pseudo_denormal(rng)
    pinf, ninf = INF, neg(INF)
    big = [f80_int(1 << k, s) for k in range(14, 23) for s in (0, 1)]    # +-2^14 ... +-2^22, and beyond
    big += [f80_int(1 << 40, 0), f80_int(1 << 63, 1), (J, 0x7FFE), (J, 0xFFFE)]
    st0 = [rand_normal(rng), den, pden, sgn(rng, ZERO), sgn(rng, INF), rand_unnormal(rng), rand_qnan(rng),
           rand_snan(rng)]
    st1 = [pinf, ninf, rand_denormal(rng), sgn(rng, ZERO), rand_qnan(rng), rand_snan(rng), rand_unnormal(rng),
           rand_pseudo(rng)] + big
    pairs = [(sgn(rng, INF), ninf), (sgn(rng, ZERO), pinf), (den, pinf), (den, ninf), (pden, pinf), (pden, ninf),
             (sgn(rng, INF), pinf), (sgn(rng, ZERO), ninf)]
    pairs += [(a, b) for a in st0 for b in st1]
    # denormals and pseudo-denormals scaled up into range, to the top and beyond
    for d in (den, pden, rand_denormal(rng)):
        for n in (rng.randint(1, 70), rng.randint(70, 0x7FFE), 0x7FFE + rng.randint(0, 70), 40000, -rng.randint(1, 70)):
            pairs.append((d, scale_by(rng, n)))
    return pairs


def prem_pair(rng, D):
    """normal ST0 / ST1 with e(ST0) - e(ST1) = D"""
    eb = rng.randint(max(1, 1 - D), min(0x7FFE, 0x7FFE - D))
    if rng.random() < 0.6:
        mid = rng.randint(0x3FFF - 300, 0x3FFF + 300)
        if 1 <= mid + D <= 0x7FFE:
            eb = mid
    return (rand_mant(rng), (rng.getrandbits(1) << 15) | (eb + D)), (rand_mant(rng), (rng.getrandbits(1) << 15) | eb)


def prem_tie(rng, delta, exact=False):
    """ST0 = (q + 1/2) * ST1 (exact: q * ST1) for a random q, moved by delta ulps of ST0"""
    nb = rng.randint(2, 30)
    B = rng.getrandbits(nb) | 1 << (nb - 1)
    q = rng.getrandbits(rng.randint(0, 61 - nb))
    if rng.random() < 0.3:
        q = (q & ~7) | rng.randrange(8)
    P = max(q, 1) * B if exact else (2 * q + 1) * B
    K = rng.randint(-300, 300)
    m, se = f80_int(P, rng.getrandbits(1), K if exact else K - 1)
    if J <= m + delta <= M64:
        m += delta
    return (m, se), f80_int(B, rng.getrandbits(1), K)


def prem_specials(rng):
    vals = [sgn(rng, INF), sgn(rng, ZERO), rand_denormal(rng), rand_pseudo_denormal(rng), rand_unnormal(rng),
            rand_qnan(rng), rand_snan(rng), rand_pseudo(rng), rand_normal(rng)]
    pairs = [(a, b) for a in vals for b in vals]
    for _ in range(12):   # a denormal against a normal near it, both ways
        d = rand_denormal(rng)
        pairs += [(d, (rand_mant(rng), rng.randint(1, 70))), ((rand_mant(rng), rng.randint(1, 70)), d),
                  (rand_denormal(rng), rand_denormal(rng))]
    return pairs


def int_store_operands(rng):
    out = []
    for k in (15, 31, 63):
        p = 1 << k
        for s in (0, 1):   # the power of two, and integers, halves, quarters and single ulps either side
            near = [(p, 0), (p - 1, 0), (p + 1, 0), (p - 2, 0), (p + 2, 0), (2 * p - 1, -1), (2 * p + 1, -1),
                    (2 * p - 3, -1), (4 * p - 1, -2), (4 * p - 3, -2), (4 * p + 1, -2)]
            out += [f80_int(v, s, sc) for v, sc in near if v.bit_length() <= 64]
            out += [(M64, (s << 15) | (0x3FFF + k - 1)), (J | 1, (s << 15) | (0x3FFF + k))]
    for s in (0, 1):
        se = s << 15
        # 2^64, [2^63, 2^64), beyond; small values with a fraction; a half, just above it, and tiny
        out += [(J, se | (0x3FFF + 64)), (rand_mant(rng), se | (0x3FFF + 63)), (M64, se | (0x3FFF + 63)),
                (rand_mant(rng), se | (0x3FFF + 64)), (rand_mant(rng), se | rng.randint(0x3FFF + 65, 0x7FFE)),
                f80_int(rng.getrandbits(14) * 4 + 2, s, -2), f80_int(rng.getrandbits(30) * 4 + 1, s, -2),
                f80_int(rng.getrandbits(61) * 4 + 3 | 1 << 62, s, -2),
                (J, se | 0x3FFE), (J | 1, se | 0x3FFE), (rand_mant(rng), se | rng.randint(1, 0x3FFD))]
    out += [rand_special(rng) for _ in range(6)]
    return out


FSQRT, FRNDINT, FSCALE, FPREM, FPREM1, FXTRACT, FXAM = "d9fa", "d9fc", "d9fd", "d9f8", "d9f5", "d9f4", "d9e5"
INT_STORES = ["df16", "df1e", "df0e", "db16", "db1e", "db0e", "df3e", "dd0e"]


def make_directed_cases(seed=0x87D1):
    """fsqrt, frndint, fscale, fprem / fprem1, fxtract, fxam and the integer
    stores over operands chosen by class (its own generator: make_cases()
    keeps its values)."""
    rng = random.Random(seed)
    cases = []

    def add(code, mem=None, **kw):
        cases.append(dict(code=code, mem=(mem or bytes(16)).hex(), **directed_state(rng, **kw)))

    # fsqrt: PC x RC uniform over every operand class
    for i in range(1200):
        add(FSQRT, st0=sqrt_operand(rng), pc=(0, 2, 3)[i % 3], rc=(i // 3) % 4,
            masks=0x3F if rng.random() < 0.8 else None)
    # frndint: every operand under all four RC
    for v in rndint_operands(rng):
        for rc in range(4):
            add(FRNDINT, st0=v, rc=rc, masks=0x3F if rng.random() < 0.75 else None)
    # fscale: in range, masked and unmasked over- / underflow, the specials
    for _ in range(1000):
        a, b = scale_pair(rng, "in")
        add(FSCALE, st0=a, st1=b, masks=0x3F if rng.random() < 0.95 else None)
    for kind in ("over", "over_far", "under", "under_far"):
        for i in range(90):
            a, b = scale_pair(rng, kind)
            add(FSCALE, st0=a, st1=b, masks=0x3F if i % 2 else 0x3F & ~(0x18 | rng.choice([0, 0, 0x20])))
    for a, b in scale_specials(rng):
        add(FSCALE, st0=a, st1=b, masks=rng.choice([0x3F, 0x3F, 0x27, 0x3E, rng.getrandbits(6)]))
    # fprem / fprem1
    for code in (FPREM, FPREM1):
        near = code == FPREM1
        for D in list(range(-2, 64)) * 8 + list(range(64, 71)) * 3 + [rng.randint(71, 0x7FFD) for _ in range(30)]:
            a, b = prem_pair(rng, D)
            add(code, st0=a, st1=b, masks=0x3F if rng.random() < 0.9 else None)
        for i in range(240 if near else 60):   # ties, and 1 ulp above and below
            a, b = prem_tie(rng, (0, 1, -1)[i % 3])
            add(code, st0=a, st1=b, masks=0x3F if rng.random() < 0.9 else None)
        for _ in range(60):                     # zero remainders of both signs
            a, b = prem_tie(rng, 0, exact=True)
            add(code, st0=a, st1=b, masks=0x3F if rng.random() < 0.9 else None)
        for a, b in prem_specials(rng):
            add(code, st0=a, st1=b, masks=rng.choice([0x3F, 0x3F, 0x3E, 0x3D, rng.getrandbits(6)]))
    # fxtract: every class with ST7 free and full
    for _ in range(10):
        power = f80_int(1, rng.getrandbits(1), rng.randint(-16000, 16000))
        for v in (sgn(rng, ZERO), rand_denormal(rng), rand_pseudo_denormal(rng), sgn(rng, INF), rand_qnan(rng),
                  rand_snan(rng), rand_unnormal(rng), rand_pseudo(rng), rand_normal(rng), power):
            for st7 in (EMPTY, EMPTY, rand_f80(rng)):
                add(FXTRACT, st0=v, st7=st7, masks=rng.choice([0x3F, 0x3F, 0x3E, 0x3B, 0x3D, rng.getrandbits(6)]))
    # fxam: class x sign x tag
    for _ in range(3):
        for v in (ZERO, rand_denormal(rng), rand_pseudo_denormal(rng), rand_normal(rng), INF, rand_qnan(rng),
                  rand_snan(rng), rand_unnormal(rng), rand_pseudo(rng)):
            for s in (0, 0x8000):
                v = (v[0], (v[1] & 0x7FFF) | s)
                st = directed_state(rng, st0=v, keep=0)
                cases.append(dict(code=FXAM, mem="00" * 16, **st))
                st = directed_state(rng, st0=v, keep=0)   # the same contents in an empty register
                st["ftw"] |= 3 << (2 * ((st["fsw"] >> 11) & 7))
                cases.append(dict(code=FXAM, mem="00" * 16, **st))
    # the integer stores at their range ends: every RC, IM masked and unmasked
    for code in INT_STORES:
        own = {"df": 15, "db": 31}[code[:2]] if code not in ("df3e", "dd0e") else 63
        for v in int_store_operands(rng):
            e = (v[1] & 0x7FFF) - 0x3FFF
            end = own - 1 <= e <= own or e >= 63
            for rc in range(4):   # every RC at the form's own range end and beyond 2^63, one in four elsewhere
                if not end and rng.random() < 0.75:
                    continue      # (the random registers go to the others, so that no RC loses its range end)
                add(code, mem=bytes(rng.getrandbits(8) for _ in range(10)), st0=v, rc=rc,
                    masks=rng.choice([0x3F, 0x3F, 0x3E, 0x1F, 0x1E]), keep=0 if end else 0.3)
    # what else the single-form paths lean on: inf x 0, and states with an exception pending
    for code in ("d8c9", "dcc9", "dec9"):
        for _ in range(4):
            add(code, st0=sgn(rng, INF), st1=sgn(rng, ZERO), masks=rng.choice([0x3F, 0x3E]), keep=0)
            add(code, st0=sgn(rng, ZERO), st1=sgn(rng, INF), masks=rng.choice([0x3F, 0x3E]), keep=0)
    for code in (FSQRT, FRNDINT, FSCALE, FPREM, FPREM1, FXTRACT, FXAM, "df1e"):
        for _ in range(3):
            st = rand_state(rng, pending=True)
            st["fcw"] &= ~1
            st["fsw"] |= 0x8081    # IE set and unmasked: #MF
            cases.append(dict(code=code, mem="00" * 16, **st))
    return cases


def run_oracle(c, buf_va):
    """One case through the oracle: (status, vector, fcw, fsw, ftw, st, fl, mem)."""
    from tests.oracle_lib import Oracle
    from tests.insn_cases import layout
    sp, regs = layout(bytes.fromhex(c["code"]), buf_va, bytes.fromhex(c["mem"]).ljust(256, b"\0"))
    regs.gpr[6] = buf_va
    case_regs(c, regs)
    pfns, blob = sp.phys()
    o = Oracle(pfns=pfns, blob=blob)
    o.restore(regs)
    ex = o.step()
    r = o.regs()
    return dict(status=ex.status if ex.status != 3 else 0, vector=ex.vector if ex.status == 5 else 0,
                fcw=r.fpcw, fsw=r.fpsw, ftw=r.fptw, st=[(r.fpst[i], r.fpse[i]) for i in range(8)],
                fl=r.rflags & 0x8D5, mem=o.read_virt(buf_va, 16).hex())


def record(cases, path, mtime=None):
    """Run every case natively and write the file (mtime=0: the same bytes on every run)."""
    from tests.insn_cases import BUF
    doc = {"buf_va": hex(BUF), "cases": []}
    for c in cases:
        out = run_oracle(c, BUF)
        doc["cases"].append(dict(c, out=out))
    with gzip.GzipFile(path, "wb", mtime=mtime) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(len(doc["cases"]), "cases ->", path)


def main():
    import sys
    if sys.argv[1:] == ["directed"]:
        record(make_directed_cases(), DIRECTED_OUT, mtime=0)
    else:
        record(make_cases(), OUT)


if __name__ == "__main__":
    main()
