#!/usr/bin/env python3
"""Native-execution golden vectors for the AVX-512 integer forms of convention
U49 (wtf_amd/csrc/engine_avx512x.h): element-wise arithmetic (family A),
shifts and rotates (B), the in-lane shuffles (C), the cross-lane permutes (D)
the widening loads (E), the 128- / 256-bit block inserts, extracts and
broadcasts (F), the mask <-> vector moves (G) and vmovd / vmovq (H).

The machinery is gen_avx512_vectors.py's (the stub, the 512-byte window across
a page boundary, the guard pages, the recorded faults). What is added here:

* every case is named from the disassembly of its own bytes (objdump), and a
  form whose bytes do not disassemble to the mnemonic it was written for stops
  the generator, so a mis-encoded form cannot pass under another's name;
* deliberate inputs on top of case_inputs(seed), stored in the case ("zov":
  whole registers, "wov": window bytes) — shuffle and permute controls with
  their high bits (and vpshufb's bit 7) set, shift counts of 0, width - 1,
  width and beyond in the imm8, xmm and per-element forms, saturating and
  0x80.. operands for the packs, vpabs and the saturating adds, and the
  destination aliasing each source. Two of them are placed, not drawn: the
  first register and memory case of every vpabs form at every length has
  0x80..0 in a selected element (place_minimum), and the first four cases of
  every shift form at every length walk the counts 0, width - 1, width and
  width + 1 (walk_count);
* per family, guard cases (the operand across the page boundary with the next
  or the previous page absent, masks on both sides of it) and the #UD
  encodings: EVEX.b without a broadcast form, vvvv / V' on two-operand forms,
  z without a mask, a mask on vpslldq / vpsrldq, lengths a form does not have,
  W where a form fixes it, undefined /digits of the shift groups.

Output: tests/golden/avx512x_vectors.json.gz. Re-run with
    python tests/golden/gen_avx512x_vectors.py
"""
import gzip
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import gen_avx512_vectors as G  # noqa: E402
from tests.golden.gen_avx512_vectors import BOUND, RSP, WIN, evex, mk_case, pick_mem, run_native  # noqa: E402
from tests.golden.gen_native_vectors import rand_val  # noqa: E402

OUT = os.path.join(HERE, "avx512x_vectors.json.gz")
REPS = 8  # cases per form and legal length


# ---------------------------------------------------------------- the forms
def F(fam, nm, mp, pp, w, opc, shape, es, **ex):
    """shape: '3' dst = reg, vvvv, r/m; '2' dst = reg, r/m (vvvv unused);
    'g' a group form: dst = vvvv, r/m, ModRM.reg = ex['digit'].
    ex: bc broadcast element bytes; mdiv memory operand = VL / mdiv; m128;
    mfix memory operand bytes at every length; imm; minll / maxll; nomask;
    memonly / regonly; regk / rmk the operand is k0-7; rmg r/m is a GPR; sp
    the deliberate inputs; ses source element bytes; tag tells apart forms
    that share a mnemonic."""
    d = {"fam": fam, "nm": nm, "mp": mp, "pp": pp, "w": w, "opc": opc, "shape": shape, "es": es}
    d.update(ex)
    return d


def forms():
    L = []
    dq = ((0, 4, "d"), (1, 8, "q"))
    # ---- A: element-wise arithmetic
    L += [F("A", "vpminsb", 2, 1, None, 0x38, "3", 1), F("A", "vpmaxsb", 2, 1, None, 0x3C, "3", 1),
          F("A", "vpminsw", 1, 1, None, 0xEA, "3", 2), F("A", "vpmaxsw", 1, 1, None, 0xEE, "3", 2)]
    for w, es, s in dq:
        L += [F("A", "vpmins" + s, 2, 1, w, 0x39, "3", es, bc=es), F("A", "vpmaxs" + s, 2, 1, w, 0x3D, "3", es, bc=es),
              F("A", "vpminu" + s, 2, 1, w, 0x3B, "3", es, bc=es), F("A", "vpmaxu" + s, 2, 1, w, 0x3F, "3", es, bc=es),
              F("A", "vpmull" + s, 2, 1, w, 0x40, "3", es, bc=es),
              F("A", "vpabs" + s, 2, 1, w, 0x1E + w, "2", es, bc=es, sp="sat")]
    L += [F("A", "vpabsb", 2, 1, None, 0x1C, "2", 1, sp="sat"), F("A", "vpabsw", 2, 1, None, 0x1D, "2", 2, sp="sat")]
    for nm, opc, es in (("vpsubusb", 0xD8, 1), ("vpsubusw", 0xD9, 2), ("vpaddusb", 0xDC, 1), ("vpaddusw", 0xDD, 2),
                        ("vpsubsb", 0xE8, 1), ("vpsubsw", 0xE9, 2), ("vpaddsb", 0xEC, 1), ("vpaddsw", 0xED, 2)):
        L.append(F("A", nm, 1, 1, None, opc, "3", es, sp="sat"))
    L += [F("A", "vpavgb", 1, 1, None, 0xE0, "3", 1), F("A", "vpavgw", 1, 1, None, 0xE3, "3", 2),
          F("A", "vpmullw", 1, 1, None, 0xD5, "3", 2), F("A", "vpmulhw", 1, 1, None, 0xE5, "3", 2, sp="sat"),
          F("A", "vpmulhuw", 1, 1, None, 0xE4, "3", 2),
          F("A", "vpmuludq", 1, 1, 1, 0xF4, "3", 8, bc=8), F("A", "vpmuldq", 2, 1, 1, 0x28, "3", 8, bc=8)]
    # ---- B: shifts and rotates
    for nm, opc, digit in (("vpsrlw", 0x71, 2), ("vpsraw", 0x71, 4), ("vpsllw", 0x71, 6)):
        L.append(F("B", nm, 1, 1, None, opc, "g", 2, digit=digit, imm="cnt"))
    for nm, w, opc, digit in (("vpsrld", 0, 0x72, 2), ("vpsrad", 0, 0x72, 4), ("vpslld", 0, 0x72, 6),
                              ("vpsraq", 1, 0x72, 4), ("vpsrlq", 1, 0x73, 2), ("vpsllq", 1, 0x73, 6),
                              ("vprord", 0, 0x72, 0), ("vprorq", 1, 0x72, 0), ("vprold", 0, 0x72, 1),
                              ("vprolq", 1, 0x72, 1)):
        L.append(F("B", nm, 1, 1, w, opc, "g", 8 if w else 4, digit=digit, imm="cnt", bc=8 if w else 4))
    L += [F("B", "vpsrldq", 1, 1, None, 0x73, "g", 1, digit=3, imm="bcnt", nomask=1),
          F("B", "vpslldq", 1, 1, None, 0x73, "g", 1, digit=7, imm="bcnt", nomask=1)]
    for nm, w, opc, es in (("vpsrlw", None, 0xD1, 2), ("vpsrld", 0, 0xD2, 4), ("vpsrlq", 1, 0xD3, 8),
                           ("vpsraw", None, 0xE1, 2), ("vpsrad", 0, 0xE2, 4), ("vpsraq", 1, 0xE2, 8),
                           ("vpsllw", None, 0xF1, 2), ("vpslld", 0, 0xF2, 4), ("vpsllq", 1, 0xF3, 8)):
        L.append(F("B", nm, 1, 1, w, opc, "3", es, m128=1, sp="xcnt", tag="x"))
    L += [F("B", "vpsrlvw", 2, 1, 1, 0x10, "3", 2, sp="vcnt"), F("B", "vpsravw", 2, 1, 1, 0x11, "3", 2, sp="vcnt"),
          F("B", "vpsllvw", 2, 1, 1, 0x12, "3", 2, sp="vcnt")]
    for w, es, s in dq:
        L += [F("B", "vpsrlv" + s, 2, 1, w, 0x45, "3", es, bc=es, sp="vcnt"),
              F("B", "vpsrav" + s, 2, 1, w, 0x46, "3", es, bc=es, sp="vcnt"),
              F("B", "vpsllv" + s, 2, 1, w, 0x47, "3", es, bc=es, sp="vcnt"),
              F("B", "vprorv" + s, 2, 1, w, 0x14, "3", es, bc=es, sp="vcnt"),
              F("B", "vprolv" + s, 2, 1, w, 0x15, "3", es, bc=es, sp="vcnt")]
    # ---- C: shuffles within 128-bit lanes
    L += [F("C", "vpshufb", 2, 1, None, 0x00, "3", 1, sp="ctl"),
          F("C", "vpshufd", 1, 1, 0, 0x70, "2", 4, bc=4, imm="any"),
          F("C", "vpshufhw", 1, 2, None, 0x70, "2", 2, imm="any"), F("C", "vpshuflw", 1, 3, None, 0x70, "2", 2, imm="any")]
    for nm, w, opc, es in (("vpunpcklbw", None, 0x60, 1), ("vpunpcklwd", None, 0x61, 2), ("vpunpckldq", 0, 0x62, 4),
                           ("vpunpcklqdq", 1, 0x6C, 8), ("vpunpckhbw", None, 0x68, 1), ("vpunpckhwd", None, 0x69, 2),
                           ("vpunpckhdq", 0, 0x6A, 4), ("vpunpckhqdq", 1, 0x6D, 8)):
        L.append(F("C", nm, 1, 1, w, opc, "3", es, bc=es if es >= 4 else 0))
    L += [F("C", "vpacksswb", 1, 1, None, 0x63, "3", 1, sp="sat", ses=2),
          F("C", "vpackuswb", 1, 1, None, 0x67, "3", 1, sp="sat", ses=2),
          F("C", "vpackssdw", 1, 1, 0, 0x6B, "3", 2, bc=4, sp="sat", ses=4),
          F("C", "vpackusdw", 2, 1, 0, 0x2B, "3", 2, bc=4, sp="sat", ses=4),
          F("C", "vpalignr", 3, 1, None, 0x0F, "3", 1, imm="acnt")]
    # ---- D: permutes across lanes
    L += [F("D", "vpermd", 2, 1, 0, 0x36, "3", 4, bc=4, minll=1, sp="idxv"),
          F("D", "vpermq", 2, 1, 1, 0x36, "3", 8, bc=8, minll=1, sp="idxv", tag="v"),
          F("D", "vpermq", 3, 1, 1, 0x00, "2", 8, bc=8, minll=1, imm="any", tag="i"),
          F("D", "vpermb", 2, 1, 0, 0x8D, "3", 1, sp="idxv"), F("D", "vpermw", 2, 1, 1, 0x8D, "3", 2, sp="idxv"),
          F("D", "vpermi2b", 2, 1, 0, 0x75, "3", 1, sp="idxd"), F("D", "vpermi2w", 2, 1, 1, 0x75, "3", 2, sp="idxd"),
          F("D", "vpermi2d", 2, 1, 0, 0x76, "3", 4, bc=4, sp="idxd"),
          F("D", "vpermi2q", 2, 1, 1, 0x76, "3", 8, bc=8, sp="idxd"),
          F("D", "vpermt2b", 2, 1, 0, 0x7D, "3", 1, sp="idxv"), F("D", "vpermt2w", 2, 1, 1, 0x7D, "3", 2, sp="idxv"),
          F("D", "vpermt2d", 2, 1, 0, 0x7E, "3", 4, bc=4, sp="idxv"),
          F("D", "vpermt2q", 2, 1, 1, 0x7E, "3", 8, bc=8, sp="idxv"),
          F("D", "valignd", 3, 1, 0, 0x03, "3", 4, bc=4, imm="any"), F("D", "valignq", 3, 1, 1, 0x03, "3", 8, bc=8, imm="any"),
          F("D", "vshufi32x4", 3, 1, 0, 0x43, "3", 4, bc=4, minll=1, imm="any"),
          F("D", "vshufi64x2", 3, 1, 1, 0x43, "3", 8, bc=8, minll=1, imm="any")]
    # ---- E: widening loads
    for t, (sfx, des, ses) in enumerate((("bw", 2, 1), ("bd", 4, 1), ("bq", 8, 1), ("wd", 4, 2), ("wq", 8, 2),
                                         ("dq", 8, 4))):
        for sgn, base in (("s", 0x20), ("z", 0x30)):
            L.append(F("E", f"vpmov{sgn}x{sfx}", 2, 1, 0 if sfx == "dq" else None, base + t, "2", des, ses=ses,
                       mdiv=des // ses, sp="sat"))
    # ---- F: 128- and 256-bit blocks
    for nm, w, es, blk, minll in (("32x4", 0, 4, 16, 1), ("64x2", 1, 8, 16, 1), ("32x8", 0, 4, 32, 2),
                                  ("64x4", 1, 8, 32, 2)):
        L += [F("F", "vinserti" + nm, 3, 1, w, 0x38 if blk == 16 else 0x3A, "3", es, mfix=blk, minll=minll, imm="any"),
              F("F", "vextracti" + nm, 3, 1, w, 0x39 if blk == 16 else 0x3B, "2", es, mfix=blk, minll=minll, imm="any",
                ext=1),
              F("F", "vbroadcasti" + nm, 2, 1, w, 0x5A if blk == 16 else 0x5B, "2", es, mfix=blk, minll=minll,
                memonly=1)]
    L.append(F("F", "vbroadcasti32x2", 2, 1, 0, 0x59, "2", 4, mfix=8))
    # ---- G: mask <-> vector
    for s, opc, w, es in (("b", 0x28, 0, 1), ("w", 0x28, 1, 2), ("d", 0x38, 0, 4), ("q", 0x38, 1, 8)):
        L += [F("G", "vpmovm2" + s, 2, 2, w, opc, "2", es, nomask=1, regonly=1, rmk=1),
              F("G", f"vpmov{s}2m", 2, 2, w, opc + 1, "2", es, nomask=1, regonly=1, regk=1, sp="sat")]
    # ---- H: vmovd / vmovq
    L += [F("H", "vmovd", 1, 1, 0, 0x6E, "2", 4, mfix=4, maxll=0, nomask=1, rmg=1, tag="l"),
          F("H", "vmovq", 1, 1, 1, 0x6E, "2", 8, mfix=8, maxll=0, nomask=1, rmg=1, tag="l"),
          F("H", "vmovd", 1, 1, 0, 0x7E, "2", 4, mfix=4, maxll=0, nomask=1, rmg=1, tag="s"),
          F("H", "vmovq", 1, 1, 1, 0x7E, "2", 8, mfix=8, maxll=0, nomask=1, rmg=1, tag="s"),
          F("H", "vmovq", 1, 2, 1, 0x7E, "2", 8, mfix=8, maxll=0, nomask=1, tag="xl"),
          F("H", "vmovq", 1, 1, 1, 0xD6, "2", 8, mfix=8, maxll=0, nomask=1, tag="xs")]
    return L


def msize(f, vlb):
    if "mfix" in f:
        return f["mfix"]
    return 16 if f.get("m128") else vlb // f.get("mdiv", 1)


def lengths(f):
    return range(f.get("minll", 0), f.get("maxll", 2) + 1)


def pick_regs(rng, f):
    """(reg, vvvv, r/m register): k0-7 and the GPRs where the form has them (rsp is never a destination)."""
    reg = rng.randrange(8) if f.get("regk") else rng.randrange(32)
    rm = rng.randrange(8) if f.get("rmk") else rng.choice([r for r in range(16) if r != RSP]) if f.get("rmg") \
        else rng.randrange(32)
    return reg, rng.randrange(32), rm


# ---------------------------------------------------------------- deliberate inputs
SATQ = (0x8000800080008000, 0x7FFF7FFF7FFF7FFF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0x80000000_80000000,
        0x7FFFFFFF_7FFFFFFF, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0, 0x00FF00FF00FF00FF, 0x0080008000800080,
        0x0000FFFF_00008000, 0xFFFF7FFF_FFFF8000, 0x00010000_FFFEFFFF)


def shift_count(rng, bits):
    return rng.choice((0, 1, bits - 1, bits, bits + 1, rng.randrange(bits), rng.randrange(256), 0xFF))


def walk_count(bits, k):
    """The four counts every shift form must meet: 0, width - 1, width, beyond the width."""
    return (0, bits - 1, bits, bits + 1)[k % 4]


def special_vec(rng, f, what, step=None):
    """64 bytes for an operand in role `what`. step: the case's place in its
    form's walk over the four named shift counts (None: past the walk)."""
    es = f["es"]
    if what == "rand":
        return rng.getrandbits(512).to_bytes(64, "little")
    if what == "sat":
        return b"".join((rng.choice(SATQ) if rng.random() < 0.7 else rng.getrandbits(64)).to_bytes(8, "little")
                        for _ in range(8))
    if what == "xcnt":  # the count is the low qword of the xmm operand
        c = rng.choice((shift_count(rng, es * 8), shift_count(rng, es * 8), 1 << 32, (1 << 63) | 3, 1 << 8))
        if step is not None:
            c = walk_count(es * 8, step)
        return c.to_bytes(8, "little") + rng.getrandbits(448).to_bytes(56, "little")
    if what == "vcnt":
        out = b""
        for j in range(64 // es):
            c = shift_count(rng, es * 8) if rng.random() < 0.8 else rng.getrandbits(es * 8)
            if step is not None:  # neighbouring elements take the four counts in turn
                c = walk_count(es * 8, step + j)
            out += (c & ((1 << (es * 8)) - 1)).to_bytes(es, "little")
        return out
    raise ValueError(what)


def q8(bs):
    return [int.from_bytes(bs[8 * i: 8 * i + 8], "little") for i in range(8)]


OV = {}  # seed -> (zov {reg: [8 u64]}, wov [(off, bytes)])
_base_case_inputs = G.case_inputs


def case_inputs_ov(seed):
    """case_inputs plus the case's deliberate inputs (run_native looks the case up by its seed)."""
    zmm, win = _base_case_inputs(seed)
    zov, wov = OV.get(seed, ({}, []))
    zmm = [list(v) for v in zmm]
    for r, v in zov.items():
        zmm[r] = list(v)
    win = bytearray(win)
    for off, bs in wov:
        win[off: off + len(bs)] = bs
    return zmm, bytes(win)


def imm_of(rng, f, step=None):
    k = f.get("imm")
    if k is None:
        return None
    if k == "any":
        return rng.randrange(256)
    if k == "cnt":
        return shift_count(rng, f["es"] * 8) if step is None else walk_count(f["es"] * 8, step)
    if k == "bcnt":
        return rng.choice((0, 1, 7, 8, 15, 16, 17, rng.randrange(16), rng.randrange(256)))
    if k == "acnt":
        return rng.choice((0, 1, 15, 16, 17, 31, 32, 33, rng.randrange(32), rng.randrange(256)))
    raise ValueError(k)


def encode(f, w, ll, z, b, aaa, reg, vvvv, rm=None, mem=None, imm=None):
    if f["shape"] == "g":   # destination in vvvv, /digit in ModRM.reg
        return evex(f["mp"], f["pp"], w, ll, z, b, aaa, f["digit"], reg, f["opc"], rm=rm, mem=mem, imm=imm)
    if f["shape"] == "2":
        vvvv = 0
    return evex(f["mp"], f["pp"], w, ll, z, b, aaa, reg, vvvv, f["opc"], rm=rm, mem=mem, imm=imm)


def gen_form_cases(rng):
    cases = []
    for f in forms():
        es = f["es"]
        for ll in lengths(f):
            vlb = 16 << ll
            for i in range(REPS):
                # the first four cases of a shift form at each length walk the named counts; the
                # lengths start the walk at different counts, so register and memory forms meet all four
                step = i + ll if i < 4 else None
                w = f["w"] if f["w"] is not None else rng.randrange(2)
                mem = (i % 2 == 1 or bool(f.get("memonly"))) and not f.get("regonly")
                aaa = 0 if (f.get("nomask") or rng.random() < 0.25) else rng.randrange(1, 8)
                z = 1 if aaa and rng.random() < 0.4 and not (f.get("ext") and mem) else 0
                b = 1 if mem and f.get("bc") and rng.random() < 0.45 else 0
                reg, vvvv, rm = pick_regs(rng, f)
                x = rng.random() if not (f.get("regk") or f.get("rmk") or f.get("rmg")) else 1.0
                if x < 0.1:  # the destination aliasing each source
                    vvvv = reg
                elif x < 0.2:
                    rm = reg
                elif x < 0.25:
                    vvvv = rm = reg
                imm = imm_of(rng, f, step)
                regs = [rand_val(rng) for _ in range(16)]
                ptrs, smalls = {RSP: 0x80}, {}
                zov, wov = {}, []
                sp = f.get("sp")
                # the first source / the index registers
                if sp == "sat" and f["shape"] == "3":
                    zov[vvvv] = q8(special_vec(rng, f, "sat"))
                if sp == "idxv":
                    zov[vvvv] = q8(special_vec(rng, f, "rand"))
                if sp == "idxd":
                    zov[reg] = q8(special_vec(rng, f, "rand"))
                rmv = special_vec(rng, f, {"sat": "sat", "xcnt": "xcnt", "vcnt": "vcnt", "ctl": "rand"}[sp], step) \
                    if sp in ("sat", "xcnt", "vcnt", "ctl") else None
                if mem:
                    osz = f["bc"] if b else msize(f, vlb)
                    toff = rng.randrange(0, WIN - osz + 1)
                    m = pick_mem(rng, regs, ptrs, smalls, toff, osz)
                    if rmv is not None:
                        if b and sp == "vcnt":
                            cnt = shift_count(rng, es * 8) if step is None else walk_count(es * 8, step)
                            rmv = cnt.to_bytes(es, "little")
                        wov.append((toff, rmv[:osz]))
                    code = encode(f, w, ll, z, b, aaa, reg, vvvv, mem=m, imm=imm)
                else:
                    if rmv is not None:
                        zov[rm] = q8(rmv)
                    code = encode(f, w, ll, z, 0, aaa, reg, vvvv, rm=rm, imm=imm)
                c = mk_case(rng, f"{f['nm']}.L{ll}.{'m' if mem else 'r'}", code, regs, ptrs, smalls, 0)
                c["want"] = f["nm"]
                if f["nm"].startswith("vpabs") and i < 2:
                    place_minimum(c, f, vlb, aaa, b, rm if not mem else None, zov, wov)
                OV[c["seed"]] = (zov, wov)
                cases.append(c)
    return cases


def place_minimum(c, f, vlb, aaa, b, rm, zov, wov):
    """vpabs's boundary operand, 0x80..0, in the highest element the case's
    mask selects (the mask gets bit 0 if it selects none): the first register
    case and the first memory case of every vpabs form at every length."""
    es = f["es"]
    n = vlb // es
    if aaa and not c["k"][aaa] & ((1 << n) - 1):
        c["k"][aaa] |= 1
    sel = c["k"][aaa] & ((1 << n) - 1) if aaa else (1 << n) - 1
    j = 0 if b else sel.bit_length() - 1
    minv = (1 << (8 * es - 1)).to_bytes(es, "little")
    if rm is None:
        off, bs = wov[-1]
        wov[-1] = (off, bs[:j * es] + minv + bs[(j + 1) * es:])
    else:
        bs = b"".join(v.to_bytes(8, "little") for v in zov[rm])
        zov[rm] = q8(bs[:j * es] + minv + bs[(j + 1) * es:])


def gen_guard_cases(rng):
    """The memory operand across the page boundary, the next page (guard 1) or
    the previous one (guard 2) absent; masks on both sides of the boundary."""
    cases = []
    pick = {"A": ("vpminsd", "vpaddsb", "vpabsw", "vpmuludq"), "B": ("vpsrld", "vpsraq", "vpsllvw", "vpslldq", "vpsrlw"),
            "C": ("vpshufb", "vpshufd", "vpunpcklbw", "vpackssdw", "vpalignr"),
            "D": ("vpermd", "vpermi2b", "vpermt2q", "valignd", "vshufi64x2", "vpermq"),
            "E": ("vpmovzxbw", "vpmovsxbq", "vpmovzxwd", "vpmovsxdq"),
            "F": ("vinserti32x4", "vinserti64x4", "vextracti32x4", "vextracti64x2", "vextracti32x8", "vbroadcasti32x2",
                  "vbroadcasti64x2", "vbroadcasti32x8"),
            "G": (), "H": ("vmovd", "vmovq")}
    for f in forms():
        if f["nm"] not in pick[f["fam"]]:
            continue
        es = f["es"]
        for ll in sorted({min(max(f.get("minll", 0), 1), f.get("maxll", 2)), f.get("maxll", 2)}):
            vlb = 16 << ll
            osz = msize(f, vlb)
            n = osz // es if "mfix" in f else vlb // es
            sesz = osz // n if not f.get("m128") else 8   # bytes of the operand per destination element
            for shift in ((0, 1) if ll == 2 or "mfix" in f else (0,)):
                toff = BOUND - osz // 2 - (shift if sesz > 1 else 0)
                first_out = (BOUND - toff + sesz - 1) // sesz if not f.get("m128") else n // 2
                first_out = min(first_out, n - 1)
                full = (1 << n) - 1
                masks = [(0, 0), (full, 5), ((full >> first_out) << first_out, 5), ((1 << first_out) - 1, 5), (0, 5),
                         ((1 << max(first_out - 1, 0)) | 1, 5)]
                nf = f["fam"] in "CD" or f.get("m128") or f["nm"].startswith("vinserti")
                if nf:
                    masks = [(0, 0), (full, 5), (0, 5)]  # no fault suppression: every mask faults alike
                if f.get("nomask"):
                    masks = [(0, 0)]
                for guard in (1, 2):
                    for kv, aaa in masks:
                        w = f["w"] if f["w"] is not None else 0
                        z = 1 if aaa and rng.random() < 0.4 else 0
                        if f.get("ext"):
                            z = 0
                        code = encode(f, w, ll, z, 0, aaa, pick_regs(rng, f)[0], rng.randrange(32),
                                      mem=(0, None, 0, 0, 4), imm=imm_of(rng, f))
                        regs = [rand_val(rng) for _ in range(16)]
                        c = mk_case(rng, f"{f['nm']}.L{ll}.m.guard", code, regs, {RSP: 0x80, 0: toff}, {}, guard)
                        c["want"] = f["nm"]
                        if aaa:
                            c["k"][aaa] = kv
                        cases.append(c)
                    if f.get("bc") and not shift:  # the broadcast element on the present / the absent page
                        for toff_b in (BOUND - f["bc"], BOUND - f["bc"] // 2):
                            for kv in ((0,) if nf else (full, 0)):
                                w = f["w"] if f["w"] is not None else 0
                                code = encode(f, w, ll, 0, 1, 5, rng.randrange(32), rng.randrange(32),
                                              mem=(0, None, 0, 0, 4), imm=imm_of(rng, f))
                                regs = [rand_val(rng) for _ in range(16)]
                                c = mk_case(rng, f"{f['nm']}.L{ll}.m.guard", code, regs, {RSP: 0x80, 0: toff_b}, {},
                                            guard)
                                c["want"] = f["nm"]
                                c["k"][5] = kv
                                cases.append(c)
    return cases


def gen_ud_cases(rng):
    """(family, rule, form, bytes): encodings whose native outcome is recorded
    (#UD for all of them on the generating host)."""
    out = []
    byname = {}
    for f in forms():
        byname.setdefault(f["nm"] + f.get("tag", ""), f)
    M0 = (0, None, 0, 0, 1)

    def add(rule, key, **kw):
        f = byname[key]
        reg, vvvv, rm = pick_regs(rng, f)
        a = {"w": f["w"] if f["w"] is not None else 0, "ll": f.get("maxll", 2), "z": 0, "b": 0, "aaa": 0, "reg": reg,
             "vvvv": vvvv, "rm": rm, "mem": None if not f.get("memonly") else M0, "imm": imm_of(rng, f)}
        a.update(kw)
        if a["mem"] is not None:
            a["rm"] = None
        if a["w"] is None:
            return  # the other W is another instruction
        if "vvvv_raw" in a:  # a two-operand form with vvvv set
            code = evex(f["mp"], f["pp"], a["w"], a["ll"], 0, 0, 0, a["reg"], a["vvvv_raw"], f["opc"], rm=a["rm"],
                        mem=a["mem"], imm=a["imm"])
        else:
            code = encode(f, a["w"], a["ll"], a["z"], a["b"], a["aaa"], a["reg"], a["vvvv"], rm=a["rm"],
                          mem=a["mem"], imm=a["imm"])
        out.append((f["fam"], rule, code))

    for _ in range(1):
        # EVEX.b: a register form, and a memory form without broadcast
        for key in ("vpminsd", "vpsrld", "vpshufd", "vpermd", "vpmovzxbw", "vpsllvq", "vpunpckldq", "valignd"):
            add("b_reg", key, b=1)
        for key in ("vpminsb", "vpaddsw", "vpsrlw", "vpsllvw", "vpshufb", "vpshufhw", "vpalignr", "vpermb", "vpermi2w",
                    "vpmovzxbw", "vpmovsxdq", "vpsrldq", "vpsrldx", "vpunpcklbw", "vpacksswb"):
            add("b_nobcast", key, b=1, mem=M0)
        # z without a mask
        for key in ("vpmaxud", "vpsraq", "vpshufb", "vpermt2d", "vpmovsxwd"):
            add("z_nomask", key, z=1)
        # vvvv != 1111 and V' on the two-operand forms
        for key in ("vpabsd", "vpshufd", "vpshuflw", "vpermqi", "vpmovzxbd", "vpmovsxwq"):
            f = byname[key]
            for vv in (rng.randrange(1, 16), 16):
                code = evex(f["mp"], f["pp"], f["w"] or 0, 2, 0, 0, 0, rng.randrange(32), vv, f["opc"],
                            rm=rng.randrange(32), imm=imm_of(rng, f))
                out.append((f["fam"], "vvvv_two" if vv < 16 else "vprime_two", code))
        # a mask on vpslldq / vpsrldq
        for key in ("vpslldq", "vpsrldq"):
            add("mask_bshift", key, aaa=rng.randrange(1, 8))
            add("mask_bshift", key, aaa=rng.randrange(1, 8), z=1)
        # lengths a form does not have
        for key in ("vpermd", "vpermqv", "vpermqi", "vshufi32x4", "vshufi64x2"):
            add("len128", key, ll=0)
        for key in ("vpminsd", "vpshufb", "vpsrld", "vpermb", "vpmovzxbw"):
            add("ll3", key, ll=3)
        # W where a form fixes it
        for key in ("vpabsd", "vpabsq", "vpmuludq", "vpmuldq", "vpshufd", "vpunpckldq", "vpunpcklqdq", "vpackssdw",
                    "vpackusdw", "vpsrld", "vpsrlq", "vpslld", "vpsllq", "vpsrldx", "vpsrlqx", "vpslldx", "vpsllqx",
                    "vpsrlvw", "vpsravw", "vpsllvw", "vpermqi", "vpmovsxdq", "vpmovzxdq"):
            f = byname[key]
            add("w_fixed", key, w=f["w"] ^ 1)
        # the block, mask and GPR moves
        for key in ("vinserti32x4", "vinserti64x2", "vextracti32x4", "vextracti64x2", "vbroadcasti32x4",
                    "vbroadcasti64x2"):
            add("len128", key, ll=0)
        for key in ("vinserti32x8", "vinserti64x4", "vextracti32x8", "vextracti64x4", "vbroadcasti32x8",
                    "vbroadcasti64x4"):
            add("len_not512", key, ll=1)
            add("len_not512", key, ll=0)
        for key in ("vinserti32x4", "vextracti64x4", "vbroadcasti32x2", "vbroadcasti64x2", "vmovdl", "vmovqxl"):
            add("b_nobcast", key, b=1, mem=M0)
        for key in ("vbroadcasti32x4", "vbroadcasti64x2", "vbroadcasti32x8", "vbroadcasti64x4"):
            add("reg_memonly", key, mem=None)
        for key in ("vextracti32x4", "vextracti64x4"):
            add("z_store", key, z=1, aaa=3, mem=M0)
        for key in ("vextracti32x4", "vbroadcasti32x2", "vpmovm2b", "vpmovd2m", "vmovdl", "vmovqs", "vmovqxl", "vmovqxs"):
            add("vvvv_two", key, vvvv_raw=rng.randrange(1, 16))
        for key in ("vpmovm2b", "vpmovm2q", "vpmovb2m", "vpmovw2m", "vpmovd2m", "vpmovq2m", "vmovdl", "vmovqs",
                    "vmovqxl", "vmovqxs"):
            add("mask_nomask", key, aaa=rng.randrange(1, 8))
        for key in ("vpmovm2w", "vpmovq2m"):
            add("mem_regonly", key, mem=M0)
        for key in ("vmovdl", "vmovds", "vmovql", "vmovqs", "vmovqxl", "vmovqxs"):
            add("len_not128", key, ll=1)
            add("len_not128", key, ll=2)
        for key in ("vmovqxl", "vmovqxs", "vbroadcasti32x2"):
            add("w_fixed", key, w=0 if key != "vbroadcasti32x2" else None)
        # undefined /digits of the shift groups
        for opc, digits in ((0x71, (0, 1, 3, 5, 7)), (0x72, (3, 5, 7)), (0x73, (0, 1, 4, 5))):
            for d in digits:
                for w in (0, 1):
                    code = evex(1, 1, w, 2, 0, 0, 0, d, rng.randrange(32), opc, rm=rng.randrange(32), imm=3)
                    out.append(("B", "digit", code))
    return out


# ---------------------------------------------------------------- names from the disassembly
def disassemble(codes):
    """The mnemonic objdump gives each byte string ('(bad)' when it decodes to none)."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "c.bin")
        with open(path, "wb") as fh:
            for c in codes:
                assert len(c) <= 15
                fh.write(c + b"\x90" * (32 - len(c)))
        txt = subprocess.run(["objdump", "-D", "-b", "binary", "-m", "i386:x86-64", "-M", "intel", "--insn-width=16", path],
                             capture_output=True, text=True, check=True).stdout
    at = {}
    for line in txt.split("\n"):
        m = re.match(r"\s*([0-9a-f]+):\t([0-9a-f ]+)\t(\S+)", line)
        if m:
            at[int(m.group(1), 16)] = (m.group(3), len(m.group(2).split()))
    out = []
    for i, c in enumerate(codes):
        mn, ln = at.get(32 * i, ("(bad)", 0))
        out.append(mn if ln == len(c) or mn == "(bad)" else "(bad)")
    return out


def main():
    rng = random.Random(0xA5129)
    cases = gen_form_cases(rng) + gen_guard_cases(rng)
    uds = gen_ud_cases(rng)
    names = disassemble([bytes.fromhex(c["code"]) for c in cases])
    for c, mn in zip(cases, names):
        want = c.pop("want")
        assert mn == want, (want, mn, c["code"])
        c["name"] = mn + c["name"][len(want):]
    udn = disassemble([bytes(code) for _, _, code in uds])
    for (fam, rule, code), mn in zip(uds, udn):
        regs = [rand_val(rng) for _ in range(16)]
        cases.append(mk_case(rng, f"ud.{fam}.{rule}.{mn}", code, regs, {RSP: 0x80, 0: 0x40}, {}, 0))
    G.case_inputs = case_inputs_ov   # run_native and window_of take a case's inputs from its seed
    try:
        run_native(cases, OUT)
    finally:
        G.case_inputs = _base_case_inputs
    with gzip.open(OUT, "rt") as fh:
        doc = json.load(fh)
    doc["generator"] = "tests/golden/gen_avx512x_vectors.py"
    for e, c in zip(doc["cases"], cases):
        zov, wov = OV.get(c["seed"], ({}, []))
        if zov:
            e["zov"] = [[r, ["%x" % v for v in q]] for r, q in sorted(zov.items())]
        if wov:
            e["wov"] = [[off, bs.hex()] for off, bs in wov]
    with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, separators=(",", ":")).encode())
    nud = sum(c.get("fault", {}).get("vec") == 6 for c in doc["cases"])
    print(f"{len(doc['cases'])} cases, {nud} #UD, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
