"""The AVX-512 integer forms of convention U49 (engine_avx512x.h): element-wise
arithmetic, shifts and rotates, in-lane shuffles, cross-lane permutes, the
widening loads, the 128- / 256-bit block moves, mask <-> vector and vmovd / q.

Native-execution vectors (tests/golden/gen_avx512x_vectors.py) pin both sides:
the oracle's restatement (oracle/x86_oracle_avx512x.inc) and the engine's
device code built for the host, generic and through the fast-loop digest, each
judged by the same check() on every case; the recorded routines
(gen_avx512x_programs.py) run on both to their int3. With the oracle pinned
here, the random programs' EVEX pool (tests/progfuzz.py) may compare the engine
with it. The GPU runs the same vectors in tests/test_gpu_avx512x.py.
"""
import pytest

from tests import simlane
from tests.avx512x_programs import PROGS, program_case, program_check, program_space
from tests.golden.gen_avx512x_vectors import forms, lengths
from tests.insn_cases import CODE_VA, get_zmm, oracle_of
from tests.vector_replay import AVX512X, replay_oracle, replay_sim, run_family
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, EXIT_UNIMPLEMENTED, regs_from_state
from wtf_amd.tools.snapshot import AddressSpace, user_state

DOC = AVX512X.doc
inputs = AVX512X.inputs
FAMILY = {f["nm"]: f["fam"] for f in forms()}


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_native_avx512x(chunk):
    """Every case of the vector file through the oracle, judged by the same
    check() as the engine's host build: GPRs, RFLAGS, zmm0-31, k0-7, the
    window, and for the guard and ud.* cases the fault's vector, error code
    and address."""
    assert len(DOC["cases"]) == 4453
    cases = DOC["cases"][chunk::2]
    fails = run_family(AVX512X, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


@pytest.mark.parametrize("fast", [False, True], ids=["exec", "fast"])
def test_engine_avx512x_code_matches_native_vectors(fast):
    """The engine's decode / exec built for the host (tests/native/sim_lane.cc);
    fast=True goes through k_run's fast-loop digest first (EVEX stays generic)."""
    fails = run_family(AVX512X, replay_sim, DOC["cases"], fast=fast)
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:5]}"


# Every mnemonic of the families that shipped, named here and
# not taken from the generator: the names in the file come from the
# disassembly of each case's own bytes.
MNEMONICS = {
    "A": "vpminsb vpminsw vpminsd vpminsq vpmaxsb vpmaxsw vpmaxsd vpmaxsq vpminud vpminuq vpmaxud vpmaxuq "
         "vpabsb vpabsw vpabsd vpabsq vpaddsb vpaddsw vpaddusb vpaddusw vpsubsb vpsubsw vpsubusb vpsubusw "
         "vpavgb vpavgw vpmullw vpmulhw vpmulhuw vpmulld vpmullq vpmuludq vpmuldq",
    "B": "vpsrlw vpsrld vpsrlq vpsraw vpsrad vpsraq vpsllw vpslld vpsllq vprold vprolq vprord vprorq "
         "vpsllvw vpsllvd vpsllvq vpsrlvw vpsrlvd vpsrlvq vpsravw vpsravd vpsravq vprolvd vprolvq vprorvd vprorvq "
         "vpslldq vpsrldq",
    "C": "vpshufb vpshufd vpshufhw vpshuflw vpunpcklbw vpunpcklwd vpunpckldq vpunpcklqdq vpunpckhbw vpunpckhwd "
         "vpunpckhdq vpunpckhqdq vpacksswb vpackuswb vpackssdw vpackusdw vpalignr",
    "D": "vpermd vpermq vpermw vpermb vpermi2b vpermi2w vpermi2d vpermi2q vpermt2b vpermt2w vpermt2d vpermt2q "
         "valignd valignq vshufi32x4 vshufi64x2",
    "E": "vpmovzxbw vpmovzxbd vpmovzxbq vpmovzxwd vpmovzxwq vpmovzxdq vpmovsxbw vpmovsxbd vpmovsxbq vpmovsxwd "
         "vpmovsxwq vpmovsxdq",
    "F": "vinserti32x4 vinserti64x2 vinserti32x8 vinserti64x4 vextracti32x4 vextracti64x2 vextracti32x8 "
         "vextracti64x4 vbroadcasti32x2 vbroadcasti32x4 vbroadcasti64x2 vbroadcasti32x8 vbroadcasti64x4",
    "G": "vpmovm2b vpmovm2w vpmovm2d vpmovm2q vpmovb2m vpmovw2m vpmovd2m vpmovq2m",
    "H": "vmovd vmovq",
}


def fields(c):
    """The EVEX fields of a case's code: (map, pp, W, L'L, z, b, aaa, reg, vvvv, opcode, mod, r/m register, imm8)."""
    x = bytes.fromhex(c["code"])
    assert x[0] == 0x62
    p0, p1, p2, opc, modrm = x[1:6]
    reg = ((modrm >> 3) & 7) | (((~p0 >> 7) & 1) << 3) | (((~p0 >> 4) & 1) << 4)
    rm = (modrm & 7) | (((~p0 >> 5) & 1) << 3) | (((~p0 >> 6) & 1) << 4)
    vvvv = ((~p1 >> 3) & 15) | (((~p2 >> 3) & 1) << 4)
    return {"map": p0 & 7, "pp": p1 & 3, "w": p1 >> 7, "ll": (p2 >> 5) & 3, "z": p2 >> 7, "b": (p2 >> 4) & 1,
            "aaa": p2 & 7, "reg": reg, "vvvv": vvvv, "opc": opc, "mod": modrm >> 6, "rm": rm, "imm": x[-1]}


def rm_operand(c, e, nbytes):
    """The first nbytes of a case's r/m operand: the register's, or the memory
    operand's as the generator placed them (wov; an embedded broadcast repeated)."""
    if e["mod"] == 3:
        zin, _ = inputs(c)
        return b"".join(v.to_bytes(8, "little") for v in zin[8 * e["rm"]: 8 * e["rm"] + 8])[:nbytes]
    bs = bytes.fromhex(c["wov"][-1][1])
    return (bs * (nbytes // len(bs)) if e["b"] else bs)[:nbytes]


def test_avx512x_vector_file_is_substantial():
    cases = DOC["cases"]
    assert 2500 < len(cases) <= 6000
    ok = [c for c in cases if not c["name"].startswith("ud.")]
    # the mnemonics objdump gave the cases are exactly the shipped ones, and the generator's table names the same
    for fam, names in MNEMONICS.items():
        assert {c["name"].split(".")[0] for c in ok if FAMILY.get(c["name"].split(".")[0]) == fam} == set(names.split())
    assert {c["name"].split(".")[0] for c in ok} == {n for v in MNEMONICS.values() for n in v.split()} == set(FAMILY)
    # every mnemonic of the families that shipped, at every length it has, at least 8 cases each,
    # from registers and from memory
    per = {}
    for c in ok:
        if c["name"].endswith(".guard"):
            continue
        nm, ll, rm = c["name"].split(".")[:3]
        per.setdefault((nm, ll), []).append(rm)
    for f in forms():
        for ll in lengths(f):
            got = per.get((f["nm"], f"L{ll}"), [])
            assert len(got) >= 8, (f["nm"], ll, got)
            assert f.get("memonly") or "r" in got, (f["nm"], ll, got)
            assert f.get("regonly") or "m" in got, (f["nm"], ll, got)
    assert {FAMILY[c["name"].split(".")[0]] for c in ok} == set("ABCDEFGH")
    # masks: about three quarters masked, a good part of those zeroing
    masked = [c for c in ok if int(c["code"][6:8], 16) & 7]
    maskable = [c for c in ok if FAMILY[c["name"].split(".")[0]] not in "GH" and "dq." not in c["name"]]
    assert 0.6 < len(masked) / len(maskable) < 0.9
    assert 0.25 < sum(int(c["code"][6:8], 16) >> 7 for c in masked) / len(masked) < 0.55
    # broadcasts were met
    assert sum((int(c["code"][6:8], 16) >> 4) & 1 for c in ok if "fault" not in c) > 150
    for fam in "ABCDEFGH":
        # memory fault suppression both ways: guard cases that fault and guard cases that complete
        # (G has no memory forms)
        guard = [c for c in ok if c["guard"] and FAMILY[c["name"].split(".")[0]] == fam]
        assert fam == "G" or sum("fault" in c for c in guard) >= 8, fam
        if fam in "AEF":  # the shuffles and permutes read their whole operand: every guard case of C / D faults
            assert sum("fault" not in c for c in guard) >= 10, fam
        # the #UD rules were met natively
        ud = [c for c in cases if c["name"].startswith(f"ud.{fam}.")]
        assert len(ud) >= 8 and all(c.get("fault", {}).get("vec") == 6 for c in ud), fam
    rules = {c["name"].split(".")[2] for c in cases if c["name"].startswith("ud.")}
    assert rules >= {"b_reg", "b_nobcast", "z_nomask", "vvvv_two", "vprime_two", "mask_bshift", "len128", "ll3",
                     "w_fixed", "digit", "len_not512", "len_not128", "reg_memonly", "mem_regonly", "z_store",
                     "mask_nomask"}
    # deliberate inputs travel with the cases
    assert sum("zov" in c or "wov" in c for c in ok) > 500


# One representative of everything that stays outside: each is
# a defined EVEX encoding, so it ends the testcase as UNIMPLEMENTED, not #UD.
STILL_OUTSIDE = {
    "vaddps zmm": "62f17c4858c1",
    "vpmovwb ymm, zmm": "62f27e4830c1",
    "vpmovdb xmm, zmm": "62f27e4831c1",
    "vpcompressd zmm{k1}, zmm": "62f27d498bc1",
    "vpexpandd zmm{k1}, zmm": "62f27d4989c1",
    "vpgatherdd zmm{k1}, [rax+zmm1*4]": "62f27d49900488",
    "vpscatterdd [rax+zmm1*4]{k1}, zmm0": "62f27d49a00488",
    "vpconflictd zmm": "62f27d48c4c1",
    "vplzcntd zmm": "62f27d4844c1",
    "vpmaddwd zmm": "62f17548f5c2",
    "vpsadbw zmm": "62f17548f6c2",
    "vpmaddubsw zmm": "62f2754804c2",
    "vpextrd eax, xmm1, 1": "62f37d0816c801",
    "vpinsrd xmm0, xmm1, eax, 1": "62f3750822c001",
    "vpmadd52luq zmm": "62f2f548b4c2",
    "vpdpbusd zmm": "62f2754850c2",
    "vpopcntb zmm": "62f27d4854c1",
    "vpopcntd zmm": "62f27d4855c1",
    "vaddph zmm": "62f57c4858c1",
}


@pytest.mark.parametrize("name", sorted(STILL_OUTSIDE))
def test_evex_forms_outside_the_subset_stay_unimplemented(name):
    c = next(c for c in DOC["cases"] if c["guard"] == 0 and "fault" not in c)
    buf_va = AVX512X.buf_va
    regs = regs_from_state(user_state(CODE_VA, 0, AddressSpace().cr3))
    AVX512X.init(regs)
    win = AVX512X.setup(c, regs)
    zin = get_zmm(regs)
    sp = AVX512X.space(bytes.fromhex(STILL_OUTSIDE[name]) + b"\xcc", CODE_VA, win, 0)
    regs.gpr[0] = buf_va
    regs.k[1] = 1
    for fast in (False, True):
        out, _, _ = simlane.run(sp, regs, fast=fast, win_va=buf_va)
        assert out.status == EXIT_UNIMPLEMENTED and out.status not in (EXIT_FAULT, EXIT_INT3), (name, out.status,
                                                                                                  out.vector)
    # the oracle ends them the same way, with nothing retired and nothing changed
    o = oracle_of(sp)
    o.restore(regs)
    ex = o.step()
    assert (ex.status, o.icount()) == (EXIT_UNIMPLEMENTED, 0), (name, ex.status, ex.vector)
    r = o.regs()
    assert get_zmm(r) == zin and list(r.k) == list(regs.k) and list(r.gpr) == list(regs.gpr)


# ---------------------------------------------------------------- the multi-instruction routines
@pytest.mark.parametrize("fast", [False, True], ids=["exec", "fast"])
def test_engine_runs_avx512x_programs(fast):
    """The natively recorded routines through the engine's host build, to their
    int3: the retired count, the GPRs and both destination areas of every case."""
    lay = PROGS["layout"]
    buf_va = int(PROGS["buf_va"], 16)
    assert {c["routine"] for c in PROGS["cases"]} == set(PROGS["routines"]) and len(PROGS["cases"]) == 32
    fails = []
    for c in PROGS["cases"]:
        sp = program_space()
        regs = regs_from_state(user_state(CODE_VA, 0, sp.cr3))
        sp.write(buf_va + lay["src"], program_case(c, regs))
        ov = simlane.page_buffer()
        out, _, cnt = simlane.run(sp, regs, fast=fast, pages=ov)
        if out.status != EXIT_INT3:
            fails.append((c["routine"], c["len"], "exit", out.status, out.vector, hex(out.rip)))
            continue
        dirty = simlane.dirty_pages(out, ov)
        area = [dirty.get(sp.translate(buf_va + lay[k]), bytes(4096))[:lay["area"]] for k in ("dst", "dst2")]
        bad = program_check(c, out.icount, list(out.gpr), area[0], area[1])
        if bad:
            fails.append((c["routine"], c["len"]) + bad)
        assert not fast or cnt > 0   # the VEX moves and the integer code took the fast loop's forms
    assert not fails, f"{len(fails)}/{len(PROGS['cases'])}, first: {fails[:4]}"


def test_oracle_runs_avx512x_programs():
    """The same 32 recorded routines through the oracle, to their int3: the
    retired count, the GPRs and both destination areas."""
    lay = PROGS["layout"]
    buf_va = int(PROGS["buf_va"], 16)
    assert len(PROGS["cases"]) == 32
    fails = []
    for c in PROGS["cases"]:
        sp = program_space()
        regs = regs_from_state(user_state(CODE_VA, 0, sp.cr3))
        sp.write(buf_va + lay["src"], program_case(c, regs))
        o = oracle_of(sp)
        o.restore(regs)
        o.set_limit(10 * c["icount"] + 1000)
        ex = o.run()
        if ex.status != EXIT_INT3:
            fails.append((c["routine"], c["len"], "exit", ex.status, ex.vector, hex(ex.rip)))
            continue
        area = [o.read_virt(buf_va + lay[k], lay["area"]) for k in ("dst", "dst2")]
        bad = program_check(c, o.icount(), list(o.regs().gpr), area[0], area[1])
        if bad:
            fails.append((c["routine"], c["len"]) + bad)
    assert not fails, f"{len(fails)}/{len(PROGS['cases'])}, first: {fails[:4]}"


@pytest.mark.parametrize("shared", [False, True], ids=["program-per-lane", "shared-programs"])
@pytest.mark.parametrize("fast", [False, True], ids=["exec", "fast"])
def test_engine_evex_code_matches_oracle_on_random_programs(fast, shared):
    """The engine's host build against the oracle on random programs from the
    EVEX pool (tests/progfuzz.py), VEX and legacy SSE forms between them, every
    lane from its own zmm0-31 and k0-7: exit, rip, retired count, GPRs, RFLAGS,
    zmm0-31, k0-7, MXCSR, the byte counter and the dirty set, per lane."""
    from tests import progfuzz

    n, seed = 192, 36
    if shared:
        sp, st, lanes = progfuzz.build_shared(n, 16, seed, sse=True, evex=True)
    else:
        sp, st, lanes = progfuzz.build(n, seed=seed, sse=True, evex=True)
    kw = progfuzz.lane_state(n, seed, True, True)
    want = progfuzz.oracle_run(sp, st, lanes, limit=2000, **kw)
    img = simlane.image(sp)
    bad = []
    for i, ((va, g, flags), w) in enumerate(zip(lanes, want)):
        regs = regs_from_state(st)
        for k in range(16):
            regs.gpr[k] = g[k]
        progfuzz.set_lane_state(regs, i, **kw)
        regs.rip, regs.rflags = va, flags
        out, fin, _ = simlane.run(img, regs, limit=2000, fast=fast)
        f = out.status == EXIT_FAULT
        got = (out.status, out.vector if f else 0, out.error if f else 0, out.addr if f else 0, out.rip, out.icount)
        f = w["status"] == EXIT_FAULT
        exp = (w["status"], w["vector"] if f else 0, w["error"] if f else 0, w["addr"] if f else 0, w["rip"], w["icount"])
        if got != exp:
            bad.append((i, "exit", got, exp))
        elif list(out.gpr) != w["gpr"] or out.rflags != w["rflags"]:
            bad.append((i, "regs"))
        elif get_zmm(fin) != w["zmm"]:
            z = get_zmm(fin)
            bad.append((i, "zmm", [(j // 8, j % 8, hex(z[j]), hex(w["zmm"][j])) for j in range(256) if z[j] != w["zmm"][j]][:3]))
        elif list(fin.k) != w["k"] or out.mxcsr != w["mxcsr"]:
            bad.append((i, "k/mxcsr", [hex(v) for v in fin.k], [hex(v) for v in w["k"]]))
        elif out.nbytes != w["bytes"]:
            bad.append((i, "bytes", out.nbytes, w["bytes"]))
        elif {out.dirty[k] for k in range(min(out.ovn, 64))} != w["dirty"]:
            bad.append((i, "dirty"))
    assert all(w["status"] != EXIT_UNIMPLEMENTED for w in want)
    assert sum(w["zmm"] != kw["zmm"][i] for i, w in enumerate(want)) > n // 2   # the EVEX forms ran
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:4]}"


def test_vpabs_meets_its_minimum_in_a_selected_element():
    """0x80..0 is vpabs's boundary operand (its own absolute value): every
    vpabs form has it in an element its mask selects, at every length, from a
    register and from memory."""
    seen = set()
    for c in DOC["cases"]:
        nm = c["name"].split(".")[0]
        if not nm.startswith("vpabs") or "fault" in c or c["guard"] or c["name"].startswith("ud."):
            continue
        e = fields(c)
        es = {"b": 1, "w": 2, "d": 4, "q": 8}[nm[-1]]
        n = (16 << e["ll"]) // es
        sel = int(c["k"][e["aaa"]], 16) if e["aaa"] else ~0
        src = rm_operand(c, e, n * es) if e["mod"] == 3 or "wov" in c else None
        if src is None:
            continue
        minv = (1 << (8 * es - 1)).to_bytes(es, "little")
        if any((sel >> j) & 1 and src[j * es: (j + 1) * es] == minv for j in range(n)):
            seen.add((nm, e["ll"], "r" if e["mod"] == 3 else "m"))
    assert seen == {(f"vpabs{s}", ll, rm) for s in "bwdq" for ll in range(3) for rm in "rm"}


def test_shift_forms_meet_the_four_named_counts():
    """Counts of 0, width - 1, width and beyond the width, in the imm8 forms,
    the xmm / m128-count forms and the per-element forms, each from a register
    and from memory."""
    SH = ("vpsrl", "vpsra", "vpsll", "vprol", "vpror")
    seen = {}
    for c in DOC["cases"]:
        nm = c["name"].split(".")[0]
        if not nm.startswith(SH) or nm.endswith("dq") or "fault" in c or c["guard"] or c["name"].startswith("ud."):
            continue
        e = fields(c)
        es = {"w": 2, "d": 4, "q": 8}[nm[-1]]
        bits = 8 * es
        if e["map"] == 1 and 0x71 <= e["opc"] <= 0x73:
            kind, counts = "imm", [e["imm"]]
        elif e["map"] == 1:
            kind, counts = "xmm", [int.from_bytes(rm_operand(c, e, 8), "little")]
        else:
            kind = "var"
            src = rm_operand(c, e, 16 << e["ll"])
            counts = [int.from_bytes(src[j: j + es], "little") for j in range(0, len(src), es)]
        got = seen.setdefault((nm, kind, "r" if e["mod"] == 3 else "m"), set())
        for k in counts:
            got.add("0" if k == 0 else "w-1" if k == bits - 1 else "w" if k == bits else ">w" if k > bits else "")
    names = MNEMONICS["B"].split()
    want = {(n, "var") for n in names if n[-2] == "v"} | {(n, "imm") for n in names if n[-2] != "v" and n[-2:] != "dq"} \
        | {(n, "xmm") for n in names if n.startswith(SH[:3]) and n[-2] != "v" and n[-2:] != "dq"}
    assert {k[:2] for k in seen} == want
    for key, got in seen.items():
        assert got >= {"0", "w-1", "w", ">w"}, (key, got)
