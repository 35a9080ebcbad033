"""The golden-vector harness itself (tests/vector_replay.py, tests/simlane.py).

Every family's check() sees each field its table (Family.fields) says it
compares: a sample of cases runs on the oracle executor and passes; then the
Outcome is perturbed one field at a time and check() must report each
perturbation. All three executors feed the same check(), so this covers the
host lane build and the GPU path too. And the one ctypes mirror of the lane
library's result struct has the library's size.
"""
import dataclasses

import pytest

from tests import simlane
from tests import vector_replay as V
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, Regs


def sample(fam):
    """The first case of each of up to 32 distinct name prefixes, and one of
    each kind of case that is judged differently (a trap, a fault, a #PF)."""
    picked, seen = [], set()
    for c in fam.doc["cases"]:
        key = c.get("name", c["code"]).split(".")[0]
        if key not in seen and len(seen) < 32:
            seen.add(key)
            picked.append(c)
    for kind in (lambda c: "trap_mx" in c, lambda c: "fault" in c, lambda c: c.get("fault", {}).get("vec") == 14,
                 lambda c: isinstance(c.get("out"), dict) and c["out"]["status"] == EXIT_FAULT):
        c = next((c for c in fam.doc["cases"] if kind(c)), None)
        if c is not None and not any(c is p for p in picked):
            picked.append(c)
    return picked


def with_regs(o, edit, **kw):
    r = Regs.from_buffer_copy(o.regs)
    edit(r)
    return dataclasses.replace(o, regs=r, **kw)


def flip(name):
    def edit(r):
        a = getattr(r, name)
        if hasattr(a[0], "__len__"):
            a[0][0] ^= 1
        else:
            a[0] ^= 1
    return edit


def perturbations(fam, c, o):
    """(field of the family's table, the perturbed Outcome) for every
    perturbation that applies to this kind of case."""
    trap = "trap_mx" in c
    fault = "fault" in c or (isinstance(c.get("out"), dict) and c["out"]["status"] == EXIT_FAULT)
    x87_fault = fault and "fault" not in c   # its whole x87 state is still compared
    out = [("status", dataclasses.replace(o, status=EXIT_INT3 if (trap or fault) else EXIT_FAULT, clean=False))]
    if trap or fault:
        out.append(("fault", dataclasses.replace(o, vector=o.vector + 1)))
    if c.get("fault", {}).get("vec") == 14:
        out.append(("fault", dataclasses.replace(o, addr=o.addr ^ 1)))
    if trap:
        return out + [("mxcsr", with_regs(o, lambda r: setattr(r, "mxcsr", r.mxcsr ^ 1)))]
    if not x87_fault:
        out.append(("icount", dataclasses.replace(o, icount=o.icount + 1)))
    if not fault:
        g = 2 if c.get("dst") == 1 else 1
        out.append(("gpr", with_regs(o, lambda r: r.gpr.__setitem__(g, r.gpr[g] ^ 1))))
        out.append(("rip", dataclasses.replace(o, rip=o.rip + 1)))
        out.append(("mxcsr", with_regs(o, lambda r: setattr(r, "mxcsr", r.mxcsr ^ 1))))
        out.append(("k", with_regs(o, lambda r: r.k.__setitem__(1, r.k[1] ^ 1))))
    if not fault or x87_fault:
        mask = fam.flag_mask(c)
        if mask:
            out.append(("flags", with_regs(o, lambda r: setattr(r, "rflags", r.rflags ^ (mask & -mask)))))
        out.append(("x87", with_regs(o, lambda r: setattr(r, "fpsw", r.fpsw ^ 1))))
    out.append(("vec", with_regs(o, flip(fam.vreg))))
    if o.mem is not None:
        out.append(("mem", dataclasses.replace(o, mem=bytes([o.mem[0] ^ 1]) + o.mem[1:])))
    return out


@pytest.mark.parametrize("fam", V.FAMILIES, ids=[f.name for f in V.FAMILIES])
def test_check_sees_every_field_it_claims_to_compare(fam):
    cases = sample(fam)
    kinds = {"trap_mx": any("trap_mx" in c for c in fam.doc["cases"]),
             "fault": any("fault" in c for c in fam.doc["cases"])}
    assert all(any(k in c for c in cases) for k, has in kinds.items() if has)
    exercised, missed = set(), []
    for c, o in zip(cases, V.replay_oracle(fam, cases), strict=True):
        assert fam.check(c, o) is None, (c.get("name"), c["code"], fam.check(c, o))
        for field, bad in perturbations(fam, c, o):
            if field in fam.fields:
                exercised.add(field)
                if fam.check(c, bad) is None:
                    missed.append((c.get("name"), c["code"], field))
    assert not missed, f"perturbations check() did not report: {missed[:8]}"
    faulting = any("trap_mx" in c or "fault" in c or isinstance(c.get("out"), dict) for c in fam.doc["cases"])
    want = set(fam.fields) - (set() if faulting else {"fault"})   # (sse4 and ext hold no case that traps)
    assert exercised == want, want - exercised


@pytest.mark.parametrize("fam", V.PLACED, ids=[f.name for f in V.PLACED])
def test_judge_sees_the_byte_count_of_a_placed_case(fam):
    """A placed replay (tests/test_page_edge.py) compares one more field, the
    executor's byte count with the oracle's for the same placed case: under
    every rule a placement is judged by, a perturbed nbytes must be reported,
    and what check() reports at the original place judge() reports here."""
    rules = set()
    for kind in V.KINDS:
        cases, seen = [], set()
        for c in V.placed_cases(fam, kind):
            key = (c.get("name", c["code"]).split(".")[0], c["at"].rule)
            if key not in seen and len(seen) < 32:
                seen.add(key)
                cases.append(c)
        for c, o in zip(cases, V.replay_oracle(fam, cases), strict=True):
            assert "bytes" in fam.fields_of(c) and "bytes" not in fam.fields
            assert V.judge(fam, c, o, o) is None
            bad = V.judge(fam, c, dataclasses.replace(o, nbytes=o.nbytes + 1), o)
            assert bad is not None and "bytes" in bad[0], (c.get("name"), c["code"], kind, bad)
            if c["at"].rule == "native" and "trap_mx" not in c:
                assert V.judge(fam, c, dataclasses.replace(o, icount=o.icount + 1), o) is not None
            rules.add(c["at"].rule)
    assert {"native", "fault"} <= rules


def test_the_binding_matches_the_library():
    L = simlane.lib()   # asserts ctypes.sizeof(SimResult) == sim_result_size()
    assert L.sim_result_size() == simlane.C.sizeof(simlane.SimResult)
    assert L is simlane.lib()
