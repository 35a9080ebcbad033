"""GPU engine vs CPU oracle on random x86-64 programs (tests/progfuzz.py).

Per lane: exit status / vector / error code / fault address, final rip,
retired instruction count, all 16 GPRs, RFLAGS, the coverage set (every rip
executed), the dirty-page set, the algorithmic byte counter and the contents
of the data window and the stack. Bit-exact.
"""
import pytest

from tests import progfuzz
from wtf_amd.abi import EXIT_FAULT, EXIT_UNIMPLEMENTED, regs_from_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_gpu_matches_oracle_on_random_programs(seed):
    n = 512
    sp, st, lanes = progfuzz.build(n, seed=seed)
    want = progfuzz.oracle_run(sp, st, lanes)
    eng, stats = progfuzz.run_gpu(sp, st, lanes)
    ex = eng.exits()
    g = eng.read_gprs()
    cov, ovf = eng.coverage()
    assert not ovf
    nb = eng.nbytes()
    bad = []
    for i, w in enumerate(want):
        e = ex[i]
        got = {"status": e.status, "vector": e.vector if e.status == 5 else 0,
               "error": e.error if e.status == 5 else 0, "addr": e.addr if e.status == 5 else 0,
               "rip": int(g[i, 16]), "icount": e.icount}
        exp = {"status": w["status"], "vector": w["vector"] if w["status"] == 5 else 0,
               "error": w["error"] if w["status"] == 5 else 0, "addr": w["addr"] if w["status"] == 5 else 0,
               "rip": w["rip"], "icount": w["icount"]}
        if got != exp:
            bad.append((i, "exit", got, exp))
            continue
        if [int(x) for x in g[i, :16]] != w["gpr"] or int(g[i, 17]) != w["rflags"]:
            bad.append((i, "regs", [hex(int(x)) for x in g[i, :18]], [hex(x) for x in w["gpr"] + [w["rflags"]]]))
            continue
        if cov.get(i, set()) != w["cov"]:
            bad.append((i, "cov", len(cov.get(i, set())), len(w["cov"])))
            continue
        if set(eng.dirty(i)) != w["dirty"]:
            bad.append((i, "dirty", sorted(eng.dirty(i)), sorted(w["dirty"])))
            continue
        if int(nb[i]) != w["bytes"]:
            bad.append((i, "bytes", int(nb[i]), w["bytes"]))
            continue
        if i % 8 == 0:
            if eng.read_virt(i, progfuzz.WIN_VA, 0x2000) != w["win"] or \
                    eng.read_virt(i, progfuzz.STACK_VA, 0x2000) != w["stack"]:
                bad.append((i, "memory"))
    assert stats.lane_retired == sum(w["icount"] for w in want)
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:3]}"


def test_gpu_matches_oracle_on_random_evex_programs():
    """A program per lane from the EVEX pool (VEX and SSE forms between the
    AVX-512 ones), every lane from its own zmm0-31 / k0-7: what the test above
    compares, and XMM / YMM-high / MXCSR, zmm0-31 and k0-7."""
    n, seed = 512, 36
    sp, st, lanes = progfuzz.build(n, seed=seed, sse=True, evex=True)
    kw = progfuzz.lane_state(n, seed, True, True)
    want = progfuzz.oracle_run(sp, st, lanes, **kw)
    from wtf_amd.engine import Engine

    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=8, cov_entries=4096)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(20000)
    eng.restore()
    regs = eng.read_regs(0, n)
    for i, (va, g, flags) in enumerate(lanes):
        r = regs[i]
        for k in range(16):
            r.gpr[k] = g[k]
        r.rip, r.rflags = va, flags
        progfuzz.set_lane_state(r, i, **kw)
    eng.write_regs(regs)
    stats = eng.run()
    ex = eng.exits()
    out = eng.read_regs(0, n)
    cov, ovf = eng.coverage()
    assert not ovf
    nb = eng.nbytes()
    bad = []
    for i, w in enumerate(want):
        e, r = ex[i], out[i]
        f = e.status == EXIT_FAULT
        got = (e.status, e.vector if f else 0, e.error if f else 0, e.addr if f else 0, r.rip, e.icount)
        f = w["status"] == EXIT_FAULT
        exp = (w["status"], w["vector"] if f else 0, w["error"] if f else 0, w["addr"] if f else 0, w["rip"], w["icount"])
        if got != exp:
            bad.append((i, "exit", got, exp))
        elif [r.gpr[k] for k in range(16)] != w["gpr"] or r.rflags != w["rflags"]:
            bad.append((i, "regs", [hex(r.gpr[k]) for k in range(16)] + [hex(r.rflags)],
                        [hex(x) for x in w["gpr"] + [w["rflags"]]]))
        elif [r.xmm[k][h] for k in range(16) for h in range(2)] != w["xmm"] or r.mxcsr != w["mxcsr"]:
            bad.append((i, "xmm/mxcsr"))
        elif [r.ymmh[k][h] for k in range(16) for h in range(2)] != w["ymmh"]:
            bad.append((i, "ymmh"))
        elif progfuzz.get_zmm(r) != w["zmm"]:
            z = progfuzz.get_zmm(r)
            bad.append((i, "zmm", [(j // 8, j % 8, hex(z[j]), hex(w["zmm"][j])) for j in range(256) if z[j] != w["zmm"][j]][:4]))
        elif [r.k[j] for j in range(8)] != w["k"]:
            bad.append((i, "k", [hex(r.k[j]) for j in range(8)], [hex(v) for v in w["k"]]))
        elif cov.get(i, set()) != w["cov"]:
            bad.append((i, "cov", len(cov.get(i, set())), len(w["cov"])))
        elif set(eng.dirty(i)) != w["dirty"]:
            bad.append((i, "dirty", sorted(eng.dirty(i)), sorted(w["dirty"])))
        elif int(nb[i]) != w["bytes"]:
            bad.append((i, "bytes", int(nb[i]), w["bytes"]))
        elif i % 8 == 0 and (eng.read_virt(i, progfuzz.WIN_VA, 0x2000) != w["win"] or
                             eng.read_virt(i, progfuzz.STACK_VA, 0x2000) != w["stack"]):
            bad.append((i, "memory"))
    assert all(w["status"] != EXIT_UNIMPLEMENTED for w in want)
    assert stats.lane_retired == sum(w["icount"] for w in want)
    assert not bad, f"{len(bad)}/{n} lanes differ; first: {bad[:3]}"
    eng.close()
