"""k_run's launch shapes over one workload of shared programs (tests/progfuzz.py:
build_shared): the workload and its oracle results, the engine set up for it,
the per-lane comparison, and every way a run can be launched. Used by
tests/test_gpu_progfuzz_shared.py, and by tests/test_gpu_paging.py with an
engine of its own (it replaces make_engine)."""
import numpy as np

from tests import progfuzz
from wtf_amd.abi import EXIT_FAULT, RUNNING, regs_from_state

N, N_PROGRAMS, LIMIT = 512, 16, 2000
CASES = progfuzz.SHARED_CASES
INT_A, INT_B, SSE, FP, EVEX = CASES
MORE = ((progfuzz.WIN2_VA, progfuzz.WIN2_LEN),)


def case_id(c):
    return f"seed{c[0]}" + ("-sse" if c[1] else "") + ("-fp" if c[2] else "") + ("-evex" if c[3] else "")


class Workload:
    """private_code: the lanes with i % 4 in {1, 3} get one byte of each page
    of their program written by the host before they run, with the value it
    has: the same programs, run from the lane's own copies of their pages
    (k_run's slow_step) next to lanes of the same program that run the pool's
    (lanes 4j .. 4j + 3 share a program). n: the lane count (the first n lanes
    of the N-lane workload)."""

    def __init__(self, case, n=N, private_code=False):
        seed, sse, fp, evex = case
        self.case = case
        self.evex = evex
        self.n = n
        self.sp, self.st, self.lanes, self.progs = progfuzz.build_shared_info(N, N_PROGRAMS, seed, sse=sse, fp=fp,
                                                                              evex=evex)
        self.lanes = self.lanes[:n]
        self.kw = {k: v[:n] for k, v in progfuzz.lane_state(N, seed, sse, evex).items()}
        self.writes = None
        if private_code:
            self.writes = [[(va + off, bytes(self.sp.pages[self.sp.translate(va + off) >> 12][:1]))
                            for off in range(0, progfuzz.SLOT, 0x1000)] if i % 4 in (1, 3) else []
                           for i, (va, _, _) in enumerate(self.lanes)]
        self.want = progfuzz.oracle_run(self.sp, self.st, self.lanes, limit=LIMIT, more=MORE, writes=self.writes,
                                        **self.kw)
        self._bp = None

    def breakpoints(self):
        """The first instruction of about a quarter of every program's blocks,
        one inside a counted loop and one jcc target among them where the
        program has any."""
        rng = np.random.RandomState(self.case[0])
        bps = set()
        for p in self.progs:
            blocks = p["blocks"]
            for sel in (lambda b: b[1], lambda b: b[2] and not b[1]):
                some = [b[0] for b in blocks if sel(b)]
                if some:
                    bps.add(some[rng.randint(len(some))])
            k = max(1, len(blocks) // 4)
            bps.update(blocks[j][0] for j in rng.choice(len(blocks), k, replace=False))
        return sorted(bps)

    def want_bp(self):
        """The oracle's run over the breakpoints: "stops" per lane, same final state."""
        if self._bp is None:
            self._bp = progfuzz.oracle_run(self.sp, self.st, self.lanes, limit=LIMIT, more=MORE,
                                           breakpoints=self.breakpoints(), follow_bps=True, writes=self.writes,
                                           **self.kw)
        return self._bp



# ---------------------------------------------------------------------------
# engine side
# ---------------------------------------------------------------------------
def make_engine(w, breakpoints=(), code_pages=False):
    """code_pages: the programs' pages get a coverage map (set_code_pages), so
    that committed rips count as covered (UC_COVERED) instead of being logged."""
    from wtf_amd.engine import Engine

    eng = Engine(0)
    pfns, blob = w.sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(w.n, overlay_pages=16, cov_entries=4096)
    eng.set_initial_state(regs_from_state(w.st))
    eng.set_limit(LIMIT)
    if breakpoints:
        eng.set_breakpoints(list(breakpoints))
    if code_pages:
        eng.set_code_pages([(p["va"] >> 12) + k for p in w.progs for k in range(progfuzz.SLOT >> 12)])
    load_lanes(eng, w)
    return eng


def load_lanes(eng, w):
    eng.restore()
    regs = eng.read_regs(0, w.n)
    for i, (va, g, flags) in enumerate(w.lanes):
        r = regs[i]
        for k in range(16):
            r.gpr[k] = g[k]
        r.rip, r.rflags = va, flags
        progfuzz.set_lane_state(r, i, **w.kw)
    eng.write_regs(regs)
    if w.writes:
        eng.apply_writes([(i, va, data) for i, ws in enumerate(w.writes) for va, data in ws])


class Totals:
    def __init__(self):
        self.calls = self.launches = self.group_steps = self.retired = 0

    def add(self, st):
        self.calls += 1
        self.launches += st.kernel_launches
        self.group_steps += st.group_steps
        self.retired += st.lane_retired


def running(eng):
    return bool((eng.exits_np()["status"] == RUNNING).any())


def run_sliced(eng, steps, tot=None, use_async=False):
    """run(max_steps=steps) until no lane is RUNNING."""
    tot = tot or Totals()
    # a wave of 64 lanes at 2000 instructions each cannot take more wave-steps
    for _ in range(64 * (LIMIT + 1) // steps + 2):
        if use_async:
            eng.run_async(0, eng.nlanes, steps)
            tot.add(eng.run_wait())
        else:
            tot.add(eng.run(max_steps=steps))
        if not running(eng):
            return tot
    raise AssertionError("lanes still running after every possible wave-step")


def differences(eng, w, want, cov=True):
    """Per-lane bit-exact comparison with the oracle's results."""
    ex = eng.exits()
    out = eng.read_regs(0, w.n)
    covs, ovf = eng.coverage()
    assert not ovf
    nb = eng.nbytes()
    bad = []
    for i, x in enumerate(want):
        e, r = ex[i], out[i]
        f = e.status == EXIT_FAULT
        got = (e.status, e.vector if f else 0, e.error if f else 0, e.addr if f else 0, r.rip, e.icount)
        f = x["status"] == EXIT_FAULT
        exp = (x["status"], x["vector"] if f else 0, x["error"] if f else 0, x["addr"] if f else 0, x["rip"], x["icount"])
        prog = progfuzz.lane_program(i, N_PROGRAMS)
        if got != exp:
            bad.append((i, prog, "exit", got, exp))
        elif [r.gpr[k] for k in range(16)] != x["gpr"] or r.rflags != x["rflags"]:
            bad.append((i, prog, "regs", [hex(r.gpr[k]) for k in range(16)] + [hex(r.rflags)],
                        [hex(v) for v in x["gpr"] + [x["rflags"]]]))
        elif w.kw and ([r.xmm[k][h] for k in range(16) for h in range(2)] != x["xmm"] or r.mxcsr != x["mxcsr"]):
            bad.append((i, prog, "xmm/mxcsr"))
        elif w.kw and [r.ymmh[k][h] for k in range(16) for h in range(2)] != x["ymmh"]:
            bad.append((i, prog, "ymmh"))
        elif w.evex and progfuzz.get_zmm(r) != x["zmm"]:
            z = progfuzz.get_zmm(r)
            bad.append((i, prog, "zmm (register, qword, got, expected)",
                        [(j // 8, j % 8, hex(z[j]), hex(x["zmm"][j])) for j in range(256) if z[j] != x["zmm"][j]][:4]))
        elif w.evex and [r.k[j] for j in range(8)] != x["k"]:
            bad.append((i, prog, "k", [hex(r.k[j]) for j in range(8)], [hex(v) for v in x["k"]]))
        elif cov and covs.get(i, set()) != x["cov"]:
            bad.append((i, prog, "cov", sorted(hex(v) for v in covs.get(i, set()) ^ x["cov"])[:8]))
        elif set(eng.dirty(i)) != x["dirty"]:
            bad.append((i, prog, "dirty", sorted(eng.dirty(i)), sorted(x["dirty"])))
        elif int(nb[i]) != x["bytes"]:
            bad.append((i, prog, "bytes", int(nb[i]), x["bytes"]))
        elif i % 8 == 0 and (eng.read_virt(i, progfuzz.WIN_VA, 0x2000) != x["win"] or
                             eng.read_virt(i, progfuzz.STACK_VA, 0x2000) != x["stack"] or
                             eng.read_virt(i, MORE[0][0], MORE[0][1]) != x["more"][0]):
            bad.append((i, prog, "memory"))
    return bad


def check(eng, w, want, shape, retired=None, cov=True):
    bad = differences(eng, w, want, cov=cov)
    assert not bad, (f"{case_id(w.case)} / {shape}: {len(bad)}/{w.n} lanes differ; "
                     f"first (lane, program, what, got, expected): {bad[:3]}")
    if retired is not None:
        assert retired == sum(x["icount"] for x in want), shape


# ---------------------------------------------------------------------------
# every launch shape: shape(workload, monkeypatch) -> (engine, lanes retired)
# ---------------------------------------------------------------------------
def accepts_run_at(eng, first):
    """Whether a run may start at lane `first`: only at a multiple of the lanes
    per wave. Asked when no lane is running: the launch retires nothing."""
    from wtf_amd.engine import EngineError

    try:
        eng.run(first=first, count=first, max_steps=1)
        return True
    except EngineError:
        return False


def shape_fixed(w, mp):
    mp.setenv("WTFGPU_REGROUP_STEPS", "0")
    eng = make_engine(w)
    st = eng.run()
    assert st.kernel_launches == 1
    assert not accepts_run_at(eng, 32) and not accepts_run_at(eng, 16)  # 64 lanes per wave
    return eng, st.lane_retired


def shape_regroup(w, mp):
    mp.setenv("WTFGPU_REGROUP_AUTO", "0")
    eng = make_engine(w)
    eng.set_regroup(64)
    st = eng.run()
    assert st.kernel_launches >= 2
    return eng, st.lane_retired


def shape_sliced(steps):
    def shape(w, mp):
        eng = make_engine(w)
        tot = run_sliced(eng, steps)
        assert tot.calls > 1
        return eng, tot.retired
    return shape


def shape_async(w, mp):
    eng = make_engine(w)
    tot = run_sliced(eng, 64, use_async=True)
    assert tot.calls > 1
    return eng, tot.retired


def shape_lpw(lpw):
    def shape(w, mp):
        mp.setenv("WTFGPU_LPW", str(lpw))
        eng = make_engine(w)
        st = eng.run()
        assert accepts_run_at(eng, lpw) and accepts_run_at(eng, 16) == (lpw == 16)
        return eng, st.lane_retired
    return shape


def shape_cold_lds(w, mp):
    mp.setenv("WTFGPU_WARM", "0")
    eng = make_engine(w)
    tot = run_sliced(eng, 64)
    assert tot.calls > 1
    return eng, tot.retired


def shape_no_guc(w, mp):
    mp.setenv("WTFGPU_GUC", "0")
    eng = make_engine(w)
    st = eng.run()
    return eng, st.lane_retired


def shape_code_pages(w, mp):
    eng = make_engine(w, code_pages=True)  # nothing committed: every rip is still new to every lane
    st = eng.run()
    return eng, st.lane_retired


def snapshot(eng):
    return eng.exits_np().tobytes(), eng.read_gprs().tobytes(), eng.nbytes().tobytes()


def shape_hot(w, mp):
    eng = make_engine(w)
    st = eng.run()
    check(eng, w, w.want, "hot caches, first pass", retired=st.lane_retired)
    first = snapshot(eng)
    load_lanes(eng, w)
    st = eng.run()
    assert snapshot(eng) == first, "the second pass differs from the first"
    return eng, st.lane_retired


def shape_combined(w, mp):
    mp.setenv("WTFGPU_REGROUP_AUTO", "0")
    mp.setenv("WTFGPU_LPW", "16")
    eng = make_engine(w)
    eng.set_regroup(64)
    tot = run_sliced(eng, 64)
    assert tot.calls > 1 and accepts_run_at(eng, 16)
    return eng, tot.retired


SHAPES = {
    "fixed-order": shape_fixed, "regroup-64": shape_regroup, "sliced-5": shape_sliced(5), "sliced-64": shape_sliced(64),
    "async-64": shape_async, "lpw-32": shape_lpw(32), "lpw-16": shape_lpw(16), "cold-lds-sliced-64": shape_cold_lds,
    "no-guc": shape_no_guc, "hot-caches": shape_hot, "code-pages": shape_code_pages,
}
