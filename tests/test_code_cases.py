"""Instructions across a page edge and on pages the lane wrote
(tests/code_cases.py), on the oracle and on the engine's lane code built for
the host (tests/native/sim_lane.cc: slow step and fast forms), bit-exact.

The host build fetches its bytes anew at every step and runs one lane, so of
k_run's slow_step it shares decode, the second page's translation and the
copy-on-write with its TLB flush; the uop cache, the cache keys and the group
splitting are tests/test_gpu_code_cases.py's. What this file adds to that one
is the tables' own conditions, computed from the oracle alone: they are
conditions, not measurements, and a table that stops meeting them fails here.

The decode fix this pins: a 16-byte instruction with 8 to 14
bytes on its first page and an absent, non-executable or supervisor second
page raises the fetch's #PF, not #GP(0)."""
import pytest

from tests import code_cases as Z
from tests import simlane
from wtf_amd.abi import EXIT_FAULT, EXIT_INT3, EXIT_TIMEOUT

SWEEP = ("b", "f")   # the programs whose every limit is run


@pytest.fixture(scope="module")
def oracle():
    return Z.new_oracle()


@pytest.fixture(scope="module")
def image():
    sp, _, _ = Z.space()
    return simlane.image(sp)


@pytest.fixture(scope="module")
def table(oracle):
    """[(lane, the oracle's result)] of every lane of both tables: computed
    once, shared, never modified."""
    lanes = Z.split_lanes() + Z.prog_lanes() + Z.prog_lanes(plain=True)
    return [(ln, Z.run_oracle(oracle, ln)) for ln in lanes]


def _report(bad):
    return f"{len(bad)} lanes differ from the oracle; first: " + "; ".join(f"{n}: {d}" for n, d in bad[:6])


# ---------------------------------------------------------------- the tables' conditions
def test_every_split_point_is_present(table):
    want = {ln.name: w for ln, w in table}
    lens = {"inc": 2, "mov64": 10, "mov64-p5": 15, "mov64-p6": 16, "alu-sib": 11, "nop10": 10, "jz-taken": 6,
            "jz-not": 6, "call": 5, "vmovdqu-rip": 8, "evex-disp32": 10, "gather": 10}
    assert {n: Z.split_len(n) for n in Z.SPLIT_INSNS} == lens
    assert len(Z.SPLIT_KINDS) == 8
    for name, n in lens.items():
        for k in range(1, n + 1):
            _, va = Z.split_va(name, k)
            assert (va & 0xFFF) == 0x1000 - k
            for kind in Z.SPLIT_KINDS:
                assert f"{name}/{k}/{kind}" in want
    assert sum(1 for ln, _ in table if ln.name.count("/") == 2 and ln.name.split("/")[0] in lens) == 8 * sum(lens.values())


def test_the_split_table_s_faults_are_the_fetch_s(table):
    """What the oracle says of the faulting kinds: the fault is the second
    page's fetch (#PF with I/D set, at the page's first byte), nothing retired,
    rip unchanged, no coverage entry for the instruction. The 16-byte
    instruction is #GP(0) wherever its bytes can be fetched and whenever 15 of
    them are on the first page."""
    codes = set()
    for ln, w in table:
        if ln.name.split("/")[0] not in Z.SPLIT_INSNS:
            continue
        name, k, kind = ln.name.split("/")[:3]
        k = int(k)
        a, va = Z.split_va(name, k, kind if kind in ("absent", "nx", "u0") else "pp")
        if kind in ("absent", "nx", "u0") and k < min(Z.split_len(name), 15):
            err = 0x14 if kind == "absent" else 0x15
            assert (w["status"], w["vector"], w["error"], w["addr"]) == (EXIT_FAULT, 14, err, a + 0x1000), ln.name
            assert w["icount"] == 0 and w["rip"] == va and va not in w["cov"] and not w["dirty"], ln.name
            codes.add((kind, err))
        elif name == "mov64-p6":
            assert (w["status"], w["vector"], w["error"], w["rip"]) == (EXIT_FAULT, 13, 0, va), ln.name
            assert w["icount"] == {"pool": 0, "host2": 0, "guest2": 2, "priv1": 2, "priv12": 3}.get(kind, 0), ln.name
            codes.add(("gp", 0))
        elif kind in ("absent", "nx", "u0"):   # the whole instruction on the first page: it retires, the int3's fetch faults
            assert (w["status"], w["vector"], w["icount"], w["rip"]) == (EXIT_FAULT, 14, 1, w["addr"]), ln.name
        else:
            assert w["status"] == EXIT_INT3, ln.name
            stores = {"guest2": 1, "priv1": 1, "priv12": 2}.get(kind, 0)
            assert w["icount"] == stores + 1 + (stores > 0), ln.name   # (the stub's jmp)
            _, _, info = Z.space()
            fa, fb = info["frames"][info["split"][name, k]]
            own = {"host2": {fb}, "guest2": {fb}, "priv1": {fa}, "priv12": {fa, fb}}.get(kind, set())
            assert own <= set(w["dirty"]), ln.name
    assert codes == {("absent", 0x14), ("nx", 0x15), ("u0", 0x15), ("gp", 0)}
    # #UD comes from the programs that patch in ud2
    assert sum(1 for ln, w in table if w["status"] == EXIT_FAULT and w["vector"] == 6) >= 2


def _steps_on_own_pages(o, lane):
    """(instructions retired from a frame that was in the oracle's dirty set
    when they were fetched, instructions retired, instructions begun from such
    a frame: the int3 or ud2 a patch put there ends the lane without retiring)."""
    Z.start_oracle(o, lane)
    own = total = begun = 0
    for _ in range(Z.LIMIT):
        rip = o.regs().rip
        gpa = o.translate(rip)
        mine = gpa is not None and (gpa & ~0xFFF) in set(o.dirty())
        before = o.icount()
        begun += mine
        ex = o.step()
        if o.icount() > before:
            total += 1
            own += mine
        if ex.status != 0:
            break
    return own, total, begun


def test_every_program_runs_code_it_wrote(oracle):
    for name in Z.PROGRAMS:
        retired = 0
        for j in range(Z.VARIANTS):
            own, total, begun = _steps_on_own_pages(oracle, Z.prog_lane(name, j))
            retired += own
            if name in ("b", "h") and not j & 1:   # the lanes that keep the pool's bytes
                assert begun == 0 and total > 0, (name, j)
            elif name in ("f", "i"):
                assert 2 * own > total, (name, j, own, total)
            else:
                assert begun >= 1, (name, j, own, total)
        assert retired >= Z.VARIANTS // 2, name


def test_the_variants_of_a_program_run_different_bytes(table):
    """Lanes at one rip that run different bytes end differently."""
    for name in Z.PROGRAMS:
        ends = {(w["status"], w["rip"], tuple(w["gpr"][:4])) for ln, w in table
                if ln.name.split("/")[0] == name and not ln.name.endswith("plain")}
        assert len(ends) >= (3 if name in ("d3", "d4", "e") else Z.VARIANTS // 2), (name, len(ends))


def test_every_breakpoint_placement_is_hit(oracle):
    bps = Z.prog_breakpoints()
    hit = set()
    for ln in Z.prog_lanes():
        w = Z.run_oracle(oracle, ln, bps=bps)
        hit |= {s[0] for s in w["stops"]}
    assert hit == set(bps) and len(bps) >= len(Z.PROGRAMS) + 2
    # the split table's: on the page-crossing instruction of every kind that reaches it
    for name, k in (("mov64", 3), ("call", 2), ("jz-taken", 5), ("gather", 7)):
        for kind in ("pool", "host2", "guest2", "priv1", "priv12"):
            _, va = Z.split_va(name, k)
            w = Z.run_oracle(oracle, Z.split_lane(name, k, kind), bps=[va])
            assert [s[0] for s in w["stops"]] == [va], (name, k, kind)
        # a breakpoint on an instruction whose second page cannot be fetched never stops: the fetch faults first
        for lane in [Z.split_lane(name, k, kind) for kind in ("absent", "nx", "u0")] + [Z.split_lane_unmapped(name, k)]:
            w = Z.run_oracle(oracle, lane, bps=Z.split_breakpoints((name,)))
            assert not w["stops"] and (w["status"], w["vector"], w["icount"]) == (EXIT_FAULT, 14, 0), lane.name


def test_the_limit_sweep_ends_on_private_pages(oracle):
    sp, _, _ = Z.space()
    for name in SWEEP:
        ends_own = 0
        lane = Z.prog_lane(name, 5)
        n = Z.run_oracle(oracle, lane)["icount"]
        assert n >= 12
        for limit in range(1, n + 1):
            w = Z.run_oracle(oracle, lane, limit=limit)
            assert w["status"] == (EXIT_TIMEOUT if limit < n else EXIT_INT3), (name, limit)
            ends_own += w["status"] == EXIT_TIMEOUT and sp.translate(w["rip"]) >> 12 in w["dirty"]
        # (b's first pass through its loop, up to the patching store, runs from the pool's page)
        assert ends_own >= (n - 4 if name == "f" else n - 7), (name, ends_own, n)


# ---------------------------------------------------------------- the host lane build
@pytest.mark.parametrize("fast", [0, 1], ids=["slow-step", "fast-forms"])
def test_host_build_matches_the_oracle(table, image, fast):
    bad, retired = [], 0
    for ln, w in table:
        got = Z.run_sim(image, ln, fast)
        retired += got["fast"]
        if d := Z.diff(got, w):
            bad.append((ln.name, d))
    assert not bad, _report(bad)
    if fast:   # the patching stores and the loops did run as fast forms
        assert retired >= len(table)


@pytest.mark.parametrize("fast", [0, 1], ids=["slow-step", "fast-forms"])
def test_host_build_matches_the_oracle_at_every_limit(oracle, image, fast):
    bad = []
    for name in SWEEP:
        for j in (0, 5):
            lane = Z.prog_lane(name, j)
            n = Z.run_oracle(oracle, lane)["icount"]
            for limit in range(1, n + 1):
                w = Z.run_oracle(oracle, lane, limit=limit)
                if d := Z.diff(Z.run_sim(image, lane, fast, limit=limit), w):
                    bad.append((f"{lane.name} limit {limit}", d))
    assert not bad, _report(bad)


def test_breakpoint_stops_leave_the_result_alone(oracle, table):
    """Followed breakpoints change nothing but the stop list (what the GPU
    test's resumed runs are compared with)."""
    bps = Z.prog_breakpoints()
    for ln, w in table:
        if ln.name.split("/")[0] in Z.PROGRAMS and not ln.name.endswith("plain"):
            got = Z.run_oracle(oracle, ln, bps=bps)
            assert got["stops"] and not Z.diff({k: v for k, v in got.items() if k != "stops"}, w), ln.name


# ---------------------------------------------------------------- the shared-program corpus on private pages
def test_the_corpus_variant_is_the_corpus_plus_its_code_frames():
    """tests/launch_shapes.py's private_code workloads: for the lanes whose
    program pages the host wrote, the ordinary results plus the two code frames
    in the dirty set, every instruction of theirs fetched from those frames;
    the other lanes of each program unchanged."""
    from tests import launch_shapes as S
    from tests import progfuzz

    for case in (S.INT_A, S.EVEX):
        plain, own = S.Workload(case), S.Workload(case, private_code=True)
        for i, (a, b) in enumerate(zip(plain.want, own.want)):
            va = own.lanes[i][0]
            frames = {own.sp.translate(va + off) & ~0xFFF for off in range(0, progfuzz.SLOT, 0x1000)}
            assert {k: v for k, v in a.items() if k != "dirty"} == {k: v for k, v in b.items() if k != "dirty"}, i
            if i % 4 in (1, 3):
                assert b["dirty"] == a["dirty"] | frames and not frames & a["dirty"], i
                assert b["cov"] and all(va <= rip < va + progfuzz.SLOT for rip in b["cov"]), i
            else:
                assert b["dirty"] == a["dirty"] and not own.writes[i], i
        assert sum(b["icount"] for i, b in enumerate(own.want) if i % 4 in (1, 3)) > 10000
