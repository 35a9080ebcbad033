"""k_run's uncached code path (slow_step, engine_run.h) against the oracle:
instructions across a page edge and instructions on pages a lane wrote, the
tables of tests/code_cases.py (tests/test_code_cases.py holds the tables to
their conditions and runs them on the host lane build). Per lane, bit exact:
exit status / vector / error / address, rip, retired count, byte counter, the
GPRs, RFLAGS, zmm0-31, the dirty frames with all their bytes, the coverage
set, and under breakpoints every stop.

What each test reaches that the host build cannot:

  test_split_table_mixed_waves   every split point's nine lanes side by side
      in one wave. The stub (lower rip) runs first, so at the instruction's rip
      the pool's lanes, the lane the host wrote, the lanes that wrote the
      first, the second or both pages themselves and the lane whose second
      page a physical edit of its own page table took away meet: slow_step's
      split by first-page pointer (L.cptr == lptr), then by second-page
      pointer (nptr == lnptr), the lanes left over coming round again, one
      lane faulting inside the group; all three branches of the byte splice.
  test_split_table_uniform_waves a whole wave at one split point of one kind:
      64 lanes through one slow_step together (pool), or 64 groups of one.
  test_split_table_launch_shapes regroup-64 and 16 lanes per wave.
  test_programs_restore_and_caches  the self-modifying programs; restore, the
      patches swapped between lanes (the same overlay slots hold other code),
      restore, nothing patched: a stale uop, LDS image or shared-cache entry
      keyed by an overlay pointer (cacheable_key) or a code-page pointer that
      outlives the copy-on-write (tlb_flush drops L.cvpn) shows here. Warm and
      cold LDS images, with and without the shared cache.
  test_hooks_*                   slow_step's own coverage, breakpoint + skip,
      RecordEdge and limit (retire) code.
  test_one_code_frame_at_four_addresses  the uop cache is keyed by the frame:
      the flags of an entry are its owner address's only (code_owner).
  test_code_page_in_the_spill_pool  the private code page is a pool page.
  test_corpus_from_private_pages tests/progfuzz.py's shared programs with half
      the lanes of every program on private copies of its pages.

The rip trace is not run here: tests/test_trace.py's helpers drive the
command-line tool on the tlv target and take no address space.

Observed on MI355X, seconds per test (the module 8.5, next to 20.0 for
tests/test_gpu_progfuzz_shared.py in the same run): mixed waves 0.28 (two
passes over 1,024 lanes), uniform waves 1.07 (55,808 lanes), launch shapes
0.12 and 0.46, programs 0.14 / 0.20 / 0.13 (hot, cold LDS, no shared cache),
coverage map 0.06, breakpoints 0.09, edges 0.08, every limit 0.25 (47 limits),
one frame at four addresses 0.03 each way,
spill pool 0.03, the corpus from private pages at 512 lanes 0.27 - 0.63 a
shape and 1.41 for seed 31 in slices of 5 wave-steps, its breakpoints 0.39."""
import numpy as np
import pytest

from tests import code_cases as Z
from tests import launch_shapes as shared
from tests import progfuzz
from wtf_amd.abi import EXIT_BREAKPOINT, EXIT_FAULT, RUNNING, regs_from_state

pytestmark = pytest.mark.gpu

SLICE = ("mov64", "jz-taken", "jz-not", "call", "gather")   # the split table's part that runs under the hooks
_WANT = {}


@pytest.fixture(scope="module")
def oracle():
    return Z.new_oracle()


def want_of(o, lane, limit=Z.LIMIT, bps=(), edges=False):
    """The oracle's result, computed once per (lane, settings) and shared."""
    key = (lane.name, limit, tuple(bps), edges)
    if key not in _WANT:
        _WANT[key] = Z.run_oracle(o, lane, limit, bps, edges)
    return _WANT[key]


def pad(lanes, to=64):
    """Whole waves: the first lanes again."""
    return lanes + lanes[:(-len(lanes)) % to]


def new_engine(n, overlay_pages=4, cov_entries=256):
    from wtf_amd.engine import Engine
    sp, st, _ = Z.space()
    eng = Engine(0)
    pfns, blob = sp.phys()
    eng.load_pool(pfns, blob)
    eng.alloc_lanes(n, overlay_pages=overlay_pages, cov_entries=cov_entries)
    eng.set_initial_state(regs_from_state(st))
    eng.set_limit(Z.LIMIT)
    return eng


def load(eng, lanes):
    eng.restore(0, len(lanes))
    eng.write_regs([ln.regs for ln in lanes])
    for phys in (False, True):
        recs = [(i, a, bytes(d)) for i, ln in enumerate(lanes) for a, d, p in ln.writes if p == phys]
        if recs:
            eng.apply_writes(recs, phys=phys)


def collect(eng, lanes, which=None):
    """Per-lane results in run_oracle's shape, of the lanes `which` (all)."""
    n = len(lanes)
    which = list(range(n)) if which is None else list(which)
    ex = eng.exits_np(0, n)
    nb = eng.nbytes(0, n)
    cov, ovf = eng.coverage(0, n)
    assert not ovf
    if len(which) == n:
        regs = dict(enumerate(eng.read_regs(0, n)))
    else:
        regs = {i: eng.read_regs(i, 1)[0] for i in which}
    dl = eng.dirty_list(np.array(which))
    pl = [i for row, i in enumerate(which) for _ in range(int(dl[row, 0]))]
    pg = [int(g) << 12 for row in range(len(which)) for g in dl[row, 1:1 + int(dl[row, 0])]]
    data = eng.gather_pages(pl, pg) if pl else np.zeros((0, 4096), dtype=np.uint8)
    out, at = {}, 0
    for row, i in enumerate(which):
        k = int(dl[row, 0])
        r = regs[i]
        out[i] = {"status": int(ex["status"][i]), "vector": int(ex["vector"][i]), "error": int(ex["error"][i]),
                  "addr": int(ex["addr"][i]), "rip": int(r.rip), "icount": int(ex["icount"][i]), "gpr": list(r.gpr),
                  "rflags": int(r.rflags), "zmm": progfuzz.get_zmm(r), "bytes": int(nb[i]),
                  "dirty": sorted(p >> 12 for p in pg[at:at + k]),
                  "mem": {pg[at + j] >> 12: data[at + j].tobytes() for j in range(k)}, "cov": cov.get(i, set())}
        at += k
    return out


def check(eng, o, lanes, what, which=None, **settings):
    got = collect(eng, lanes, which)
    bad = [(i, lanes[i].name, d) for i in got if (d := Z.diff(got[i], want_of(o, lanes[i], **settings)))]
    assert not bad, f"{what}: {len(bad)}/{len(got)} lanes differ from the oracle; first (lane, case, what): {bad[:4]}"
    return got


# ---------------------------------------------------------------- the split table
def mixed_lanes():
    """Every split point's eight kinds and its page-table-edit lane, side by side."""
    lanes = []
    for name, k in Z.split_points():
        lanes += [Z.split_lane(name, k, kind) for kind in Z.SPLIT_KINDS] + [Z.split_lane_unmapped(name, k)]
    return pad(lanes)


@pytest.fixture(scope="module")
def eng():
    e = new_engine(len(mixed_lanes()))
    yield e
    e.close()


def test_split_table_mixed_waves(eng, oracle):
    lanes = mixed_lanes()
    # the table's placement: in every wave, at one rip, lanes on the pool's first page, lanes on a private one,
    # and behind one first page the pool's second page, private ones and an absent one
    for w in range(0, len(lanes), 64):
        kinds = {}
        for ln in lanes[w:w + 64]:
            name, k, kind = ln.name.split("/")
            kinds.setdefault((name, k), set()).add(kind)
        assert any(ks >= {"pool", "host2", "guest2", "priv1", "priv12", "edit"} for ks in kinds.values())
    load(eng, lanes)
    st = eng.run(0, len(lanes))
    got = check(eng, oracle, lanes, "mixed waves")
    assert st.lane_retired == sum(g["icount"] for g in got.values())
    # the edit took the second page away from its lane alone
    edits = [i for i, ln in enumerate(lanes) if ln.name.endswith("/edit")]
    assert sum(got[i]["status"] == EXIT_FAULT and got[i]["vector"] == 14 and got[i]["error"] == 0x14 for i in edits) >= 96
    eng.restore(0, len(lanes))
    assert not eng.dirty_counts(0, len(lanes)).any()
    # again from the caches the first pass left: the same results
    load(eng, lanes)
    eng.run(0, len(lanes))
    check(eng, oracle, lanes, "mixed waves, second pass")


def test_split_table_uniform_waves(oracle):
    """One (split point, kind) per wave, its 64 lanes alternating between two
    register sets. Every lane's exit, registers, dirty count and byte counter;
    the first two lanes of every wave in full."""
    base = [(Z.split_lane(name, k, kind, 0), Z.split_lane(name, k, kind, 1)) for name, k in Z.split_points()
            for kind in Z.SPLIT_KINDS]
    lanes = [pair[j & 1] for pair in base for j in range(64)]
    n = len(lanes)
    assert n == 64 * 8 * len(Z.split_points())
    e = new_engine(n, cov_entries=16)
    try:
        load(e, lanes)
        e.run(0, n)
        ex, g, nb, dc = e.exits_np(0, n), e.read_gprs(0, n), e.nbytes(0, n), e.dirty_counts(0, n)
        bad = []
        for w, pair in enumerate(base):
            for j in (0, 1):
                x = want_of(oracle, pair[j])
                sel = slice(64 * w + j, 64 * w + 64, 2)
                f = x["status"] == EXIT_FAULT
                exp = (x["status"], x["rip"], x["icount"]) + ((x["vector"], x["error"], x["addr"]) if f else ())
                for fields in zip(*(ex[k][sel] for k in ("status", "rip", "icount") + (("vector", "error", "addr") if f else ()))):
                    if tuple(int(v) for v in fields) != exp:
                        bad.append((pair[j].name, "exit", fields, exp))
                        break
                if not (g[sel, :16] == np.array(x["gpr"], dtype=np.uint64)).all() or \
                        not (g[sel, 16] == np.uint64(x["rip"])).all() or not (g[sel, 17] == np.uint64(x["rflags"])).all():
                    bad.append((pair[j].name, "registers"))
                if not (dc[sel] == len(x["dirty"])).all() or not (nb[sel] == x["bytes"]).all():
                    bad.append((pair[j].name, "dirty count / bytes"))
        assert not bad, f"{len(bad)} differ; first: {bad[:4]}"
        check(e, oracle, lanes, "uniform waves", which=[64 * w + j for w in range(len(base)) for j in (0, 1)])
    finally:
        e.close()


@pytest.mark.parametrize("shape", ["regroup-64", "lpw-16"])
def test_split_table_launch_shapes(shape, oracle, monkeypatch):
    lanes = mixed_lanes()

    def make_engine(_w):
        e = new_engine(len(lanes))
        load(e, lanes)
        return e

    monkeypatch.setattr(shared, "make_engine", make_engine)
    e, retired = shared.SHAPES[shape](None, monkeypatch)
    try:
        got = check(e, oracle, lanes, shape)
        assert retired == sum(g["icount"] for g in got.values())
    finally:
        e.close()


# ---------------------------------------------------------------- the programs
def program_lanes(**kw):
    """Four copies of every program's variants: the variants of a program are
    neighbours (one group at its first rip, different bytes after the patch)."""
    return pad(Z.prog_lanes(**kw) * 4)


@pytest.mark.parametrize("caches", ["hot-caches", "cold-lds", "no-guc"])
def test_programs_restore_and_caches(caches, oracle, monkeypatch):
    if caches == "cold-lds":
        monkeypatch.setenv("WTFGPU_WARM", "0")
    if caches == "no-guc":
        monkeypatch.setenv("WTFGPU_GUC", "0")
    first, swapped, plain = program_lanes(), program_lanes(swap=True), program_lanes(plain=True)
    e = new_engine(len(first))
    try:
        passes = [("first pass", first), ("patches swapped", swapped), ("nothing patched", plain)]
        if caches == "hot-caches":   # once more over warm LDS images and a filled shared cache
            passes.insert(1, ("second pass", first))
        for what, lanes in passes:
            load(e, lanes)
            if caches == "cold-lds":   # launch boundaries inside the programs
                for _ in range(64 * (Z.LIMIT + 1) // 8 + 2):
                    e.run(0, len(lanes), max_steps=8)
                    if not (e.exits_np(0, len(lanes))["status"] == RUNNING).any():
                        break
            else:
                e.run(0, len(lanes))
            check(e, oracle, lanes, f"{caches}, {what}")
    finally:
        e.close()


def hook_lanes():
    split = []
    for name, k in Z.split_points():
        if name in SLICE:
            split += [Z.split_lane(name, k, kind) for kind in Z.SPLIT_KINDS] + [Z.split_lane_unmapped(name, k)]
    return pad(Z.prog_lanes() + split)


def test_hooks_coverage_map_over_the_code_pages(oracle):
    """Coverage without a map is every other test's; here the code pages have
    one (nothing committed: every rip is still new to every lane). Program g's
    fresh page has none: its rips go to the extra set."""
    lanes = hook_lanes()
    e = new_engine(len(lanes))
    try:
        e.set_code_pages(Z.code_vpns())
        assert Z.FRESH_VA >> 12 not in Z.code_vpns()
        load(e, lanes)
        e.run(0, len(lanes))
        got = check(e, oracle, lanes, "code pages")
        assert any(Z.FRESH_VA in g["cov"] for g in got.values())
    finally:
        e.close()


def test_hooks_breakpoints_followed(oracle):
    """Breakpoints on the patched instruction of every program, on loop heads
    in private pages and on the page-crossing instructions in every view: every
    stop against the oracle's, resumed with skip; the final state as without
    them. Where the second page cannot be fetched (the absent, NX and U = 0
    views, the lanes whose page table was edited) the fetch's fault comes
    first and the breakpoint on the instruction never stops the lane."""
    lanes = hook_lanes()
    bps = sorted(set(Z.prog_breakpoints()) | set(Z.split_breakpoints(SLICE)))
    want = [want_of(oracle, ln, bps=bps) for ln in lanes]
    assert sum(len(w["stops"]) for w in want) >= len(lanes) // 2
    unfetched = [w for ln, w in zip(lanes, want) if ln.name.split("/")[-1] in ("absent", "nx", "u0", "edit")
                 and w["icount"] == 0]
    assert len(unfetched) >= 100 and not any(w["stops"] for w in unfetched)
    e = new_engine(len(lanes))
    try:
        e.set_breakpoints(bps)
        load(e, lanes)
        pos = [0] * len(lanes)
        bad = []
        for _ in range(Z.LIMIT):
            e.run(0, len(lanes))
            ex = e.exits_np(0, len(lanes))
            stopped = [int(i) for i in np.flatnonzero(ex["status"] == EXIT_BREAKPOINT)]
            if not stopped:
                break
            g = e.read_gprs(0, len(lanes))
            for i in stopped:
                got = (int(ex["rip"][i]), int(ex["icount"][i]), [int(v) for v in g[i, :16]])
                stops = want[i]["stops"]
                if pos[i] >= len(stops) or got != stops[pos[i]]:
                    bad.append((i, lanes[i].name, pos[i], got, stops[pos[i]] if pos[i] < len(stops) else None))
                pos[i] += 1
            assert not bad, f"(lane, case, stop number, got, expected): {bad[:3]}"
            e.resume(stopped, [1] * len(stopped))
        else:
            raise AssertionError("lanes still stopping after every possible round")
        assert pos == [len(w["stops"]) for w in want]
        check(e, oracle, lanes, "breakpoints followed", bps=bps)
    finally:
        e.close()


@pytest.mark.parametrize("first", ["present-view-first", "aliases-first"])
def test_one_code_frame_at_four_addresses(first, oracle):
    """The split table's four views share their frames, and the uop cache is
    keyed by the frame. Breakpoints and a coverage map with its rips committed
    on the present view alone: lanes that run the same frame at the other three
    addresses stop at no breakpoint and log every rip of theirs, whichever
    address ran the frame first (the frame's cached entries belong to that one,
    the others run uncached: code_owner)."""
    names = ("inc", "mov64", "jz-taken", "call", "nop10")
    kinds = ("pool", "absent", "nx", "u0") if first == "present-view-first" else ("u0", "nx", "absent", "pool")
    lanes = pad([Z.split_lane(name, k, kind) for name, k in Z.split_points() if name in names for kind in kinds])
    bps = Z.split_breakpoints(names, views=("pp",))
    want = [want_of(oracle, ln, bps=bps) for ln in lanes]
    committed = set().union(*(w["cov"] for ln, w in zip(lanes, want) if ln.name.endswith("/pool")))
    whole = [w for ln, w in zip(lanes, want) if not ln.name.endswith("/pool") and w["icount"] == 1]
    assert len(whole) >= 3 * len(names) and all(w["cov"] and not w["cov"] & committed and not w["stops"] for w in whole)
    e = new_engine(len(lanes))
    try:
        e.set_code_pages(sorted({va >> 12 for va in bps} | {(va >> 12) + 1 for va in bps}))
        e.commit_coverage(committed)
        e.set_breakpoints(bps)
        load(e, lanes)
        e.run(0, len(lanes))
        ex = e.exits_np(0, len(lanes))
        stopped = [int(i) for i in np.flatnonzero(ex["status"] == EXIT_BREAKPOINT)]
        expect = [i for i, w in enumerate(want) if w["stops"]]
        assert stopped == expect and all(int(ex["rip"][i]) == want[i]["stops"][0][0] for i in stopped)
        e.resume(stopped, [1] * len(stopped))
        e.run(0, len(lanes))
        got = collect(e, lanes)
        bad = [(i, lanes[i].name, d) for i in got
               if (d := Z.diff(got[i], dict(want[i], cov=want[i]["cov"] - committed)))]
        assert not bad, f"{len(bad)}/{len(got)} lanes differ from the oracle; first (lane, case, what): {bad[:4]}"
    finally:
        e.close()


def test_hooks_edges(oracle):
    """RecordEdge in slow_step: the page-crossing jz (taken and not), the
    stub's indirect jump onto pages the lane has just written, e's indirect
    jump and g's indirect call into written code. (The direct call records
    no edge; it is here because the oracle says so.)"""
    lanes = hook_lanes()
    e = new_engine(len(lanes))
    try:
        e.set_edges(True)
        load(e, lanes)
        e.run(0, len(lanes))
        got = check(e, oracle, lanes, "edges", edges=True)
        plain = [want_of(oracle, ln) for ln in lanes]
        assert sum(len(got[i]["cov"]) > len(plain[i]["cov"]) for i in got) >= len(lanes) // 4
    finally:
        e.close()


def test_hooks_every_limit(oracle):
    """Programs b and f at every limit from 1 to their length: the timeout
    retire() raises on this path, instruction by instruction."""
    lanes = pad(Z.prog_lanes(("b", "f")))
    top = max(want_of(oracle, ln)["icount"] for ln in lanes)
    e = new_engine(len(lanes))
    try:
        for limit in range(1, top + 1):
            e.set_limit(limit)
            load(e, lanes)
            e.run(0, len(lanes))
            ex = e.exits_np(0, len(lanes))
            want = [want_of(oracle, ln, limit=limit) for ln in lanes]
            bad = [(i, lanes[i].name, (int(ex["status"][i]), int(ex["icount"][i]), hex(int(ex["rip"][i]))),
                    (w["status"], w["icount"], hex(w["rip"]))) for i, w in enumerate(want)
                   if (int(ex["status"][i]), int(ex["icount"][i]), int(ex["rip"][i])) != (w["status"], w["icount"], w["rip"])]
            assert not bad, f"limit {limit}: (lane, case, got, expected) {bad[:3]}"
            if limit in (top // 2, top):
                check(e, oracle, lanes, f"limit {limit}", limit=limit)
    finally:
        e.close()


def test_code_page_in_the_spill_pool(oracle):
    """Program i with one overlay page per lane and the spill pool on: the
    data store takes the lane's own page, the second data page and the code
    page's copy are pool pages, and the lane runs on from there."""
    lanes = pad(Z.prog_lanes(("i", "f", "a")) * 2)
    e = new_engine(len(lanes), overlay_pages=1)
    try:
        e.alloc_spill(4 * len(lanes), 4)
        load(e, lanes)
        e.run(0, len(lanes))
        check(e, oracle, lanes, "spilled code page")
        st = e.spill_stats()
        assert st["lanes_spilled"] >= sum(ln.name.startswith("i/") for ln in lanes) and not st["pool_empty"]
        e.restore(0, len(lanes))
        assert e.spill_stats()["in_use"] == 0
    finally:
        e.close()


# ---------------------------------------------------------------- the shared-program corpus
_CORPUS = {}


@pytest.mark.parametrize("shape", ["fixed-order", "regroup-64", "sliced-5", "lpw-16", "code-pages"])
@pytest.mark.parametrize("case", [shared.INT_A, shared.EVEX], ids=shared.case_id)
def test_corpus_from_private_pages(case, shape, monkeypatch):
    """tests/progfuzz.py's shared programs, lanes 4j + 1 and 4j + 3 of every
    program on private copies of its pages (the host wrote one byte of each,
    with the value it had): the corpus's forms, faults and coverage through
    slow_step, in groups that mix pool and private lanes at one rip."""
    if case not in _CORPUS:
        _CORPUS[case] = shared.Workload(case, private_code=True)
    w = _CORPUS[case]
    private = [i for i, ws in enumerate(w.writes) if ws]
    assert len(private) == w.n // 2 and all({4 * (i // 4) + 1, 4 * (i // 4) + 3} <= set(private) for i in private)
    frames = [{w.sp.translate(va) & ~0xFFF for va, _ in w.writes[i]} for i in private]
    assert all(len(f) == 2 and f <= w.want[i]["dirty"] for i, f in zip(private, frames))
    e, retired = shared.SHAPES[shape](w, monkeypatch)
    try:
        shared.check(e, w, w.want, shape + ", private code pages", retired=retired)
    finally:
        e.close()


def test_corpus_breakpoints_from_private_pages(monkeypatch):
    """The corpus's breakpoints (want_bp), followed through the host's resume,
    with half the lanes stopping in slow_step."""
    monkeypatch.setenv("WTFGPU_REGROUP_STEPS", "0")
    case = shared.INT_A
    if case not in _CORPUS:
        _CORPUS[case] = shared.Workload(case, private_code=True)
    w = _CORPUS[case]
    want = w.want_bp()
    assert sum(len(x["stops"]) for x in want) > w.n
    e = shared.make_engine(w, breakpoints=w.breakpoints())
    try:
        pos = [0] * w.n
        bad = []
        retired = 0
        for _ in range(shared.LIMIT):
            retired += e.run().lane_retired
            ex = e.exits_np()
            stopped = [int(i) for i in np.flatnonzero(ex["status"] == EXIT_BREAKPOINT)]
            if not stopped:
                break
            g = e.read_gprs()
            for i in stopped:
                got = (int(ex["rip"][i]), int(ex["icount"][i]), [int(v) for v in g[i, :16]])
                stops = want[i]["stops"]
                if pos[i] >= len(stops) or got != stops[pos[i]]:
                    bad.append((i, pos[i], got, stops[pos[i]] if pos[i] < len(stops) else None))
                pos[i] += 1
            assert not bad, f"(lane, stop number, got, expected): {bad[:3]}"
            e.resume(stopped, [1] * len(stopped))
        else:
            raise AssertionError("lanes still stopping after every possible round")
        assert pos == [len(x["stops"]) for x in want]
        shared.check(e, w, want, "breakpoints, private code pages", retired=retired)
    finally:
        e.close()
