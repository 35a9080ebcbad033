"""The analyzer on the GPU: k_analyze_feeds and k_cov_signature against
tests/analyze_model.py through the C ABI, and `wtfgpu analyze` against
`wtf_twin analyze` byte for byte.

The candidates: a context of 320 lanes; k_analyze_feeds takes MUT_WAVES
candidates a block, so lists of 1, MUT_WAVES - 1, MUT_WAVES, MUT_WAVES + 1 and
257 lanes give partial blocks, full ones, and both. The base sits at every
alignment in the arena (an entry of 1, 2 or 3 bytes before it).

The signatures: the 320-lane rig of tests/test_gpu_minimize_coverage.py, whose
64-slot tables k_run fills with empty sets, overflowed sets and, after a
restore and another run, slots of the earlier generation; and the same rig with
256-slot tables, where the scan takes four steps. The reference is the model's
signature over each lane's set as Engine.coverage() reads it."""
import json
import struct

import numpy as np
import pytest

from tests import analyze_model as M
from tests import covkeep_model as KM
from tests import tlv_harness as H
from tests.test_analyze import (CASES, COUNT_KEYS, analyze, base_of, byte_indices, feed_of, session_inputs)
from tests.test_gpu_minimize import NL, make_engine
from tests.test_gpu_minimize_coverage import COV_ENTRIES, Rig
from wtf_amd import abi

pytestmark = pytest.mark.gpu

MUT_WAVES = 4  # csrc/engine_kernels.h: candidates a block
BYTE_SIZES = [1, 3, 4, 5, 255, 256, 257, 16380]
LIST_SIZES = (1, MUT_WAVES - 1, MUT_WAVES, MUT_WAVES + 1, 257)
SIG_LISTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


def lane_lists(n):
    return {"ascending": np.arange(n), "sparse": np.random.default_rng(n).permutation(NL)[:n]}


def spread(indices, n, salt):
    """n of the indices, neighbours far apart."""
    return [indices[(i * 37 + salt * 11) % len(indices)] for i in range(n)]


def check_candidates(eng, base, entry, indices, feed, what):
    for n in LIST_SIZES:
        for style, lanes in lane_lists(n).items():
            idx = spread(indices, n, n + len(style))
            eng.analyze_feed_lanes(lanes, entry, idx)
            got = eng.read_whole_feed_lanes(lanes, stride=max(len(base) + 4, 8))
            want = [(b"" if feed else struct.pack("<I", len(base))) + M.candidate(base, i) for i in idx]
            bad = [(i, int(lanes[i]), idx[i], None if g is None else len(g), len(w))
                   for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad, (what, n, style, bad[:5])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("U", BYTE_SIZES)
def test_kernel_matches_the_model_on_byte_buffers(eng, U, shift):
    """The base at arena byte offset `shift`: whole-word loads only at shift 0."""
    base = base_of(U)
    eng.corpus_alloc(2, U + 4)
    entry = 0
    if shift:
        assert eng.corpus_add(b"\xee" * shift) == 0
        entry = 1
    assert eng.corpus_add(base) == entry
    ix = byte_indices(U)
    # the word that holds the last byte, and the byte on each side of a word edge
    ix += [4 * p + v for p in {U - 1, min(3, U - 1), min(4, U - 1), (U - 1) & ~3} for v in range(4)]
    check_candidates(eng, base, entry, ix, False, (U, shift))


@pytest.mark.parametrize("P", [1, 5])
def test_kernel_matches_the_model_on_feeds(eng, P):
    feeds = [feed_of(2), feed_of(P)]  # (an entry before it: the offsets are the entry's own)
    eng.corpus_alloc(2, sum(len(f) + 8 + 4 * 5 + 4 for f in feeds))
    assert [eng.corpus_add_feed(f) for f in feeds] == [0, 1]
    check_candidates(eng, feeds[1], 1, M.indices(feeds[1], feed=True), True, ("feed", P))


def test_an_index_gives_the_same_bytes_on_any_lane_and_queue(eng):
    base = base_of(257)
    eng.corpus_alloc(2, 300)
    assert eng.corpus_add(b"x") == 0 and eng.corpus_add(base) == 1
    g = 4 * 255 + 2
    want = struct.pack("<I", 257) + M.candidate(base, g)
    eng.select_queue(0)
    eng.analyze_feed_lanes([1, 2, 3, 4], 1, [9, g, g, 7])
    first = eng.read_whole_feed_lanes([2, 3], stride=264)
    eng.select_queue(1)
    try:
        eng.analyze_feed_lanes([200], 1, [g])
        second = eng.read_whole_feed_lanes([200], stride=264)[0]
    finally:
        eng.select_queue(0)
    assert first == [want, want] and second == want


def test_candidate_argument_errors_queue_nothing():
    e = make_engine(overlay_pages=2)
    try:
        assert e.analyze_feed_lanes_rc([5], 0, [0]) == abi.ERR_INVALID  # no arena
        e.corpus_alloc(4, 1 << 16)
        assert e.analyze_feed_lanes_rc([5], 0, [0]) == abi.ERR_INVALID  # no entry yet
        base = base_of(9)
        assert e.corpus_add(base) == 0 and e.corpus_add(b"") == 1
        assert e.corpus_add(bytes(abi.FEED_STRIDE - 3)) == 2  # longer than a region's chunk
        T = M.total(9)
        for lanes, entry, idx in (([5, 6], 3, [0, 0]),        # an entry not added
                                  ([5, 6], 0, [0, T]),        # an index at 4 * U
                                  ([5, 6], 0, [T - 1, 1 << 40]),
                                  ([5], 1, [0]),              # U = 0: no index exists
                                  ([5], 2, [0]),              # the entry does not fit a region
                                  ([5, NL], 0, [0, 0]),       # a lane outside the context
                                  (None, 0, [0]), ([5], 0, None)):  # null pointers
            assert e.analyze_feed_lanes_rc(lanes, entry, idx) == abi.ERR_INVALID, (lanes, entry, idx)
        assert e.read_whole_feed_lanes([5, 6]) == [None, None]
        e.analyze_feed_lanes([5, 6], 0, [0, T - 1])  # a valid call still works
        head = struct.pack("<I", 9)
        assert e.read_whole_feed_lanes([5, 6, 7]) == [head + M.candidate(base, 0), head + M.candidate(base, T - 1), None]
        # an arena of feeds: framing positions are refused, their neighbours are not
        e.corpus_alloc(2, 1 << 16)
        feed = feed_of(5)
        off = M.chunk_offsets(feed)
        assert e.corpus_add_feed(feed) == 0
        e.analyze_feed_lanes([5], 0, [4 * 4])
        before = e.read_whole_feed_lanes([5, 7])
        assert before == [M.candidate(feed, 16), None]
        for p in [o + k for o in off[:-1] for k in range(4)]:
            assert e.analyze_feed_lanes_rc([5, 7], 0, [4 * 4, 4 * p + 1]) == abi.ERR_INVALID, p
        assert e.analyze_feed_lanes_rc([5, 7], 0, [M.total(len(feed)), 16]) == abi.ERR_INVALID
        assert e.read_whole_feed_lanes([5, 7]) == before
        last = 4 * (len(feed) - 1) + 3
        e.analyze_feed_lanes([5, 7], 0, [4 * (off[1] - 1), last])
        assert e.read_whole_feed_lanes([5, 7]) == [M.candidate(feed, 4 * (off[1] - 1)), M.candidate(feed, last)]
        e.corpus_alloc(0, 0)
        assert e.analyze_feed_lanes_rc([5], 0, [16]) == abi.ERR_INVALID
    finally:
        e.close()


# ---- signatures

@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def check_signatures(eng, lanes, sets, ovf):
    sig, size, overflow = eng.coverage_signature(lanes)
    want = [M.sig(sets[l]) for l in lanes]
    assert [(int(s), int(n)) for s, n in zip(sig, size)] == want
    assert overflow.tolist() == [int(ovf[l]) for l in lanes]
    return want


def test_signature_matches_the_model(rig):
    eng = rig.eng
    rig.run(0)
    sets, ovf = rig.state()
    assert all(not sets[l] for l in rig.idle) and any(ovf) and not all(ovf)
    assert any(0 < len(s) < KM.cap(COV_ENTRIES) for s in sets) and len({frozenset(s) for s in sets}) >= 8
    for n in SIG_LISTS:
        for lanes in lane_lists(n).values():
            check_signatures(eng, lanes, sets, ovf)
    want = check_signatures(eng, np.arange(NL), sets, ovf)
    # lanes that ran the same path have the same signature, the others do not
    groups = {}
    for l in range(NL):
        groups.setdefault(frozenset(sets[l]), set()).add(want[l])
    assert all(len(g) == 1 for g in groups.values()) and len({next(iter(g)) for g in groups.values()}) == len(groups)
    assert all(want[l] == (0, 0) for l in rig.idle)
    after, _ = rig.state()
    assert after == sets  # the call reads the sets and leaves them


def test_slots_of_the_run_before_do_not_count(rig):
    eng = rig.eng
    rig.run(1)
    first, _ = rig.state()
    rig.run(2)
    sets, ovf = rig.state()
    assert sum(1 for l in range(NL) if first[l] - sets[l]) > NL // 4  # lanes lost values they had
    lanes = np.arange(NL)
    check_signatures(eng, lanes, sets, ovf)
    # the same after sets were emptied without a restore
    some = [l for l in range(NL) if sets[l]][:70]
    eng.clear_coverage_lanes(some)
    emptied = [set() if l in set(some) else sets[l] for l in range(NL)]
    check_signatures(eng, lanes, emptied, [False if l in set(some) else ovf[l] for l in range(NL)])


def test_signature_twice_and_on_both_queues_the_same(rig):
    eng = rig.eng
    rig.run(3)
    sets, ovf = rig.state()
    lanes = lane_lists(257)["sparse"]
    a = [x.tolist() for x in eng.coverage_signature(lanes)]
    b = [x.tolist() for x in eng.coverage_signature(lanes)]
    eng.select_queue(1)
    try:
        c = [x.tolist() for x in eng.coverage_signature(lanes)]
    finally:
        eng.select_queue(0)
    assert a == b == c
    check_signatures(eng, lanes, sets, ovf)


def test_signature_over_larger_tables():
    """256 slots: four steps a lane, no set fills up, and the early stop cuts
    the scan of a short set."""
    r = Rig(cov_entries=256)
    try:
        for salt in (5, 6):  # the second run leaves the first's slots behind
            r.run(salt)
            cov, any_ovf = r.eng.coverage()
            assert not any_ovf
            sets = [cov.get(l, set()) for l in range(NL)]
            assert max(len(s) for s in sets) > 64 and any(0 < len(s) < 30 for s in sets)
            for n in SIG_LISTS:
                for lanes in lane_lists(n).values():
                    check_signatures(r.eng, lanes, sets, [False] * NL)
            cov2, _ = r.eng.coverage()
            assert [cov2.get(l, set()) for l in range(NL)] == sets
    finally:
        r.close()


def test_signature_argument_errors_return_their_codes():
    r = Rig()
    try:
        eng = r.eng
        r.run(4)
        sets, ovf = r.state()
        assert eng.coverage_signature_rc(None)[0] == abi.ERR_INVALID
        assert eng.coverage_signature_rc([1, 2], want_out=False)[0] == abi.ERR_INVALID
        assert eng.coverage_signature_rc([1, NL])[0] == abi.ERR_INVALID
        assert eng.coverage_signature_rc([])[0] == 0
        check_signatures(eng, np.array([0, 1, 2, NL - 1]), sets, ovf)  # a valid call still works
        after, _ = r.state()
        assert after == sets
    finally:
        r.close()
    for kw in ({"cov_entries": 0}, {"lanes": 0}):  # coverage off; no lanes
        r = Rig(**kw)
        try:
            assert r.eng.coverage_signature_rc([0])[0] == abi.ERR_STATE, kw
        finally:
            r.close()


# ---- `wtfgpu analyze` against `wtf_twin analyze`

FEW = [(64, "device", "device", False), (4096, "device", "device", False), (4096, "host", "device", True),
       (4096, "device", "host", False)]
ALL = [(lanes, sig, cand, attrib) for lanes in (64, 4096) for sig in ("device", "host") for cand in ("device", "host")
       for attrib in (False, True)]
SESSIONS = [("hevd", "www_ok_pad", False, *c) for c in ALL] + \
           [(t, n, False, *c) for t, n in CASES if n != "www_ok_pad" for c in FEW] + \
           [("tlv_server", "multi", True, 4096, "device", "device", False)]


@pytest.fixture(scope="module")
def targets(tmp_path_factory):
    d = tmp_path_factory.mktemp("analyze_gpu")
    dirs = {"hevd": H.build_hevd_target(str(d / "hevd")), "tlv_server": H.build_target(str(d / "tlv"))}
    paths = {}
    for name, (_, data) in session_inputs().items():
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return dirs, paths


@pytest.fixture(scope="module")
def twin(targets, tmp_path_factory):
    """The twin's session, once an (input, edges) asked for."""
    d = tmp_path_factory.mktemp("analyze_twin")
    done = {}

    def get(tname, name, edges):
        if (name, edges) not in done:
            dirs, paths = targets
            done[(name, edges)] = analyze(H.TWIN, dirs[tname], tname, paths[name], str(d / f"{name}{int(edges)}.map"),
                                          extra=("--edges",) if edges else ())
        return done[(name, edges)]

    return get


@pytest.mark.parametrize("tname,name,edges,lanes,sig,cand,attrib", SESSIONS)
def test_wtfgpu_analyzes_as_the_twin_does(targets, twin, tmp_path, tname, name, edges, lanes, sig, cand, attrib):
    dirs, paths = targets
    want_st, want = twin(tname, name, edges)
    env = {"WTFGPU_COVSIG_HOST": "1" if sig == "host" else "0", "WTFGPU_ANALYZE_HOST": "1" if cand == "host" else "0"}
    extra = (("--edges",) if edges else ()) + (("--device-attrib",) if attrib else ())
    st, got = analyze(H.WTFGPU, dirs[tname], tname, paths[name], str(tmp_path / "gpu.map"), lanes=lanes, extra=extra,
                      env=env)
    print({k: st[k] for k in COUNT_KEYS}, "seconds", st["seconds"], "sig_readback_values", st["sig_readback_values"],
          "covlog_ms", st["executor"]["covlog_ms"], "attrib_ms", st["executor"]["attrib_ms"])
    assert got == want
    assert {k: st[k] for k in COUNT_KEYS} == {k: want_st[k] for k in COUNT_KEYS}
    assert st["sig_on_device"] is (sig == "device") and st["on_device"] is (cand == "device")
    values = json.loads(got)["base"]["values"]
    if sig == "device":
        assert st["sig_readback_values"] == values  # only the input's own set came back
    else:
        assert st["sig_readback_values"] > values
