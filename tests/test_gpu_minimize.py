"""The minimiser on the GPU: k_minimize_feeds against tests/minimize_model.py
through the C ABI, the declared insert after it, the argument checks, and
`wtfgpu minimize` against `wtf_twin minimize` byte for byte.

The context has 320 lanes: k_minimize_feeds takes four candidates a block, so
lists of 1, 63, 64, 65 and 257 lanes give partial blocks, full ones, and both.
Every list mixes the levels of its base inside each wave."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import minimize_model as M
from tests import spill_lib as S
from tests import tlv_harness as H
from tests.hevd_inputs import crafted
from wtf_amd import abi

pytestmark = pytest.mark.gpu

NL = 320
BYTE_BASES = [1, 4, 5, 65, 257, 1028, 16380]
FEED_BASES = [1, 2, 33, 64]
HEAD, PTR, LEN, LEN_ARG = 1, 2, 8, 5  # the declared insert: rcx, rdx, r8, the fifth argument's home
OPS = {M.REMOVE: abi.MIN_REMOVE, M.ZERO: abi.MIN_ZERO}


def make_engine(overlay_pages=8):
    from wtf_amd.engine import Engine

    sp, r0, _ = S.space()
    e = Engine(0)
    pfns, blob = sp.phys()
    e.load_pool(pfns, blob)
    e.alloc_lanes(NL, overlay_pages=overlay_pages, cov_entries=64)
    e.set_initial_state(r0)
    e.set_limit(1000)
    e.restore()
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


@pytest.fixture
def byte_arena(eng):
    """Entry i: M.byte_base(BYTE_BASES[i]); odd lengths leave later entries unaligned."""
    bases = [M.byte_base(n, n) for n in BYTE_BASES]
    eng.corpus_alloc(len(bases), sum(len(b) for b in bases))
    assert [eng.corpus_add(b) for b in bases] == list(range(len(bases)))
    return bases


@pytest.fixture
def feed_arena(eng):
    feeds = [M.feed_base(n, n) for n in FEED_BASES]
    eng.corpus_alloc(len(feeds), sum(len(f) + 8 + 4 * n + 4 for f, n in zip(feeds, FEED_BASES)))
    assert [eng.corpus_add_feed(f) for f in feeds] == list(range(len(feeds)))
    return feeds


def lane_lists(n):
    sparse = np.random.default_rng(n).permutation(NL)[:n]
    return {"ascending": np.arange(n), "sparse": sparse}


def mixed_indices(U, n, salt):
    """n indices of a base of U units, neighbours on different levels."""
    lv, starts, at = M.levels(U), [], 0
    for _, c in lv:
        starts.append(at)
        at += c
    return [starts[(i + salt) % len(lv)] + (i * 7 + salt * 13) % lv[(i + salt) % len(lv)][1] for i in range(n)]


@pytest.mark.parametrize("entry", range(len(BYTE_BASES)), ids=[str(n) for n in BYTE_BASES])
def test_kernel_matches_the_model_on_byte_buffers(eng, byte_arena, entry):
    base = byte_arena[entry]
    for op in (M.REMOVE, M.ZERO):
        for n in (1, 63, 64, 65, 257):
            for style, lanes in lane_lists(n).items():
                idx = mixed_indices(len(base), n, n + len(style) + op)
                eng.minimize_feed_lanes(lanes, entry, OPS[op], idx)
                got = eng.read_feed_lanes(lanes, stride=max(len(base), 4))
                want = [M.candidate(base, op, i) for i in idx]
                bad = [(i, int(lanes[i]), idx[i], None if g is None else len(g), len(w))
                       for i, (g, w) in enumerate(zip(got, want)) if g != w]
                assert not bad, (len(base), op, n, style, bad[:5])


@pytest.mark.parametrize("entry", range(len(FEED_BASES)), ids=[str(n) for n in FEED_BASES])
def test_kernel_matches_the_model_on_feeds(eng, feed_arena, entry):
    feed = feed_arena[entry]
    for n in (1, 63, 64, 65, 257):
        for style, lanes in lane_lists(n).items():
            idx = mixed_indices(FEED_BASES[entry], n, n + len(style))
            eng.minimize_feed_lanes(lanes, entry, abi.MIN_REMOVE, idx)
            got = eng.read_whole_feed_lanes(lanes, stride=max(len(feed), 4))
            want = [M.candidate_feed(feed, i) for i in idx]
            bad = [(i, int(lanes[i]), idx[i], None if g is None else len(g), len(w))
                   for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad, (FEED_BASES[entry], n, style, bad[:5])


def test_an_index_gives_the_same_bytes_on_any_lane_and_queue(eng, byte_arena):
    entry = BYTE_BASES.index(1028)
    base = byte_arena[entry]
    g = M.total(1028) - 700
    for op in (M.REMOVE, M.ZERO):
        want = M.candidate(base, op, g)
        eng.select_queue(0)
        eng.minimize_feed_lanes([1, 2, 3, 4], entry, OPS[op], [9, g, g, 7])
        first = eng.read_feed_lanes([2, 3], stride=1028)
        eng.select_queue(1)
        try:
            eng.minimize_feed_lanes([200], entry, OPS[op], [g])
            second = eng.read_feed_lanes([200], stride=1028)[0]
        finally:
            eng.select_queue(0)
        assert first == [want, want] and second == want


def test_insert_after_candidates_equals_insert_after_upload(eng, byte_arena):
    """Lanes A get candidates from the kernel, lanes B the model's bytes through
    wtfgpu_set_feed_lanes; the declared insert runs after both. Results of 4 and
    5 bytes (a head alone, a head and one byte) and of a thousand; payloads are
    written 40 bytes below a page edge on every other lane."""
    groups = []
    for U, op in ((5, M.REMOVE), (5, M.ZERO), (65, M.REMOVE), (1028, M.REMOVE), (1028, M.ZERO)):
        entry = BYTE_BASES.index(U)
        T = M.total(U)
        idx = sorted({0, 1, T // 2, T - U, T - 1} | set(mixed_indices(U, 6, U + op)))
        groups.append((entry, op, idx))
    sizes = set()
    eng.set_insert(HEAD, PTR, LEN, LEN_ARG)
    try:
        for entry, op, idx in groups:
            base = byte_arena[entry]
            n = len(idx)
            A, B = np.arange(10, 10 + n), np.arange(150, 150 + n)
            tcs = [M.candidate(base, op, i) for i in idx]
            sizes |= {len(t) for t in tcs}
            eng.restore()
            g0 = eng.read_gprs()
            for i in range(n):
                ptr = S.DATA_VA + 0x2000 * (i % 3) + (0x1000 - 40 if i % 2 == 0 else 0x100)
                g0[A[i], PTR] = g0[B[i], PTR] = ptr
            eng.write_gprs(g0)
            eng.minimize_feed_lanes(A, entry, OPS[op], idx)
            eng.set_feed_lanes(B, tcs)
            after = eng.read_gprs()
            assert eng.read_feed_lanes(A, stride=1028) == tcs
            da, db = eng.dirty_list(A), eng.dirty_list(B)
            for i, t in enumerate(tcs):
                a, b = int(A[i]), int(B[i])
                assert after[a].tolist() == after[b].tolist(), (entry, op, i, len(t))
                assert da[i, :da[i, 0] + 1].tolist() == db[i, :db[i, 0] + 1].tolist(), (entry, op, i, len(t))
                if len(t) >= 4:
                    assert int(after[a, HEAD]) == int.from_bytes(t[:4], "little")
                    assert int(after[a, LEN]) == len(t) - 4
                    ptr = int(after[a, PTR])
                    assert eng.read_virt(a, ptr, len(t) - 4) == t[4:] == eng.read_virt(b, ptr, len(t) - 4)
                else:  # left alone
                    assert after[a].tolist() == g0[a].tolist() and int(da[i, 0]) == 0
    finally:
        eng.L.wtfgpu_set_insert(eng.ctx, None)
    assert {4, 5} <= sizes and max(sizes) > 1000 and min(sizes) < 4


def test_argument_errors_queue_nothing():
    e = make_engine(overlay_pages=2)
    try:
        rm, zero = abi.MIN_REMOVE, abi.MIN_ZERO
        assert e.minimize_feed_lanes_rc([5], 0, rm, [0]) == abi.ERR_INVALID  # no arena
        e.corpus_alloc(4, 1 << 16)
        assert e.minimize_feed_lanes_rc([5], 0, rm, [0]) == abi.ERR_INVALID  # no entry yet
        assert e.corpus_add(M.byte_base(9)) == 0 and e.corpus_add(b"") == 1
        assert e.corpus_add(bytes(abi.FEED_STRIDE - 3)) == 2  # longer than a region's chunk
        T = M.total(9)
        for lanes, entry, op, idx in (([5, 6], 3, rm, [0, 0]),       # an entry not added
                                      ([5, 6], 0, rm, [0, T]),       # an index at T(U)
                                      ([5, 6], 0, zero, [T - 1, 1 << 40]),
                                      ([5], 1, rm, [0]),             # T(0) = 0: no index exists
                                      ([5], 2, rm, [0]),             # the entry does not fit a region
                                      ([5, NL], 0, rm, [0, 0]),      # a lane outside the context
                                      ([5], 0, 2, [0]),              # an unknown op
                                      (None, 0, rm, [0]), ([5], 0, rm, None)):  # null pointers
            assert e.minimize_feed_lanes_rc(lanes, entry, op, idx) == abi.ERR_INVALID, (lanes, entry, op, idx)
        assert e.read_feed_lanes([5, 6]) == [None, None]
        e.minimize_feed_lanes([5, 6], 0, zero, [0, T - 1])
        assert e.read_feed_lanes([5, 6, 7]) == [M.candidate(M.byte_base(9), M.ZERO, 0),
                                                M.candidate(M.byte_base(9), M.ZERO, T - 1), None]
        # an arena of feeds: REMOVE works, ZERO is a state error and leaves the feed as it was
        e.corpus_alloc(2, 1 << 16)
        feed = M.feed_base(5)
        assert e.corpus_add_feed(feed) == 0
        e.minimize_feed_lanes([5], 0, rm, [0])
        before = e.read_whole_feed_lanes([5, 7])
        assert before == [M.candidate_feed(feed, 0), None]
        assert e.minimize_feed_lanes_rc([5, 7], 0, zero, [1, 1]) == abi.ERR_STATE
        assert e.minimize_feed_lanes_rc([5, 7], 0, rm, [M.total(5), 0]) == abi.ERR_INVALID
        assert e.read_whole_feed_lanes([5, 7]) == before
        e.corpus_alloc(0, 0)
        assert e.minimize_feed_lanes_rc([5], 0, rm, [0]) == abi.ERR_INVALID
    finally:
        e.close()


# ---- `wtfgpu minimize` against `wtf_twin minimize`

KEYS = ("input_bytes", "output_bytes", "rounds", "remove_rounds", "zero_rounds", "candidates", "skipped", "crash",
        "stopped_by_rounds")


def minimize(exe, target, name, src, out, lanes, env=None):
    r = subprocess.run([exe, "minimize", "--name", name, "--target", target, "--input", src, "--output", out,
                        "--lanes", str(lanes), "--limit", "100000"], capture_output=True, text=True, timeout=300,
                       env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]), open(out, "rb").read()


def check_against_twin(target, name, src, tmp_path):
    want_st, want = minimize(H.TWIN, target, name, src, str(tmp_path / "twin.min"), 64)
    assert not want_st["on_device"]
    for tag, lanes, env, on_device in (("l64", 64, None, True), ("l4096", 4096, None, True),
                                       ("host", 4096, {"WTFGPU_MINIMIZE_HOST": "1"}, False)):
        st, got = minimize(H.WTFGPU, target, name, src, str(tmp_path / (tag + ".min")), lanes, env)
        print(tag, {k: st[k] for k in KEYS}, "seconds", st["seconds"], "upload_bytes", st["upload_bytes"])
        assert got == want, tag
        assert {k: st[k] for k in KEYS} == {k: want_st[k] for k in KEYS}, tag
        assert st["on_device"] is on_device, tag
    return want_st


@pytest.fixture(scope="module")
def hevd_target(tmp_path_factory):
    return H.build_hevd_target(str(tmp_path_factory.mktemp("hevd_min") / "base"))


@pytest.mark.parametrize("name", ["integer_wrap", "stack_ret_overrun", "stack_gs_cookie"])
def test_wtfgpu_minimize_equals_the_twin_on_hevd(hevd_target, tmp_path, name):
    data = crafted()[name]
    assert len(data) <= 1028
    src = str(tmp_path / name)
    with open(src, "wb") as f:
        f.write(data)
    st = check_against_twin(hevd_target, "hevd", src, tmp_path)
    assert st["rounds"] >= 2 and st["candidates"] > 10 * 64  # rounds far larger than 64 lanes


def test_wtfgpu_minimize_equals_the_twin_on_tlv(tmp_path):
    from tests.test_minimize import tlv_crash

    target = H.build_target(str(tmp_path / "tlv"))
    src = tlv_crash(target, tmp_path)
    st = check_against_twin(target, "tlv_server", src, tmp_path)
    assert st["remove_rounds"] >= 2 and st["zero_rounds"] == 0
