"""The device mutator on the GPU, through the C ABI: k_mutate_feeds against
tests/mutate_model.py bit for bit, read back with wtfgpu_read_feed_lanes.

The corpus is all five corpora of tests/test_device_mutate.py in one arena (50
entries; lengths 0..16380; zeros, 0xff, digits, random), the per-lane ncorpus
values 1, 2, 10, 23 and 50 mixed inside every wave. The context has 320 lanes:
k_mutate_feeds takes four testcases a block, so the lists of 1, 63, 64, 65 and
257 lanes give partial blocks, full ones, and both."""
import numpy as np
import pytest

from tests import mutate_model as M
from tests import spill_lib as S
from wtf_amd import abi

pytestmark = pytest.mark.gpu

NL = 320
SEED = 0xD1CE
NCS = [1, 2, 10, 23, 50]
HEAD, PTR, LEN, LEN_ARG = 1, 2, 8, 5  # the declared insert: rcx, rdx, r8, the fifth argument's home


@pytest.fixture(scope="module")
def corpus():
    return [e for entries in M.corpora().values() for e in entries]


@pytest.fixture(scope="module")
def eng(corpus):
    from wtf_amd.engine import Engine

    sp, r0, _ = S.space()
    e = Engine(0)
    pfns, blob = sp.phys()
    e.load_pool(pfns, blob)
    e.alloc_lanes(NL, overlay_pages=8, cov_entries=64)
    e.set_initial_state(r0)
    e.set_limit(1000)
    e.restore()
    e.corpus_alloc(len(corpus), sum(len(c) for c in corpus))
    assert [e.corpus_add(c) for c in corpus] == list(range(len(corpus)))
    yield e
    e.close()


def lane_lists(n):
    """Ascending from 0, and sparse in no order."""
    sparse = np.random.default_rng(n).permutation(NL)[:n]
    return {"ascending": np.arange(n), "sparse": sparse}


def orders(n, salt):
    """Per-lane (index, ncorpus): indices far apart and not in lane order."""
    idx = [(i * 0x9E37 + salt * 1000003) % (1 << 20) + ((1 << 40) if i % 5 == 0 else 0) for i in range(n)]
    ncs = [NCS[(i * 3 + salt) % len(NCS)] for i in range(n)]
    return idx, ncs


@pytest.mark.parametrize("max_len", [4, 1028, 16380])
def test_kernel_matches_the_model(eng, corpus, max_len):
    for n in (1, 63, 64, 65, 257):
        for style, lanes in lane_lists(n).items():
            idx, ncs = orders(n, n + len(style))
            eng.mutate_feed_lanes(lanes, SEED, idx, ncs, max_len)
            got = eng.read_feed_lanes(lanes, stride=max_len)
            want = [M.testcase(SEED, g, corpus, nc, max_len) for g, nc in zip(idx, ncs)]
            bad = [(i, int(lanes[i]), idx[i], ncs[i], None if g is None else len(g), len(w))
                   for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad, (n, style, bad[:5])


def test_read_back_reports_the_size_beyond_the_stride(eng, corpus):
    """lens is the chunk's size; the bytes are cut to the caller's stride."""
    import ctypes as C
    lanes = np.array([7, 300], dtype=np.uint32)
    idx, ncs = [11, 12], [50, 50]
    eng.mutate_feed_lanes(lanes, SEED, idx, ncs, 16380)
    want = [M.testcase(SEED, g, corpus, 50, 16380) for g in idx]
    lens = np.zeros(2, dtype=np.uint32)
    out = np.zeros((2, 3), dtype=np.uint8)
    rc = eng.L.wtfgpu_read_feed_lanes(eng.ctx, lanes.ctypes.data_as(C.POINTER(C.c_uint32)), 2,
                                      lens.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.c_void_p), 3)
    assert rc == 0 and lens.tolist() == [len(w) for w in want]
    assert [out[i, :min(3, len(w))].tobytes() for i, w in enumerate(want)] == [w[:3] for w in want]


def test_an_index_gives_the_same_bytes_on_any_lane_and_queue(eng, corpus):
    g, nc, max_len = 123456, 50, 1028
    want = M.testcase(SEED, g, corpus, nc, max_len)
    eng.select_queue(0)
    eng.mutate_feed_lanes([1, 2, 3, 4], SEED, [9, 8, g, 7], [nc] * 4, max_len)
    first = eng.read_feed_lanes([3], stride=max_len)[0]
    eng.select_queue(1)
    try:
        eng.mutate_feed_lanes([200], SEED, [g], [nc], max_len)
        second = eng.read_feed_lanes([200], stride=max_len)[0]
    finally:
        eng.select_queue(0)
    assert first == want and second == want


def _pick(corpus, max_len, sizes, nc=50):
    """Indices whose testcases have the sizes asked for, found with the model."""
    found = {}
    for g in range(100000):
        n = len(M.testcase(SEED, g, corpus, nc, max_len))
        for s in sizes:
            if s not in found and (n == s if isinstance(s, int) else s[0] <= n <= s[1]):
                found[s] = g
        if len(found) == len(sizes):
            return [found[s] for s in sizes]
    raise AssertionError(f"no index for {set(sizes) - set(found)}")


def test_insert_after_mutation_equals_insert_after_upload(eng, corpus):
    """Lanes A get their testcases from the device mutator, lanes B the model's
    bytes through wtfgpu_set_feed_lanes; the declared insert runs after both.
    Sizes 1, 2, 3 (left alone), 4 (a head, no payload), 5, and payloads of a few
    hundred bytes, written 40 bytes below a page edge on every other lane; a
    second round with max_len 0 gives the empty testcase."""
    max_len = 1028
    sizes = [1, 2, 3, 4, 5, (300, 600), (900, 1027), 1028]
    idx = _pick(corpus, max_len, sizes)
    n = len(idx)
    A, B = np.arange(10, 10 + n), np.arange(150, 150 + n)
    want = [M.testcase(SEED, g, corpus, 50, max_len) for g in idx]
    eng.set_insert(HEAD, PTR, LEN, LEN_ARG)
    try:
        for round_, (mx, ix, tcs) in enumerate([(max_len, idx, want), (0, idx, [b""] * n)]):
            eng.restore()
            g0 = eng.read_gprs()
            for i in range(n):
                ptr = S.DATA_VA + 0x2000 * (i % 3) + (0x1000 - 40 if i % 2 == 0 else 0x100)
                g0[A[i], PTR] = g0[B[i], PTR] = ptr
            eng.write_gprs(g0)
            eng.mutate_feed_lanes(A, SEED, ix, [50 if mx else 1] * n, mx)
            eng.set_feed_lanes(B, tcs)
            after = eng.read_gprs()
            assert eng.read_feed_lanes(A, stride=max_len) == tcs
            da, db = eng.dirty_list(A), eng.dirty_list(B)
            for i, t in enumerate(tcs):
                a, b = int(A[i]), int(B[i])
                assert after[a].tolist() == after[b].tolist(), (round_, i, len(t))
                assert da[i, :da[i, 0] + 1].tolist() == db[i, :db[i, 0] + 1].tolist(), (round_, i, len(t))
                if len(t) >= 4:  # inserted: head, payload, its size in the register and in the argument's home
                    assert int(after[a, HEAD]) == int.from_bytes(t[:4], "little")
                    assert int(after[a, LEN]) == len(t) - 4
                    ptr = int(after[a, PTR])
                    assert eng.read_virt(a, ptr, len(t) - 4) == t[4:] == eng.read_virt(b, ptr, len(t) - 4)
                    home = int(after[a, 4]) + 8 + 8 * LEN_ARG
                    assert eng.read_virt(a, home, 8) == (len(t) - 4).to_bytes(8, "little")
                    assert int(da[i, 0]) >= 1
                else:  # left alone
                    assert after[a].tolist() == g0[a].tolist() and int(da[i, 0]) == 0
    finally:
        eng.L.wtfgpu_set_insert(eng.ctx, None)


def test_argument_errors_queue_nothing(corpus):
    """ncorpus 0, ncorpus above the entries added, max_len 16381, a lane out of
    range, no arena: WTFGPU_ERR_INVALID, and the lane still has no feed. A full
    arena: WTFGPU_ERR_FULL, by entries and by bytes, the arena unchanged."""
    from wtf_amd.engine import DeviceCorpusFull, Engine

    sp, r0, _ = S.space()
    e = Engine(0)
    try:
        pfns, blob = sp.phys()
        e.load_pool(pfns, blob)
        e.alloc_lanes(NL, overlay_pages=2, cov_entries=64)
        e.set_initial_state(r0)
        e.restore()
        assert e.mutate_feed_lanes_rc([5], SEED, [0], [1], 64) == abi.ERR_INVALID  # no arena
        e.corpus_alloc(2, 64)
        assert e.mutate_feed_lanes_rc([5], SEED, [0], [1], 64) == abi.ERR_INVALID  # no entry yet
        assert e.corpus_add(b"A" * 40) == 0
        with pytest.raises(DeviceCorpusFull):
            e.corpus_add(b"B" * 25)  # 65 bytes
        assert e.corpus_add(b"B" * 24) == 1
        with pytest.raises(DeviceCorpusFull):
            e.corpus_add(b"")  # a third entry
        for lanes, ncs, max_len in (([5, 6], [1, 0], 64), ([5, 6], [3, 1], 64), ([5], [1], abi.FEED_STRIDE - 3),
                                    ([5, NL], [1, 1], 64)):
            assert e.mutate_feed_lanes_rc(lanes, SEED, [0] * len(lanes), ncs, max_len) == abi.ERR_INVALID
        assert e.read_feed_lanes([5, 6]) == [None, None]
        e.mutate_feed_lanes([5, 6], SEED, [0, 1], [2, 2], abi.FEED_STRIDE - 4)
        two = [b"A" * 40, b"B" * 24]
        assert e.read_feed_lanes([5, 6, 7]) == [M.testcase(SEED, 0, two, 2, 16380), M.testcase(SEED, 1, two, 2, 16380),
                                                None]
        e.corpus_alloc(0, 0)
        assert e.mutate_feed_lanes_rc([5], SEED, [0], [1], 64) == abi.ERR_INVALID
    finally:
        e.close()


# ---- campaigns: `wtfgpu fuzz --device-mutate` on the HEVD target
import json  # noqa: E402
import os  # noqa: E402
import shutil  # noqa: E402

from tests import tlv_harness as H  # noqa: E402

HEVD_KW = dict(name="hevd", lanes=512, limit=10_000_000, max_len=1028, seed=1337)


@pytest.fixture(scope="module")
def hevd_base(tmp_path_factory):
    return H.build_hevd_target(str(tmp_path_factory.mktemp("hevd") / "base"))


def _campaign(base, d, runs, extra=()):
    shutil.copytree(base, d, ignore=shutil.ignore_patterns("outputs", "crashes", "work", "errors"))
    st = H.fuzz(H.WTFGPU, d, runs=runs, extra=("--device-mutate", *extra), timeout=300, **HEVD_KW)
    files = tuple(sorted(os.listdir(os.path.join(d, sub))) if os.path.isdir(os.path.join(d, sub)) else []
                  for sub in ("outputs", "crashes", "errors"))
    return st, files


def test_campaign_reproduces(hevd_base, tmp_path):
    (a, fa), (b, fb) = (_campaign(hevd_base, str(tmp_path / k), 8192) for k in ("one", "two"))
    assert {k: a[k] for k in H.STREAM_KEYS} == {k: b[k] for k in H.STREAM_KEYS}
    assert fa == fb
    assert a["execs"] == 8192 and a["errors"] == 0 and a["device_mutate"] == 1
    assert any(n.startswith("crash-0x") for n in fa[1]), fa[1]
    be = a["backend"]
    print({k: a[k] for k in H.STREAM_KEYS}, "readback_tcs", be["readback_tcs"], "mutate_dev_ms", be["mutate_dev_ms"],
          "up_feed_ms", be["up_feed_ms"], "device_corpus_dropped", a["device_corpus_dropped"])
    assert 0 < be["readback_tcs"] < a["execs"]
    assert a["device_corpus_dropped"] == 0


def test_what_was_read_back_is_what_ran(hevd_base, tmp_path):
    """Every testcase of a 2,048-run campaign sampled: the bytes the device
    handed back, replayed alone on the twin, give the result, crash name,
    retired count and registers the lane reported."""
    sample = str(tmp_path / "sample.jsonl")
    st, _ = _campaign(hevd_base, str(tmp_path / "c"), 2048, extra=("--sample", sample, "--sample-every", "1"))
    assert st["execs"] == 2048 and st["errors"] == 0
    # the first fill of the 512 lanes happens before any result, so before there
    # is a corpus: those are the inputs and repeats of them, as bytes; every
    # later testcase is made on the device, and sampled, so read back
    assert st["backend"]["readback_tcs"] == 2048 - HEVD_KW["lanes"]
    with open(sample) as f:
        got = [json.loads(line) for line in f]
    assert len(got) == 2048
    inp = str(tmp_path / "replay")
    os.makedirs(inp)
    for i, g in enumerate(got):
        with open(os.path.join(inp, f"s{i:06d}"), "wb") as f:
            f.write(bytes.fromhex(g["tc"]))
    want = H.run(H.TWIN, hevd_base, inp, str(tmp_path / "twin.jsonl"), lanes=1024, limit=10_000_000, name="hevd",
                 timeout=600)
    assert len(want) == len(got)
    bad = [(i, k, g[k], w[k]) for i, (g, w) in enumerate(zip(got, want))
           for k in ("result", "crash", "error", "icount", "gprs") if g[k] != w[k]]
    assert not bad, f"{len(bad)} differ; first: {bad[:5]}"
    assert {g["result"] for g in got} >= {"ok", "crash"}
    assert max(len(g["tc"]) for g in got) <= 2 * 1028
