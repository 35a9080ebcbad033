"""The device packet mutator on the GPU, through the C ABI: k_mutate_packets
against tests/packet_mutate_model.py bit for bit, read back with
wtfgpu_read_whole_feed_lanes, on the synthetic tlv snapshot with its three
breakpoint actions (ProcessPacket: Feed, the return address: SetGprs, printf:
SimulateReturn), so that a lane runs the feed it was given.

The corpus is tests/test_device_packets.py's (0 to 64 packets, chunks of
0x1000 bytes, insert-copy results of exactly 16384 and of 16385 bytes), the
per-lane ncorpus values mixed inside every wave. The context has 320 lanes:
k_mutate_packets takes four testcases a block, so the lists of 1, 63, 64, 65
and 257 lanes give partial blocks, full ones, and both.

feed_pos and feed_end have no accessor of their own. feed_end is the length
wtfgpu_read_whole_feed_lanes reports; feed_pos is checked by running: the lanes
are reused from test to test with their feeds consumed (feed_pos at the end),
and a lane whose position the kernel had not put back to its region's first
byte would run a different testcase than the lane that got the same bytes by
upload."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import packet_mutate_model as M
from tests import tlv_harness as H
from wtf_amd import abi

pytestmark = pytest.mark.gpu

NL = 320
SEED = 0xD1CE
NCS = [1, 3, 7, 9, 12]
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def corpus():
    return M.corpus()


@pytest.fixture(scope="module")
def eng(corpus, tmp_path_factory):
    from wtf_amd.engine import Engine
    from wtf_amd.tools import tlv

    sp, st, symbols, syms = tlv.space(str(tmp_path_factory.mktemp("tlvspace")))
    e = Engine(0)
    pfns, blob = sp.phys()
    e.load_pool(pfns, blob)
    e.alloc_lanes(NL, overlay_pages=32, cov_entries=1024)
    r0 = abi.regs_from_state(st)
    e.set_initial_state(r0)
    e.set_limit(100000)
    e.set_code_pages([symbols["tlv_server!ProcessPacket"] >> 12])
    acts = (abi.BpAction * 3)()
    acts[0].gva, acts[0].kind, acts[0].value = symbols["tlv_server!ProcessPacket"], abi.BPACT_FEED, 0x1000
    acts[0].gprs[0], acts[0].gprs[1] = 1, 2  # the packet ends at rcx + 0x1000, its size goes to rdx
    acts[1].gva, acts[1].kind = syms["ServerLoopReturn"], abi.BPACT_SET_GPRS  # [rsp]: back into the receive loop
    for i in range(16):
        acts[1].gprs[i] = r0.gpr[i]
    acts[1].gprs[16] = r0.rip
    acts[2].gva, acts[2].kind, acts[2].value = symbols["tlv_server!printf"], abi.BPACT_RETURN, 0
    e.set_breakpoints([a.gva for a in acts])
    assert e.L.wtfgpu_set_breakpoint_actions(e.ctx, acts, 3) == 0
    e.restore()
    e.corpus_alloc(64, 1 << 20)
    assert [e.corpus_add_feed(f) for f in corpus] == list(range(len(corpus)))
    yield e
    e.close()


def upload(e, lanes, feeds):
    """The feeds as they are (no size in front), through wtfgpu_set_feed_lanes; waits for the copy."""
    la = np.ascontiguousarray(lanes, dtype=np.uint32)
    off = np.zeros(len(la) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in feeds])
    blob = b"".join(feeds)
    assert e.L.wtfgpu_set_feed_lanes(e.ctx, la.ctypes.data_as(U32P), len(la), off.ctypes.data_as(U64P), None, blob,
                                     len(blob)) == 0
    e.read_whole_feed_lanes(la[:1], stride=4)  # a call that returns data waits for the queue: blob may go


def lane_lists(n):
    """Ascending from 0, and sparse in no order."""
    sparse = np.random.default_rng(n).permutation(NL)[:n]
    return {"ascending": np.arange(n), "sparse": sparse}


def orders(n, salt):
    """Per-lane (index, ncorpus): indices far apart and not in lane order."""
    idx = [(i * 0x9E37 + salt * 1000003) % (1 << 20) + ((1 << 40) if i % 5 == 0 else 0) for i in range(n)]
    ncs = [NCS[(i * 3 + salt) % len(NCS)] for i in range(n)]
    return idx, ncs


@pytest.fixture(scope="module")
def full_size(corpus):
    """Indices over the whole corpus whose results fill the region: an
    insert-copy of exactly 16384 bytes, and the 16384-byte base left alone."""
    found = {}
    for g in range(200000):
        out, what = M.mutate(SEED, g, corpus, len(corpus))
        if len(out) == M.MAX_FEED:
            found.setdefault("insert" if what == M.INSERT else "base", g)
            if len(found) == 2:
                return found
    raise AssertionError(found)


@pytest.mark.parametrize("queue", [0, 1])
def test_kernel_matches_the_model(eng, corpus, queue):
    seen = set()
    eng.select_queue(queue)
    try:
        for n in (1, 63, 64, 65, 257):
            for style, lanes in lane_lists(n).items():
                idx, ncs = orders(n, n + len(style) + queue)
                eng.mutate_packets_lanes(lanes, SEED, idx, ncs, M.TLV)
                got = eng.read_whole_feed_lanes(lanes)
                want = [M.mutate(SEED, g, corpus, nc) for g, nc in zip(idx, ncs)]
                seen |= {k for _, k in want}
                bad = [(i, int(lanes[i]), idx[i], ncs[i], M.WHAT[w[1]], None if g is None else len(g), len(w[0]))
                       for i, (g, w) in enumerate(zip(got, want)) if g != w[0]]
                assert not bad, (n, style, bad[:5])
    finally:
        eng.select_queue(0)
    assert seen >= {M.GENERATE, M.INSERT, M.INSERT_TOO_MANY, M.INSERT_TOO_LONG, M.COPY_ID, M.COPY_COMMAND,
                    M.COPY_BODY_SIZE, M.COPY_BODY, M.ERASE, M.ERASE_EMPTY}, [M.WHAT[k] for k in seen]


def test_no_byte_outside_the_lanes_region(eng, corpus, full_size):
    """Lanes 9 and 11 hold sentinel feeds that fill their regions; lane 10, between
    them, is ordered the 16384-byte insert-copy, lane 12 the 16384-byte base,
    lane 8 an empty feed's mutation. The sentinels are unchanged afterwards."""
    sentinel = [bytes([0xA5 ^ k]) * M.MAX_FEED for k in (0, 1)]
    upload(eng, [9, 11], sentinel)
    empty = next(g for g in range(1000) if M.mutate(SEED, g, corpus, 1)[1] == M.ERASE_EMPTY)
    lanes, idx, ncs = [10, 12, 8], [full_size["insert"], full_size["base"], empty], [len(corpus), len(corpus), 1]
    eng.mutate_packets_lanes(lanes, SEED, idx, ncs, M.TLV)
    got = eng.read_whole_feed_lanes([8, 9, 10, 11, 12])
    want = [M.testcase(SEED, g, corpus, nc) for g, nc in zip(idx, ncs)]
    assert [len(w) for w in want] == [M.MAX_FEED, M.MAX_FEED, 0]
    assert got[1] == sentinel[0] and got[3] == sentinel[1]
    assert (got[2], got[4], got[0]) == tuple(want)  # a feed of zero bytes is a feed: b"", not None


def test_an_index_gives_the_same_bytes_on_any_lane_and_queue(eng, corpus):
    g, nc = 123456, len(corpus)
    want = M.testcase(SEED, g, corpus, nc)
    eng.select_queue(0)
    eng.mutate_packets_lanes([1, 2, 3, 4], SEED, [9, 8, g, 7], [nc] * 4, M.TLV)
    first = eng.read_whole_feed_lanes([3])[0]
    eng.select_queue(1)
    try:
        eng.mutate_packets_lanes([200], SEED, [g], [nc], M.TLV)
        second = eng.read_whole_feed_lanes([200])[0]
    finally:
        eng.select_queue(0)
    assert first == want and second == want


def test_run_after_mutation_equals_run_after_upload(eng, corpus):
    """Lanes 0..159 get their feeds from the device mutator, lanes 160..319 the
    model's bytes through wtfgpu_set_feed_lanes; all 320 run. Exits, retired
    counts, registers, dirty lists and coverage are equal pair by pair."""
    n = NL // 2
    A, B = np.arange(n), np.arange(n, 2 * n)
    idx, ncs = orders(n, 41)
    want = [M.testcase(SEED, g, corpus, nc) for g, nc in zip(idx, ncs)]
    eng.restore()
    eng.coverage()  # empties the lanes' sets
    upload(eng, B, want)
    eng.mutate_packets_lanes(A, SEED, idx, ncs, M.TLV)
    assert eng.read_whole_feed_lanes(A) == want
    eng.run()
    ex = eng.exits_np()
    regs = eng.read_gprs()
    da, db = eng.dirty_list(A), eng.dirty_list(B)
    cov, overflow = eng.coverage()
    assert not overflow
    bad = []
    for i in range(n):
        a, b = int(A[i]), int(B[i])
        if ex[a].tolist() != ex[b].tolist() or regs[a].tolist() != regs[b].tolist() or \
                sorted(da[i, 1:da[i, 0] + 1].tolist()) != sorted(db[i, 1:db[i, 0] + 1].tolist()) or \
                da[i, 0] != db[i, 0] or cov.get(a, set()) != cov.get(b, set()):
            bad.append((i, idx[i], ncs[i], len(want[i]), ex[a].tolist(), ex[b].tolist()))
    assert not bad, bad[:3]
    # the lanes did run their packets: several retired counts, some coverage, and no lane left running
    assert len({int(x) for x in ex["icount"][:n]}) > 10 and cov
    assert not (ex["status"] == abi.RUNNING).any()


def test_argument_errors_queue_nothing(corpus):
    """Every WTFGPU_ERR_INVALID and WTFGPU_ERR_STATE case: nothing is queued (the
    lanes still have no feed) and the arena is unchanged (the next entry's
    index shows it)."""
    from tests import spill_lib as S
    from wtf_amd.engine import DeviceCorpusFull, Engine

    sp, r0, _ = S.space()
    e = Engine(0)
    try:
        pfns, blob = sp.phys()
        e.load_pool(pfns, blob)
        e.alloc_lanes(NL, overlay_pages=2, cov_entries=64)
        e.set_initial_state(r0)
        e.restore()
        good = M.feed_of([(1, 2, 3, b"abc"), (4, 5, 6, b"")])  # 27 bytes; its entry has 48
        mut = lambda lanes, ncs, params=M.TLV: e.mutate_packets_lanes_rc(lanes, SEED, [0] * len(lanes), ncs, params)  # noqa: E731
        assert mut([5], [1]) == abi.ERR_INVALID and e.corpus_add_feed_rc(good)[0] == abi.ERR_INVALID  # no arena
        e.corpus_alloc(2, 100)
        assert mut([5], [1]) == abi.ERR_INVALID  # no entry yet
        big = M.feed_of([(0, 0, 0, bytes(8192 - 12)), (0, 0, 0, bytes(8193 - 12))])
        assert len(big) == 16385
        for bad in (good[:-1], good[:14], struct_size7(), good + b"\0", big):
            assert e.corpus_add_feed_rc(bad) == (abi.ERR_INVALID, 0xffffffff)
        assert e.corpus_add_feed(good) == 0
        assert e.L.wtfgpu_corpus_add(e.ctx, b"x", 1, None) == abi.ERR_STATE  # an arena of feeds
        assert e.mutate_feed_lanes_rc([5], SEED, [0], [1], 64) == abi.ERR_STATE
        with pytest.raises(DeviceCorpusFull):
            e.corpus_add_feed(M.feed_of([(0, 0, 0, bytes(40))]))  # 48 + 64 bytes
        assert e.corpus_add_feed(good) == 1
        with pytest.raises(DeviceCorpusFull):
            e.corpus_add_feed(b"")  # a third entry
        for lanes, ncs in (([5, 6], [1, 0]), ([5, 6], [3, 1]), ([5, NL], [1, 1])):
            assert mut(lanes, ncs) == abi.ERR_INVALID
        for params in ((64, 11, 245, 3, 10), (0, 11, 100, 3, 10), (65, 11, 0, 3, 10), (10, 0, 100, 3, 10),
                       (10, 11, 100, 0, 10)):
            assert mut([5], [1], params) == abi.ERR_INVALID
        assert e.read_whole_feed_lanes([5, 6]) == [None, None]
        e.mutate_packets_lanes([5, 6], SEED, [0, 1], [2, 2], M.TLV)
        assert e.read_whole_feed_lanes([5, 6, 7]) == [M.testcase(SEED, 0, [good, good], 2),
                                                       M.testcase(SEED, 1, [good, good], 2), None]
        # an arena of byte buffers takes no feed and no packet orders
        e.corpus_alloc(2, 100)
        assert e.corpus_add(b"abcd") == 0
        assert e.corpus_add_feed_rc(good)[0] == abi.ERR_STATE and mut([7], [1]) == abi.ERR_STATE
        assert e.read_whole_feed_lanes([7]) == [None]
        e.corpus_alloc(0, 0)
        assert mut([5], [1]) == abi.ERR_INVALID
    finally:
        e.close()


def struct_size7():
    return (7).to_bytes(4, "little") + bytes(7)


# ---- campaigns: `wtfgpu fuzz --device-packets` on the tlv target
TLV_KW = dict(name="tlv_server", lanes=512, seed=1337)


@pytest.fixture(scope="module")
def tlv_base(tmp_path_factory):
    return H.build_target(str(tmp_path_factory.mktemp("tlv") / "base"))


def _campaign(base, d, runs, extra=()):
    shutil.copytree(base, d, ignore=shutil.ignore_patterns("outputs", "crashes", "work", "errors"))
    st = H.fuzz(H.WTFGPU, d, runs=runs, extra=("--device-packets", *extra), timeout=300, **TLV_KW)
    files = tuple(sorted(os.listdir(os.path.join(d, sub))) if os.path.isdir(os.path.join(d, sub)) else []
                  for sub in ("outputs", "crashes", "errors"))
    return st, files


def test_campaign_reproduces(tlv_base, tmp_path):
    (a, fa), (b, fb) = (_campaign(tlv_base, str(tmp_path / k), 8192) for k in ("one", "two"))
    assert {k: a[k] for k in H.STREAM_KEYS} == {k: b[k] for k in H.STREAM_KEYS}
    assert fa == fb
    assert a["execs"] == 8192 and a["errors"] == 0 and a["device_packets"] == 1 and a["device_mutate"] == 0
    be = a["backend"]
    print({k: a[k] for k in H.STREAM_KEYS}, "readback_tcs", be["readback_tcs"], "mutate_dev_ms", be["mutate_dev_ms"],
          "up_feed_ms", be["up_feed_ms"], "mutate_cpu_ms", a["mutate_cpu_ms"], "device_corpus_dropped",
          a["device_corpus_dropped"])
    assert a["corpus"] > 4 and len(fa[0]) == a["corpus"] and a["crashes"] > 0 and fa[1]
    assert 0 < be["readback_tcs"] < a["execs"]
    assert a["device_corpus_dropped"] == 0 and a["mutate_cpu_ms"] == 0


def test_what_was_read_back_is_what_ran(tlv_base, tmp_path):
    """Every testcase of a 2,048-run campaign sampled: the testcase made of the
    feed the device handed back, replayed alone on the twin, gives the result,
    crash name, retired count and registers the lane reported."""
    sample = str(tmp_path / "sample.jsonl")
    st, _ = _campaign(tlv_base, str(tmp_path / "c"), 2048, extra=("--sample", sample, "--sample-every", "1"))
    assert st["execs"] == 2048 and st["errors"] == 0
    # the first fill of the 512 lanes happens before any result, so before there
    # is a corpus: those are the inputs and repeats of them, as bytes; every
    # later testcase is made on the device, and sampled, so read back
    assert st["backend"]["readback_tcs"] == 2048 - TLV_KW["lanes"]
    with open(sample) as f:
        got = [json.loads(line) for line in f]
    assert len(got) == 2048
    inp = str(tmp_path / "replay")
    os.makedirs(inp)
    for i, g in enumerate(got):
        with open(os.path.join(inp, f"s{i:06d}"), "wb") as f:
            f.write(bytes.fromhex(g["tc"]))
    want = H.run(H.TWIN, tlv_base, inp, str(tmp_path / "twin.jsonl"), lanes=1024, timeout=600)
    assert len(want) == len(got)
    bad = [(i, k, g[k], w[k]) for i, (g, w) in enumerate(zip(got, want))
           for k in ("result", "crash", "error", "icount", "gprs") if g[k] != w[k]]
    assert not bad, f"{len(bad)} differ; first: {bad[:5]}"
    assert {g["result"] for g in got} >= {"ok", "crash"}
    assert all(bytes.fromhex(g["tc"]).startswith(b'{"Packets":[') for g in got)


def test_a_batch_run_on_the_device_executor_is_refused(tlv_base):
    r = subprocess.run([H.WTFGPU, "fuzz", "--name", "tlv_server", "--target", tlv_base, "--runs", "64", "--lanes", "64",
                        "--device-packets", "--slice-steps", "0"], capture_output=True, text=True, timeout=120)
    lines = [x for x in (r.stdout + r.stderr).splitlines() if "--device-packets" in x]
    assert r.returncode != 0 and len(lines) == 1 and "streaming run" in lines[0], r.stdout + r.stderr
    assert "--device-mutate" not in r.stdout + r.stderr
