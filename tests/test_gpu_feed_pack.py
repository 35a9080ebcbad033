"""The packed feed read-back on the GPU, through the C ABI:
wtfgpu_read_feeds_packed (k_feed_lens, a 64-bit scan, k_feed_pack) against the
two strided calls it supersedes in the host path, against the mutators' models
and against tests/feed_pack_model.py's layout; then the campaigns of
`wtfgpu fuzz --device-packets` and `--device-mutate`, which read back through
it and only the results the session keeps.

The context is tests/test_gpu_device_packets.py's: 320 lanes on the synthetic
tlv snapshot. k_feed_pack takes four listed lanes a block, so the lists of 1,
63, 64, 65 and 257 lanes give partial blocks, full ones, and both."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from tests import feed_pack_model as F
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
    acts[0].gprs[0], acts[0].gprs[1] = 1, 2
    acts[1].gva, acts[1].kind = syms["ServerLoopReturn"], abi.BPACT_SET_GPRS
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
    """The feeds as they are (no size in front; None: the lane is left without
    a feed), through wtfgpu_set_feed_lanes; waits for the copy."""
    la = np.ascontiguousarray(lanes, dtype=np.uint32)
    off = np.zeros(len(la) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([0 if f is None else len(f) for f in feeds])
    has = bytes(0 if f is None else 1 for f in feeds)
    blob = b"".join(f for f in feeds if f is not None)
    assert e.L.wtfgpu_set_feed_lanes(e.ctx, la.ctypes.data_as(U32P), len(la), off.ctypes.data_as(U64P), has, blob,
                                     len(blob)) == 0
    e.read_whole_feed_lanes(la[:1], stride=4)  # a call that returns data waits for the queue: blob may go


def packed(e, lanes, whole=True):
    rc, lens, offs, buf, total, _ = e.read_feeds_packed_raw(lanes, whole)
    assert rc == 0
    return [int(x) for x in lens], [int(x) for x in offs], total, buf


def feeds_in(lens, offs, buf):
    return [None if n == F.NO_FEED else buf[o:o + n] for n, o in zip(lens, offs)]


def noise(n, salt):
    """n bytes, none of them zero: a zero in the packed buffer is padding."""
    return np.random.default_rng(salt).integers(1, 256, n, dtype=np.uint8).tobytes()


def lane_lists(n):
    sparse = np.random.default_rng(n).permutation(NL)[:n]
    return {"ascending": np.arange(n), "sparse": sparse}


def orders(n, salt):
    idx = [(i * 0x9E37 + salt * 1000003) % (1 << 20) + ((1 << 40) if i % 5 == 0 else 0) for i in range(n)]
    ncs = [NCS[(i * 3 + salt) % len(NCS)] for i in range(n)]
    return idx, ncs


@pytest.mark.parametrize("queue", [0, 1])
def test_packed_equals_strided_equals_model(eng, corpus, queue):
    eng.select_queue(queue)
    try:
        for n in (1, 63, 64, 65, 257):
            for style, lanes in lane_lists(n).items():
                idx, ncs = orders(n, n + len(style) + queue)
                eng.mutate_packets_lanes(lanes, SEED, idx, ncs, M.TLV)
                want = [M.testcase(SEED, g, corpus, nc) for g, nc in zip(idx, ncs)]
                strided = eng.read_whole_feed_lanes(lanes)
                lens, offs, total, buf = packed(eng, lanes)
                w_lens, w_offs, w_total, w_buf = F.pack(want)
                assert strided == want, (n, style)
                assert lens == w_lens and lens == [len(s) for s in strided], (n, style)
                assert offs == w_offs and total == w_total, (n, style)
                assert F.padding_is_zero(lens, offs, total, buf), (n, style)
                assert buf == w_buf, (n, style)
                assert eng.read_feeds_packed(lanes) == want, (n, style)
    finally:
        eng.select_queue(0)


def test_exact_lengths_by_upload(eng):
    """Feeds of every length around a 16-byte unit and the region's end, lanes
    without a feed between them, a lane listed twice; the lanes on both sides
    of the 16,384-byte one hold sentinels that fill their regions, so a copy
    that runs over its region's end, or its place's, shows."""
    sizes = [0, 1, 15, 16, 17, 4095, 16383, 16384]
    lanes = [20, 22, 24, 26, 28, 30, 32, 41]
    feeds = [noise(n, 100 + n) for n in sizes]
    sentinel = [bytes([0xA5 ^ k]) * F.STRIDE for k in (0, 1)]
    upload(eng, lanes + [40, 42] + [21, 23, 31], feeds + sentinel + [None, None, None])
    listed = [21, 20, 22, 23, 24, 26, 28, 26, 30, 31, 32, 40, 41, 42, 41, 21]
    by_lane = dict(zip(lanes + [40, 42, 21, 23, 31], feeds + sentinel + [None, None, None]))
    want = [by_lane[l] for l in listed]
    lens, offs, total, buf = packed(eng, listed)
    assert (lens, offs, total) == F.pack(want)[:3]
    assert F.padding_is_zero(lens, offs, total, buf)
    assert feeds_in(lens, offs, buf) == want
    assert eng.read_whole_feed_lanes(listed) == want
    assert eng.read_whole_feed_lanes([40, 42]) == sentinel  # the regions themselves are as uploaded


def test_first_chunks_without_their_size(eng):
    """whole = 0 is wtfgpu_read_feed_lanes packed: the chunk after its u32
    size, 4-aligned in the region, and the same clamp of a size word that
    claims more than the region holds."""
    sizes = [0, 1, 3, 4, 5, 17, 16380]
    lanes = [50, 51, 52, 53, 54, 55, 56]
    tcs = [noise(n, 200 + n) for n in sizes]
    eng.set_feed_lanes(lanes, tcs)
    liar = (0xFFFFFFF0).to_bytes(4, "little") + noise(F.STRIDE - 4, 999)
    upload(eng, [58, 57], [liar, None])
    listed = lanes + [57, 58, 56, 52]
    want = tcs + [None, liar[4:], tcs[6], tcs[2]]
    strided = eng.read_feed_lanes(listed)
    assert strided == want
    lens, offs, total, buf = packed(eng, listed, whole=False)
    assert lens == [F.NO_FEED if w is None else len(w) for w in want] and lens[8] == F.chunk_len(0xFFFFFFF0)
    assert (lens, offs, total) == F.pack(want)[:3]
    assert F.padding_is_zero(lens, offs, total, buf)
    assert feeds_in(lens, offs, buf) == strided
    assert eng.read_feeds_packed(listed, whole=False) == strided


def test_a_queues_buffer_lives_until_its_next_packed_read(eng):
    small = [noise(n, 300 + n) for n in (5, 33, 16)]
    upload(eng, [1, 2, 3], small)
    big_lanes = list(range(60, 60 + 257))
    eng.select_queue(0)
    rc, lens0, offs0, buf0, total0, ptr0 = eng.read_feeds_packed_raw([1, 2, 3])
    assert rc == 0 and feeds_in(lens0, offs0, buf0) == small
    eng.select_queue(1)
    try:
        big = [bytes([1 + i % 255]) * F.STRIDE for i in range(257)]
        upload(eng, big_lanes, big)
        rc, lens1, offs1, buf1, total1, ptr1 = eng.read_feeds_packed_raw(big_lanes)
        assert rc == 0 and total1 == 257 * F.STRIDE and ptr1 != ptr0
        assert feeds_in(lens1, offs1, buf1) == big
        assert C.string_at(ptr0, total0) == buf0  # queue 0's bytes, untouched by queue 1's read and growth
        rc, lens2, offs2, buf2, _, _ = eng.read_feeds_packed_raw([3, 1])  # after the growth
        assert rc == 0 and feeds_in(lens2, offs2, buf2) == [small[2], small[0]]
        assert C.string_at(ptr0, total0) == buf0
    finally:
        eng.select_queue(0)
    assert eng.read_feeds_packed([2]) == [small[1]]


def test_edge_arguments(eng):
    from tests import spill_lib as S
    from wtf_amd.engine import Engine

    assert eng.read_feeds_packed_raw([])[0::4] == (0, 0) and eng.read_feeds_packed([]) == []
    upload(eng, [5], [b"abc"])
    for bad in (dict(lanes=[5, NL]), dict(lanes=[5], whole=2), dict(lanes=[5], null_lens=True)):
        assert eng.read_feeds_packed_raw(**bad)[0] == abi.ERR_INVALID, bad
    assert eng.read_feeds_packed([5]) == [b"abc"]
    sp, r0, _ = S.space()
    e = Engine(0)
    try:  # a context before its first feed
        pfns, blob = sp.phys()
        e.load_pool(pfns, blob)
        e.alloc_lanes(NL, overlay_pages=2, cov_entries=64)
        e.set_initial_state(r0)
        e.restore()
        for whole in (False, True):
            rc, lens, offs, buf, total, _ = e.read_feeds_packed_raw([5, 6, 5], whole)
            assert (rc, list(lens), list(offs), buf, total) == (0, [F.NO_FEED] * 3, [0, 0, 0], b"", 0)
        assert e.read_feeds_packed_raw([NL])[0] == abi.ERR_INVALID
        assert e.read_feeds_packed([]) == []
    finally:
        e.close()


# ---- campaigns through `wtfgpu fuzz`: the harvest reads back packed, and only what the session keeps
def _campaign(base, d, flag, runs, **kw):
    shutil.copytree(base, d, ignore=shutil.ignore_patterns("outputs", "crashes", "work", "errors"))
    st = H.fuzz(H.WTFGPU, d, runs=runs, extra=(flag,), timeout=300, **kw)
    files = tuple(sorted(os.listdir(os.path.join(d, sub))) if os.path.isdir(os.path.join(d, sub)) else []
                  for sub in ("outputs", "crashes", "errors"))
    return st, files


def _reads_only_what_is_kept(base, tmp_path, flag, runs, **kw):
    (a, fa), (b, fb) = (_campaign(base, str(tmp_path / k), flag, runs, **kw) for k in ("one", "two"))
    be = a["backend"]
    print({k: a[k] for k in H.STREAM_KEYS}, {k: be[k] for k in ("readback_tcs", "readback_bytes", "readback_ms",
                                                                 "readback_skipped")})
    assert {k: a[k] for k in H.STREAM_KEYS} == {k: b[k] for k in H.STREAM_KEYS}
    assert fa == fb
    assert a["execs"] == runs and a["errors"] == 0
    assert len(fa[0]) == a["corpus"] and len(fa[1]) == a["unique_crashes"] > 0
    assert be["readback_skipped"] > 0
    assert 0 < be["readback_tcs"] < a["crashes"]
    assert be["readback_tcs"] == b["backend"]["readback_tcs"] and be["readback_bytes"] == b["backend"]["readback_bytes"]
    assert 0 < be["readback_bytes"] <= be["readback_tcs"] * F.STRIDE and be["readback_bytes"] % 16 == 0
    return a


def test_packet_campaign_reads_only_what_is_kept(tmp_path_factory, tmp_path):
    """`wtfgpu fuzz --device-packets` on tlv, 512 lanes, seed 1337, 65,536 runs,
    twice: one campaign, and fewer testcases read back than crashes. Before the
    filter every crash was read (readback_tcs >= crashes).

    Why it must hold: a result is read for an engine error (none here), for new
    coverage (at most `coverage` results), or for a crash whose name the
    session did not know when its half was harvested. A name is unknown in one
    harvest only, since the results of a harvest are accounted before the next
    one, so it is read at most `lanes` times; with twice that for slack, reads
    < 2 * unique_crashes * lanes + coverage. `wtf_twin fuzz --device-packets`
    with the same arguments: crashes 10,420, unique_crashes 5, coverage 228,
    corpus 6: 10,420 > 2 * 5 * 512 + 228 = 5,348."""
    base = H.build_target(str(tmp_path_factory.mktemp("tlv") / "base"))
    a = _reads_only_what_is_kept(base, tmp_path, "--device-packets", 65536, name="tlv_server", lanes=512, seed=1337)
    assert a["device_packets"] == 1 and a["crashes"] > 2 * a["unique_crashes"] * 512 + a["coverage"]


HEVD_KW = dict(name="hevd", lanes=512, limit=10_000_000, max_len=1028, seed=1337)


def test_byte_buffer_campaign_reads_only_what_is_kept(tmp_path_factory, tmp_path):
    """The same on the HEVD look-alike with --device-mutate, at
    tests/test_gpu_device_mutate.py's 512 lanes.

    The twin check that fixes tlv's run count cannot be met here at a run count
    a test can afford: HEVD's crash names carry the faulting address, so
    `wtf_twin fuzz --device-mutate` with these arguments gives, at 65,536 /
    262,144 / 1,048,576 runs, crashes 9,309 / 37,645 / 151,006 against
    unique_crashes 651 / 1,812 / 4,032 (coverage 723, corpus 18 at each): the
    names keep coming, and 2 * unique_crashes * lanes + coverage is 667,347 /
    1,856,211 / 4,129,491, 72, 49 and 27 times the crashes; the last of these
    takes the twin a minute. The worst case behind that bound, a full slice of
    lanes crashing with one new name, is what the factor `lanes` pays for, and
    with names this fine nearly every one is first seen on one lane. So the
    run count is tlv's, the assertions are the same, and here the inequality
    is asserted without the twin's condition behind it: reads are new-name
    crashes (the twin: 651 names among 9,309 crashes) plus at most `coverage`
    new-coverage results."""
    base = H.build_hevd_target(str(tmp_path_factory.mktemp("hevd") / "base"))
    a = _reads_only_what_is_kept(base, tmp_path, "--device-mutate", 65536, **HEVD_KW)
    assert a["device_mutate"] == 1
