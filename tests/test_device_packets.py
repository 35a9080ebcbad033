"""The device packet mutator's stream on the CPU: the definition in
wtf_amd/csrc/engine_mutate_packets.h, built for the host
(tests/native/sim_packets.cc), against its restatement in Python
(tests/packet_mutate_model.py), byte for byte; the tlv module's conversions
between a feed and the testcase it keeps; and `--device-packets` campaigns on
the twin, which materialises the orders on the host from the same header.

The corpus (packet_mutate_model.corpus()): 0, 1, 2, 10, 11, 12 and 64 packets;
bodies of 0, 1, 2, 3, 5, 100, 4083 and 4084 bytes; insert-copy results of
exactly 16384 and of 16385 bytes (the latter must be the base); a base of
16384 bytes; a copy-body that would pass 16384. ncorpus runs from 1 to the
whole corpus, 20,480 indices each: 204,800 testcases."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import packet_mutate_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")
HOSTLIB = os.path.join(ROOT, "wtf_amd", "host", "libwtfhost.a")
CXX = os.environ.get("CXX", "g++")
SEED = 0x5EED
COUNT = 20480
PARAMS = (*M.TLV, M.MAX_FEED)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """libsimpackets.so: tests/native/sim_packets.cc, built as test_device_mutate.py builds libsimmutate.so."""
    so = str(tmp_path_factory.mktemp("simpackets") / "libsimpackets.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_packets.cc")])
    L = C.CDLL(so)
    U32, U64 = C.c_uint32, C.c_uint64
    L.sim_packets_many.argtypes = [U64, C.POINTER(U64), U32, C.c_char_p, C.POINTER(U64), U32, C.POINTER(U32),
                                   C.c_void_p, U64, C.POINTER(U32), C.POINTER(U32)]
    L.sim_packets_many.restype = None
    L.sim_packets_params_valid.argtypes = [C.POINTER(U32)]
    L.sim_packets_entry_packets.argtypes = [C.c_char_p, U64, U32]
    L.sim_packets_entry_packets.restype = C.c_int64
    L.sim_packets_entry_bytes.argtypes = [U64, U64]
    L.sim_packets_entry_bytes.restype = U64
    L.sim_packets_entry_write.argtypes = [C.c_char_p, U64, U64, C.c_void_p]
    L.sim_packets_entry_write.restype = None
    return L


def native(L, corpus, indices, ncorpus, params=PARAMS, seed=SEED):
    """[(feed, what)] from the host build."""
    arena, off = M.pack(corpus)
    ix = np.ascontiguousarray(indices, dtype=np.uint64)
    n = len(ix)
    stride = params[5]
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    info = np.zeros((n, 2), dtype=np.uint32)
    L.sim_packets_many(seed, ix.ctypes.data_as(C.POINTER(C.c_uint64)), n, arena, (C.c_uint64 * len(off))(*off), ncorpus,
                       (C.c_uint32 * 6)(*params), out.ctypes.data_as(C.c_void_p), stride,
                       lens.ctypes.data_as(C.POINTER(C.c_uint32)), info.ctypes.data_as(C.POINTER(C.c_uint32)))
    return [(out[i, :lens[i]].tobytes(), int(info[i, 0])) for i in range(n)]


def checksum(outs):
    """As tests/test_device_mutate.py's (tests/native/sim_packets_main.cc prints the same)."""
    d = np.frombuffer(b"".join(struct.pack("<I", len(o)) + o for o in outs), dtype=np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        w = np.arange(1, len(d) + 1, dtype=np.uint64) * np.uint64(M.G)
        return int(((d + np.uint64(1)) * w).sum(dtype=np.uint64))


@pytest.fixture(scope="module")
def runs(sim):
    """Every case once, model and host build side by side: per ncorpus the
    first differences, how often each kind of testcase came up, the sizes that
    matter, the model's checksum, and a sample of the feeds for the round trip."""
    corpus = M.corpus()
    out = {}
    for nc in M.NCORPUS:
        want = [M.mutate(SEED, i, corpus, nc) for i in range(COUNT)]
        got = native(sim, corpus, range(COUNT), nc)
        diff = [(i, M.WHAT[w[1]], g[1], len(g[0]), len(w[0])) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        what = [0] * len(M.WHAT)
        for o, k in want:
            assert len(o) <= M.MAX_FEED
            what[k] += 1
        out[nc] = {"diff": diff[:5], "what": what,
                   "full_insert": sum(k == M.INSERT and len(o) == M.MAX_FEED for o, k in want),
                   "gen_packets": {len(M.packets_of(o)) for o, k in want if k == M.GENERATE},
                   "sum": checksum([o for o, _ in want]),
                   "feeds": [o for o, _ in want[:1024]]}
    return out


def test_host_build_matches_the_model(runs):
    assert len(runs) * COUNT >= 200_000
    bad = {k: v["diff"] for k, v in runs.items() if v["diff"]}
    assert not bad, bad


def test_the_cases_reach_every_operator_and_every_refusal(runs):
    what = [sum(v["what"][k] for v in runs.values()) for k in range(len(M.WHAT))]
    print(dict(zip(M.WHAT, what)), "insert-copies of 16384 bytes:", sum(v["full_insert"] for v in runs.values()))
    assert all(n >= 20 for n in what), dict(zip(M.WHAT, what))
    assert sum(v["full_insert"] for v in runs.values()) >= 1
    assert set().union(*(v["gen_packets"] for v in runs.values())) == set(range(1, 11))
    # alone, the empty feed: generated testcases and the three refusals on no packets
    one = runs[1]["what"]
    assert sum(one) == one[M.GENERATE] + one[M.INSERT_EMPTY] + one[M.COPY_EMPTY] + one[M.ERASE_EMPTY]


def test_the_16385_byte_insert_copy_is_the_base(sim):
    """Entry 9 alone (chunks of 5461 and 5463 bytes): every insert-copy is one
    byte or three too long, and the result is the entry itself; entry 8 alone
    gives 16384 bytes when its first chunk is copied."""
    corpus = M.corpus()
    for entry, kinds in ((9, {M.INSERT_TOO_LONG}), (8, {M.INSERT, M.INSERT_TOO_LONG})):
        only = [corpus[entry]]
        got = native(sim, only, range(4096), 1)
        ins = [(o, k) for o, k in got if k in (M.INSERT, M.INSERT_TOO_LONG)]
        assert {k for _, k in ins} == kinds
        assert all(o == only[0] for o, k in ins if k == M.INSERT_TOO_LONG)
        assert all(len(o) == M.MAX_FEED for o, k in ins if k == M.INSERT)
        assert got == [M.mutate(SEED, i, only, 1) for i in range(4096)]


def test_an_index_does_not_depend_on_its_neighbours(sim):
    corpus = M.corpus()
    rng = np.random.default_rng(7)
    alone = {g: native(sim, corpus, [g], 12)[0] for g in (0, 1, 77, 4095, 1 << 40)}
    order = list(alone) + [int(x) for x in rng.integers(0, 1 << 20, 50)]
    for _ in range(3):
        rng.shuffle(order)
        for g, r in zip(order, native(sim, corpus, order, 12)):
            if g in alone:
                assert r == alone[g], g
    for g in alone:
        assert alone[g] == M.mutate(SEED, g, corpus, 12)


def test_the_gate_refuses_malformed_feeds(sim):
    """entry_packets, the check wtfgpu_corpus_add_feed makes: a truncated
    chunk, a Size of 7, one trailing byte, 16385 bytes; and the entry it writes
    is the model's."""
    good = M.feed_of([(1, 2, 3, b"abc"), (4, 5, 6, b"")])
    pk = lambda f: sim.sim_packets_entry_packets(f, len(f), M.MAX_FEED)  # noqa: E731
    assert pk(good) == 2 and pk(b"") == 0
    assert pk(good[:-1]) == -1 and pk(good[:14]) == -1 and pk(good[:3]) == -1
    assert pk(struct.pack("<I", 7) + bytes(7)) == -1
    assert pk(good + b"\0") == -1
    big = M.feed_of([(0, 0, 0, bytes(8192 - 12)), (0, 0, 0, bytes(8193 - 12))])
    assert len(big) == 16385 and pk(big) == -1 and pk(M.corpus()[10]) == 2
    for feed in M.corpus():
        n = sim.sim_packets_entry_bytes(pk(feed), len(feed))
        buf = C.create_string_buffer(n)
        sim.sim_packets_entry_write(feed, len(feed), pk(feed), buf)
        assert buf.raw == M.pack([feed])[0]


def test_params_out_of_range_are_refused(sim):
    ok = lambda *p: sim.sim_packets_params_valid((C.c_uint32 * 6)(*p))  # noqa: E731
    assert ok(*PARAMS)
    assert ok(64, 11, 244, 3, 10, 16384) and not ok(64, 11, 245, 3, 10, 16384)  # 64 * (12 + 244) = 16384
    assert not ok(0, 11, 100, 3, 10, 16384) and not ok(65, 11, 0, 3, 10, 16384)
    assert not ok(10, 0, 100, 3, 10, 16384) and not ok(10, 11, 100, 0, 10, 16384)


def test_host_build_runs_clean_under_the_sanitizers(tmp_path, runs):
    """The same cases through tests/native/sim_packets_main.cc, a program of
    its own, with AddressSanitizer and UndefinedBehaviorSanitizer: the arena
    holds exactly the entries in use and the output exactly MaxFeed bytes."""
    exe = str(tmp_path / "sim_packets_main")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(NATIVE, "sim_packets_main.cc")])
    corpus = M.corpus()
    blob = struct.pack("<I", len(corpus)) + b"".join(struct.pack("<I", len(f)) + f for f in corpus)
    blob += struct.pack("<6I", *PARAMS) + struct.pack(f"<I{len(M.NCORPUS)}I", len(M.NCORPUS), *M.NCORPUS)
    cases = tmp_path / "cases.bin"
    cases.write_bytes(blob)
    r = subprocess.run([exe, str(cases), hex(SEED), str(COUNT)], capture_output=True, text=True)
    lines = r.stdout.split()
    assert r.returncode == 0 and lines[-1:] == ["ok"], r.stdout[-2000:] + r.stderr[-4000:]
    assert lines[:-1] == ["%016x" % v["sum"] for v in runs.values()]


needs_hostlib = pytest.mark.skipif(not os.path.exists(HOSTLIB), reason="wtf_amd/host/libwtfhost.a not built")


@needs_hostlib
def test_feed_to_testcase_round_trips(tmp_path, runs):
    """tests/native/packets_roundtrip.cc over the corpus and 1,024 results per
    ncorpus: TestcaseToFeed(FeedToTestcase(f)) == f, and FeedToTestcase(f) is
    what Serialize writes for the packets parsed from it. The module declares
    the params the model uses."""
    exe = str(tmp_path / "packets_roundtrip")
    subprocess.check_call([CXX, "-O2", "-std=c++20", "-fopenmp", "-o", exe, os.path.join(NATIVE, "packets_roundtrip.cc"),
                           "-Wl,--whole-archive", HOSTLIB, "-Wl,--no-whole-archive"])
    feeds = M.corpus() + [f for v in runs.values() for f in v["feeds"]]
    path = tmp_path / "feeds.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(f)) + f for f in feeds))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == f"ok {len(feeds)}", r.stdout[-2000:] + r.stderr[-2000:]
    assert lines[0] == "params " + " ".join(str(p) for p in M.TLV)


# ---- campaigns: the twin materialises the orders on the host, from the same header
from tests import tlv_harness as H  # noqa: E402

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")
TLV = ("tlv_server", 12000, 512)
# `wtf_twin fuzz --name tlv_server --runs 12000 --lanes 512 --seed 1337 --limit 100000 --max_len 4096`, streaming,
# without the flag, at the parent of the commit that added the flag
PARENT_COUNTS = {"execs": 12000, "retired": 3765744, "coverage": 228, "corpus": 7, "crashes": 2569,
                 "unique_crashes": 5, "timeouts": 0, "cr3": 0, "errors": 0, "error_retired": 0}


@pytest.fixture(scope="module")
def tlv_base(tmp_path_factory):
    return H.build_target(str(tmp_path_factory.mktemp("tlv") / "base"))


def _summary(d, extra):
    out = subprocess.run([H.TWIN, "fuzz", "--name", "tlv_server", "--target", d, "--runs", "64", "--lanes", "16", *extra],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return H.last_json(out)


@needs_twin
def test_twin_campaigns_agree_and_reproduce(tlv_base, tmp_path):
    """Batch, streaming and --serial-mutation streaming campaigns with
    --device-packets: the stream is indexed by the testcase's number alone, so
    all three are one campaign, and a second run gives it again. All four
    synthetic tlv inputs convert to feeds, so nothing is dropped."""
    dp = ("--device-packets",)
    inputs = len(os.listdir(os.path.join(tlv_base, "inputs")))
    a = H.stream_campaign(tlv_base, str(tmp_path / "batch"), *TLV, stream=False, extra=dp)
    b = H.stream_campaign(tlv_base, str(tmp_path / "stream"), *TLV, stream=True, extra=dp)
    c = H.stream_campaign(tlv_base, str(tmp_path / "serial"), *TLV, stream=True, extra=dp + ("--serial-mutation",))
    d = H.stream_campaign(tlv_base, str(tmp_path / "again"), *TLV, stream=True, extra=dp)
    print(a[0])
    assert a[0]["execs"] == TLV[1] and a[0]["errors"] == 0
    assert a == b and a == c and a == d
    assert a[0]["corpus"] > inputs and len(a[1][0]) == a[0]["corpus"]
    st = _summary(str(tmp_path / "again"), dp)
    assert st["device_packets"] == 1 and st["device_mutate"] == 0 and st["device_corpus_dropped"] == 0
    assert st["mutate_cpu_ms"] == 0


@needs_twin
def test_without_the_flag_the_campaign_is_the_parents(tlv_base, tmp_path):
    got = H.stream_campaign(tlv_base, str(tmp_path / "off"), *TLV, stream=True)
    assert got[0] == PARENT_COUNTS
    assert (len(got[1][0]), len(got[1][1])) == (7, 5)
    assert _summary(str(tmp_path / "off"), ())["device_packets"] == 0


def _refused(args, flag="--device-packets", env=None, mode="fuzz"):
    r = subprocess.run([H.TWIN, mode, *args], capture_output=True, text=True, timeout=120,
                       env={**os.environ, **(env or {})})
    assert r.returncode != 0, r.stdout
    lines = [x for x in (r.stdout + r.stderr).splitlines() if flag in x]
    assert len(lines) == 1, r.stdout + r.stderr
    if flag == "--device-packets":
        assert "--device-mutate" not in r.stdout + r.stderr
        assert '"execs"' not in r.stdout  # before any lane ran
    return lines[0]


@needs_twin
def test_refusals(tlv_base, tmp_path):
    hevd = H.build_hevd_target(str(tmp_path / "hevd"))
    common = ["--runs", "64", "--lanes", "16"]
    tlv = ["--name", "tlv_server", "--target", tlv_base, *common, "--device-packets"]
    assert "no packet mutator" in _refused(["--name", "hevd", "--target", hevd, *common, "--device-packets"])
    # the environment variable is the flag
    assert "no packet mutator" in _refused(["--name", "hevd", "--target", hevd, *common],
                                            env={"WTFGPU_DEVICE_PACKETS": "1"})
    assert "byte-buffer device mutator" in _refused([*tlv, "--device-mutate"])
    assert "--world > 1" in _refused([*tlv, "--rank", "0", "--world", "2"])
    assert "--address" in _refused([*tlv, "--address", "tcp://127.0.0.1:1"])
    assert "--module-so" in _refused([*tlv, "--module-so", "/nonexistent.so"])
    assert "master" in _refused(["--name", "tlv_server", "--target", tlv_base, "--device-packets", "--address",
                                 "tcp://127.0.0.1:1", "--nodes", "1"], mode="master")


@needs_twin
def test_device_mutate_on_tlv_still_prints_its_old_line(tlv_base):
    """The check of the check: the byte-buffer flag's refusal of tlv is as it was."""
    line = _refused(["--name", "tlv_server", "--target", tlv_base, "--runs", "64", "--lanes", "16", "--device-mutate"],
                    flag="--device-mutate")
    assert "mutator of its own" in line and "--device-packets" not in line
