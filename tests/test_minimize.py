"""`minimize` on the CPU: the candidate stream of wtf_amd/csrc/engine_minimize.h
built for the host (tests/native/sim_minimize.cc) against its restatement in
Python (tests/minimize_model.py), and the session (`wtf_twin minimize`) against
the model's reference loop, whose predicate is `wtf_twin run` over a directory
of one round's candidates."""
import ctypes as C
import json
import os
import random
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import minimize_model as M
from tests import packet_mutate_model as PM
from tests import tlv_harness as H
from tests.hevd_inputs import crafted
from wtf_amd.tools.tlv import packets_json

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
UNITS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
BIG = 16380
FEED_PACKETS = [0, 1, 2, 3, 5, 33, 64]
HEVD_MAX_PAYLOAD = 1024  # fuzzer_hevd.cc: the declared insert's MaxPayload
# HEVD inputs of the end-to-end tests: integer_wrap shrinks (REMOVE and ZERO
# rounds accepted), stack_ret_overrun's crash name holds bytes of the input at
# a fixed offset (no removal is accepted, many ZERO rounds are), and
# stack_gs_cookie's first REMOVE round has no match
HEVD_INPUTS = ["integer_wrap", "stack_ret_overrun", "stack_gs_cookie"]

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")


# ---- the stream

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simmin") / "libsimminimize.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_minimize.cc")])
    L = C.CDLL(so)
    U32, U64 = C.c_uint32, C.c_uint64
    L.sim_min_total.argtypes, L.sim_min_total.restype = [U32], U64
    L.sim_min_locate.argtypes, L.sim_min_locate.restype = [U32, U64, C.POINTER(U32)], None
    L.sim_min_bytes.argtypes = [C.c_char_p, U32, U32, C.POINTER(U64), U32, C.c_void_p, U64, C.POINTER(U32)]
    L.sim_min_bytes.restype = None
    L.sim_min_feed.argtypes = [C.c_char_p, U32, C.POINTER(U64), U32, C.c_void_p, U64, C.POINTER(U32)]
    L.sim_min_feed.restype = C.c_int
    return L


def native(L, base, op, indices, feed=False):
    ix = np.ascontiguousarray(indices, dtype=np.uint64)
    n, stride = len(ix), max(len(base), 1)
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    args = (ix.ctypes.data_as(C.POINTER(C.c_uint64)), n, out.ctypes.data_as(C.c_void_p), stride,
            lens.ctypes.data_as(C.POINTER(C.c_uint32)))
    if feed:
        assert L.sim_min_feed(base, len(base), *args) == len(PM.packets_of(base))
    else:
        L.sim_min_bytes(base, len(base), op, *args)
    return [out[i, :lens[i]].tobytes() for i in range(n)]


def big_indices():
    """At U = 16380: the first and last index of every level, and 512 drawn ones."""
    ix, at = [], 0
    for _, n in M.levels(BIG):
        ix += [at, at + n - 1]
        at += n
    rng = random.Random(0x16380)
    return sorted(set(ix)) + [rng.randrange(M.total(BIG)) for _ in range(512)]


def byte_cases():
    """(base, op, indices or None for all)"""
    for U in UNITS:
        for op in (M.REMOVE, M.ZERO):
            yield M.byte_base(U, U), op, None
    for op in (M.REMOVE, M.ZERO):
        yield M.byte_base(BIG, 9), op, big_indices()


def test_host_build_matches_the_model_on_byte_buffers(sim):
    for base, op, ix in byte_cases():
        ix = list(range(M.total(len(base)))) if ix is None else ix
        got = native(sim, base, op, ix)
        want = [M.candidate(base, op, i) for i in ix]
        bad = [(len(base), op, i) for i, g, w in zip(ix, got, want) if g != w]
        assert not bad, bad[:5]


def test_host_build_matches_the_model_on_feeds(sim):
    for P in FEED_PACKETS:
        feed = M.feed_base(P)
        pk = PM.packets_of(feed)
        assert len(pk) == P and (P == 0 or (len(pk[0][3]) == 0 and len(pk[-1][3]) == 0))
        assert all(len(p[3]) <= 40 for p in pk)
        ix = list(range(M.total(P)))
        got = native(sim, feed, M.REMOVE, ix, feed=True)
        want = [M.candidate_feed(feed, i) for i in ix]
        assert got == want, P
        for w in want:  # the surviving chunks still tile the result
            assert PM.packets_of(w) is not None
        if P and P & (P - 1) == 0:  # one chunk of all packets: a feed of zero bytes
            assert want[0] == b""


def test_locate_is_a_bijection_onto_the_levels(sim):
    out = (C.c_uint32 * 4)()
    for U in UNITS + [BIG]:
        lv = M.levels(U)
        closed = sum(-(-U // (1 << k)) for k in range(U.bit_length())) if U else 0
        assert M.total(U) == closed == sim.sim_min_total(U)
        assert len(lv) <= 15
        seen = set()
        ix = range(M.total(U)) if U != BIG else big_indices()
        for i in ix:
            k, j, lo, hi = M.locate(U, i)
            sim.sim_min_locate(U, i, out)
            assert tuple(out) == (k, j, lo, hi)
            assert lo == j << k and hi == min(U, lo + (1 << k)) and lo < hi
            seen.add((k, j))
        if U != BIG:
            assert seen == {(k, j) for k, n in lv for j in range(n)}
    assert M.total(0) == 0 and M.total(1) == 1 and M.total(5) == 2 + 3 + 5


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same cases in a program of its own, built with
    -fsanitize=address,undefined: every base and result in a heap buffer of
    exactly its size. Its per-case CRC-32 must be the model's."""
    exe = str(tmp_path / "sim_minimize")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(NATIVE, "sim_minimize_main.cc"),
                           os.path.join(NATIVE, "sim_minimize.cc")])
    want, blob = [], b""
    for base, op, ix in byte_cases():
        blob += struct.pack("<IIII", 0, op, len(base), 0xffffffff if ix is None else len(ix)) + base
        if ix is not None:
            blob += struct.pack(f"<{len(ix)}Q", *ix)
        ix = range(M.total(len(base))) if ix is None else ix
        crc = 0
        for i in ix:
            c = M.candidate(base, op, i)
            crc = zlib.crc32(struct.pack("<I", len(c)) + c, crc)
        want.append("%d %08x" % (len(ix), crc))
    for P in FEED_PACKETS:
        feed = M.feed_base(P)
        blob += struct.pack("<IIII", 1, 0, len(feed), 0xffffffff) + feed
        crc = 0
        for i in range(M.total(P)):
            c = M.candidate_feed(feed, i)
            crc = zlib.crc32(struct.pack("<I", len(c)) + c, crc)
        want.append("%d %08x" % (M.total(P), crc))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want


# ---- the session on the twin

def twin_minimize(target, name, src, out, lanes=64, extra=(), env=None):
    r = subprocess.run([H.TWIN, "minimize", "--name", name, "--target", target, "--input", src, "--output", out,
                        "--lanes", str(lanes), "--limit", "100000", *extra], capture_output=True, text=True,
                       timeout=300, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stdout + r.stderr
    return H.last_json(r.stdout)


class Predicate:
    """matches() of the reference loop: `wtf_twin run` over a directory holding
    one round's candidates, one file each; a candidate matches iff its result
    is a crash of the wanted name and no engine error."""

    def __init__(self, target, name, work, crash):
        self.target, self.name, self.work, self.crash, self.round = target, name, str(work), crash, 0

    def results(self, testcases):
        d = os.path.join(self.work, "round%04d" % self.round)
        self.round += 1
        os.makedirs(d)
        for i, t in enumerate(testcases):
            with open(os.path.join(d, "%06d" % i), "wb") as f:
                f.write(t)
        res = H.run(H.TWIN, self.target, d, d + ".jsonl", lanes=64, full_coverage=False, name=self.name)
        shutil.rmtree(d)
        by = {r["input"]: r for r in res}
        return [by["%06d" % i] for i in range(len(testcases))]

    def __call__(self, testcases):
        return [r["result"] == "crash" and r["crash"] == self.crash and not r["error"] for r in self.results(testcases)]


@pytest.fixture(scope="module")
def hevd_target(tmp_path_factory):
    return H.build_hevd_target(str(tmp_path_factory.mktemp("hevd_min")))


@pytest.fixture(scope="module")
def hevd_reference(hevd_target, tmp_path_factory):
    """The reference loop on every HEVD input, once: {name: (input path, crash,
    final bytes, log, counts)}."""
    work = tmp_path_factory.mktemp("hevd_ref")
    out = {}
    for name in HEVD_INPUTS:
        data = crafted()[name]
        src = str(work / name)
        with open(src, "wb") as f:
            f.write(data)
        first = Predicate(hevd_target, "hevd", work / (name + "_first"), None).results([data])[0]
        assert first["result"] == "crash" and first["crash"]
        pred = Predicate(hevd_target, "hevd", work / (name + "_rounds"), first["crash"])
        final, log, counts = M.minimize(data, M.ByteStream(HEVD_MAX_PAYLOAD), pred)
        out[name] = (src, first["crash"], final, log, counts, pred)
    return out


@needs_twin
def test_the_hevd_inputs_exercise_both_phases(hevd_reference):
    """Non-vacuity: the reference loop accepts at least two REMOVE rounds and
    two ZERO rounds over the inputs, and one input's first round has no match."""
    acc = {op: sum(1 for _, _, _, log, _, _ in hevd_reference.values() for r in log
                   if r["op"] == op and r["winner"] is not None) for op in (M.REMOVE, M.ZERO)}
    print("accepted rounds", acc, {k: v[4] for k, v in hevd_reference.items()})
    assert acc[M.REMOVE] >= 2 and acc[M.ZERO] >= 2, acc
    assert hevd_reference["stack_gs_cookie"][3][0]["winner"] is None
    assert hevd_reference["integer_wrap"][3][0]["winner"] is not None


@needs_twin
@pytest.mark.parametrize("name", HEVD_INPUTS)
def test_twin_minimize_is_the_reference_loop_on_hevd(hevd_target, hevd_reference, tmp_path, name):
    src, crash, final, log, counts, pred = hevd_reference[name]
    out = str(tmp_path / "min")
    st = twin_minimize(hevd_target, "hevd", src, out)
    got = open(out, "rb").read()
    assert got == final
    assert {k: st[k] for k in counts} == counts
    assert st["crash"] == crash and st["input_bytes"] == len(crafted()[name]) and st["output_bytes"] == len(final)
    # the output still crashes under the same name
    assert pred([final]) == [True]
    # and removing any one byte of it no longer does: the last REMOVE round had
    # no match, and its smallest chunks are the single bytes
    last = [r for r in log if r["op"] == M.REMOVE][-1]
    assert last["winner"] is None and len(last["base"]) == len(final)
    T, U = M.total(len(final)), len(final)
    singles = [M.candidate(last["base"], M.REMOVE, i) for i in range(T - U, T)]
    assert singles == [last["base"][:i] + last["base"][i + 1:] for i in range(U)]
    assert last["ordered"] + last["skipped"] == T
    # the default output path
    shutil.copy(src, str(tmp_path / "again"))
    r = subprocess.run([H.TWIN, "minimize", "--name", "hevd", "--target", hevd_target, "--input",
                        str(tmp_path / "again"), "--lanes", "64", "--limit", "100000"], capture_output=True, text=True)
    assert r.returncode == 0 and open(str(tmp_path / "again.min"), "rb").read() == final


@needs_twin
@pytest.mark.parametrize("lanes,stream", [(1, "0"), (7, "1"), (512, "1"), (512, "0")])
def test_lane_count_and_path_do_not_change_the_output(hevd_target, hevd_reference, tmp_path, lanes, stream):
    src, _, final, _, counts, _ = hevd_reference["integer_wrap"]
    out = str(tmp_path / "min")
    st = twin_minimize(hevd_target, "hevd", src, out, lanes=lanes, env={"WTF_TWIN_STREAM": stream})
    assert open(out, "rb").read() == final and {k: st[k] for k in counts} == counts


@needs_twin
def test_rounds_limit_is_reported(hevd_target, hevd_reference, tmp_path):
    src, crash, _, log, _, _ = hevd_reference["integer_wrap"]
    out = str(tmp_path / "min")
    st = twin_minimize(hevd_target, "hevd", src, out, extra=("--rounds", "1"))
    assert st["stopped_by_rounds"] is True and st["rounds"] == 1
    assert open(out, "rb").read() == log[1]["base"]  # the first round's winner


def tlv_crash(target, work):
    """One crash file of a short fixed-seed twin campaign: the largest."""
    d = os.path.join(str(work), "campaign")
    shutil.copytree(target, d, ignore=shutil.ignore_patterns("outputs", "crashes", "work", "errors"))
    H.fuzz(H.TWIN, d, runs=3072, lanes=512, seed=1337)
    files = sorted(os.listdir(os.path.join(d, "crashes")))
    assert files
    return max((os.path.join(d, "crashes", f) for f in files), key=lambda p: (os.path.getsize(p), p))


def tlv_feed(testcase: bytes) -> bytes:
    return PM.feed_of([(p["Command"], p["Id"], p["BodySize"], bytes(p["Body"]))
                       for p in json.loads(testcase)["Packets"]])


def tlv_testcase(feed: bytes) -> bytes:
    return packets_json(PM.packets_of(feed))


@needs_twin
def test_twin_minimize_is_the_reference_loop_on_tlv(tmp_path):
    target = H.build_target(str(tmp_path / "tlv"))
    src = tlv_crash(target, tmp_path)
    data = open(src, "rb").read()
    first = Predicate(target, "tlv_server", tmp_path / "first", None).results([data])[0]
    assert first["result"] == "crash" and first["crash"]
    pred = Predicate(target, "tlv_server", tmp_path / "rounds", first["crash"])
    final, log, counts = M.minimize(tlv_feed(data), M.FeedStream(tlv_testcase), pred)
    print("tlv", len(data), counts, [r["winner"] for r in log])
    assert sum(1 for r in log if r["winner"] is not None) >= 1  # non-vacuity: a removal is accepted
    assert counts["zero_rounds"] == 0
    out = str(tmp_path / "min")
    st = twin_minimize(target, "tlv_server", src, out)
    assert open(out, "rb").read() == tlv_testcase(final)
    assert {k: st[k] for k in counts} == counts and st["crash"] == first["crash"]
    assert pred([tlv_testcase(final)]) == [True]


@needs_twin
@pytest.mark.parametrize("args,stream", [
    (["minimize", "--input", "@integer_ok"], "stdout"),
    (["minimize", "master", "--input", "@integer_wrap"], "stderr"),
    (["minimize", "--address", "tcp://127.0.0.1:1", "--input", "@integer_wrap"], "stderr"),
    (["minimize", "--world", "2", "--input", "@integer_wrap"], "stderr"),
])
def test_refusals(hevd_target, tmp_path, args, stream):
    """One line, a non-zero exit, no candidate run (no output file)."""
    args = list(args)
    name = args[-1][1:]
    src = str(tmp_path / name)
    with open(src, "wb") as f:
        f.write(crafted()[name])
    args[-1] = src
    r = subprocess.run([H.TWIN, *args, "--name", "hevd", "--target", hevd_target, "--lanes", "16", "--limit", "100000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    text = getattr(r, stream)
    assert len(text.strip().splitlines()) == 1 and "minimi" in text, (r.stdout, r.stderr)
    assert not os.path.exists(src + ".min")
    assert "candidates" not in r.stdout
