"""The packed feed read-back on the CPU: the layout rule in
wtf_amd/csrc/engine_feedpack.h, built for the host
(tests/native/feed_pack_main.cc), against its restatement in Python
(tests/feed_pack_model.py), as a plain build and under AddressSanitizer and
UndefinedBehaviorSanitizer with every array in a block of exactly its size;
and the decision which results' bytes the session looks at
(KeepsTestcase, wtf_amd/host/runner.h; tests/native/keep_filter_main.cc),
which FuzzSession::AccountStep and the device executor's read-back share.

The `--device-packets` and `--device-mutate` campaigns on the twin are
tests/test_device_packets.py's and tests/test_device_mutate.py's, unchanged:
the twin materialises the orders on the host and goes through the same
AccountStep."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import feed_pack_model as F

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("feedpack_" + request.param) / "feed_pack_main")
    subprocess.check_call([CXX, *BUILDS[request.param], "-std=c++17", "-Wall", "-Werror", "-o", out,
                           os.path.join(NATIVE, "feed_pack_main.cc")])
    return out


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1:] == ["ok"], r.stdout[-2000:] + r.stderr[-4000:]
    return lines[:-1]


def native_pack(exe, tmp_path, feeds):
    lens = [F.NO_FEED if f is None else len(f) for f in feeds]
    cases, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.write_bytes(struct.pack(f"<I{len(lens)}I", len(lens), *lens) + b"".join(f for f in feeds if f))
    run(exe, "pack", str(cases), str(out))
    blob = out.read_bytes()
    total, = struct.unpack_from("<Q", blob)
    offs = list(struct.unpack_from(f"<{len(lens)}Q", blob, 8))
    return lens, offs, total, blob[8 + 8 * len(lens):]


def feeds_of(lens, salt=0):
    rng = np.random.default_rng(1234 + salt)
    # no zero byte in a feed: a zero in the output is padding, nothing else
    return [None if n is None else rng.integers(1, 256, n, dtype=np.uint8).tobytes() for n in lens]


EDGE = [0, 1, 15, 16, 17, 16383, 16384]
LISTS = {
    "edges": EDGE,
    "edges_reversed": EDGE[::-1],
    "empty_list": [],
    "one_lane_without_a_feed": [None],
    "no_lane_has_a_feed": [None] * 5,
    "only_empty_feeds": [0, 0, 0],
    **{f"no_feed_at_{p}": EDGE[:p] + [None] + EDGE[p:] for p in range(len(EDGE) + 1)},
    "no_feed_between_all": [x for n in EDGE for x in (None, n)] + [None],
}


@pytest.mark.parametrize("name", list(LISTS))
def test_offsets_and_pack_match_the_model(exe, tmp_path, name):
    feeds = feeds_of(LISTS[name], len(name))
    want = F.pack(feeds)
    got = native_pack(exe, tmp_path, feeds)
    assert got[:3] == want[:3]
    assert got[3] == want[3]
    assert F.padding_is_zero(*got)
    for f, n, o in zip(feeds, got[0], got[1]):
        assert f is None or got[3][o:o + n] == f


def test_a_lane_listed_twice_has_two_places(exe, tmp_path):
    a, b = feeds_of([17, 16383], 7)
    feeds = [a, b, a, None, b, a]
    lens, offs, total, buf = native_pack(exe, tmp_path, feeds)
    assert (lens, offs, total, buf) == F.pack(feeds)
    assert offs == [0, 32, 32 + 16384, 64 + 16384, 64 + 16384, 64 + 2 * 16384] and total == 96 + 2 * 16384
    assert len({o for o, f in zip(offs, feeds) if f is not None}) == 5


def test_the_sum_is_64_bits_wide(exe):
    """262,144 lanes of 16 KiB are exactly 2^32 bytes: one lane more, and a
    32-bit sum would give 16,384 for the total and 0 for the last offset."""
    last, total = (int(x) for x in run(exe, "lens", "262145", "16384")[0].split())
    assert F.offsets([16384] * 3) == ([0, 16384, 32768], 49152)
    assert (last, total) == (2 ** 32, 2 ** 32 + 16384)
    last, total = (int(x) for x in run(exe, "lens", "262144", "16384")[0].split())
    assert (last, total) == (2 ** 32 - 16384, 2 ** 32)


def test_lengths_clamps_and_masks(exe):
    got = run(exe, "words")
    want = []
    for w in (0, 1, 16379, 16380, 16381, 0x7fffffff, 0xffffffff):
        want.append(f"chunk {w} {F.chunk_len(w)} {F.NO_FEED}")
    for n in (0, 1, 16383, 16384, 16385, 3 * 16384):
        want.append(f"whole {n} {F.whole_len(n)} {F.NO_FEED}")
    word = bytes.fromhex("D4C3B2A1")  # 0xA1B2C3D4, little-endian
    for n in (0, 1, 2, 3, 4, 5, 16, 17):
        for at in (0, 4, 12, 16):
            kept = max(0, min(4, n - at))  # bytes of the word below the length
            want.append("mask %d %d %08x" % (n, at, int.from_bytes(word[:kept] + bytes(4 - kept), "little")))
    for v in (0, 1, 15, 16, 17, 16383, 16384, 0xfffffff0, 0xfffffffe, 0xffffffff):
        want.append(f"pad {v} {F.pad16(v)}")
    assert got == want


KEEP = {  # which results' bytes the session looks at, with one crash name known
    "error": 1, "error_with_coverage": 1,
    "timeout": 0, "timeout_with_coverage": 0,
    "crash_known_name": 0, "crash_known_name_with_coverage": 1,
    "crash_new_name": 1, "crash_empty_name": 0,
    "ok": 0, "ok_with_coverage": 1, "cr3": 0, "cr3_with_coverage": 1,
}


def test_keep_function(tmp_path):
    out = str(tmp_path / "keep_filter_main")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++20", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(NATIVE, "keep_filter_main.cc")])
    got = dict((k, int(v)) for k, v in (line.split() for line in run(out)))
    want = dict(KEEP)
    want.update({"every_" + k: 1 for k in KEEP})  # --sample: every result
    want.update({"plain": 0, "every_plain": 1, "before_insert": 1, "after_insert": 0})
    assert got == want
