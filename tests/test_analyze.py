"""`analyze` on the CPU: the rule of wtf_amd/csrc/engine_analyze.h built for the
host (tests/native/sim_analyze.cc) against its restatement in Python
(tests/analyze_model.py), the same cases in a stand-alone program under the
sanitizers, and the session (`wtf_twin analyze`) on HEVD and tlv_server inputs:
the same map at every lane count, batched and streaming, classes that match an
independent loop over `wtf_twin run --full-coverage`, the maps the inputs were
chosen for, and the refusals."""
import ctypes as C
import functools
import itertools
import json
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import analyze_model as M
from tests import covkeep_model as KM
from tests import tlv_harness as H
from tests.hevd_inputs import crafted
from tests.test_minimize_coverage import hevd_inputs, tlv_inputs
from wtf_amd.tools.tlv import packets_json

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 16380]
FEED_PACKETS = [0, 1, 2, 5]
TABLE_H = 64

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")


# ---- the cases of the rule (the GPU test draws its bases the same way)

def base_of(U: int) -> bytes:
    return random.Random(0xA11A + U).randbytes(U)


def byte_indices(U: int) -> list[int]:
    """Every index where U <= 65; else all four variants of the first, the
    last and 64 seeded positions."""
    if U <= 65:
        return list(range(M.total(U)))
    rng = random.Random(0xB17E + U)
    pos = [0, U - 1] + [rng.randrange(U) for _ in range(64)]
    return [4 * p + v for p in pos for v in range(4)]


def feed_of(P: int) -> bytes:
    """P packets with bodies of 0, 1 and 3 bytes in turn."""
    rng = random.Random(0xFEED + P)
    return M.make_feed([(rng.randrange(4), k, rng.randrange(1 << 16), rng.randbytes((0, 1, 3)[k % 3]))
                        for k in range(P)])


@functools.lru_cache(maxsize=None)
def sig_cases():
    """[(name, Table, its live values)]: sets of 0, 1, 2 and 48 values with 0
    and 2^64 - 1 among them, and covkeep_model's directed tables (wrapped
    chains, stale generations, an overflowed set)."""
    out = []
    rng = random.Random(0x516)
    for name, vals in (("none", []), ("zero", [0]), ("ones", [KM.M64]), ("zero_ones", [0, KM.M64]),
                       ("48", [0, KM.M64] + [rng.getrandbits(64) for _ in range(46)])):
        t = KM.Table(TABLE_H)
        for v in vals:
            t.insert(v)
        assert t.count == len(vals) and not t.overflow
        out.append((name, t, vals))
    for name, t, _ in KM.tables(TABLE_H):
        out.append((name, t, t.live()))
    return out


def alphabet():
    """Three outcomes that differ pairwise, in kind, in set or in size."""
    return [M.outcome("ok", values=[1, 2, 3]), M.outcome("ok", values=[1, 2, 4]), M.outcome("crash", "c", [1, 2, 3])]


@functools.lru_cache(maxsize=None)
def class_cases():
    """[(five outcomes)]: the 243 assignments of the alphabet to (base, v0..v3),
    then each with one of the five marked overflowed (by turns), then with all."""
    A = alphabet()
    plain = [tuple(A[k] for k in pick) for pick in itertools.product(range(3), repeat=5)]
    assert len(plain) == 243
    ovf = lambda o: o[:4] + (True,)
    one = [tuple(ovf(o) if j == i % 5 else o for j, o in enumerate(c)) for i, c in enumerate(plain)]
    every = [tuple(ovf(o) for o in c) for c in plain]
    return plain + one + every


NAME_IDS = {"": 0, "c": 1, "d": 2}
KIND_IDS = {"ok": 0, "crash": 1, "timedout": 2, "cr3": 3, "error": 4}


def outcome_arrays(five):
    kind = np.array([KIND_IDS[o[0]] for o in five], dtype=np.uint32)
    name = np.array([NAME_IDS[o[1]] for o in five], dtype=np.uint32)
    sig = np.array([o[2] for o in five], dtype=np.uint64)
    size = np.array([o[3] for o in five], dtype=np.uint32)
    ovf = np.array([int(o[4]) for o in five], dtype=np.uint32)
    return kind, name, sig, size, ovf


def check_the_model():
    """The restated rule has the properties the comment claims."""
    for b in range(256):
        vs = [M.variant(b, v) for v in range(4)]
        assert len({b, *vs}) == 5 and all(0 <= x < 256 for x in vs), b
    want = {M.NONE: 0, M.MINOR: 0, M.FIXED: 0, M.VARIABLE: 0}
    for five in class_cases()[:243]:
        want[M.classify(five[0], list(five[1:]))] += 1
    assert all(want.values()) and want[M.NONE] == 3  # base and all four equal: once a letter
    a = M.outcome("ok", values=[5], overflow=True)
    assert not M.same(a, a)
    for five in class_cases()[2 * 243:]:  # all overflowed: every variant differs, from the base and each other
        assert M.classify(five[0], list(five[1:])) == M.VARIABLE
    # the crash name counts only for crashes
    assert M.same(M.outcome("ok", "x"), M.outcome("ok", "y")) and not M.same(M.outcome("crash", "x"), M.outcome("crash", "y"))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simana") / "libsimanalyze.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_analyze.cc")])
    L = C.CDLL(so)
    U32, U64, p32, p64 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.sim_ana_total.argtypes, L.sim_ana_total.restype = [U32], U64
    L.sim_ana_variant.argtypes, L.sim_ana_variant.restype = [U32, U32], U32
    L.sim_ana_bytes.argtypes, L.sim_ana_bytes.restype = [C.c_char_p, U32, p64, U32, C.c_void_p, U64], None
    L.sim_ana_feed.argtypes = [C.c_char_p, U32, p64, U32, C.c_void_p, U64, C.c_void_p]
    L.sim_ana_feed.restype = C.c_int
    L.sim_ana_sig_list.argtypes, L.sim_ana_sig_list.restype = [p64, U64, p64], U32
    L.sim_ana_sig_table.argtypes, L.sim_ana_sig_table.restype = [p64, p32, U32, U32, p64], U32
    L.sim_ana_classify.argtypes, L.sim_ana_classify.restype = [p32, p32, p64, p32, p32], C.c_int
    L.sim_ana_same.argtypes, L.sim_ana_same.restype = [p32, p32, p64, p32, p32, U32, U32], C.c_int
    return L


def native(L, base, indices, feed=False):
    """(candidates, framing map or None)"""
    ix = np.ascontiguousarray(indices, dtype=np.uint64)
    n, stride = len(ix), max(len(base), 1)
    out = np.zeros((n, stride), dtype=np.uint8)
    fr = np.zeros(max(len(base), 1), dtype=np.uint8)
    pix = ix.ctypes.data_as(C.POINTER(C.c_uint64))
    if feed:
        assert L.sim_ana_feed(base, len(base), pix, n, out.ctypes.data_as(C.c_void_p), stride,
                              fr.ctypes.data_as(C.c_void_p)) == len(M.chunk_offsets(base)) - 1
    else:
        L.sim_ana_bytes(base, len(base), pix, n, out.ctypes.data_as(C.c_void_p), stride)
    return [out[i, :len(base)].tobytes() for i in range(n)], (fr[:len(base)].astype(bool).tolist() if feed else None)


def test_host_build_matches_the_model(sim):
    check_the_model()
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    for b in range(256):
        assert [sim.sim_ana_variant(b, v) for v in range(4)] == [M.variant(b, v) for v in range(4)]
    # byte buffers
    for U in SIZES:
        base, ix = base_of(U), byte_indices(U)
        assert sim.sim_ana_total(U) == M.total(U) == 4 * U
        got, _ = native(sim, base, ix)
        assert got == [M.candidate(base, i) for i in ix], U
        assert all(len(g) == U and sum(x != y for x, y in zip(g, base)) == 1 for g in got)
    # feeds: every non-framing index, and every framing position refused by the engine's helper
    for P in FEED_PACKETS:
        feed = feed_of(P)
        want_fr = M.framing(feed)
        assert sum(want_fr) == 4 * P and len(feed) == 12 * P + sum((0, 1, 3)[k % 3] for k in range(P))
        ix = M.indices(feed, feed=True)
        assert len(ix) == 4 * (len(feed) - 4 * P)
        got, fr = native(sim, feed, ix, feed=True)
        assert fr == want_fr, P
        assert got == [M.candidate(feed, i) for i in ix], P
        # a candidate's chunks tile it as the base's do
        assert all(M.chunk_offsets(g) == M.chunk_offsets(feed) for g in got)
    # signatures: the list form and the table form, any order
    rng = random.Random(7)
    for name, t, vals in sig_cases():
        want = M.sig(t.live())
        assert want == M.sig(vals) if name != "overflowed" else True
        rip, gen = np.array(t.rip, dtype=np.uint64), np.array(t.gen, dtype=np.uint32)
        s = C.c_uint64(0)
        n = sim.sim_ana_sig_table(rip.ctypes.data_as(p64), gen.ctypes.data_as(p32), t.H, t.g, C.byref(s))
        assert (s.value, n) == want, name
        for _ in range(3):
            order = t.live()
            rng.shuffle(order)
            lst = np.array(order + [0], dtype=np.uint64)  # (a pointer to pass for the empty list)
            n = sim.sim_ana_sig_list(lst.ctypes.data_as(p64), len(order), C.byref(s))
            assert (s.value, n) == want, name
            t2 = KM.Table(TABLE_H)  # another insertion order: other slots, the same signature
            for v in order:
                t2.insert(v)
            rip2, gen2 = np.array(t2.rip, dtype=np.uint64), np.array(t2.gen, dtype=np.uint32)
            n = sim.sim_ana_sig_table(rip2.ctypes.data_as(p64), gen2.ctypes.data_as(p32), t2.H, t2.g, C.byref(s))
            assert (s.value, n) == want, name
    assert M.sig([]) == (0, 0) and M.sig([0])[0] == KM.mix64(0)
    # classes
    for five in class_cases():
        arr = outcome_arrays(five)
        ptrs = [a.ctypes.data_as(p64 if a.dtype == np.uint64 else p32) for a in arr]
        assert chr(sim.sim_ana_classify(*ptrs)) == M.classify(five[0], list(five[1:])), five
        for a in range(5):
            for b in range(5):
                assert bool(sim.sim_ana_same(*ptrs, a, b)) == M.same(five[a], five[b])


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same cases in a program of its own, built with
    -fsanitize=address,undefined: every base, candidate, table and list in a
    heap buffer of exactly its size."""
    exe = str(tmp_path / "sim_analyze_san")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(NATIVE, "sim_analyze_main.cc"),
                           os.path.join(NATIVE, "sim_analyze.cc")])
    blob, want = b"", []
    for U in SIZES:
        base, ix = base_of(U), byte_indices(U)
        every = U <= 65
        blob += struct.pack("<IIII", 0, U, 0xffffffff if every else len(ix), 0) + base
        if not every:
            blob += np.array(ix, dtype=np.uint64).tobytes()
        crc = 0
        for i in ix:
            crc = zlib.crc32(M.candidate(base, i), crc)
        want.append("%d %08x" % (len(ix), crc))
    for P in FEED_PACKETS:
        feed = feed_of(P)
        blob += struct.pack("<IIII", 1, len(feed), 0xffffffff, 0) + feed
        crc, ix = 0, M.indices(feed, feed=True)
        for i in ix:
            crc = zlib.crc32(M.candidate(feed, i), crc)
        want.append("%d %08x %s" % (len(ix), crc, "".join(str(int(f)) for f in M.framing(feed))))
    for _, t, _ in sig_cases():
        live = t.live()
        blob += struct.pack("<IIII", 2, t.H, t.g, len(live))
        blob += np.array(t.rip, dtype=np.uint64).tobytes() + np.array(t.gen, dtype=np.uint32).tobytes()
        blob += np.array(live, dtype=np.uint64).tobytes()
        s, n = M.sig(live)
        want.append("%016x %d %016x %d" % (s, n, s, n))
    cases = class_cases()
    blob += struct.pack("<IIII", 3, len(cases), 0, 0)
    for five in cases:
        for o in five:
            blob += struct.pack("<IIQII", KIND_IDS[o[0]], NAME_IDS[o[1]], o[2], o[3], int(o[4]))
    want.append("".join(M.classify(five[0], list(five[1:])) for five in cases))
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want


# ---- the session on the twin

CASES = [("hevd", "integer_big"), ("hevd", "www_ok_pad"), ("tlv_server", "multi"), ("hevd", "integer_wrap")]
COUNT_KEYS = ("bytes", "positions", "candidates", "none", "minor", "fixed", "variable", "framing", "overflowed")


def session_inputs() -> dict[str, tuple[str, bytes]]:
    """{input: (target name, bytes)}: the three inputs of
    tests/test_minimize_coverage.py that end ok, and one HEVD crash."""
    out = {name: ("hevd", data) for name, data in hevd_inputs().items()}
    out["multi"] = ("tlv_server", tlv_inputs()["multi"])
    out["integer_wrap"] = ("hevd", crafted()["integer_wrap"])
    return out


def analyze_cmd(exe, target, name, src, out, lanes, extra=()):
    return [exe, "analyze", "--name", name, "--target", target, "--input", src, "--output", out, "--lanes", str(lanes),
            "--limit", "100000", *extra]


def analyze(exe, target, name, src, out, lanes=64, extra=(), env=None):
    """(summary, map file's bytes)"""
    r = subprocess.run(analyze_cmd(exe, target, name, src, out, lanes, extra), capture_output=True, text=True,
                       timeout=600, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return H.last_json(r.stdout), open(out, "rb").read()


def feed_from_testcase(data: bytes) -> bytes:
    """A tlv testcase (the packets as JSON) as the feed the target makes of it."""
    return M.make_feed([(p["Command"], p["Id"], p["BodySize"], bytes(p["Body"])) for p in json.loads(data)["Packets"]])


def feed_as_testcase(feed: bytes) -> bytes:
    off = M.chunk_offsets(feed)
    pk = []
    for k in range(len(off) - 1):
        cmd, pid, bodysize = struct.unpack_from("<IHH", feed, off[k] + 4)
        pk.append((cmd, pid, bodysize, feed[off[k] + 12:off[k + 1]]))
    return packets_json(pk)


@pytest.fixture(scope="module")
def targets(tmp_path_factory):
    """{target name: target dir}, {input name: path}"""
    d = tmp_path_factory.mktemp("analyze")
    dirs = {"hevd": H.build_hevd_target(str(d / "hevd")), "tlv_server": H.build_target(str(d / "tlv"))}
    paths = {}
    for name, (_, data) in session_inputs().items():
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return dirs, paths


@pytest.fixture(scope="module")
def reference(targets, tmp_path_factory):
    """`wtf_twin analyze` once an input at 64 lanes: {input: (summary, map bytes)}."""
    dirs, paths = targets
    d = tmp_path_factory.mktemp("analyze_ref")
    return {name: analyze(H.TWIN, dirs[tname], tname, paths[name], str(d / f"{name}.map")) for tname, name in CASES}


@needs_twin
@pytest.mark.parametrize("tname,name", CASES)
def test_the_map_matches_an_independent_loop(targets, reference, tmp_path, tname, name):
    """The first, the last and 24 seeded positions: the test makes the four
    variants itself, runs them with `wtf_twin run --full-coverage` next to the
    input, and classifies with the model."""
    dirs, paths = targets
    st, raw = reference[name]
    m = json.loads(raw)
    data = open(paths[name], "rb").read()
    feed = tname == "tlv_server"
    base = feed_from_testcase(data) if feed else data
    assert m["bytes"] == len(base) == len(m["classes"]) == st["bytes"]
    tested = [p for p in range(len(base)) if not (feed and M.framing(base)[p])]
    rng = random.Random(0xC1A55 + len(base))
    pos = [tested[0], tested[-1]] + rng.sample(tested[1:-1], 24)
    ind = tmp_path / "in"
    ind.mkdir()
    (ind / "base").write_bytes(data)
    for p in pos:
        for v in range(4):
            c = M.candidate(base, 4 * p + v)
            (ind / f"p{p}v{v}").write_bytes(feed_as_testcase(c) if feed else c)
    rows = {r["input"]: r for r in H.run(H.TWIN, dirs[tname], str(ind), str(tmp_path / "run.jsonl"), lanes=16,
                                         name=tname)}
    assert len(rows) == 1 + 4 * len(pos)

    def outcome(r):
        return M.outcome("error" if r["error"] else r["result"], r["crash"], sorted(set(r["coverage"])))

    b = outcome(rows["base"])
    assert m["base"] == {"kind": b[0], "crash": b[1], "values": b[3]}
    for p in pos:  # none skipped
        want = M.classify(b, [outcome(rows[f"p{p}v{v}"]) for v in range(4)])
        assert m["classes"][p] == want, (name, p)
    # the file's other parts follow from the classes
    assert m["ranges"] == M.ranges(m["classes"], base if feed else None)
    assert raw == (json.dumps(m, separators=(",", ":")) + "\n").encode()
    cls = m["classes"]
    assert [st[k] for k in ("none", "minor", "fixed", "variable", "framing")] == [cls.count(c) for c in ".mFV#"]
    assert st["positions"] == len(tested) and st["candidates"] == 4 * len(tested) and st["mode"] == "analyze"
    assert st["on_device"] is False and st["sig_on_device"] is False
    assert st["sig_readback_values"] > m["base"]["values"]  # every candidate's set came back


@needs_twin
def test_the_inputs_show_every_class(reference):
    """What the inputs were chosen for."""
    maps = {name: json.loads(raw) for name, (_, raw) in reference.items()}
    big = maps["integer_big"]["classes"]
    assert big[-77:] == "." * 77                       # behind the copy: never read
    for name in ("integer_big", "www_ok_pad", "integer_wrap"):
        assert "." not in maps[name]["classes"][:4]    # the IOCTL code
    assert set("".join(m["classes"] for m in maps.values())) == set(".mFV#")
    assert set("".join(maps[n]["classes"] for n in maps if n != "multi")) == set(".mFV")
    assert maps["integer_wrap"]["base"]["kind"] == "crash" and maps["integer_wrap"]["base"]["crash"]
    # tlv: framing exactly at each chunk's Size, and a header byte that matters
    data = session_inputs()["multi"][1]
    feed = feed_from_testcase(data)
    cls = maps["multi"]["classes"]
    assert [c == "#" for c in cls] == M.framing(feed) and cls.count("#") == 4 * 11
    f = M.fields(feed)
    assert any(cls[p] != "." for p in range(len(feed)) if f[p][1] in ("command", "id", "bodysize"))
    assert {r["field"] for r in maps["multi"]["ranges"]} == {"size", "command", "id", "bodysize", "body"}
    assert all(st["overflowed"] == 0 for st, _ in reference.values())


@needs_twin
def test_a_candidate_that_overflows(targets, reference, tmp_path):
    """integer_wrap's own set (88 values) fits a set of 128 slots (96 values);
    some candidates' sets do not, and those are different from everything."""
    dirs, paths = targets
    st, raw = analyze(H.TWIN, dirs["hevd"], "hevd", paths["integer_wrap"], str(tmp_path / "m"),
                      extra=("--cov-set", "128"))
    assert json.loads(raw)["base"]["values"] <= KM.cap(128)
    assert st["overflowed"] >= 1 and raw != reference["integer_wrap"][1]


@needs_twin
@pytest.mark.parametrize("lanes", [1, 7, 512])
@pytest.mark.parametrize("path", ["batched", "streaming"])
@pytest.mark.parametrize("tname,name", CASES)
def test_lane_count_and_path_do_not_change_the_map(targets, reference, tmp_path, tname, name, path, lanes):
    dirs, paths = targets
    want_st, want = reference[name]
    st, got = analyze(H.TWIN, dirs[tname], tname, paths[name], str(tmp_path / "map"), lanes=lanes,
                      env={"WTF_TWIN_STREAM": "1"}, extra=("--slice-steps", "0") if path == "batched" else ())
    assert got == want
    assert {k: st[k] for k in COUNT_KEYS} == {k: want_st[k] for k in COUNT_KEYS}
    assert st["sig_readback_values"] == want_st["sig_readback_values"]


@needs_twin
def test_the_default_output_path(targets, reference, tmp_path):
    dirs, paths = targets
    src = str(tmp_path / "www")
    with open(src, "wb") as f:
        f.write(open(paths["www_ok_pad"], "rb").read())
    r = subprocess.run([H.TWIN, "analyze", "--name", "hevd", "--target", dirs["hevd"], "--input", src, "--lanes", "16",
                        "--limit", "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(src + ".map", "rb").read() == reference["www_ok_pad"][1]


@needs_twin
@pytest.mark.parametrize("case", ["cov-set", "too-long", "empty", "exists", "master", "address", "world", "module-so",
                                  "fuzz"])
def test_refusals(targets, tmp_path, case):
    """One line, a non-zero exit, nothing written."""
    dirs, paths = targets
    src = str(tmp_path / "in")
    data = open(paths["integer_big"], "rb").read()
    if case == "too-long":
        data = data[:8] + b"L" * 16373  # 16381 bytes: one more than a lane's feed region holds
    elif case == "empty":
        data = b""
    with open(src, "wb") as f:
        f.write(data)
    out = str(tmp_path / "out.map")
    name, target = "hevd", dirs["hevd"]
    args = ["analyze", "--name", name, "--target", target, "--input", src, "--output", out, "--lanes", "16", "--limit",
            "100000"]
    if case == "cov-set":
        args += ["--cov-set", "16"]
    elif case == "exists":
        with open(out, "wb") as f:
            f.write(b"mine")
    elif case == "master":
        args = ["master", "--nodes", "1", "--address", "tcp://127.0.0.1:1"] + args
    elif case == "address":
        args += ["--address", "tcp://127.0.0.1:1"]
    elif case == "world":
        args += ["--world", "2", "--rank", "0"]
    elif case == "module-so":
        args += ["--module-so", str(tmp_path / "m.so")]
    elif case == "fuzz":
        args = ["fuzz"] + args
    r = subprocess.run([H.TWIN, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    text = [x for x in (r.stdout + r.stderr).splitlines() if x.strip()]
    assert len(text) == 1, (r.stdout, r.stderr)
    assert "candidates" not in r.stdout
    if case == "exists":
        assert open(out, "rb").read() == b"mine" and "exists" in text[0]
    else:
        assert not os.path.exists(out)
    if case == "cov-set":
        assert "--cov-set" in text[0] and "filled up" in text[0]
    elif case == "too-long":
        assert "longer than a lane's feed region" in text[0]
    elif case == "empty":
        assert "zero bytes" in text[0]
    elif case != "exists":
        assert "analyze is one in-process session" in text[0]


@needs_twin
def test_minimize_and_distill_command_lines_behave_as_before(targets, tmp_path):
    """The mode word does not mix with the family's other two, and theirs still run."""
    dirs, paths = targets
    for other in (["minimize"], ["distill", "--output", str(tmp_path / "kept0")]):
        r = subprocess.run([H.TWIN, "analyze", *other, "--name", "hevd", "--target", dirs["hevd"], "--input",
                            paths["integer_wrap"], "--lanes", "16", "--limit", "100000"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and not os.path.exists(paths["integer_wrap"] + ".map")
    r = subprocess.run([H.TWIN, "minimize", "--name", "hevd", "--target", dirs["hevd"], "--input", paths["integer_wrap"],
                        "--output", str(tmp_path / "min"), "--lanes", "16", "--limit", "100000"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = H.last_json(r.stdout)
    assert st["mode"] == "crash" and st["output_bytes"] < st["input_bytes"] == 612
    ind = tmp_path / "corpus"
    ind.mkdir()
    for k in ("integer_big", "www_ok_pad"):
        (ind / k).write_bytes(open(paths[k], "rb").read())
    r = subprocess.run([H.TWIN, "distill", "--name", "hevd", "--target", dirs["hevd"], "--input", str(ind), "--output",
                        str(tmp_path / "kept"), "--lanes", "16", "--limit", "100000"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = H.last_json(r.stdout)
    assert st["mode"] == "distill" and st["inputs"] == 2 and st["kept"] >= 1
