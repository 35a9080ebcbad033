"""The device mutator's stream on the CPU: the definition in
wtf_amd/csrc/engine_mutate.h, built for the host (tests/native/sim_mutate.cc),
against its restatement in Python (tests/mutate_model.py), byte for byte.

The corpora: entries of 0, 1, 3, 4, 5, 63, 64, 65, 1028 and 16380 bytes, all
zero, all 0xff, ASCII digits behind a '-', random, and a mix of them; max_len
4, 5, 64, 1028, 16380; the first 1, 2 or all 10 entries; indices 0..4095.

The 100-failures exit. No operator can fail 100 times on a base of 4 bytes
with max_len 4: EraseBytes, ChangeByte, ChangeBit, ShuffleBytes and CopyPart
apply to every testcase of 2 bytes or more, so each attempt succeeds with
probability 1/2 at the least, whatever the index. The exit needs a base on
which all ten fail, and by the operators' conditions that is the empty
testcase with max_len 0 alone (EraseBytes needs 2 bytes, the two inserts need
room, the other seven need a byte). It is reached and checked there;
test_four_bytes_at_max_len_4_never_exhaust_the_attempts states the other half."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mutate_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
SEED = 0x5EED
COUNT = 4096


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """libsimmutate.so: tests/native/sim_mutate.cc, built with the flags tests/native/Makefile gives libsimlane.so."""
    so = str(tmp_path_factory.mktemp("simmutate") / "libsimmutate.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_mutate.cc")])
    L = C.CDLL(so)
    U32, U64 = C.c_uint32, C.c_uint64
    L.sim_mutate_many.argtypes = [U64, C.POINTER(U64), U32, C.c_char_p, C.POINTER(U64), U32, U32, C.c_void_p, U64,
                                  C.POINTER(U32), C.POINTER(U32)]
    L.sim_mutate_many.restype = None
    return L


def native(L, entries, indices, ncorpus, max_len, seed=SEED):
    """[(bytes, op or None, [failed ops])] from the host build."""
    arena, off = M.pack(entries)
    ix = np.ascontiguousarray(indices, dtype=np.uint64)
    n = len(ix)
    stride = max(max_len, 1)
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    info = np.zeros((n, 3), dtype=np.uint32)
    L.sim_mutate_many(seed, ix.ctypes.data_as(C.POINTER(C.c_uint64)), n, arena, (C.c_uint64 * len(off))(*off), ncorpus,
                      max_len, out.ctypes.data_as(C.c_void_p), stride, lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                      info.ctypes.data_as(C.POINTER(C.c_uint32)))
    return [(out[i, :lens[i]].tobytes(), None if info[i, 0] == 10 else int(info[i, 0]), int(info[i, 1]),
             int(info[i, 2])) for i in range(n)]


def checksum(outs):
    """sum((D[k] + 1) * (k + 1) * G) mod 2^64 over the stream D of u32 sizes and
    bytes (tests/native/sim_mutate_main.cc prints the same)."""
    d = np.frombuffer(b"".join(struct.pack("<I", len(o)) + o for o in outs), dtype=np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        w = np.arange(1, len(d) + 1, dtype=np.uint64) * np.uint64(M.G)
        return int(((d + np.uint64(1)) * w).sum(dtype=np.uint64))


@pytest.fixture(scope="module")
def runs(sim):
    """Every case once, model and host build side by side: per (corpus,
    max_len, ncorpus) the first differences, what each operator did, how many
    results have max_len bytes, and the model's checksum. The bytes are dropped."""
    out = {}
    for name, entries in M.corpora().items():
        for max_len in M.MAX_LENS:
            for nc in M.NCORPUS:
                want = [M.mutate(SEED, i, entries, nc, max_len) for i in range(COUNT)]
                got = native(sim, entries, range(COUNT), nc, max_len)
                diff = [(i, "op %r / %r" % (g[1], w[1]), len(g[0]), len(w[0])) for i, (g, w) in enumerate(zip(got, want))
                        if g != (w[0], w[1], len(w[2]), sum(1 << o for o in set(w[2])))]
                ok, failed = [0] * 10, [0] * 10
                for o, op, fl in want:
                    assert len(o) <= max_len
                    if op is not None:
                        ok[op] += 1
                    for f in fl:
                        failed[f] += 1
                out[name, max_len, nc] = {"diff": diff[:5], "ok": ok, "failed": failed,
                                          "full": sum(len(o) == max_len for o, _, _ in want),
                                          "sum": checksum([o for o, _, _ in want])}
    return out


def test_host_build_matches_the_model(runs):
    assert len(runs) == 5 * len(M.MAX_LENS) * len(M.NCORPUS)
    bad = {k: v["diff"] for k, v in runs.items() if v["diff"]}
    assert not bad, bad


def test_the_cases_reach_every_operator_and_every_edge(runs):
    ok = [sum(v["ok"][o] for v in runs.values()) for o in range(10)]
    failed = [sum(v["failed"][o] for v in runs.values()) for o in range(10)]
    full = {m: sum(v["full"] for k, v in runs.items() if k[1] == m) for m in M.MAX_LENS}
    print("succeeded", dict(zip(M.OPS, ok)), "failed", dict(zip(M.OPS, failed)), "at max_len", full)
    assert all(n >= 50 for n in ok), dict(zip(M.OPS, ok))
    assert all(n >= 1 for n in failed), dict(zip(M.OPS, failed))
    assert all(n >= 1 for n in full.values()), full


def test_a_hundred_failures_return_the_base_unchanged(sim):
    """All ten operators fail on the empty testcase with max_len 0 and on
    nothing else (module docstring): 100 attempts, then the base."""
    entries = [b"", b"abcd"]
    for i in range(64):
        out, op, fl = M.mutate(SEED, i, entries, 1, 0)
        assert (out, op, len(fl)) == (b"", None, 100)
        assert set(fl) == set(range(10))
    assert [g[:3] for g in native(sim, entries, range(64), 1, 0)] == [(b"", None, 100)] * 64
    # a longer base is clipped to max_len first, and comes back clipped
    assert {M.mutate(SEED, i, entries, 2, 0)[0] for i in range(64)} == {b""}


def test_four_bytes_at_max_len_4_never_exhaust_the_attempts():
    """The other half of the module docstring's argument, on the digit-free
    corpora: the attempts stay far below 100 whenever the base has 2 bytes or more."""
    worst = 0
    for name in ("zero", "ff"):
        entries = M.corpora()[name]
        four = [e[:4] for e in entries if len(e) >= 4][:1]
        for i in range(COUNT):
            out, op, fl = M.mutate(SEED, i, four, 1, 4)
            assert op is not None and len(out) <= 4
            worst = max(worst, len(fl))
    print("most failed attempts before a success:", worst)
    assert worst < 100


def test_an_index_does_not_depend_on_its_neighbours(sim):
    entries = M.corpora()["mixed"]
    rng = np.random.default_rng(7)
    for max_len, nc in ((64, 10), (1028, 2), (16380, 10)):
        alone = {g: native(sim, entries, [g], nc, max_len)[0] for g in (0, 1, 77, 4095, 1 << 40)}
        order = list(alone) + [int(x) for x in rng.integers(0, 1 << 20, 50)]
        for _ in range(3):
            rng.shuffle(order)
            got = native(sim, entries, order, nc, max_len)
            for g, r in zip(order, got):
                if g in alone:
                    assert r == alone[g], (g, max_len, nc)
        for g in alone:
            assert alone[g][0] == M.testcase(SEED, g, entries, nc, max_len)


def test_host_build_runs_clean_under_the_sanitizers(tmp_path, runs):
    """The same cases through tests/native/sim_mutate_main.cc with
    AddressSanitizer and UndefinedBehaviorSanitizer: the arena holds exactly
    the entries in use and the output exactly max_len bytes."""
    exe = str(tmp_path / "sim_mutate_main")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-DWTFGPU_HOST_SIM", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(NATIVE, "sim_mutate_main.cc")])
    corp = M.corpora()
    blob = struct.pack("<I", len(corp))
    for entries in corp.values():
        arena, off = M.pack(entries)
        blob += struct.pack("<I", len(entries)) + struct.pack(f"<{len(off)}Q", *off) + arena
    blob += struct.pack(f"<I{len(M.MAX_LENS)}I", len(M.MAX_LENS), *M.MAX_LENS)
    blob += struct.pack(f"<I{len(M.NCORPUS)}I", len(M.NCORPUS), *M.NCORPUS)
    cases = tmp_path / "cases.bin"
    cases.write_bytes(blob)
    r = subprocess.run([exe, str(cases), hex(SEED), str(COUNT)], capture_output=True, text=True)
    lines = r.stdout.split()
    assert r.returncode == 0 and lines[-1:] == ["ok"], r.stdout[-2000:] + r.stderr[-4000:]
    assert lines[:-1] == ["%016x" % v["sum"] for v in runs.values()]


# ---- campaigns: the twin materialises the orders on the host, from the same header
from tests import tlv_harness as H  # noqa: E402

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")
HEVD = ("hevd", 12000, 512)
HEVD_KW = {"limit": 10_000_000, "max_len": 1028}
# `wtf_twin fuzz --name hevd --runs 12000 --lanes 512 --seed 1337 --limit 10000000 --max_len 1028`,
# streaming, without the flag, at the parent of the commit that added the flag
PARENT_COUNTS = {"execs": 12000, "retired": 1662784, "coverage": 729, "corpus": 17, "crashes": 2094,
                 "unique_crashes": 99, "timeouts": 0, "cr3": 0, "errors": 0, "error_retired": 0}


@pytest.fixture(scope="module")
def hevd_base(tmp_path_factory):
    return H.build_hevd_target(str(tmp_path_factory.mktemp("hevd") / "base"))


@needs_twin
def test_twin_campaigns_agree_and_reproduce(hevd_base, tmp_path):
    """Batch, streaming and --serial-mutation streaming campaigns with
    --device-mutate: the stream is indexed by the testcase's number alone, so
    all three are one campaign, and a second run gives it again."""
    dm = ("--device-mutate",)
    a = H.stream_campaign(hevd_base, str(tmp_path / "batch"), *HEVD, stream=False, extra=dm, **HEVD_KW)
    b = H.stream_campaign(hevd_base, str(tmp_path / "stream"), *HEVD, stream=True, extra=dm, **HEVD_KW)
    c = H.stream_campaign(hevd_base, str(tmp_path / "serial"), *HEVD, stream=True, extra=dm + ("--serial-mutation",),
                          **HEVD_KW)
    d = H.stream_campaign(hevd_base, str(tmp_path / "again"), *HEVD, stream=True, extra=dm, **HEVD_KW)
    assert a[0]["execs"] == HEVD[1] and a[0]["errors"] == 0
    assert a == b and a == c and a == d
    assert a[0]["crashes"] > 0 and a[0]["corpus"] > 1 and any(n.startswith("crash-0x") for n in a[1][1])


@needs_twin
def test_without_the_flag_the_campaign_is_the_parents(hevd_base, tmp_path):
    got = H.stream_campaign(hevd_base, str(tmp_path / "off"), *HEVD, stream=True, **HEVD_KW)
    assert got[0] == PARENT_COUNTS
    assert (len(got[1][0]), len(got[1][1])) == (17, 99)


def _refused(tmp_path, args, env=None):
    import subprocess as sp
    r = sp.run([H.TWIN, "fuzz", *args], capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    assert r.returncode != 0, r.stdout
    lines = [x for x in (r.stdout + r.stderr).splitlines() if "--device-mutate" in x]
    assert len(lines) == 1, r.stdout + r.stderr
    return lines[0]


@needs_twin
def test_refusals(hevd_base, tmp_path):
    tlv = H.build_target(str(tmp_path / "tlv"))
    common = ["--runs", "64", "--lanes", "16", "--device-mutate"]
    assert "mutator of its own" in _refused(tmp_path, ["--name", "tlv_server", "--target", tlv, *common])
    # the environment variable is the flag
    assert "mutator of its own" in _refused(tmp_path, ["--name", "tlv_server", "--target", tlv, "--runs", "64",
                                                        "--lanes", "16"], env={"WTFGPU_DEVICE_MUTATE": "1"})
    hevd = ["--name", "hevd", "--target", hevd_base, *common]
    assert "--world > 1" in _refused(tmp_path, [*hevd, "--rank", "0", "--world", "2"])
    assert "--address" in _refused(tmp_path, [*hevd, "--address", "tcp://127.0.0.1:1"])
    assert "--module-so" in _refused(tmp_path, [*hevd, "--module-so", "/nonexistent.so"])
    r = __import__("subprocess").run([H.TWIN, "master", "--name", "hevd", "--target", hevd_base, "--device-mutate",
                                      "--address", "tcp://127.0.0.1:1", "--nodes", "1"], capture_output=True, text=True,
                                     timeout=60)
    assert r.returncode != 0 and "--device-mutate" in r.stderr
