"""`distill` on the CPU: the rule of wtf_amd/csrc/engine_distill.h built for the
host (tests/native/sim_distill.cc: distill_host) against its restatement in
Python (tests/distill_model.py), the properties the header promises, and the
session (`wtf_twin distill`) on the tlv and HEVD test corpora: the same output
at every lane count, batched and streaming, equal to the model's cover of the
sets `wtf_twin run --full-coverage` reports."""
import ctypes as C
import filecmp
import functools
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import distill_model as M
from tests import hevd_inputs, tlv_inputs
from tests import tlv_harness as H

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
SOURCES = [os.path.join(NATIVE, "sim_distill_main.cc"), os.path.join(NATIVE, "sim_distill.cc")]
# 1,500 tlv inputs hold one that covers every rip of the eligible ones (kept
# would be 1); among the first 500 none does
TLV_COUNT, HEVD_COUNT = 500, 400
SUMMARY_KEYS = ("mode", "inputs", "eligible", "kept", "universe", "entries", "rounds", "excluded", "on_device")

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")


# ---- the rule

@functools.lru_cache(maxsize=None)
def instances():
    """Every directed shape and 200 random instances, with the model's answer:
    [(name, sets, eligible, (index, gain, universe))], computed once."""
    out = [(name, sets, el, M.distill(sets, el)) for name, sets, el in M.shapes()]
    rng = random.Random(0xD157)
    for k in range(200):
        sets, el = M.random_instance(rng)
        out.append((f"random{k}", sets, el, M.distill(sets, el)))
    return out


def encode(sets, eligible):
    off, val = M.flatten(sets)
    blob = struct.pack("<II", len(sets), 0 if eligible is None else 1) + off.tobytes()
    blob += val[:int(off[-1])].tobytes()
    return blob + (b"" if eligible is None else bytes(int(bool(e)) for e in eligible))


def line_of(answer, rc=0):
    index, gain, universe = answer
    return " ".join(["%d %d %d" % (rc, universe, len(index))] + ["%d:%d" % p for p in zip(index, gain)])


def run_program(exe):
    blob = b"".join(encode(sets, el) for _, sets, el, _ in instances())
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], input=blob, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.decode().split("\n")[:-1]
    want = [line_of(a) for _, _, _, a in instances()]
    bad = [(instances()[i][0], g[:80], w[:80]) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, bad[:5]


def test_host_build_matches_the_model(tmp_path):
    exe = str(tmp_path / "sim_distill")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-o", exe, *SOURCES])
    run_program(exe)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same cases with -fsanitize=address,undefined: every input and
    output in a heap buffer of exactly its size."""
    exe = str(tmp_path / "sim_distill_san")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, *SOURCES])
    run_program(exe)


def test_the_model_has_the_promised_properties():
    """Union preserved, gains >= 1 and non-increasing, idempotence; and the
    directed shapes come out as their docstrings say."""
    by = {}
    for name, sets, el, (index, gain, universe) in instances():
        M.check_properties(sets, el, index, gain, universe)
        by[name] = (index, gain, universe)
    assert by["identical"] == ([1], [70], 70)
    assert by["far_tie"][0][:2] == [5, 70] and by["far_tie"][1][:2] == [30, 30]
    assert by["chain"] == ([64], [65], 65)
    assert by["order_dependent"] == ([2, 1, 0], [8, 4, 3], 15)
    assert by["singletons"] == (list(range(300)), [1] * 300, 300)
    assert by["all_ineligible"] == ([], [], 0) and by["none"] == ([], [], 0) and by["empty_sets"] == ([], [], 0)
    assert all(i % 3 != 1 for i in by["eligible_mixed"][0]) and len(by["eligible_mixed"][0]) >= 2
    for U in M.UNIVERSES:
        assert by[f"universe{U}"][2] == U
    assert sum(1 for n, *_ in instances() if n.startswith("random")) == 200
    assert sum(len(a[0]) >= 3 for *_, a in instances()[-200:]) >= 50  # the random ones are not trivial


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simdis") / "libsimdistill.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_distill.cc")])
    L = C.CDLL(so)
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.sim_distill.argtypes = [C.c_uint32, p64, p64, C.POINTER(C.c_uint8), p32, p32, p32, p64]
    L.sim_distill.restype = C.c_int
    return L


def argument_errors():
    """(what, n, offsets, values, eligible-or-None, null output pointers?) of
    every argument error wtfgpu_distill and distill_host name."""
    good_off, good_val = [0, 2, 3], [5, 9, 7]
    return [("null offsets", 2, None, good_val, False, False),
            ("null values", 2, good_off, None, False, False),
            ("null outputs", 2, good_off, good_val, True, False),
            ("null counts", 2, good_off, good_val, False, True),
            ("offsets[0] != 0", 2, [1, 2, 3], good_val, False, False),
            ("offsets decrease", 2, [0, 3, 2], good_val, False, False),
            ("equal neighbours", 2, good_off, [5, 5, 7], False, False),
            ("descending", 2, good_off, [9, 5, 7], False, False),
            ("descending above 2^63", 1, [0, 2], [(1 << 63) + 1, 1 << 63], False, False),
            ("2^32 entries", 1, [0, 1 << 32], [1], False, False)]


def test_host_argument_errors(sim):
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    for what, n, off, val, no_out, no_counts in argument_errors():
        o = None if off is None else np.array(off, dtype=np.uint64)
        v = None if val is None else np.array(val, dtype=np.uint64)
        oi, og = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
        kept, uni = C.c_uint32(77), C.c_uint64(77)
        rc = sim.sim_distill(n, None if o is None else o.ctypes.data_as(p64), None if v is None else v.ctypes.data_as(p64),
                             None, None if no_out else oi.ctypes.data_as(p32), None if no_out else og.ctypes.data_as(p32),
                             None if no_counts else C.byref(kept), None if no_counts else C.byref(uni))
        assert rc == -1, what
    kept, uni = C.c_uint32(77), C.c_uint64(77)
    assert sim.sim_distill(0, None, None, None, None, None, C.byref(kept), C.byref(uni)) == 0
    assert kept.value == 0 and uni.value == 0


# ---- the session on the twin

def distill(exe, target, name, inputs, out, lanes, extra=(), env=None, results=None):
    cmd = [exe, "distill", "--name", name, "--target", target, "--input", inputs, "--output", out,
           "--lanes", str(lanes), "--limit", "100000", *extra]
    if results:
        cmd += ["--results", results]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(x) for x in open(results)] if results else None
    return H.last_json(r.stdout), rows


def kept_names(rows):
    return [r["input"] for r in sorted((r for r in rows if r["kept"]), key=lambda r: r["order"])]


@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    """{name: (target, inputs dir)}: the tlv and HEVD snapshots and their test corpora."""
    d = tmp_path_factory.mktemp("distill")
    tlv = H.build_target(str(d / "tlv"))
    tlv_inputs.write_inputs(str(d / "tlv_in"), TLV_COUNT)
    hevd = H.build_hevd_target(str(d / "hevd"))
    hevd_inputs.write_inputs(str(d / "hevd_in"), HEVD_COUNT)
    return {"tlv_server": (tlv, str(d / "tlv_in")), "hevd": (hevd, str(d / "hevd_in"))}


@pytest.fixture(scope="module")
def twin_reference(corpora, tmp_path_factory):
    """`wtf_twin distill` once a corpus at 64 lanes: {name: (summary, rows, output dir)}."""
    d = tmp_path_factory.mktemp("distill_ref")
    out = {}
    for name, (target, inputs) in corpora.items():
        o = str(d / name)
        st, rows = distill(H.TWIN, target, name, inputs, o, 64, results=o + ".jsonl")
        out[name] = (st, rows, o)
    return out


@needs_twin
@pytest.mark.parametrize("name", ["tlv_server", "hevd"])
def test_twin_distill_is_the_model_on_the_replayed_sets(corpora, twin_reference, tmp_path, name):
    target, inputs = corpora[name]
    st, rows, out = twin_reference[name]
    print(name, {k: st[k] for k in SUMMARY_KEYS}, "replay_ms", st["replay_ms"], "cover_ms", st["cover_ms"])
    # rank order: (file size, file name)
    files = sorted(os.listdir(inputs), key=lambda f: (os.path.getsize(os.path.join(inputs, f)), f))
    assert [r["input"] for r in rows] == files
    assert [r["bytes"] for r in rows] == [os.path.getsize(os.path.join(inputs, f)) for f in files]
    # the sets, as `run --full-coverage` reports them
    res = {r["input"]: r for r in H.run(H.TWIN, target, inputs, str(tmp_path / "run.jsonl"), lanes=64, name=name)}
    sets = [sorted(res[f]["coverage"]) for f in files]
    eligible = [res[f]["result"] == "ok" and not res[f]["error"] for f in files]
    assert [r["eligible"] for r in rows] == eligible and [r["values"] for r in rows] == [len(s) for s in sets]
    assert [r["result"] for r in rows] == ["error" if res[f]["error"] else res[f]["result"] for f in files]
    index, gain, universe = M.distill(sets, eligible)
    M.check_properties(sets, eligible, index, gain, universe)
    assert kept_names(rows) == [files[i] for i in index]
    assert [r["gain"] for r in sorted((r for r in rows if r["kept"]), key=lambda r: r["order"])] == gain
    assert all(r["order"] == -1 and r["gain"] == 0 for r in rows if not r["kept"])
    assert (st["kept"], st["universe"], st["inputs"], st["eligible"]) == (len(index), universe, len(files), sum(eligible))
    assert st["entries"] == sum(len(s) for s, e in zip(sets, eligible) if e) and st["rounds"] == len(index) + 1
    assert st["mode"] == "distill" and st["on_device"] is False
    # it cannot pass vacuously
    assert 2 <= st["kept"] <= st["eligible"] // 2
    assert st["excluded"]["crash"] >= 1
    assert sum(st["excluded"].values()) == st["inputs"] - st["eligible"]
    # the output directory: exactly the kept files, byte for byte
    assert sorted(os.listdir(out)) == sorted(kept_names(rows))
    for f in os.listdir(out):
        assert filecmp.cmp(os.path.join(out, f), os.path.join(inputs, f), shallow=False)
    # its coverage is the eligible inputs' coverage
    after = H.run(H.TWIN, target, out, str(tmp_path / "after.jsonl"), lanes=64, name=name)
    union = set().union(*[set(s) for s, e in zip(sets, eligible) if e])
    assert set().union(*[set(r["coverage"]) for r in after]) == union and len(union) == universe
    # distilling the output keeps all of it
    st2, rows2 = distill(H.TWIN, target, name, out, str(tmp_path / "again"), 64, results=str(tmp_path / "again.jsonl"))
    assert st2["kept"] == st2["inputs"] == st["kept"] and st2["universe"] == universe
    assert sorted(kept_names(rows2)) == sorted(kept_names(rows)) and sorted(r["gain"] for r in rows2) == sorted(gain)


@needs_twin
@pytest.mark.parametrize("lanes,stream", [(1, "0"), (1, "1"), (7, "0"), (7, "1"), (512, "0"), (512, "1")])
@pytest.mark.parametrize("name", ["tlv_server", "hevd"])
def test_lane_count_and_path_do_not_change_the_output(corpora, twin_reference, tmp_path, name, lanes, stream):
    target, inputs = corpora[name]
    want_st, want_rows, want_out = twin_reference[name]
    out = str(tmp_path / "out")
    st, rows = distill(H.TWIN, target, name, inputs, out, lanes, env={"WTF_TWIN_STREAM": stream},
                       results=str(tmp_path / "r.jsonl"))
    assert rows == want_rows
    assert {k: st[k] for k in SUMMARY_KEYS} == {k: want_st[k] for k in SUMMARY_KEYS}
    assert sorted(os.listdir(out)) == sorted(os.listdir(want_out))


@needs_twin
@pytest.mark.parametrize("case", ["non-empty output", "output is a file", "no --output", "no inputs", "--address",
                                  "master", "--world"])
def test_refusals(corpora, tmp_path, case):
    """One line, a non-zero exit, nothing written."""
    target, inputs = corpora["hevd"]
    out, results = tmp_path / "out", tmp_path / "r.jsonl"
    args = ["distill", "--name", "hevd", "--target", target, "--input", inputs, "--output", str(out),
            "--results", str(results), "--lanes", "16", "--limit", "100000"]
    if case == "non-empty output":
        out.mkdir()
        (out / "precious").write_bytes(b"keep me")
    elif case == "output is a file":
        out.write_bytes(b"keep me")
    elif case == "no --output":
        del args[args.index("--output"):args.index("--output") + 2]
    elif case == "no inputs":
        (tmp_path / "empty").mkdir()
        args[args.index("--input") + 1] = str(tmp_path / "empty")
    elif case == "--address":
        args += ["--address", "tcp://127.0.0.1:1"]
    elif case == "master":
        args.insert(1, "master")
    elif case == "--world":
        args += ["--world", "2"]
    r = subprocess.run([H.TWIN, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    text = [x for x in (r.stdout + r.stderr).splitlines() if x.strip()]
    assert len(text) == 1 and "distill" in text[0], (r.stdout, r.stderr)
    assert not results.exists() and '"mode"' not in r.stdout
    if case == "non-empty output":
        assert os.listdir(out) == ["precious"] and (out / "precious").read_bytes() == b"keep me"
    elif case == "output is a file":
        assert out.read_bytes() == b"keep me"
    else:
        assert not out.exists()
