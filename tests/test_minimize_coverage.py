"""`minimize --keep-coverage` on the CPU: the rule of
wtf_amd/csrc/engine_covkeep.h built for the host (tests/native/sim_covkeep.cc)
against its restatement in Python (tests/covkeep_model.py) on tables filled the
way the engine fills them, the same as a stand-alone program under the
sanitizers, and the session (`wtf_twin minimize --keep-coverage`) on HEVD and
tlv_server inputs that end ok: the same bytes at every lane count, batched and
streaming, an output whose whole coverage set holds the input's, a fixed point,
and the refusals."""
import ctypes as C
import functools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import covkeep_model as M
from tests import tlv_harness as H
from tests.hevd_inputs import crafted
from wtf_amd.tools.hevd import testcase as hevd_testcase
from wtf_amd.tools.tlv import packets_json

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CXX = os.environ.get("CXX", "g++")
TABLE_H = 64
TARGET_SIZES = (0, 1, 63, 64, 65, 200)

needs_twin = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")


# ---- the inputs of the sessions (tests/test_gpu_minimize_coverage.py runs the same ones)

def hevd_inputs() -> dict[str, bytes]:
    """Non-crashing entries of hevd_inputs.crafted(), padded. integer_big: the
    integer-overflow handler's in-range copy of 300 bytes, 77 bytes the handler
    never reads behind it. www_ok_pad: write-what-where between two user
    addresses, 93 bytes behind its two pointers."""
    return {
        "integer_big": hevd_testcase(0x222017, struct.pack("<I", 300) + b"i" * 300 + b"Q" * 77),
        "www_ok_pad": crafted()["write_what_where_ok"] + b"W" * 93,
    }


def tlv_inputs() -> dict[str, bytes]:
    """Eleven packets that end ok: allocations, edits and deletes, several of
    them repeating what an earlier one already covered."""
    return {
        "multi": packets_json([(0, 1, 8, b"a" * 8), (0, 2, 16, b"b" * 16), (1, 1, 4, b"abcd"), (0, 3, 12, b"c" * 12),
                               (1, 3, 6, b"efghij"), (2, 2, 0, b""), (0, 4, 8, b"d" * 8), (1, 1, 4, b"wxyz"),
                               (2, 1, 0, b""), (0, 1, 0, b""), (1, 4, 2, b"zz")]),
    }


CASES = [("hevd", "integer_big"), ("hevd", "www_ok_pad"), ("tlv_server", "multi")]


# ---- the rule

@functools.lru_cache(maxsize=None)
def rule_cases():
    """[(name, table, target)]: every directed table against targets of every
    size, drawn from the union of the sets, the tables' stale and dropped
    values, and values in no set."""
    tabs = M.tables(TABLE_H)
    union = [v for _, t, _ in tabs for v in t.live()]
    extras = [v for _, _, x in tabs for v in x]
    rng = random.Random(0x7A26E7)
    out = []
    for name, t, x in tabs:
        own = [t.live(), t.live()[::3]]  # inside the set: nothing missing
        for tgt in M.targets(union, extras, rng, TARGET_SIZES) + [sorted(set(x))] + own:
            out.append((f"{name}/{len(tgt)}", t, tgt))
    return out


def check_the_directed_tables():
    """The tables and targets are what the cases need: sizes, overflow, stale
    values in the probe path, and both outcomes."""
    tabs = {name: (t, x) for name, t, x in M.tables(TABLE_H)}
    assert [tabs[n][0].count for n in ("empty", "one", "cap_minus_one", "cap")] == [0, 1, 47, 48] and M.cap(64) == 48
    assert tabs["overflowed"][0].overflow and not tabs["cap"][0].overflow
    # stale values equal to target values sit in the probe path and read as absent
    for name in ("stale_in_path", "stale_wrap", "stale_same_values"):
        t, x = tabs[name]
        stale = [v for v in x if v in t.rip and v not in t.live()]
        assert stale and not any(t.has(v) for v in stale), name
    t, x = tabs["stale_same_values"]
    assert sum(t.has(v) for v in x) == 20  # the same values again, live this time
    # the probe agrees with the set's definition everywhere
    for name, t, tgt in rule_cases():
        assert [t.has(v) for v in tgt] == [v in set(t.live()) for v in tgt], name
    sizes = {len(tgt) for _, _, tgt in rule_cases()}
    assert set(TARGET_SIZES) <= sizes
    miss = [M.missing(t.live(), tgt) for _, t, tgt in rule_cases()]
    assert any(m == 0 for m, (_, _, tgt) in zip(miss, rule_cases()) if tgt) and any(m > 0 for m in miss)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simkeep") / "libsimcovkeep.so")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(NATIVE, "sim_covkeep.cc")])
    L = C.CDLL(so)
    U32, U64, p32, p64 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.sim_covkeep_mix64.argtypes, L.sim_covkeep_mix64.restype = [U64], U64
    L.sim_covkeep_cap.argtypes, L.sim_covkeep_cap.restype = [U32], U32
    L.sim_covkeep_table.argtypes = [p64, p32, U32, U32, p64, U32, C.POINTER(C.c_uint8)]
    L.sim_covkeep_table.restype = U32
    L.sim_covkeep_sorted.argtypes, L.sim_covkeep_sorted.restype = [p64, U64, p64, U64], U64
    L.sim_covkeep_keeps.argtypes, L.sim_covkeep_keeps.restype = [C.c_int, C.c_int, C.c_int, U64], C.c_int
    return L


def test_host_build_matches_the_model(sim):
    check_the_directed_tables()
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rng = random.Random(5)
    for v in [0, 1, M.M64, 0x140001000] + [rng.getrandbits(64) for _ in range(200)]:
        assert sim.sim_covkeep_mix64(v) == M.mix64(v)
    for H_ in (1, 2, 4, 64, 8192):
        assert sim.sim_covkeep_cap(H_) == M.cap(H_)
    for name, t, tgt in rule_cases():
        rip, gen = np.array(t.rip, dtype=np.uint64), np.array(t.gen, dtype=np.uint32)
        tg = np.array(tgt + [0], dtype=np.uint64)  # (a pointer to pass for the empty target)
        live = np.array(t.live() + [0], dtype=np.uint64)
        present = np.zeros(len(tgt) + 1, dtype=np.uint8)
        got = sim.sim_covkeep_table(rip.ctypes.data_as(p64), gen.ctypes.data_as(p32), t.H, t.g, tg.ctypes.data_as(p64),
                                    len(tgt), present.ctypes.data_as(C.POINTER(C.c_uint8)))
        want = M.missing(t.live(), tgt)
        assert got == want, name
        assert present[:len(tgt)].tolist() == [int(t.has(v)) for v in tgt], name
        assert sim.sim_covkeep_sorted(live.ctypes.data_as(p64), len(t.live()), tg.ctypes.data_as(p64), len(tgt)) == want
    for ok in (0, 1):
        for err in (0, 1):
            for ovf in (0, 1):
                for miss in (0, 1, 1 << 40):
                    assert bool(sim.sim_covkeep_keeps(ok, err, ovf, miss)) == M.keeps(bool(ok), bool(err), bool(ovf), miss)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same comparison in a program of its own, built with
    -fsanitize=address,undefined: every table, set and target in a heap
    buffer of exactly its size."""
    exe = str(tmp_path / "sim_covkeep_san")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(NATIVE, "sim_covkeep_main.cc"),
                           os.path.join(NATIVE, "sim_covkeep.cc")])
    blob, want = b"", []
    for _, t, tgt in rule_cases():
        live = t.live()
        blob += struct.pack("<IIII", t.H, t.g, len(live), len(tgt))
        blob += np.array(t.rip, dtype=np.uint64).tobytes() + np.array(t.gen, dtype=np.uint32).tobytes()
        blob += np.array(live, dtype=np.uint64).tobytes() + np.array(tgt, dtype=np.uint64).tobytes()
        m = M.missing(live, tgt)
        want.append("%d %d %s" % (m, m, "".join(str(int(t.has(v))) for v in tgt)))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want


# ---- the session on the twin

def minimize_cmd(exe, target, name, src, out, lanes, extra=()):
    return [exe, "minimize", "--keep-coverage", "--name", name, "--target", target, "--input", src, "--output", out,
            "--lanes", str(lanes), "--limit", "100000", *extra]


def keep_coverage(exe, target, name, src, out, lanes=64, extra=(), env=None):
    r = subprocess.run(minimize_cmd(exe, target, name, src, out, lanes, extra), capture_output=True, text=True,
                       timeout=600, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return H.last_json(r.stdout)


def coverage_of(target, name, path, work, edges=False):
    """(result row, whole coverage set) of one file, as `wtf_twin run --full-coverage` reports them."""
    os.makedirs(work, exist_ok=True)
    d = os.path.join(work, "in")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "tc"), "wb") as f:
        f.write(open(path, "rb").read())
    row = H.run(H.TWIN, target, d, os.path.join(work, "run.jsonl"), lanes=1, name=name,
                extra=("--edges",) if edges else ())[0]
    return row, set(row["coverage"])


@pytest.fixture(scope="module")
def targets(tmp_path_factory):
    """{target name: (target dir, {input name: path})}"""
    d = tmp_path_factory.mktemp("keepcov")
    out = {"hevd": (H.build_hevd_target(str(d / "hevd")), {}), "tlv_server": (H.build_target(str(d / "tlv")), {})}
    for tname, inputs in (("hevd", hevd_inputs()), ("tlv_server", tlv_inputs())):
        for name, data in inputs.items():
            p = str(d / name)
            with open(p, "wb") as f:
                f.write(data)
            out[tname][1][name] = p
    return out


@pytest.fixture(scope="module")
def reference(targets, tmp_path_factory):
    """`wtf_twin minimize --keep-coverage` once an input, with and without
    --edges, at 64 lanes: {(input, edges): (summary, output bytes)}."""
    d = tmp_path_factory.mktemp("keepcov_ref")
    out = {}
    for tname, name in CASES:
        target, paths = targets[tname]
        for edges in (False, True):
            o = str(d / f"{name}{int(edges)}.min")
            st = keep_coverage(H.TWIN, target, tname, paths[name], o, extra=("--edges",) if edges else ())
            out[(name, edges)] = (st, open(o, "rb").read())
    return out


@needs_twin
@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("tname,name", CASES)
def test_the_output_is_smaller_and_covers_the_input(targets, reference, tmp_path, tname, name, edges):
    target, paths = targets[tname]
    st, got = reference[(name, edges)]
    data = open(paths[name], "rb").read()
    print(name, edges, {k: v for k, v in st.items() if k != "executor"})
    # the conditions the inputs were chosen for
    row, T = coverage_of(target, tname, paths[name], str(tmp_path / "a"), edges)
    assert row["result"] == "ok" and not row["error"]
    assert len(got) < len(data) and st["output_bytes"] == len(got) and st["input_bytes"] == len(data)
    assert st["ok_but_missing"] >= 1  # the coverage rule decided: some candidate ended ok and lost a value
    # the summary
    assert st["mode"] == "coverage" and st["cov_on_device"] is False and st["on_device"] is False
    assert st["values"] == len(T) and st["overflowed"] == 0 and st["crash"] == ""
    assert st["cov_readback_values"] > st["values"]  # every candidate's set came back
    assert st["rounds"] == st["remove_rounds"] + st["zero_rounds"] and not st["stopped_by_rounds"]
    # the output ends ok and covers at least what the input covered
    out_path = str(tmp_path / "out")
    with open(out_path, "wb") as f:
        f.write(got)
    row2, S = coverage_of(target, tname, out_path, str(tmp_path / "b"), edges)
    assert row2["result"] == "ok" and not row2["error"]
    assert S >= T and st["output_values"] == len(S)
    # a fixed point: the session on its own output changes nothing
    st2 = keep_coverage(H.TWIN, target, tname, out_path, str(tmp_path / "again"), extra=("--edges",) if edges else ())
    assert open(str(tmp_path / "again"), "rb").read() == got
    assert st2["values"] == len(S) and st2["output_bytes"] == st2["input_bytes"] == len(got)


@needs_twin
def test_the_inputs_exercise_zero_rounds_and_supersets(reference):
    """Non-vacuity over the cases: a ZERO round matches on HEVD (a session with
    a match runs at least one more ZERO round after it), --edges gives another
    target, and one output covers strictly more than its input (keeping is a
    superset, not equality)."""
    assert reference[("integer_big", False)][0]["zero_rounds"] >= 2
    assert reference[("www_ok_pad", False)][0]["zero_rounds"] >= 2
    assert reference[("multi", False)][0]["zero_rounds"] == 0  # feeds have no ZERO
    for _, name in CASES:
        assert reference[(name, True)][0]["values"] > reference[(name, False)][0]["values"]
    assert any(st["output_values"] > st["values"] for st, _ in reference.values())


@needs_twin
@pytest.mark.parametrize("lanes", [1, 7, 512])
@pytest.mark.parametrize("path", ["batched", "streaming"])
@pytest.mark.parametrize("tname,name", CASES)
def test_lane_count_and_path_do_not_change_the_output(targets, reference, tmp_path, tname, name, path, lanes):
    target, paths = targets[tname]
    want_st, want = reference[(name, False)]
    out = str(tmp_path / "min")
    st = keep_coverage(H.TWIN, target, tname, paths[name], out, lanes=lanes, env={"WTF_TWIN_STREAM": "1"},
                       extra=("--slice-steps", "0") if path == "batched" else ())
    assert open(out, "rb").read() == want
    keys = ("values", "output_values", "rounds", "remove_rounds", "zero_rounds", "candidates", "skipped",
            "ok_but_missing", "overflowed", "cov_readback_values")
    assert {k: st[k] for k in keys} == {k: want_st[k] for k in keys}


@needs_twin
def test_the_default_output_path(targets, reference, tmp_path):
    target, paths = targets["hevd"]
    src = str(tmp_path / "www")
    with open(src, "wb") as f:
        f.write(open(paths["www_ok_pad"], "rb").read())
    r = subprocess.run([H.TWIN, "minimize", "--keep-coverage", "--name", "hevd", "--target", target, "--input", src,
                        "--lanes", "16", "--limit", "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(src + ".min", "rb").read() == reference[("www_ok_pad", False)][1]


@needs_twin
@pytest.mark.parametrize("case", ["crash", "timeout", "cr3", "cov-set", "fuzz", "run", "distill"])
def test_refusals(targets, tmp_path, case):
    """One line, a non-zero exit, no candidate run (no output file)."""
    target, paths = targets["hevd"]
    data = {"crash": crafted()["integer_wrap"], "cr3": crafted()["wait_swapcontext"]}.get(case)
    src = str(tmp_path / "in")
    with open(src, "wb") as f:
        f.write(data if data else open(paths["integer_big"], "rb").read())
    args = ["minimize", "--keep-coverage", "--name", "hevd", "--target", target, "--input", src, "--lanes", "16",
            "--limit", "100000"]
    if case == "timeout":
        args[args.index("--limit") + 1] = "50"
    elif case == "cov-set":
        args += ["--cov-set", "16"]
    elif case in ("fuzz", "run"):
        args[0] = case
    elif case == "distill":
        args = ["distill", "--output", str(tmp_path / "kept")] + args[1:]
    r = subprocess.run([H.TWIN, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    text = [x for x in (r.stdout + r.stderr).splitlines() if x.strip()]
    assert len(text) == 1, (r.stdout, r.stderr)
    assert not os.path.exists(src + ".min") and "candidates" not in r.stdout
    if case == "crash":
        assert "crashes" in text[0] and "drop --keep-coverage" in text[0]
    elif case == "timeout":
        assert "does not end ok (timedout)" in text[0]
    elif case == "cr3":
        assert "does not end ok (cr3)" in text[0]
    elif case == "cov-set":
        assert "--cov-set" in text[0] and "filled up" in text[0]
    else:
        assert "--keep-coverage is for minimize" in text[0]


@needs_twin
def test_without_the_flag_nothing_changes(targets, tmp_path):
    """A non-crashing input is still refused with the old line, and a crashing
    one is minimised as before (the summary only gains "mode")."""
    target, paths = targets["hevd"]
    r = subprocess.run([H.TWIN, "minimize", "--name", "hevd", "--target", target, "--input", paths["integer_big"],
                        "--lanes", "16", "--limit", "100000"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert r.stdout.strip() == f"minimize: {paths['integer_big']} does not crash (ok): nothing to minimise"
    assert not os.path.exists(paths["integer_big"] + ".min")
    src = str(tmp_path / "wrap")
    with open(src, "wb") as f:
        f.write(crafted()["integer_wrap"])
    r = subprocess.run([H.TWIN, "minimize", "--name", "hevd", "--target", target, "--input", src, "--lanes", "16",
                        "--limit", "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = H.last_json(r.stdout)
    assert st["mode"] == "crash" and st["crash"] and "values" not in st and "cov_on_device" not in st
    assert st["output_bytes"] < st["input_bytes"]
