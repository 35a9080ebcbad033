"""The corpus distiller on the GPU: wtfgpu_distill (k_distill_ids,
k_distill_gain, k_distill_take) against tests/distill_model.py through the C
ABI, exactly; the argument errors; and `wtfgpu distill` against `wtf_twin
distill` on the tlv and HEVD test corpora.

The context has no lanes and no snapshot. k_distill_gain counts a set with 16
lanes, four sets a wave and 16 a block, so calls of 1, 63, 64, 65 and 257 sets
give partial waves and blocks, full ones, and both; every call mixes set sizes
of 0, 1, 63, 64, 65, 300 and 8,192 inside each block."""
import os
import subprocess

import pytest

from tests import distill_model as M
from tests import tlv_harness as H
from tests.test_distill import SUMMARY_KEYS, TLV_COUNT, HEVD_COUNT, argument_errors, distill, instances, kept_names
from wtf_amd import abi

pytestmark = pytest.mark.gpu

ERR_OOM = -3
DIRECTED = [name for name, *_ in M.shapes()]


@pytest.fixture(scope="module")
def eng():
    from wtf_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def by_name(name):
    return next(x for x in instances() if x[0] == name)


@pytest.mark.parametrize("name", DIRECTED)
def test_kernels_match_the_model(eng, name):
    """out_index, out_gain, kept and universe are the model's, exactly.
    `singletons` is 300 rounds of gain 1 in index order: rounds are queued 64 a
    batch (DIS_BATCH, engine_kernels.h), so it crosses four batch boundaries,
    and `mixed257` crosses as many as its cover has rounds / 64."""
    _, sets, el, want = by_name(name)
    assert eng.distill(sets, el) == want


def test_kernels_match_the_model_on_random_instances(eng):
    bad = []
    for name, sets, el, want in instances()[-200:]:
        got = eng.distill(sets, el)
        if got != want:
            bad.append((name, got, want))
    assert not bad, bad[:3]


def test_the_same_call_gives_the_same_output_again_and_on_queue_1(eng):
    for name in ("mixed257", "far_tie", "universe4097"):
        _, sets, el, want = by_name(name)
        assert eng.distill(sets, el) == want
        assert eng.distill(sets, el) == want
        eng.select_queue(1)
        try:
            assert eng.distill(sets, el) == want
        finally:
            eng.select_queue(0)


def test_argument_errors_queue_nothing_and_a_valid_call_still_works(eng):
    for what, n, off, val, no_out, no_counts in argument_errors():
        rc, index, gain, universe = eng.distill_rc(n, off, val, None, want_out=not no_out, want_counts=not no_counts)
        assert rc == abi.ERR_INVALID and index == [] and universe == 0, what
    # a null eligible array is every set; n == 0 is no error, with nothing kept
    assert eng.distill_rc(0, None, None, None) == (0, [], [], 0)
    assert eng.distill_rc(0, None, None, None, want_out=False) == (0, [], [], 0)
    _, sets, el, want = by_name("order_dependent")
    assert eng.distill(sets, el) == want
    assert eng.distill(sets, [True, False, True]) == M.distill(sets, [True, False, True])


# ---- `wtfgpu distill` against `wtf_twin distill`

@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    from tests import hevd_inputs, tlv_inputs

    d = tmp_path_factory.mktemp("gpu_distill")
    tlv = H.build_target(str(d / "tlv"))
    tlv_inputs.write_inputs(str(d / "tlv_in"), TLV_COUNT)
    hevd = H.build_hevd_target(str(d / "hevd"))
    hevd_inputs.write_inputs(str(d / "hevd_in"), HEVD_COUNT)
    return {"tlv_server": (tlv, str(d / "tlv_in")), "hevd": (hevd, str(d / "hevd_in"))}


@pytest.fixture(scope="module")
def twin(corpora, tmp_path_factory):
    """{(name, edges): (summary, rows, output dir)} of `wtf_twin distill`."""
    d = tmp_path_factory.mktemp("gpu_distill_twin")
    out = {}
    for name, (target, inputs) in corpora.items():
        for edges in (False, True):
            o = str(d / (name + ("_edges" if edges else "")))
            st, rows = distill(H.TWIN, target, name, inputs, o, 64, extra=("--edges",) if edges else (),
                               results=o + ".jsonl")
            assert 2 <= st["kept"] <= st["eligible"] // 2 and st["excluded"]["crash"] >= 1
            out[name, edges] = (st, rows, o)
    return out


CONFIGS = {
    "l64": (64, (), None, True),
    "l4096": (4096, (), None, True),
    "host": (4096, (), {"WTFGPU_DISTILL_HOST": "1"}, False),
    "attrib": (4096, ("--device-attrib",), None, True),
    "attrib_host": (64, ("--device-attrib",), {"WTFGPU_DISTILL_HOST": "1"}, False),
    "edges": (4096, ("--edges",), None, True),
    "edges_attrib": (64, ("--edges", "--device-attrib"), None, True),
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["tlv_server", "hevd"])
def test_wtfgpu_distill_equals_the_twin(corpora, twin, tmp_path, name, config):
    lanes, extra, env, on_device = CONFIGS[config]
    target, inputs = corpora[name]
    want_st, want_rows, want_out = twin[name, "--edges" in extra]
    out = str(tmp_path / "out")
    st, rows = distill(H.WTFGPU, target, name, inputs, out, lanes, extra=extra, env=env,
                       results=str(tmp_path / "r.jsonl"))
    print(name, config, {k: st[k] for k in SUMMARY_KEYS}, "replay_ms", st["replay_ms"], "cover_ms", st["cover_ms"])
    assert kept_names(rows) == kept_names(want_rows)
    assert rows == want_rows
    keys = [k for k in SUMMARY_KEYS if k != "on_device"]
    assert {k: st[k] for k in keys} == {k: want_st[k] for k in keys}
    assert st["on_device"] is on_device and want_st["on_device"] is False
    assert sorted(os.listdir(out)) == sorted(os.listdir(want_out))
    for f in os.listdir(out):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(inputs, f), "rb").read()


def test_a_coverage_set_that_fills_up_is_refused(corpora, tmp_path):
    target, inputs = corpora["tlv_server"]
    out = tmp_path / "out"
    r = subprocess.run([H.WTFGPU, "distill", "--name", "tlv_server", "--target", target, "--input", inputs,
                        "--output", str(out), "--results", str(tmp_path / "r.jsonl"), "--lanes", "64",
                        "--limit", "100000", "--cov-set", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    line = [x for x in r.stdout.splitlines() if x.startswith("distill:")]
    assert len(line) == 1 and "--cov-set" in line[0], (r.stdout, r.stderr)
    assert not out.exists() and not (tmp_path / "r.jsonl").exists() and '"mode"' not in r.stdout
