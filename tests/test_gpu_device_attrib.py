"""--device-attrib at the product level: `wtfgpu` with new coverage attributed
on the device (wtfgpu_attribute_coverage) reports, testcase by testcase, what
the oracle twin reports and what `wtfgpu` reports with the host loop; a fixed
seed campaign ends with the same counts, crash names and corpus either way."""
import os
import shutil

import pytest

from tests import tlv_harness as H
from tests.tlv_inputs import write_inputs

pytestmark = pytest.mark.gpu

FIELDS = ("result", "crash", "error", "icount", "gprs", "coverage")  # test_gpu_tlv.py's
_SAME = ("execs", "retired", "coverage", "corpus", "crashes", "unique_crashes", "timeouts", "cr3", "errors")
FLAG = ("--device-attrib",)
STREAM = ("--stream-run", "--slice-steps", "64")
LOW_LIMIT = 400


@pytest.fixture(scope="module")
def target(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tlv_attrib"))
    H.build_target(d)
    write_inputs(os.path.join(d, "parity"), 1500)
    return d


def _diff(a, b):
    assert len(a) == len(b)
    bad = []
    for x, y in zip(a, b):
        assert x["input"] == y["input"]
        for k in FIELDS:
            if x[k] != y[k]:
                bad.append((x["input"], k, x[k] if k != "coverage" else len(x[k]),
                            y[k] if k != "coverage" else len(y[k])))
    return bad


@pytest.fixture(scope="module")
def runs(target, tmp_path_factory):
    """The parity inputs, lane-order coverage, 256 lanes: results by (who, mode, limit), each run once."""
    made = {}
    inp = os.path.join(target, "parity")

    def get(who, mode, limit):
        key = (who, mode if who != "twin" else "", limit)
        if key not in made:
            out = str(tmp_path_factory.mktemp("res") / "r.jsonl")
            extra = STREAM if mode == "stream" else ()
            if who == "twin":  # takes the flag and has nothing to switch
                made[key] = H.run(H.TWIN, target, inp, out, lanes=256, limit=limit, full_coverage=False, extra=FLAG)
            else:
                made[key] = H.run(H.WTFGPU, target, inp, out, lanes=256, limit=limit, full_coverage=False,
                                  extra=(*extra, *(FLAG if who == "device" else ())))
            assert len(made[key]) == len(os.listdir(inp))
        return made[key]

    return get


def _check_low_limit(twin):
    assert sum(r["result"] == "timedout" for r in twin) >= 10
    assert sum(r["result"] == "ok" for r in twin) >= 10


@pytest.mark.parametrize("limit", [100000, LOW_LIMIT])
@pytest.mark.parametrize("mode", ["batch", "stream"])
def test_tlv_equals_the_host_loop(runs, mode, limit):
    """--limit 400 exercises the revoke rule, chosen with the twin alone: of
    the 1,508 parity inputs 742 time out (they report their rips and commit
    none, so later testcases report them again), 412 end ok and 354 crash."""
    d = runs("device", mode, limit)
    bad = _diff(d, runs("host", mode, limit))
    assert not bad, bad[:10]
    assert sum(len(r["coverage"]) for r in d) > 100
    if limit == LOW_LIMIT:
        _check_low_limit(runs("twin", mode, limit))


@pytest.mark.parametrize("limit", [100000, LOW_LIMIT])
def test_tlv_equals_the_twin(runs, limit):
    d = runs("device", "batch", limit)
    bad = _diff(d, runs("twin", "batch", limit))
    assert not bad, bad[:10]
    if limit == LOW_LIMIT:
        _check_low_limit(runs("twin", "batch", limit))


@pytest.mark.parametrize("limit", [100000, LOW_LIMIT])
def test_tlv_stream_run_equals_the_twin(runs, limit):
    """`run --stream-run --slice-steps 64`: testcases finish in another order
    than they were given, so the replay takes every testcase's whole set from
    the executor (WTFGPU_ATTRIB_ALL on the device path) and walks them in
    input order itself, as the twin does."""
    d = runs("device", "stream", limit)
    bad = _diff(d, runs("twin", "stream", limit))
    assert not bad, (len(bad), bad[:10])


def test_tlv_full_coverage(target, tmp_path):
    inp = os.path.join(target, "parity")
    d = H.run(H.WTFGPU, target, inp, str(tmp_path / "d.jsonl"), lanes=512, extra=FLAG)
    t = H.run(H.TWIN, target, inp, str(tmp_path / "t.jsonl"), lanes=512)
    bad = _diff(d, t)
    assert not bad, bad[:10]


def test_hevd_io_lane_order_attribution(tmp_path):
    target = H.build_hevd_io_target(str(tmp_path / "hevd_io"))
    inp = os.path.join(target, "inputs")
    kw = dict(lanes=256, limit=10_000_000, full_coverage=False, name="hevd")
    g = H.run(H.WTFGPU, target, inp, str(tmp_path / "g.jsonl"), **kw)
    d = H.run(H.WTFGPU, target, inp, str(tmp_path / "d.jsonl"), extra=FLAG, **kw)
    assert len(d) == len(os.listdir(inp)) > 0
    bad = _diff(d, g)
    assert not bad, bad[:10]
    assert sum(len(r["coverage"]) for r in d) > 100


@pytest.mark.parametrize("edges", [False, True], ids=["rips", "edges"])
def test_tlv_fixed_seed_campaign(tmp_path, edges):
    base = H.build_target(str(tmp_path / "tlv"))
    out = []
    for k, flag in enumerate(((), FLAG)):
        t = str(tmp_path / f"tlv{k}")
        shutil.copytree(base, t)
        st = H.fuzz(H.WTFGPU, t, runs=8192, lanes=4096, seed=1337,
                    extra=(*(("--edges",) if edges else ()), *flag))
        out.append((st, sorted(os.listdir(os.path.join(t, "crashes"))), sorted(os.listdir(os.path.join(t, "outputs")))))
    (a, ca, oa), (b, cb, ob) = out
    assert a["execs"] == 8192
    assert {k: a[k] for k in _SAME} == {k: b[k] for k in _SAME}
    assert ca == cb and oa == ob
    assert oa and ca and a["coverage"] >= 150  # (test_gpu_tlv.py's smoke bound: the campaign found its coverage)
    assert a["backend"]["device_attrib"] == 0 and b["backend"]["device_attrib"] == 1
