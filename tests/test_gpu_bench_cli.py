"""The benchmark's command line on the GPU: a plain run is the headline alone
(no legs, no CPU baselines), --steps sets the number of timed steps, the
result line carries ms_per_step, and --dump-outputs writes the node's outputs
after the last timed step as float64 .npy files. One short run at 4,096 lanes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bench_cli") / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--lanes", "4096", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), d


def test_plain_run_is_the_headline_alone(plain_run):
    out, _ = plain_run
    assert out["metric"] == bench.METRIC and out["unit"] == "execs/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u64" and out["n_gpus"] == 1 and (out["steps"], out["warmup"]) == (STEPS, WARMUP)
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value is the timed steps' testcases over their wall time, ms_per_step that time per step
    assert out["value"] * STEPS * out["ms_per_step"] / 1e3 == pytest.approx(out["node_timed"]["execs"], rel=1e-6)
    assert out["node_timed"]["batches"] == STEPS and out["node_summary"]["batches"] == STEPS + WARMUP
    for moved in ("hevd", "hevd_bare", "syn", "vs_cpu", "cpu_node"):
        assert moved not in out
    assert out["cpu_baseline"] is None


def test_dump_outputs_hold_the_last_step(plain_run):
    out, d = plain_run
    assert sorted(os.listdir(d)) == ["corpus.npy", "crashes.npy", "last_step.npy", "stats.npy"]
    arrs = {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_MAX_BYTES
    stats = dict(zip(bench.DUMP_COUNTERS, arrs["stats"].tolist()))
    last = dict(zip(bench.DUMP_COUNTERS, arrs["last_step"].tolist()))
    summ = out["node_summary"]
    assert stats["batches"] == STEPS + WARMUP and last["batches"] == 1
    assert stats["execs"] == summ["execs"] and stats["retired"] == summ["retired"]
    assert stats["coverage"] == summ["coverage"] and stats["crashes"] == summ["crashes"] and stats["errors"] == 0
    assert 0 <= last["execs"] <= stats["execs"] and 0 <= last["retired"] <= stats["retired"]
    assert arrs["corpus"].ndim == 2 and arrs["corpus"].shape[1] == 2
    assert arrs["crashes"].shape == (summ["unique_crashes"], 2)
