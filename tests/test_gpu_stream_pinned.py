"""Pinned streaming campaigns: the GPU node's fixed-seed campaigns
(`wtfgpu fuzz --seed 1337 --runs N`) must reproduce, count for count, crash
name for crash name and corpus entry for corpus entry, what
tests/golden/stream_campaigns.json records (scripts/gen_stream_campaigns.py,
run on the MI355X from the commit before the step thread's harvest, refill and
accounting passes were fused). That fixes the three orders those passes must
keep: testcases go to the lowest free lanes in order, results are accounted in
lane order per half, and every MakeBatch sees the same corpus.

Configs (a few seconds each):
  * tlv, 256 lanes (the smallest count that pipelines: two halves of two
    waves), 256-step slices regrouped every 64: lanes live across several
    slices, so parts are partly finished at every harvest;
  * the same with WTFGPU_DEVICE_BP_ACTIONS=0: every hit goes through
    service_hits and the touched-view paths;
  * tlv, 16,384 lanes, default slice: halves of 8,192 lanes cross every
    "parallel above N lanes" threshold;
  * the bare HEVD look-alike at 256 and 16,384 lanes: host handlers,
    StopWithArgs naming, handler-fault engine errors;
  * the first and the fourth again with WTFGPU_STREAM_PARTS=1: one part, not
    pipelined, so the harvest runs in the refill's call and reads the exits,
    byte and dirty counts and StopWithArgs arguments itself.

Every recorded key must match. The recording build ran each config twice:
the tlv configs agreed with themselves on every key; the HEVD configs
differed from themselves in the kernel's group_steps alone (885592 / 885566,
619582 / 619589 and, one part, 941267 / 941266), so the fixture lists that key
as unstable for them and holds them to every other key (counts, crash names,
corpus entries). The two one-part records were added later, recorded with the
other five again (which came out unchanged) from the commit before the
streaming step was split into named phases.
"""
import importlib.util
import json
import os

import pytest

from tests import tlv_harness as H

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gen_stream_campaigns",
                                               os.path.join(H.ROOT, "scripts", "gen_stream_campaigns.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(H.ROOT, "tests", "golden", "stream_campaigns.json")) as _f:
    FIXTURE = {c["config"]["id"]: c for c in json.load(_f)["configs"]}

IDS = ("tlv_256_short_slices", "tlv_256_short_slices_host_bp", "tlv_16384", "hevd_bare_256", "hevd_bare_16384",
       "tlv_256_short_slices_one_part", "hevd_bare_256_one_part")


def test_fixture_holds_every_config():
    assert sorted(FIXTURE) == sorted(IDS)
    for cfg in G.CONFIGS:  # recorded with the generator's present settings
        assert FIXTURE[cfg["id"]]["config"] == cfg
        # a tlv campaign reproduces every key; elsewhere only the kernel's step count may be unstable
        assert set(FIXTURE[cfg["id"]]["unstable"]) <= (set() if cfg["target"] == "tlv" else {"group_steps"})


@pytest.fixture(scope="module")
def bases(tmp_path_factory):
    return G.build_bases(str(tmp_path_factory.mktemp("bases")), [c["target"] for c in G.CONFIGS])


@pytest.mark.parametrize("cid", IDS)
def test_campaign_reproduces_recorded(cid, bases, tmp_path):
    cfg, want = FIXTURE[cid]["config"], FIXTURE[cid]["expect"]
    got = G.run_config(cfg, bases[cfg["target"]], str(tmp_path / "t"))
    assert got["execs"] == cfg["runs"]
    # every recorded key; the fixture leaves out only the keys on which the
    # recording build disagreed with itself (FIXTURE[cid]["unstable"])
    assert set(got) == set(want) | set(FIXTURE[cid]["unstable"])
    for k in want:  # named, so a failure says which count moved
        assert got[k] == want[k], k
