"""test_stream_twin.py's comparison on tlv at a width that reaches the
parallel paths of the fuzz loop's streaming bookkeeping: at --lanes 8192 every
"parallel above N lanes" threshold of runner.cc (4096, 8192) is crossed, so
the ready queue's ranges, the chunked fill of the step's testcases and the
chunked accounting pass all run on the host threads (the existing test's 512
lanes keep every one of them serial). The batch campaign, the streaming
campaign and the streaming campaign with --sample (every result through the
one-by-one path) must agree count for count, crash name for crash name and
corpus entry for corpus entry."""
import os

import pytest

from tests import tlv_harness as H

pytestmark = pytest.mark.skipif(not os.path.exists(H.TWIN), reason="oracle/wtf_twin not built")

LANES, RUNS = 8192, 24576


def test_wide_streaming_campaign_equals_batch(tmp_path):
    base = H.build_target(str(tmp_path / "base"))
    args = ("tlv_server", RUNS, LANES)
    a = H.stream_campaign(base, str(tmp_path / "batch"), *args, stream=False)
    b = H.stream_campaign(base, str(tmp_path / "stream"), *args, stream=True)
    c = H.stream_campaign(base, str(tmp_path / "serial"), *args, stream=True,
                  extra=("--sample", str(tmp_path / "s.jsonl"), "--sample-every", "997"))
    assert a[0]["execs"] == RUNS
    assert a == b
    assert a == c
    assert a[0]["crashes"] > 0
