"""GPU engine vs native x86-64 execution: every golden vector is one lane.

All 1007 encodings of tests/golden/native_vectors.json.gz live in one code
region (one 32-byte slot each, followed by int3); each lane gets its vector's
registers and its own copy of the 256-byte data window (copy-on-write through
wtfgpu_apply_writes), runs one instruction, and stops at the int3.
"""
import pytest

from tests.vector_replay import NATIVE, replay_gpu, run_family

pytestmark = pytest.mark.gpu


def test_gpu_matches_native_vectors():
    cases = NATIVE.doc["cases"]
    fails = run_family(NATIVE, replay_gpu, cases)
    total = len(cases)
    assert total == len(NATIVE.doc["cases"])
    if fails:
        import collections
        print("failing classes:", collections.Counter(f[0] for f in fails).most_common())
    assert not fails, f"{len(fails)}/{total} mismatches, first: {fails[:6]}"
