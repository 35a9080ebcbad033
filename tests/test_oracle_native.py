"""Pin the CPU oracle against native-execution golden vectors (tests/golden).

Each vector executed one instruction natively on an x86-64 host
(tests/golden/gen_native_vectors.py). The oracle executes the same bytes from a
synthetic ring-3 address space whose data window sits at the same virtual
address, and must reproduce every GPR, the defined RFLAGS bits (fmask) and
every byte of the 256-byte memory window.
"""
import pytest

from tests.vector_replay import NATIVE, replay_oracle, run_family

DOC = NATIVE.doc


@pytest.mark.parametrize("chunk", range(8))
def test_oracle_matches_native_execution(chunk):
    cases = DOC["cases"][chunk::8]
    failures = run_family(NATIVE, replay_oracle, cases)
    assert not failures, f"{len(failures)}/{len(cases)} mismatches, first: {failures[:8]}"


def test_vector_file_is_substantial():
    assert len(DOC["cases"]) > 5000
    assert len({c["code"] for c in DOC["cases"]}) > 900
