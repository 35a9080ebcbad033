"""The extensions beyond SSE4.1 / AVX2 (convention U45; engine_ext.h,
oracle/x86_oracle_ext.inc): BMI1 / BMI2, ADX, MOVBE, CRC32, SSE4.2, AES and
PCLMULQDQ, which cpuid_leaf now enumerates.

Native-execution vectors (tests/golden/gen_ext_vectors.py, run on this host's
CPU, which executes every one of these forms) pin the oracle and the engine's
device code built for the host; the GPU runs them in tests/test_gpu_sse.py.
The string compares (which the oracle computes in C, not natively) are covered
under all 128 control bytes each. Hand-checked:
the CPUID bits, and #UD / UNIMPLEMENTED rules (tests/test_avx.py).
"""
import pytest

from tests.vector_replay import EXT, replay_oracle, replay_sim, run_family

DOC = EXT.doc


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_matches_native_ext(chunk):
    cases = DOC["cases"][chunk::2]
    fails = run_family(EXT, replay_oracle, cases)
    assert not fails, f"{len(fails)}/{len(cases)} mismatches, first: {fails[:5]}"


def test_engine_ext_code_matches_native_vectors():
    fails = run_family(EXT, replay_sim, DOC["cases"])
    assert not fails, f"{len(fails)}/{len(DOC['cases'])} mismatches, first: {fails[:5]}"


def test_ext_vector_file_is_substantial():
    names = {c["name"].split(".")[0] for c in DOC["cases"]}
    assert len(DOC["cases"]) > 4000
    for n in ("andn", "blsr", "blsmsk", "blsi", "bzhi", "bextr", "shlx", "sarx", "shrx", "pdep", "pext", "mulx",
              "rorx", "adcx", "adox", "movbe16", "movbe32", "movbe64", "crc32b", "crc32w", "crc32d", "crc32q",
              "pcmpgtq", "vpcmpgtq", "pcmpestri", "pcmpestrm", "pcmpistri", "pcmpistrm", "vpcmpestri", "vpcmpistrm",
              "aesenc", "aesenclast", "aesdec", "aesdeclast", "aesimc", "aeskeygenassist", "vaesenc",
              "pclmulqdq", "vpclmulqdq", "sha1rnds4", "sha1nexte", "sha1msg1", "sha1msg2", "sha256rnds2",
              "sha256msg1", "sha256msg2"):
        assert n in names, n
