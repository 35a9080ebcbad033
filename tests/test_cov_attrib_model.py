"""The attribution model (tests/cov_attrib_model.py) pinned to hand-written
cases, and the declarations of wtfgpu_attribute_coverage (no GPU calls)."""
import os
import re

from tests.cov_attrib_model import attribute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_owner_revoked():
    # 7 is owned by three lanes; the first owner timed out: it reports 7, the
    # second owner reports and commits it, the third finds it committed
    sets = [{7, 1}, {7}, {7, 9}]
    assert attribute(sets, [True, False, False]) == [(0, 1), (0, 7), (1, 7), (2, 9)]


def test_all_owners_revoked():
    sets = [{7}, {7}, {7}]
    assert attribute(sets, [True, True, True]) == [(0, 7), (1, 7), (2, 7)]
    assert attribute(sets) == [(0, 7)]


def test_value_in_aggregate_is_never_emitted():
    sets = [{5, 7}, {7}, {5}]
    assert attribute(sets, None, aggregate={7}) == [(0, 5)]
    assert attribute(sets, [True, True, True], aggregate={5, 7}) == []


def test_empty_lane():
    assert attribute([set(), {3}, set()]) == [(1, 3)]
    assert attribute([]) == []


def test_order_is_the_list_order():
    # the same three lanes listed as 2, 0, 1: positions, not lane ids, decide
    lanes = {0: {1, 2}, 1: {2, 3}, 2: {3, 1}}
    assert attribute([lanes[l] for l in (2, 0, 1)]) == [(0, 1), (0, 3), (1, 2)]
    assert attribute([lanes[l] for l in (0, 1, 2)]) == [(0, 1), (0, 2), (1, 3)]


def test_values_sorted_inside_a_position():
    assert attribute([{9, 2, 5}]) == [(0, 2), (0, 5), (0, 9)]


def test_full_mode_is_each_sorted_set():
    sets = [{7, 1}, set(), {7}]
    assert attribute(sets, [True, False, False], aggregate={7}, full=True) == [(0, 1), (0, 7), (2, 7)]


def test_abi_declares_the_prototype():
    import ctypes as C

    from wtf_amd import abi

    lib = abi.load_hip_library()
    fn = lib.wtfgpu_attribute_coverage
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[2] == C.POINTER(C.c_uint8) and fn.argtypes[7] is C.c_uint64
    assert abi.ATTRIB_ALL == 1


def test_header_declares_it():
    text = open(os.path.join(ROOT, "include", "wtfgpu.h")).read()
    assert re.search(r"\bint\s+wtfgpu_attribute_coverage\s*\(\s*wtfgpu_ctx\s*\*", text)
    assert re.search(r"#define\s+WTFGPU_ATTRIB_ALL\s+1u", text)
    assert re.search(r"#define\s+WTFGPU_ABI_VERSION\s+4\b", text)
    assert "wtfgpu_attribute_coverage" in abi_symbols()


def abi_symbols():
    from wtf_amd.abi import exported_symbols_from_header

    return exported_symbols_from_header(os.path.join(ROOT, "include", "wtfgpu.h"))
