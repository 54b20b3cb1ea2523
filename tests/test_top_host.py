"""CPU: the top-k order (hm_top_*, csrc/k_top.h) without a GPU -- the host execution of the kernels' key, digit and
comparator code (hm_selftest_top_records) and the numpy form (readside.top_of) against Python's sorted on every case of
tests/top_cases.py, whole records bit for bit; the error codes; the ABI."""
import ctypes

import numpy as np
import pytest

import top_cases as tc

CASES = tc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_execution_equals_numpy_equals_sorted(mobheat_lib, case):
    from mobheat import _lib, readside
    recs = case["recs"]
    for k in case["ks"]:
        want = tc.ref_top(recs, k)
        assert want.size == min(k, recs.size)
        tc.same(readside.top_of(recs, k), want, f"{case['name']} k {k}: readside.top_of against sorted")
        tc.same(_lib.top_records_selftest(recs, k), want, f"{case['name']} k {k}: host execution against sorted")


def test_top_of_against_sorted_by_hand():
    from mobheat import readside
    recs = tc.records([3, 9, 3, -1, 9, 0, tc.INT64_MIN, tc.INT64_MAX], [50, 40, 30, 20, 40, 10, 5, 60], tag=True)
    #                  2  1a  2   4  1b  3   5             0        <- rank groups; 1a before 1b by index, cell 30 before 50
    order = [7, 1, 4, 2, 0, 5, 3, 6]
    for k in range(10):
        tc.same(readside.top_of(recs, k), recs[order[:k]], f"k {k}")
        tc.same(tc.ref_top(recs, k), recs[order[:k]], f"the reference itself, k {k}")
    # cells compare as uint64: a cell with bit 63 set ranks after every other
    recs = tc.records([1, 1, 1], np.array([1 << 63, 5, (1 << 63) + 1], np.uint64))
    assert readside.top_of(recs, 3)["cell"].tolist() == [5, 1 << 63, (1 << 63) + 1]
    with pytest.raises(ValueError):
        readside.top_of(recs, tc.TOP_MAX + 1)
    with pytest.raises(ValueError):
        readside.top_of(recs, -1)


def test_the_cases_are_what_they_claim():
    by = {c["name"]: c for c in CASES}
    assert {c["recs"].size for c in CASES} >= set(tc.SIZES) | {tc.SECOND_ITERATION, tc.TOP_MAX + 1, 70000}
    assert max(c["recs"].size for c in CASES) == 70000
    vary = lambda a: int(np.bitwise_or.reduce(a.view(np.uint64)) ^ np.bitwise_and.reduce(a.view(np.uint64)))
    byte_set = lambda v: {b for b in range(8) if (v >> (8 * b)) & 0xff}
    assert byte_set(vary(by["counts differ in byte 4"]["recs"]["count"])) == {4}
    assert byte_set(vary(by["counts differ in byte 7"]["recs"]["count"])) == {7}
    assert byte_set(vary(by["a constant byte between two varying"]["recs"]["count"])) == {0, 2}
    assert vary(by["counts all equal"]["recs"]["count"]) == 0
    assert vary(by["cells differ in the last digit"]["recs"]["cell"]) == 7 << 21
    assert {int(c) >> 52 & 0xf for c in by["mixed resolutions"]["recs"]["cell"]} == {6, 8, 9}
    dup = by["repeated (count, cell) straddles k"]["recs"]
    pairs = list(zip(dup["count"].tolist(), dup["cell"].tolist()))
    assert max(pairs.count(p) for p in set(pairs)) == 50
    for k in by["repeated (count, cell) straddles k"]["ks"]:   # the lower indices of the repeated pair win
        got = tc.ref_top(dup, k)
        rep = got[got["count"] == 4]
        assert 0 < rep.size < 50 and rep["reserved"].tolist() == dup[dup["count"] == 4]["reserved"][:rep.size].tolist()
    ext = by["count extremes"]["recs"]["count"]
    assert {0, -1, tc.INT64_MIN, tc.INT64_MAX} <= set(ext.tolist())


def test_error_codes(mobheat_lib):
    from mobheat import _lib
    recs = tc.records([1, 2, 3], tc.cells_of(3))
    out = np.zeros(4, _lib.STATE_REC_DTYPE)
    n = ctypes.c_int64(-7)
    call = lambda r, cnt, k, o, pn: mobheat_lib.hm_selftest_top_records(r, cnt, k, o, pn)
    assert call(recs.ctypes.data, 3, tc.TOP_MAX + 1, out.ctypes.data, ctypes.byref(n)) == _lib.HM_E_INVALID
    assert call(recs.ctypes.data, 3, -1, out.ctypes.data, ctypes.byref(n)) == _lib.HM_E_INVALID
    assert call(recs.ctypes.data, -1, 1, out.ctypes.data, ctypes.byref(n)) == _lib.HM_E_INVALID
    assert call(None, 3, 1, out.ctypes.data, ctypes.byref(n)) == _lib.HM_E_INVALID
    assert call(recs.ctypes.data, 3, 1, None, ctypes.byref(n)) == _lib.HM_E_INVALID
    assert call(recs.ctypes.data, 3, 1, out.ctypes.data, None) == _lib.HM_E_INVALID
    assert n.value == -7   # nothing touched
    assert call(recs.ctypes.data, 3, 0, None, ctypes.byref(n)) == 0 and n.value == 0
    assert call(None, 0, 5, None, ctypes.byref(n)) == 0 and n.value == 0
    assert call(recs.ctypes.data, 3, tc.TOP_MAX, out.ctypes.data, ctypes.byref(n)) == 0 and n.value == 3
    assert out["count"][:3].tolist() == [3, 2, 1]
    # without a context the info and the state calls refuse
    v = (ctypes.c_int64 * 7)()
    assert mobheat_lib.hm_top_info(None, v, 7) == _lib.HM_E_INVALID
    p = ctypes.c_void_p()
    assert mobheat_lib.hm_top_records(None, recs.ctypes.data, 3, 0, 1, 0, ctypes.byref(p), ctypes.byref(n)) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_window_top(None, 0, 8, None, 1, 0, ctypes.byref(p), ctypes.byref(n)) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_positions_density_top(None, 8, 0, None, 1, 0, ctypes.byref(p), ctypes.byref(n)) == _lib.HM_E_INVALID


def test_abi_is_still_13(mobheat_lib):
    from mobheat import _lib, readside
    assert mobheat_lib.hm_abi_version() == _lib.HM_ABI_VERSION == 13
    assert _lib.HM_TOP_MAX == readside.TOP_MAX == tc.TOP_MAX == 65536
    for name in ("hm_top_records", "hm_window_top", "hm_window_geojson_top", "hm_positions_density_top", "hm_selftest_top_records",
                 "hm_top_info"):
        assert name in _lib.SIGNATURES and hasattr(mobheat_lib, name)
