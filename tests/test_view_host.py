"""CPU: the viewport rule of csrc/k_view.h executed on the host (hm_selftest_cells_in_view) and its pure-Python
comparison forms in mobheat/readside.py, against the tests' own statement of the rule (tests/view_cases.py).  Verdicts
equal; no tolerance anywhere."""
import ctypes
import math

import numpy as np
import pytest

import view_cases as vc


@pytest.fixture(scope="module")
def cs(mobheat_lib):
    return vc.case_set()


def test_cells_in_view_selftest_equals_reference(cs):
    from mobheat import _lib
    for i, v in enumerate(cs.views):
        got = _lib.cells_in_view_selftest(cs.cells, v)
        bad = np.nonzero(got != cs.expect[i])[0]
        assert bad.size == 0, f"view {v}: cells {[hex(int(cs.cells[k])) for k in bad[:5]]} ({[cs.cls[k] for k in bad[:5]]})"
    assert _lib.cells_in_view_selftest(np.zeros(0, np.uint64), vc.WORLD).size == 0


def test_pole_cells_are_the_librarys(cs):
    """the cells the case set marks as polar are the ones the library's host latLngToCell gives"""
    from mobheat import readside
    for r in (0, 1, 8, 15):
        north, south = readside.pole_cells(r)
        k, m = cs.cells.tolist().index(north), cs.cells.tolist().index(south)
        assert cs.pole[k] == 1 and cs.pole[m] == -1 and north != south


def test_ring_in_view_equals_reference(cs):
    from mobheat import readside
    name = {1: "north", -1: "south", 0: None}
    for i, v in enumerate(cs.views):
        for k in range(cs.cells.size):
            ring = [[lo, la] for la, lo in zip(cs.lats[k], cs.lngs[k])]
            if ring:
                ring.append(ring[0])   # closed, as readside.rings builds it
            assert readside.ring_in_view(ring, v, name[cs.pole[k]]) == bool(cs.expect[i, k]), (v, hex(int(cs.cells[k])))


def test_point_in_view_equals_reference():
    from mobheat import readside
    rng = np.random.default_rng(5)
    views = vc.FIXED_VIEWS + [(170.0, -10.0, -170.0, 10.0), (-10.0, -5.0, 10.0, 5.0)]
    for v in views:
        w, s, e, n = v
        pts = [(la, lo) for la in (s, n, math.nextafter(s, -math.inf), math.nextafter(n, math.inf), math.nextafter(s, math.inf), 0.5 * (s + n))
               for lo in (w, e, math.nextafter(w, -math.inf), math.nextafter(e, math.inf), math.nextafter(w, math.inf),
                          math.nextafter(e, -math.inf), 180.0, -180.0, 0.0)]
        pts += [(float("nan"), 0.0), (0.0, float("nan")), (90.0, 0.0), (-90.0, 0.0)]
        pts += list(zip(rng.uniform(-90, 90, 200).tolist(), rng.uniform(-180, 180, 200).tolist()))
        got = [readside.point_in_view(la, lo, v) for la, lo in pts]
        want = [vc.ref_point(la, lo, v) for la, lo in pts]
        assert got == want, v
        if v not in (vc.WORLD,):
            assert any(want) and not all(want), v


def test_view_from_bbox():
    from mobheat import readside
    for v in vc.FIXED_VIEWS + [(-71.1, 42.3, -71.0, 42.4), (1e-7, -0.0, 5e-324, 0.1)]:
        text = ",".join(repr(x) for x in v)
        assert readside.view_from_bbox(text) == v
        assert ",".join(repr(x) for x in readside.view_from_bbox(text)) == text
    assert readside.view_from_bbox(" -71.1, 42.3 ,-71 ,42.4") == (-71.1, 42.3, -71.0, 42.4)
    for text in ("", "1,2,3", "1,2,3,4,5", "a,b,c,d", "1,2,,4", "1;2;3;4", "0,0,1", "nan,0,1,1", "0,0,inf,1", "0,2,1,1",
                 "0,-91,1,1", "0,0,1,90.5", "-181,0,1,1", "0,0,180.5,1", "0x10,0,1,1"):
        with pytest.raises(ValueError):
            readside.view_from_bbox(text)
    for v in vc.INVALID_VIEWS:
        assert not readside.view_valid(v) and not vc.ref_valid(v)
        with pytest.raises(ValueError):
            readside.view_from_bbox(",".join(repr(x) for x in v))


def test_invalid_views_are_refused(cs, mobheat_lib):
    from mobheat import _lib
    keep = np.full(cs.cells.size, 9, np.uint8)
    for v in vc.INVALID_VIEWS:
        hv = _lib.view_struct(v)
        rc = mobheat_lib.hm_selftest_cells_in_view(_lib.ptr(cs.cells), cs.cells.size, ctypes.byref(hv), _lib.ptr(keep))
        assert rc == _lib.HM_E_INVALID, v
        # (refused before any device is looked at: the same answer with or without a GPU)
        assert mobheat_lib.hm_cells_in_view(_lib.ptr(cs.cells), cs.cells.size, _lib.HM_MEM_HOST, 0, ctypes.byref(hv),
                                            _lib.ptr(keep)) == _lib.HM_E_INVALID, v
    assert (keep == 9).all(), "an invalid view wrote verdicts"
    assert mobheat_lib.hm_selftest_cells_in_view(_lib.ptr(cs.cells), cs.cells.size, None, _lib.ptr(keep)) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_window_geojson_view(None, 0, 0, None, 0, None, None, None, None, None) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_positions_geojson_view(None, None, 0, None, None, None, None, None) == _lib.HM_E_INVALID
    for v in vc.FIXED_VIEWS:
        assert vc.ref_valid(v)
