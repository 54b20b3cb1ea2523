"""CPU: the raster's per-pixel code executed on the host (hm_selftest_window_raster) against the rule restated with the
oracle (tests/raster_cases.py), its argument errors, and the Python layers that need no GPU -- the slippy-map pixel grid
(readside.tile_grid) and the indexed PNG (readside.png_from_classes).  No tolerance: counts and classes are integers."""
import math
import zlib

import numpy as np
import pytest

import raster_cases as rc


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("res", [0, 1, 2, 7, 8, 15])
def test_edge_grid_equals_oracle(res):
    """one record per distinct cell the oracle finds on the edge grid, counts 1..k"""
    from mobheat import _lib, readside
    lat, lon, nf = rc.edge_grid()
    cells = np.unique(rc.pixel_cells(res, lat, lon))
    cells = cells[cells != 0]
    recs = rc.records(cells, np.arange(1, cells.size + 1))
    thr = readside.COUNT_THRESHOLDS
    counts, classes = _lib.window_raster_selftest(recs, res, lat, lon, thr)
    ec, ek = rc.expected(recs, res, lat, lon, thr)
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(classes, ek)
    assert counts.dtype == np.uint32 and classes.dtype == np.uint8 and counts.shape == (lat.size, lon.size)
    assert np.count_nonzero(counts) >= 20 and np.count_nonzero(np.diag(counts)[:nf]) == nf   # the face centres
    # the NaN / out-of-range rows and columns: no cell, although every cell on the grid has a record
    bad_r = np.nonzero(~(np.abs(lat) <= 90.0))[0]
    bad_c = np.nonzero(~(np.abs(lon) <= 180.0))[0]
    assert bad_r.size >= 4 and bad_c.size >= 3   # NaN, 91, +-inf and just-outside values
    assert not counts[bad_r].any() and not counts[:, bad_c].any() and not classes[bad_r].any() and not classes[:, bad_c].any()
    ok = np.ix_(np.abs(lat) <= 90.0, np.abs(lon) <= 180.0)
    assert counts[ok].all()
    # counts alone (no thresholds): the same grid
    np.testing.assert_array_equal(_lib.window_raster_selftest(recs, res, lat, lon), ec)


def test_thresholds_and_saturation(oracle_h3):
    from mobheat import _lib, readside
    rng = np.random.default_rng(4201)
    n = len(rc.EDGE_COUNTS)
    lat, lon = rng.uniform(-60, 60, n), rng.uniform(-170, 170, n)
    cells = oracle_h3.latlng_to_cell(lat, lon, 5)   # pixel (k, k) in cell k
    assert np.unique(cells).size == n
    recs = rc.records(cells, rc.EDGE_COUNTS)
    counts, classes = _lib.window_raster_selftest(recs, 5, lat, lon, readside.COUNT_THRESHOLDS)
    ec, ek = rc.expected(recs, 5, lat, lon, readside.COUNT_THRESHOLDS)
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(classes, ek)
    assert np.diag(classes).tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6]
    assert np.diag(counts).tolist() == rc.EDGE_COUNTS[:11] + [0xFFFFFFFF] * 3
    # a class comes from the 64-bit count: 2^33 separates 2^32 from 2^40 although both saturate
    counts, classes = _lib.window_raster_selftest(recs, 5, lat, lon, [2 ** 33])
    assert np.diag(classes).tolist() == [0] * 13 + [1] and np.diag(counts)[-2:].tolist() == [0xFFFFFFFF] * 2
    # records of equal cell add up
    twice = np.concatenate([recs, recs])
    counts, classes = _lib.window_raster_selftest(twice, 5, lat, lon, readside.COUNT_THRESHOLDS)
    ec, ek = rc.expected(twice, 5, lat, lon, readside.COUNT_THRESHOLDS)
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(classes, ek)
    assert int(counts[0, 0]) == 2


def test_argument_errors():
    from mobheat import _lib
    from mobheat._lib import HM_E_INVALID
    lib = _lib.load()
    recs = rc.records(np.array([0x85283473fffffff], np.uint64), [3])
    lat, lon = np.array([37.3, 37.4]), np.array([-121.9, -121.8, -121.7])
    st = lambda thr, res=5: _lib.window_raster_selftest(recs, res, lat, lon, thr)
    assert st([0, 2, 5])[0].shape == (2, 3)
    for thr in ([5, 2], [2, 2], [-1, 3], list(range(16))):
        assert _code(lambda: st(thr)) == HM_E_INVALID, thr
    assert st(list(range(15)))[1].shape == (2, 3)
    assert _code(lambda: st(None, 16)) == HM_E_INVALID
    assert _code(lambda: st(None, -1)) == HM_E_INVALID
    out = np.full(6, 7, np.uint32)
    call = lambda rows, cols: lib.hm_selftest_window_raster(recs.ctypes.data, 1, 5, lat.ctypes.data, rows, lon.ctypes.data, cols,
                                                            None, 0, out.ctypes.data, None)
    assert call(-1, 3) == HM_E_INVALID and call(2, -1) == HM_E_INVALID and call(16385, 1) == HM_E_INVALID
    assert call(16384, 8192) == HM_E_INVALID   # rows * cols = 2^27
    assert call(0, 3) == 0 and call(2, 0) == 0 and (out == 7).all()   # nothing written
    assert call(2, 3) == 0 and not (out == 7).any()


# ---- readside.tile_grid ----
def test_tile_grid_world():
    from mobheat import readside
    lat, lon = readside.tile_grid(0, 0, 0)
    assert lat.shape == lon.shape == (256,) and lat.dtype == lon.dtype == np.float64
    np.testing.assert_array_equal(lat, -lat[::-1])   # symmetric about the equator to the last bit
    assert (np.diff(lat) < 0).all() and (np.diff(lon) > 0).all()
    top = math.degrees(math.atan(math.sinh(math.pi)))   # the projection's edge, 85.0511...
    # half a pixel below the edge: d lat / d v = -360 / cosh(pi (1 - 2 v)) degrees, its magnitude least at the edge
    # (360 / cosh(pi)) and below 360 / cosh(pi (1 - 1 / 256)) over that half pixel
    dv = 0.5 / 256
    assert top - dv * 360.0 / math.cosh(math.pi * (1 - 2 * dv)) < lat[0] < top - dv * 360.0 / math.cosh(math.pi)
    assert lon[0] == -180.0 + 360.0 * 0.5 / 256 and lon[-1] == 180.0 - 360.0 * 0.5 / 256
    one_lat, one_lon = readside.tile_grid(0, 0, 0, size=1)
    assert one_lat.tolist() == [0.0] and one_lon.tolist() == [0.0]


def test_tile_grid_neighbours_and_errors():
    from mobheat import readside
    la, lo = readside.tile_grid(5, 9, 11)
    lb, lob = readside.tile_grid(5, 10, 11)
    np.testing.assert_array_equal(la, lb)   # one row of tiles, one set of latitudes
    step = 360.0 / 32 / 256
    both = np.r_[lo, lob]
    # x + 1 continues x with the same step (|lon| < 180: an ulp is 2.9e-14, the two roundings of a difference below 1e-13)
    assert (np.diff(both) > 0).all() and np.abs(np.diff(both) - step).max() < 1e-13
    assert readside.tile_grid(5, 9, 12)[0][0] < la[-1]   # the tile to the south continues southwards
    tx, ty = rc.tile_of(42.36, -71.06, 12)
    lat, lon = readside.tile_grid(12, tx, ty)
    assert lat[-1] < 42.36 < lat[0] and lon[0] < -71.06 < lon[-1]
    for bad in ((-1, 0, 0), (31, 0, 0), (3, 8, 0), (3, 0, 8), (3, -1, 0), (3, 0, -1)):
        with pytest.raises(ValueError):
            readside.tile_grid(*bad)
    for size in (0, 4097, -5):
        with pytest.raises(ValueError):
            readside.tile_grid(3, 1, 1, size=size)
    assert readside.tile_grid(30, 2 ** 30 - 1, 2 ** 30 - 1, size=4096)[0].size == 4096


# ---- readside.png_from_classes ----
@pytest.mark.parametrize("shape", [(1, 1), (1, 257), (256, 256)])
def test_png_round_trip(shape):
    from mobheat import readside
    rng = np.random.default_rng(shape[1])
    classes = rng.integers(0, len(readside.COUNT_PALETTE), shape).astype(np.uint8)
    png = readside.png_from_classes(classes, readside.COUNT_PALETTE)
    assert isinstance(png, bytes)
    back, plte, trns = rc.decode_png(png)
    np.testing.assert_array_equal(back, classes)
    assert plte == [p[:3] for p in readside.COUNT_PALETTE] and list(trns) == [p[3] for p in readside.COUNT_PALETTE]
    assert zlib.crc32(b"IEND") & 0xFFFFFFFF == int.from_bytes(png[-4:], "big")


def test_palette_is_the_reference_pages():
    from mobheat import readside
    assert readside.COUNT_THRESHOLDS == (0, 2, 5, 10, 20, 50)
    hexes = ["#%02X%02X%02X" % p[:3] for p in readside.COUNT_PALETTE]
    assert hexes[1:] == ["#FEB24C", "#FD8D3C", "#FC4E2A", "#E31A1C", "#BD0026", "#800026"]
    assert len(hexes) == len(readside.COUNT_THRESHOLDS) + 1
    assert readside.COUNT_PALETTE[0][3] == 0 and all(p[3] > 0 for p in readside.COUNT_PALETTE[1:])
    with pytest.raises(ValueError):
        readside.png_from_classes(np.full((2, 2), 7, np.uint8), readside.COUNT_PALETTE)
    with pytest.raises(ValueError):
        readside.png_from_classes(np.zeros((0, 4), np.uint8))
