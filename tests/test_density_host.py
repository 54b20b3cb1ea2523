"""CPU: the density's per-key code executed on the host (hm_selftest_positions_density) against the contract restated with
the oracle and numpy (tests/density_cases.py), its argument errors, and readside's collection / PNG plumbing on a stub
engine.  The cases also prove here that their inputs reach the regime they claim -- how many keys take the exact path, how
many groups, how many unsnapped -- so that tests/test_gpu_density.py's device runs mean what they say."""
import json

import numpy as np
import pytest

import density_cases as dc
import raster_cases as rc


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _host(recs, res, since=None):
    from mobheat import _lib
    return _lib.positions_density_selftest(recs, res, since)


def _fast_misses(recs, res, since=None):
    """kept keys the fast latLngToCell hands to the exact path (host execution of the same code)"""
    from mobheat import _lib
    kept = recs[recs["ts_us"] >= (dc.INT64_MIN if since is None else since)]
    _, fb = _lib.latlng_to_cell_fast_host_selftest(kept["lat"], kept["lon"], res)
    return int(fb.sum())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_sizes(n):
    recs = dc.sized(n)
    for res in (8, 0):
        want, bad = dc.expected(recs, res)
        got, unsnapped = _host(recs, res)
        dc.check(got, want, what=f"n {n} res {res}")
        assert unsnapped == bad == 0
        assert int(got["count"].sum()) == n
    if n >= 63:
        assert dc.expected(recs, 8)[0]["count"].max() > 1   # several keys in one cell


def test_hot_cell_regimes():
    from mobheat import _lib
    recs = dc.hot_cell()
    assert np.unique(np.stack([recs["lat"], recs["lon"]]), axis=1).shape[1] == recs.size == 50_000
    want0, _ = dc.expected(recs, 0)
    assert want0.size == 1 and int(want0["count"][0]) == 50_000   # one res-0 cell holds the whole fleet
    got0, _ = _host(recs, 0)
    dc.check(got0, want0, dyadic=True, what="hot cell res 0")
    want15, _ = dc.expected(recs, 15)
    assert want15.size > 40_000   # far beyond the 1024 keys an LDS front table takes: the spill regime
    got15, _ = _host(recs, 15)
    dc.check(got15, want15, dyadic=True, what="hot cell res 15")
    assert _lib.positions_density_selftest(recs, 15)[0].size == want15.size


@pytest.mark.parametrize("res", [9, 5, 0])
def test_exact_path_and_cell_zero(res):
    recs = dc.edges()
    want, bad = dc.expected(recs, res)
    got, unsnapped = _host(recs, res)
    dc.check(got, want, what=f"edges res {res}")
    assert unsnapped == bad == 7   # edge_points(): two just-outside latitudes, NaN, +-inf, one just-outside and one NaN longitude
    assert _fast_misses(recs, res) >= 20   # at least the face centres


def test_unsnappable_records():
    recs, at = dc.with_bad()
    clean = np.delete(recs, at)
    for res in (8, 3):
        want, bad = dc.expected(recs, res)
        got, unsnapped = _host(recs, res)
        assert bad == unsnapped == 4
        dc.check(got, want, what="with bad")
        dc.check(got, dc.expected(clean, res)[0], what="the rest unchanged")


def test_since_edges():
    recs, since = dc.since_edges()
    for res in (8, 15, 0):
        for s in (since - 1, since, since + 1, since + 2, None):
            want, _ = dc.expected(recs, res, s)
            got, _ = _host(recs, res, s)
            dc.check(got, want, what=f"res {res} since {s}")
    want, _ = dc.expected(recs, 8, since)
    assert want.size == 3 and sorted(want["count"].tolist()) == [1, 1, 2]   # pb's cell vanished, pa lost one of three
    assert sorted(want["window_start_us"].tolist()) == [since, since + 1, since + 1]
    assert dc.expected(recs, 8, since + 2)[0].size == 0 and _host(recs, 8, since + 2)[0].size == 0


def test_ts_extremes_ties_and_negatives():
    recs = dc.ts_extremes()
    want, _ = dc.expected(recs, 8)
    got, _ = _host(recs, 8)
    dc.check(got, want, what="INT64_MIN keeps every key")
    assert sorted(want["window_start_us"].tolist()) == [dc.INT64_MIN, -3, dc.INT64_MAX]
    assert sorted(want["count"].tolist()) == [1, 5, 6]
    got, _ = _host(recs, 8, dc.INT64_MAX)
    want, _ = dc.expected(recs, 8, dc.INT64_MAX)
    dc.check(got, want, what="INT64_MAX keeps only that ts")
    assert want.size == 1 and int(want["count"][0]) == 2 and int(want["window_start_us"][0]) == dc.INT64_MAX
    got, _ = _host(recs, 8, -3)
    dc.check(got, dc.expected(recs, 8, -3)[0], what="since -3")


def test_contract_errors():
    from mobheat import _lib
    from mobheat._lib import HM_E_INVALID
    recs = dc.boston(50)
    assert _code(lambda: _host(recs, -1)) == HM_E_INVALID
    assert _code(lambda: _host(recs, 16)) == HM_E_INVALID
    groups = dc.expected(recs, 8)[0].size
    assert groups > 1
    assert _lib.positions_density_selftest(recs, 8, cap=groups)[0].size == groups
    assert _code(lambda: _lib.positions_density_selftest(recs, 8, cap=groups - 1)) == HM_E_INVALID
    none, bad = _host(recs[:0], 8)
    assert none.size == 0 and bad == 0


# ---- readside on a stub engine: the collection is the specification of the body ----
class _StubEngine:
    """positions_density* from the host execution; the rings from the host execution of cellToBoundary"""
    device = 0
    h3_res = 8

    def __init__(self, recs):
        self.recs = recs

    def positions_density(self, res=None, since_us=None, view=None, copy=True):
        from mobheat import _lib
        return _lib.positions_density_selftest(self.recs, self.h3_res if res is None else res, since_us)[0]

    def positions_density_raster(self, lat, lon, res=None, since_us=None, thresholds=None, copy=True):
        from mobheat import _lib
        res = self.h3_res if res is None else res
        return _lib.window_raster_selftest(self.positions_density(res, since_us), res, lat, lon, thresholds)


def test_readside_collection_and_png(monkeypatch):
    import datetime as dt

    from mobheat import _lib, readside

    def host_rings(cells, device=0):
        la, lo, nv = _lib.cells_to_boundary_host_selftest(np.array([int(c) for c in cells], np.uint64))
        out = []
        for k in range(len(nv)):
            ring = [[float(lo[k, v]), float(la[k, v])] for v in range(nv[k])]
            if ring and ring[0] != ring[-1]:
                ring.append(ring[0])
            out.append(ring)
        return out
    monkeypatch.setattr(readside, "rings", host_rings)
    recs = dc.boston(2000)
    eng = _StubEngine(recs)
    tz = dt.timezone(dt.timedelta(hours=-4))
    since = dc.T0 + 100 * dc.SEC
    fc = readside.positions_density_from_engine(eng, 8, since, tz, dc.T0 + 200 * dc.SEC)
    want, _ = dc.expected(recs, 8, since)
    assert len(fc["features"]) == want.size > 100
    by = {int(f["properties"]["cellId"], 16): f for f in fc["features"]}
    assert sorted(by) == want["cell"].tolist()
    for c, k in zip(want["cell"].tolist(), want["count"].tolist()):
        p = by[c]["properties"]
        assert p["count"] == k and p["avgSpeedKmh"] == 0.0 and list(p) == ["cellId", "count", "avgSpeedKmh", "windowStart", "windowEnd"]
        assert p["windowStart"] == "2025-10-04T06:01:40" and p["windowEnd"] == "2025-10-04T06:03:20"
        assert by[c]["geometry"]["type"] == "Polygon" and len(by[c]["geometry"]["coordinates"][0]) == 7
    # the body is the tile encoder's: its host execution on the same records gives json.dumps of the collection
    ordered = eng.positions_density(8, since)
    body, offs = _lib.tile_features_selftest(ordered, "2025-10-04T06:01:40", "2025-10-04T06:03:20")
    assert bytes(body) == json.dumps(fc, separators=(",", ":")).encode()
    # None texts are empty strings, and a view filters by the cell's ring
    fc0 = readside.positions_density_from_engine(eng, 8)
    assert {f["properties"]["windowStart"] for f in fc0["features"]} == {""} == {f["properties"]["windowEnd"] for f in fc0["features"]}
    body0, _ = _lib.tile_features_selftest(eng.positions_density(8), "", "")
    assert bytes(body0) == json.dumps(fc0, separators=(",", ":")).encode()
    view = (-71.10, 42.30, -71.00, 42.40)
    fcv = readside.positions_density_from_engine(eng, 8, view=view)
    wantv = dc.in_view(dc.expected(recs, 8)[0], 8, view)
    assert sorted(int(f["properties"]["cellId"], 16) for f in fcv["features"]) == wantv["cell"].tolist()
    assert 0 < wantv.size < dc.expected(recs, 8)[0].size
    # the PNG: tile_grid + density raster + png_from_classes
    tx, ty = rc.tile_of(42.33, -71.07, 12)
    png = readside.positions_density_png(eng, 12, tx, ty, res=8)
    lat, lon = readside.tile_grid(12, tx, ty)
    ec, ek = rc.expected(dc.expected(recs, 8)[0], 8, lat, lon, readside.COUNT_THRESHOLDS)
    classes, plte, _ = rc.decode_png(png)
    np.testing.assert_array_equal(classes, ek)
    assert ek.any() and png == readside.png_from_classes(ek)
