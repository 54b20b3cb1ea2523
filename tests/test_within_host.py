"""CPU: the geofences' host execution (the kernels' HM_HD predicate: hm_selftest_points_in_zones,
hm_selftest_positions_within, hm_selftest_tiles_within) against the comparison form in mobheat/readside.py
(points_in_zones in numpy) and against the rule in exact rational arithmetic (within_cases.exact).  There is no
tolerance: labels and hit counts are equal on every point, on-edge points and vertices included."""
import json

import numpy as np
import pytest

import density_cases as dc
import within_cases as wc


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value


@pytest.mark.parametrize("name", wc.ALL)
def test_host_execution_equals_numpy(name):
    from mobheat import _lib, readside
    zones = wc.zone_set(name)
    for what, lat, lon in wc.point_sets(name, 3000 if name in wc.SMALL else 600):
        first, hits = _lib.points_in_zones_selftest(zones, lat, lon)
        nfirst, nhits = readside.points_in_zones(zones, lat, lon)
        assert np.array_equal(first, nfirst) and np.array_equal(hits, nhits), f"{name} {what}: {int((hits != nhits).sum())} differ"
        assert np.all((first >= 0) == (hits > 0)) and np.all(first < zones.n_zones)
        if what == "special":
            assert not hits[:7].any(), "a NaN or infinite coordinate is in no zone"
    if name in wc.SMALL:
        assert hits.size and _lib.points_in_zones_selftest(zones, *wc.random_points(3000, 1))[1].any()


def test_limits_of_the_large_sets():
    from mobheat import _lib
    assert wc.circles().lat.size == _lib.HM_ZONE_VERTS_MAX and wc.circles().lat.size // wc.circles().n_zones > wc.STAGE
    assert wc.triangles4096().n_zones == _lib.HM_ZONES_MAX > wc.ZLDS


@pytest.mark.parametrize("name", wc.SMALL)
def test_both_agree_with_the_exact_rule(name):
    """random points off the edges: the exact margin decides, and binary64 agrees with it"""
    from mobheat import _lib, readside
    zones = wc.zone_set(name)
    lat, lon = wc.random_points(400, seed=7)
    efirst, ehits, decided = wc.exact(zones, lat, lon)
    assert decided.mean() > 0.99, "random points are off the edges"
    first, hits = _lib.points_in_zones_selftest(zones, lat, lon)
    nfirst, nhits = readside.points_in_zones(zones, lat, lon)
    for got in ((first, hits), (nfirst, nhits)):
        assert np.array_equal(got[0][decided], efirst[decided]) and np.array_equal(got[1][decided], ehits[decided])
    assert ehits.any() and not ehits.all() or name == "degenerate"


def test_known_memberships():
    from mobheat import _lib
    hole = wc.square_with_hole()
    first, hits = _lib.points_in_zones_selftest(hole, [42.27, 42.32, 42.45], [-71.12, -71.07, -71.07])
    assert hits.tolist() == [1, 0, 0]   # the ring, the hole, outside
    two = wc.overlapping_squares()
    first, hits = _lib.points_in_zones_selftest(two, [42.27, 42.32, 42.38, 42.20], [-71.12, -71.07, -71.02, -71.02])
    assert first.tolist() == [0, 0, 1, -1] and hits.tolist() == [1, 2, 1, 0]   # the label is the lowest containing zone
    c = wc.concave_c()
    assert _lib.points_in_zones_selftest(c, [42.24, 42.32, 42.32], [-71.05, -71.05, -71.16])[1].tolist() == [1, 0, 1]
    d = wc.degenerate()
    first, hits = _lib.points_in_zones_selftest(d, *wc.random_points(2000, 3))
    assert set(first.tolist()) <= {-1, 2} and hits.max() == 1   # the zero-area rings hold nothing
    h = wc.horizontal_edge()
    la, lo = wc.horizontal_points()
    first, hits = _lib.points_in_zones_selftest(h, la, lo)
    # the bottom edges' latitude belongs to its zone (half-open from below: the square from its west side up to, not
    # including, its east side; the triangle likewise), the square's top edge's latitude does not (the triangle's
    # inside is all that holds a point there)
    assert first.tolist() == [-1, 0, 0, 1, 1, -1, -1] + [-1, -1, -1, -1, 1, -1, -1]


def test_mesh_partitions_its_box():
    """zones that tile a region: every interior point is in exactly one triangle -- vertices and on-edge points too"""
    from mobheat import _lib
    zones = wc.mesh()
    la, lo = wc.mesh_vertices()
    sets = [("random", *wc.random_points(200_000, 5, margin=0.0)), ("vertices", la[1:-1, 1:-1].ravel(), lo[1:-1, 1:-1].ravel())]
    ela, elo = wc.edge_points(zones)
    inner = (ela > wc.BOX[0]) & (ela < wc.BOX[1]) & (elo > wc.BOX[2]) & (elo < wc.BOX[3])
    sets.append(("on edges", ela[inner], elo[inner]))
    for what, lat, lon in sets:
        ok = (lat >= wc.BOX[0]) & (lat < wc.BOX[1]) & (lon > wc.BOX[2]) & (lon < wc.BOX[3])
        first, hits = _lib.points_in_zones_selftest(zones, lat[ok], lon[ok])
        assert ok.sum() > 40 and np.all(hits == 1), f"{what}: {np.bincount(hits).tolist()} points by number of zones"
    first, hits = _lib.points_in_zones_selftest(zones, *wc.random_points(5000, 6))
    assert np.all(hits <= 1) and (hits == 0).any()   # outside the box: none


def test_validation_errors():
    from mobheat import _lib
    Z = _lib.Zones
    tri = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.5)]
    pts = ([0.1], [0.5])
    call = lambda z: _lib.points_in_zones_selftest(z, *pts)
    assert call(Z.from_rings([[tri]]))[1].tolist() == [1]
    assert call(Z.from_rings([]))[1].tolist() == [0]   # no zone: in none
    assert call(Z.from_rings([[tri]] * _lib.HM_ZONES_MAX))[1].tolist() == [_lib.HM_ZONES_MAX]
    cases = {
        "too many zones": Z.from_rings([[tri]] * (_lib.HM_ZONES_MAX + 1)),
        "too many vertices": Z.from_rings([[[(0.0, 0.0), (0.0, 1.0)] + [(1.0, 1.0 - k / 70000) for k in range(_lib.HM_ZONE_VERTS_MAX - 1)]]]),
        "a ring of two vertices": Z.from_rings([[tri, tri[:2]]]),
        "a NaN vertex": Z.from_rings([[[(0.0, 0.0), (np.nan, 1.0), (1.0, 0.5)]]]),
        "an infinite vertex": Z.from_rings([[[(0.0, 0.0), (0.0, np.inf), (1.0, 0.5)]]]),
        "lat above 90": Z.from_rings([[[(0.0, 0.0), (90.0001, 1.0), (1.0, 0.5)]]]),
        "lon below -180": Z.from_rings([[[(0.0, -180.0001), (0.0, 1.0), (1.0, 0.5)]]]),
        "zone_rings not from 0": Z([1, 1], [0, 3], *zip(*tri)),
        "a zone without a ring": Z([0, 0, 1], [0, 3], *zip(*tri)),
        "ring_verts not from 0": Z([0, 1], [1, 3], *zip(*tri)),
        "ring_verts descending": Z([0, 2], [0, 3, 2], *zip(*(tri + tri))),
    }
    for what, z in cases.items():
        assert _code(lambda: call(z)).code == _lib.HM_E_INVALID, what
        assert _code(lambda: _lib.positions_within_selftest(z, dc.boston(5))).code == _lib.HM_E_INVALID, what
    assert call(Z.from_rings([[[(-90.0, -180.0), (90.0, -180.0), (90.0, 180.0), (-90.0, 180.0)]]]))[1].tolist() == [1]   # the limits themselves


def test_zones_from_geojson_round_trips():
    from mobheat import readside
    poly = {"type": "Polygon", "coordinates": [[[-71.15, 42.25], [-71.0, 42.25], [-71.0, 42.4], [-71.15, 42.4], [-71.15, 42.25]],
                                               [[-71.1, 42.3], [-71.05, 42.3], [-71.05, 42.35], [-71.1, 42.3]]]}
    multi = {"type": "MultiPolygon", "coordinates": [poly["coordinates"], [[[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [0.5, 1.0, 5.0]]]]}
    fc = {"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": poly, "properties": {}},
                                                    {"type": "Feature", "geometry": multi, "properties": {"name": "m"}}]}
    z = readside.zones_from_geojson(poly)
    assert z.n_zones == 1 and z.zone_rings.tolist() == [0, 2] and z.ring_verts.tolist() == [0, 4, 7]
    assert z.lat[:4].tolist() == [42.25, 42.25, 42.4, 42.4] and z.lon[:4].tolist() == [-71.15, -71.0, -71.0, -71.15]
    m = readside.zones_from_geojson(multi)
    assert m.n_zones == 1 and m.ring_verts.tolist() == [0, 4, 7, 10]   # one zone of all its rings; an open ring keeps its last vertex
    both = readside.zones_from_geojson(json.dumps(fc))
    assert both.n_zones == 2 and both.zone_rings.tolist() == [0, 2, 5]
    assert readside.zones_from_geojson(fc["features"][0]).lat.tolist() == z.lat.tolist()
    back = readside.zones_from_geojson(readside.zones_to_geojson(both))
    for f in ("zone_rings", "ring_verts", "lat", "lon"):
        assert np.array_equal(getattr(back, f), getattr(both, f)), f
    for name in wc.SMALL:
        a = wc.zone_set(name)
        b = readside.zones_from_geojson(json.loads(json.dumps(readside.zones_to_geojson(a))))
        if name != "degenerate":   # (its out-and-back ring ends where it starts: closing it is a no-op that the reader undoes)
            assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("zone_rings", "ring_verts", "lat", "lon")), name
    with pytest.raises(ValueError):
        readside.zones_from_geojson({"type": "Point", "coordinates": [0, 0]})


def _tiles(n=4000, seed=2, dyadic=True):
    """STATE_REC_DTYPE records with centroids over BOX (and a few outside), counts 1..9 and speeds"""
    from mobheat._lib import STATE_REC_DTYPE
    rng = np.random.default_rng(seed)
    la, lo = wc.random_points(n, seed)
    r = np.zeros(n, STATE_REC_DTYPE)
    r["cell"] = np.arange(n) + (8 << 52)
    r["count"] = rng.integers(1, 10, n)
    r["n_speed"] = rng.integers(0, 3, n)
    speed = rng.integers(0, 4096, n) / 64.0 if dyadic else rng.uniform(0.0, 120.0, n)
    r["sum_speed"] = np.where(r["n_speed"] > 0, speed * r["n_speed"], 0.0)
    r["sum_lat"], r["sum_lon"] = la * r["count"], lo * r["count"]
    return r


@pytest.mark.parametrize("name", wc.SMALL + ("triangles4096",))
def test_query_selftests_against_numpy(name):
    from mobheat import _lib
    zones = wc.zone_set(name)
    n = 3000 if name in wc.SMALL else 400
    recs = dc.boston(n, seed=11)
    la, lo = wc.edge_points(zones, stride=1 if name in wc.SMALL else 41)
    recs["lat"][:la.size][: n // 2], recs["lon"][:lo.size][: n // 2] = la[: n // 2], lo[: n // 2]
    for since in (None, dc.T0 + 100 * dc.SEC, dc.T0 + 10_000 * dc.SEC):
        out, zone, tot = _lib.positions_within_selftest(zones, recs, since)
        wout, wzone, wtot = wc.positions_expected(zones, recs, since)
        assert out.tobytes() == wout.tobytes() and np.array_equal(zone, wzone), f"{name} since {since}"
        wc.same_totals(tot, wtot, f"{name} since {since}")
        assert np.all(tot["n_speed"] == 0) and tot["sum_speed"].tobytes() == np.zeros(tot.size).tobytes()
        if since is not None and since > dc.T0 + 1000 * dc.SEC:
            assert out.size == 0 and np.all(tot["newest_us"] == dc.INT64_MIN) and not tot["n"].any()
    tiles = _tiles(n)
    out, zone, tot = _lib.tiles_within_selftest(zones, tiles)
    wout, wzone, wtot = wc.tiles_expected(zones, tiles)
    assert out.tobytes() == wout.tobytes() and np.array_equal(zone, wzone), name
    wc.same_totals(tot, wtot, name)
    assert not tot["newest_us"].any() and (out.size > 0 or name == "degenerate")
    if name == "overlapping_squares":   # a point counts in every zone that contains it
        assert tot["n"].sum() > out.size


@pytest.mark.parametrize("name", wc.STAGED)
def test_staged_sets_host_execution(name):
    """the sets at the LDS staging's and the LDS totals' edges: their geometry is what their names say, the host execution
    equals numpy on random points, vertices and on-edge points, and the exact rule wherever it decides"""
    from mobheat import _lib, readside
    zones = wc.zone_set(name)
    edges = np.diff(zones.ring_verts)[np.asarray(zones.zone_rings[:-1])]   # (one ring per zone)
    assert zones.n_zones == zones.ring_verts.size - 1
    if name == "stage_span":
        assert edges.tolist() == [3, 1500, 3] and 3 % wc.STAGE and 1503 % wc.STAGE and 1503 > 2 * wc.STAGE
    if name == "stage_end":
        assert edges.tolist() == [509, 3, 512] and 509 + 3 == wc.STAGE
    if name.startswith("triangles"):
        assert zones.n_zones == {"triangles1024": wc.ZLDS, "triangles1025": wc.ZLDS + 1}[name] and np.all(edges == 3)
    la, lo = wc.random_points(3000, seed=17)
    ela, elo = wc.edge_points(zones, stride=3)
    lat, lon = np.r_[la, zones.lat[::5], ela], np.r_[lo, zones.lon[::5], elo]
    first, hits = _lib.points_in_zones_selftest(zones, lat, lon)
    nfirst, nhits = readside.points_in_zones(zones, lat, lon)
    assert np.array_equal(first, nfirst) and np.array_equal(hits, nhits), f"{name}: {int((hits != nhits).sum())} differ"
    assert hits.any() and np.all((first >= 0) == (hits > 0)) and np.all(first < zones.n_zones)
    if name in ("stage_span", "stage_end"):   # every zone of the set holds some point, the ones behind a stage end too
        assert (readside.zone_totals_of(zones, la, lo, ts_us=np.zeros(la.size, np.int64))[1]["n"] > 0).all()
    xla, xlo = wc.random_points(60 if name.startswith("triangles") else 150, seed=23)
    efirst, ehits, decided = wc.exact(zones, xla, xlo)
    xfirst, xhits = _lib.points_in_zones_selftest(zones, xla, xlo)
    assert decided.mean() > 0.9
    assert np.array_equal(xfirst[decided], efirst[decided]) and np.array_equal(xhits[decided], ehits[decided])
    recs = dc.boston(2000, seed=19)
    out, zone, tot = _lib.positions_within_selftest(zones, recs)
    wout, wzone, wtot = wc.positions_expected(zones, recs)
    assert out.tobytes() == wout.tobytes() and np.array_equal(zone, wzone), name
    wc.same_totals(tot, wtot, name)
    tiles = _tiles(2000)
    out, zone, tot = _lib.tiles_within_selftest(zones, tiles)
    wout, wzone, wtot = wc.tiles_expected(zones, tiles)
    assert out.tobytes() == wout.tobytes() and np.array_equal(zone, wzone), name
    wc.same_totals(tot, wtot, name)
