"""CPU: the radius queries' host execution (the kernels' HM_HD code: hm_selftest_near_distances, hm_selftest_positions_near,
hm_selftest_tiles_near) against the comparison form in mobheat/readside.py (near_distance_m through the running glibc,
near_order).  Equality is bit equality: there is no tolerance."""
import math

import numpy as np
import pytest

import near_cases as nc


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def test_distances_random_pairs(oracle_h3):
    from mobheat import _lib, readside
    rng = np.random.default_rng(0)
    n = 1_000_000
    la, lo = nc.sphere(rng, n)
    # a third of them within a few km of the query, where sin's small-argument paths run
    for q, (lat0, lon0) in enumerate(nc.QUERIES):
        part = slice(q * n // 6, (q + 1) * n // 6)
        lat, lon = la[part].copy(), lo[part].copy()
        near = np.arange(lat.size) % 3 == 0
        lat[near] = np.clip(lat0 + rng.normal(0.0, 0.02, int(near.sum())), -90.0, 90.0)
        lon[near] = lon0 + rng.normal(0.0, 0.02, int(near.sum()))
        got = _lib.near_distances_selftest(lat0, lon0, lat, lon)
        want = readside.near_distance_m(lat0, lon0, lat, lon)
        assert np.array_equal(_bits(got), _bits(want)), f"query {q}: {int((_bits(got) != _bits(want)).sum())} distances differ"
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= nc.PI_R_UP) and not np.any(np.signbit(got))


@pytest.mark.parametrize("q", range(len(nc.QUERIES)))
def test_distances_cases(oracle_h3, q):
    from mobheat import _lib, readside
    lat0, lon0 = nc.QUERIES[q]
    for name, lat, lon, _ in nc.candidates(lat0, lon0):
        got = _lib.near_distances_selftest(lat0, lon0, lat, lon)
        want = readside.near_distance_m(lat0, lon0, lat, lon)
        assert np.array_equal(_bits(got), _bits(want)), name
        assert np.all((got >= 0.0) & (got <= nc.PI_R_UP)), name
        one = [readside.near_distance_m(lat0, lon0, float(a), float(b)) for a, b in zip(lat[:20], lon[:20])]   # scalar form
        assert np.array_equal(_bits(one), _bits(got[:20])), name
        if name == "special":
            assert _bits(got[:1])[0] == 0, "the query point itself: +0.0"
            if q == 0:   # (a == 1 exactly at (0, 0); elsewhere its roundings may leave r a few ulps below 1)
                assert got[1] == (2.0 * nc.R) * math.asin(1.0), "the antipode: pi R rounded"


def test_distance_symmetry_and_nan(oracle_h3):
    from mobheat import _lib
    lat, lon = nc.mirror_pairs()
    d = _lib.near_distances_selftest(0.0, 0.0, lat, lon).reshape(4, -1)
    assert all(np.array_equal(_bits(d[0]), _bits(d[k])) for k in (1, 2, 3)), "mirror images around an equatorial query"
    bad = _lib.near_distances_selftest(10.0, 20.0, [np.nan, 1.0, np.inf, 1.0], [1.0, np.nan, 1.0, -np.inf])
    assert np.all(np.isnan(bad))


def _check(kind, lat0, lon0, lat, lon, key, what):
    from mobheat import _lib, readside
    if kind == "positions":
        recs, host, ref = nc.position_records(lat, lon, key), _lib.positions_near_selftest, readside.positions_near_of
        plat, plon = lat, lon
    else:
        recs, host, ref = nc.tile_records(lat, lon, key), _lib.tiles_near_selftest, readside.tiles_near_of
        plat, plon = recs["sum_lat"] / recs["count"], recs["sum_lon"] / recs["count"]
    dist = readside.near_distance_m(lat0, lon0, plat, plon)
    for r in nc.radii(dist):
        within = int(((dist == dist) & (dist <= r)).sum())
        for k in nc.ks(recs.size):
            got, gd = host(recs, lat0, lon0, r, k)
            # the order by numpy on the Python distances
            o = np.flatnonzero((dist == dist) & (dist <= r))
            o = o[readside.near_order(dist[o], key[o], k)]
            nc.same(got, recs[o], f"{what} r {r} k {k}: host execution against near_order")
            assert np.array_equal(_bits(gd), _bits(dist[o])), f"{what} r {r} k {k}: distances"
            want, wd = ref(recs, lat0, lon0, r, k)
            nc.same(got, want, f"{what} r {r} k {k}: readside form")
            assert np.array_equal(_bits(gd), _bits(wd)) and got.size == min(k, within)
    own = nc.radii(dist)[2]
    assert int((dist <= own).sum()) > int((dist <= math.nextafter(own, 0.0)).sum()), f"{what}: the closed comparison decides"


@pytest.mark.parametrize("kind", ["positions", "tiles"])
@pytest.mark.parametrize("q", range(len(nc.QUERIES)))
def test_near_host_cases(oracle_h3, kind, q):
    lat0, lon0 = nc.QUERIES[q]
    for name, lat, lon, key in nc.candidates(lat0, lon0):
        _check(kind, lat0, lon0, lat, lon, key, f"{kind} query {q} {name}")


def test_mirror_pairs_tie_on_the_key(oracle_h3):
    lat, lon = nc.mirror_pairs()
    key = np.random.default_rng(3).permutation(lat.size).astype(np.uint64)
    _check("positions", 0.0, 0.0, lat, lon, key, "mirror pairs")


def test_since_and_nan_candidates(oracle_h3):
    from mobheat import _lib, readside
    rng = np.random.default_rng(6)
    lat, lon = nc.sphere(rng, 500)
    lat[::50] = np.nan
    lon[7::50] = np.inf
    ts = nc.T0 + rng.integers(0, 100, 500) * nc.SEC
    recs = nc.position_records(lat, lon, np.arange(500, dtype=np.uint64), ts)
    for since in (None, nc.INT64_MIN, int(ts.min()) - 1, int(ts[3]), int(ts.max()) + 1):
        got, gd = _lib.positions_near_selftest(recs, 42.0, -71.0, math.inf, 500, since)
        want, wd = readside.positions_near_of(recs, 42.0, -71.0, math.inf, 500, since)
        nc.same(got, want, f"since {since}")
        assert np.array_equal(_bits(gd), _bits(wd)) and not np.any(np.isnan(gd))
        kept = recs if since is None else recs[recs["ts_us"] >= since]
        assert got.size == int((np.isfinite(kept["lat"]) & np.isfinite(kept["lon"])).sum())
    assert _lib.positions_near_selftest(recs, 42.0, -71.0, math.inf, 500, int(ts[3]))[0]["ts_us"].min() == ts[3]   # equal: kept


def test_near_from_query():
    from mobheat import readside
    assert readside.near_from_query("42.36", "-71.05", "500") == (42.36, -71.05, 500.0)
    assert readside.near_from_query("-90", "180", None) == (-90.0, 180.0, math.inf)
    assert readside.near_from_query(0, -180, "") == (0.0, -180.0, math.inf)
    assert readside.near_from_query("1", "2", "inf")[2] == math.inf and readside.near_from_query("1", "2", "0")[2] == 0.0
    for bad in [("x", "1", "2"), ("1", None, "2"), ("nan", "1", "2"), ("1", "nan", "2"), ("1", "2", "nan"), ("90.0001", "1", "2"),
                ("1", "-180.0001", "2"), ("1", "2", "-1"), ("inf", "1", "2"), ("1", "2", "-inf")]:
        with pytest.raises(ValueError):
            readside.near_from_query(*bad)


@pytest.mark.parametrize("q", [(math.nan, 0.0, 1.0), (90.0001, 0.0, 1.0), (0.0, -180.0001, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, math.nan),
                               (0.0, math.inf, 1.0), (0.0, 0.0, -math.inf)])
def test_invalid_queries(mobheat_lib, q):
    from mobheat import _lib
    recs = nc.position_records(np.zeros(3), np.zeros(3), np.arange(3))
    tiles = nc.tile_records(np.zeros(3), np.zeros(3), np.arange(3))
    assert _code(lambda: _lib.positions_near_selftest(recs, *q)) == _lib.HM_E_INVALID
    assert _code(lambda: _lib.tiles_near_selftest(tiles, *q)) == _lib.HM_E_INVALID
    qs = _lib.near_struct(*q)
    out = np.zeros(3)
    import ctypes
    assert mobheat_lib.hm_selftest_near_distances(ctypes.byref(qs), out.ctypes.data, out.ctypes.data, 3, out.ctypes.data) == _lib.HM_E_INVALID


def test_k_out_of_range(mobheat_lib):
    from mobheat import _lib
    recs = nc.position_records(np.zeros(3), np.zeros(3), np.arange(3))
    for k in (-1, nc.TOP_MAX + 1):
        assert _code(lambda: _lib.positions_near_selftest(recs, 0.0, 0.0, 1.0, k)) == _lib.HM_E_INVALID
    assert _lib.positions_near_selftest(recs, 0.0, 0.0, 1.0, 0)[0].size == 0


# ---- the feature encoders with a distance per record ----
def _with_distance(collection, dist):
    out = []
    for f, d in zip(collection["features"], dist):
        f = dict(f)
        f["properties"] = dict(f["properties"], distanceM=float(d))
        out.append(f)
    return {"type": "FeatureCollection", "features": out}


def _distances(n, seed=9):
    """distances of every shape float.__repr__ takes: +0.0, pi R, integers, tiny and 17-digit values"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, nc.PI_R_UP, n)
    d[:6] = [0.0, math.pi * nc.R, 500.0, 1e-7, 1.5e16, 123456.78901234567][:min(n, 6)]
    return d


@pytest.mark.parametrize("n", [0, 1, 300])
def test_tile_features_with_distance_equal_json_dumps(n):
    import geojson_cases as gc
    from mobheat import _lib
    cells = gc.tile_cells(_lib.cells_to_boundary_host_selftest)
    recs = gc.tile_records(cells)[:n]
    dist = _distances(n)
    body, offs = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT, dist)
    want = _with_distance(gc.tile_collection(recs, gc.WS_TEXT, gc.WE_TEXT, _lib.cells_to_boundary_host_selftest), dist)
    gc.check_body(body, offs, want)
    if n:
        assert bytes(body[offs[0]: offs[1] - 1]).endswith(b',"distanceM":0.0}}')
        assert max(int(offs[i + 1] - offs[i]) for i in range(n)) <= 872 + 38
    else:
        assert bytes(body) == b'{"type":"FeatureCollection","features":[]}'
    # without distances: the bytes of the existing encoder (its own tests pin those)
    plain, po = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    gc.check_body(plain, po, gc.tile_collection(recs, gc.WS_TEXT, gc.WE_TEXT, _lib.cells_to_boundary_host_selftest))
    assert b"distanceM" not in bytes(plain)


def test_null_distances_reproduce_the_existing_encoders(mobheat_lib):
    """the new entry points with dist_m NULL write what hm_selftest_tile_features / _position_features write"""
    import ctypes

    import geojson_cases as gc
    from mobheat import _lib
    cells = gc.tile_cells(_lib.cells_to_boundary_host_selftest)
    recs = gc.tile_records(cells)
    old, oo = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    cfg, keep = _lib.geojson_cfg(gc.WS_TEXT, gc.WE_TEXT)
    buf, offs = np.zeros(64 + 920 * recs.size, np.uint8), np.zeros(recs.size + 1, np.int64)
    assert mobheat_lib.hm_selftest_tile_features_near(ctypes.byref(cfg), recs.ctypes.data, recs.size, None, buf.ctypes.data, buf.size,
                                                      offs.ctypes.data) == 0
    assert np.array_equal(offs, oo) and bytes(buf[:old.size]) == bytes(old)
    rows = gc.position_rows()
    ids, bo = gc.bucket_table([r[2] for r in rows])
    precs = gc.position_records(rows, gc.POSITION_STRINGS, gc.POSITION_STRINGS)
    d = gc.dictionary(gc.POSITION_STRINGS)
    old, oo = _lib.position_features_selftest(precs, d, d, ids, bo)
    pcfg, keep2 = _lib.position_dicts_cfg(d, d)
    bi, bf = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(bo, np.int64)
    pcfg.n_buckets, pcfg.bucket_ids, pcfg.bucket_offset_s = bi.size, bi.ctypes.data, bf.ctypes.data
    buf, offs = np.zeros(old.size + 64, np.uint8), np.zeros(precs.size + 1, np.int64)
    assert mobheat_lib.hm_selftest_position_features_near(ctypes.byref(pcfg), precs.ctypes.data, precs.size, None, buf.ctypes.data,
                                                          buf.size, offs.ctypes.data) == 0
    assert np.array_equal(offs, oo) and bytes(buf[:old.size]) == bytes(old)


@pytest.mark.parametrize("n", [0, 1, None])
def test_position_features_with_distance_equal_json_dumps(n):
    """strings that need escaping, every ts shape, and a distance of every shape"""
    import geojson_cases as gc
    from mobheat import _lib
    rows = gc.position_rows()
    rows = rows if n is None else rows[5:5 + n]
    ids, bo = gc.bucket_table([r[2] for r in rows])
    recs = gc.position_records(rows, gc.POSITION_STRINGS, gc.POSITION_STRINGS)
    d = gc.dictionary(gc.POSITION_STRINGS)
    dist = _distances(len(rows))
    body, o = _lib.position_features_selftest(recs, d, d, ids, bo, dist)
    gc.check_body(body, o, _with_distance(gc.position_collection(rows, ids, bo), dist))
    if n is None:
        assert b'\\u0000\\u0001' in bytes(body) and bytes(body).count(b',"distanceM":') == len(rows)
