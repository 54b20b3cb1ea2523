"""GPU: the polygon geofences (hm_points_in_zones, hm_positions_within, hm_window_within and their bodies; k_within.h).
Device == host execution of the same predicate (hm_selftest_*): labels, hit counts, kept records, counts, n, n_speed and
newest_us exactly; sum_speed bit-equal on dyadic speeds and by density_cases.REL on the average otherwise.
tests/test_within_host.py ties the host execution to numpy and to the exact rule on the CPU."""
import json

import numpy as np
import pytest

import density_cases as dc
import geojson_cases as gc
import within_cases as wc

pytestmark = pytest.mark.gpu
EMPTY = b'{"type":"FeatureCollection","features":[]}'


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _engine(**kw):
    import mobheat
    return mobheat.HeatmapEngine(h3_res=8, device=0, **kw)


@pytest.mark.parametrize("name", wc.ALL)
def test_points_device_equals_host(name):
    from mobheat import _lib
    zones = wc.zone_set(name)
    sets = wc.point_sets(name, 5000)   # (5,000 random points against every set, the 65,536-vertex one included)
    sets.append(("one point", np.array([42.3]), np.array([-71.07])))
    sets.append(("a tile and one", *wc.random_points(wc.TILE + 1, 9)))
    for what, lat, lon in sets:
        first, hits = _lib.points_in_zones_selftest(zones, lat, lon, device=0)
        hfirst, hhits = _lib.points_in_zones_selftest(zones, lat, lon)
        assert np.array_equal(first, hfirst) and np.array_equal(hits, hhits), f"{name} {what}: {int((hits != hhits).sum())} differ"
    assert hhits.any()


def test_mesh_partitions_its_box_on_the_device():
    from mobheat import _lib
    zones = wc.mesh()
    lat, lon = wc.random_points(50_000, 5, margin=0.0)
    ela, elo = wc.edge_points(zones)
    vla, vlo = wc.mesh_vertices()
    lat, lon = np.r_[lat, ela, vla.ravel()], np.r_[lon, elo, vlo.ravel()]
    ok = (lat > wc.BOX[0]) & (lat < wc.BOX[1]) & (lon > wc.BOX[2]) & (lon < wc.BOX[3])
    first, hits = _lib.points_in_zones_selftest(zones, lat[ok], lon[ok], device=0)
    assert ok.sum() > 50_000 and np.all(hits == 1), np.bincount(hits).tolist()


def _by_key(recs, zone):
    o = np.argsort((recs["provider"].astype(np.uint64) << np.uint64(32)) | recs["vehicle"].astype(np.uint64), kind="stable")
    return recs[o].tobytes(), zone[o].tolist()


def _check_positions(eng, zones, since, what):
    from mobheat import _lib
    pos = eng.positions()[0]
    got, gz, gt = eng.positions_within(zones, since)
    info = eng.within_info()
    want, wz, wt = _lib.positions_within_selftest(zones, pos, since)
    assert _by_key(got, gz) == _by_key(want, wz), f"{what} since {since}: records and labels"
    wc.same_totals(gt, wt, f"{what} since {since}")
    none, nz, only = eng.positions_within(zones, since, records=False)   # the totals-only form
    assert none is None and nz is None
    wc.same_totals(only, wt, f"{what} since {since}, totals only")
    kept = pos.size if since is None else int((pos["ts_us"] >= since).sum())
    hits = _lib.points_in_zones_selftest(zones, pos["lat"], pos["lon"])[1]
    inside = int(((hits > 0) & (True if since is None else pos["ts_us"] >= since)).sum())
    for i in (info, eng.within_info()):
        assert (i["scanned"], i["kept_since"], i["in_zone"], i["zones"], i["vertices"]) == \
            (eng.positions_info()["capacity"], kept, inside, zones.n_zones, zones.lat.size), i
    assert got.size == inside
    return got, gt


@pytest.fixture(scope="module")
def state():
    """a positions state of more than one scan tile's slots, free slots between the live ones: Boston vehicles, half of
    them moved onto the mesh's and the other sets' edges and vertices, density_cases.since_edges' keys, two NaN points"""
    recs = dc.boston(4000, seed=13)
    k = 0
    for name in wc.ALL:
        z = wc.zone_set(name)
        la, lo = wc.edge_points(z, stride=1 if name in wc.SMALL else 211)
        la, lo = np.r_[la, z.lat[::7][:60]][:330], np.r_[lo, z.lon[::7][:60]][:330]
        recs["lat"][k:k + la.size], recs["lon"][k:k + la.size] = la, lo
        k += la.size
    assert k < 3500
    edge, since = dc.since_edges()
    recs["lat"][k:k + edge.size], recs["lon"][k:k + edge.size], recs["ts_us"][k:k + edge.size] = edge["lat"], edge["lon"], edge["ts_us"]
    recs["lat"][-1], recs["lon"][-2] = np.nan, np.nan
    eng = _engine()
    assert eng.within_info() == dict.fromkeys(eng.within_info(), 0)   # all 0 before the first call
    dc.load(eng, recs)
    cap = eng.positions_info()["capacity"]
    assert cap >= wc.TILE + 1 and cap >= 2 * recs.size
    yield eng, since
    eng.close()


@pytest.mark.parametrize("name", wc.ALL)
def test_positions_within(state, name):
    eng, since = state
    zones = wc.zone_set(name)
    for s in (None, since - 1, since, since + 1, since + 10_000 * dc.SEC):
        got, tot = _check_positions(eng, zones, s, name)
    assert got.size == 0 and not tot["n"].any() and np.all(tot["newest_us"] == dc.INT64_MIN)   # nobody that new
    got, tot = _check_positions(eng, zones, None, name)
    assert got.size > 0 and eng.within_info()["scan_us"] > 0
    if name == "overlapping_squares":
        assert tot["n"].sum() > got.size   # a vehicle counts in every zone that contains it
    if name == "mesh":
        assert tot["n"].sum() == got.size and (tot["n"] > 0).all()


def test_positions_within_reads_only_and_allocates_nothing_twice(state):
    eng, _ = state
    zones = wc.mesh()
    version, pos0 = eng.state_version(), np.sort(eng.positions()[0], order="vehicle").tobytes()
    keep = []
    for _ in range(2):
        c0 = eng.last_counts()
        r, z, t = eng.positions_within(zones)
        keep.append((_by_key(r, z), t.tobytes()))
        c1 = eng.last_counts()
    assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
    assert keep[0] == keep[1] and eng.state_version() == version
    assert np.sort(eng.positions()[0], order="vehicle").tobytes() == pos0


def _window_engine(dyadic):
    from mobheat import synth
    eng = _engine()
    b = synth.c1_boston(n=6000)
    if dyadic:   # sums that are exact in any order: two roll-ups of one window give the same bytes
        b["lat"], b["lon"] = np.round(b["lat"] * 4096) / 4096, np.round(b["lon"] * 4096) / 4096
        b["speed"] = np.round(b["speed"] * 64) / 64
    eng.process_batch(0, **b)
    return eng


@pytest.mark.parametrize("dyadic", (True, False))
def test_window_within(dyadic):
    from mobheat import _lib
    eng = _window_engine(dyadic)
    try:
        ws = int(eng.live_windows()[0][-1])
        for res in (8, 5):
            recs = eng.window_records(ws, res)
            assert recs.size > 3
            for name in wc.ALL:
                zones = wc.zone_set(name)
                got, gz, gt = eng.window_within(zones, ws, res)
                info = eng.within_info()
                want, wz, wt = _lib.tiles_within_selftest(zones, recs)
                o, p = np.argsort(got["cell"]), np.argsort(want["cell"])
                what = f"{name} res {res}"
                assert np.array_equal(got["cell"][o], want["cell"][p]) and np.array_equal(gz[o], wz[p]), what
                for f in ("count", "n_speed", "window_start_us"):
                    assert np.array_equal(got[f][o], want[f][p]), f"{what}: {f}"
                if dyadic:
                    assert got[o].tobytes() == want[p].tobytes(), what
                wc.same_totals(gt, wt, what, dyadic=dyadic)
                assert not gt["newest_us"].any()
                assert (info["scanned"], info["kept_since"], info["in_zone"], info["zones"], info["vertices"]) == \
                    (recs.size, recs.size, want.size, zones.n_zones, zones.lat.size), info
                _, _, only = eng.window_within(zones, ws, res, records=False)
                wc.same_totals(only, wt, what + ", totals only", dyadic=dyadic)
                if name in ("mesh", "concave_c"):
                    assert got.size > 0, what
        got, gz, gt = eng.window_within(wc.mesh(), ws + 7, 8)   # a window that is not live
        assert got.size == 0 and gz.size == 0 and gt.size == 128 and not gt["n"].any() and not gt["count"].any()
    finally:
        eng.close()


def _batches():
    from positions_ref import Batch
    rng = np.random.default_rng(12)
    n = 1500
    la, lo = rng.uniform(42.20, 42.45, n), rng.uniform(-71.20, -70.95, n)
    rows = [("p", f"v{k}", dc.T0 + k % 60 * dc.SEC, la[k], lo[k]) for k in range(n)]
    rows += [("q\"\\", f"w\n{k}é", dc.T0 + (100 + k % 60) * dc.SEC, la[k] + 0.001, lo[k]) for k in range(0, n, 3)]
    return [Batch(rows)]


def _sorted_features(collection):
    return sorted(gc.dumps(f) for f in collection["features"])


def test_bodies():
    """both bodies equal readside's comparison collections, feature order apart (the compaction fixes none); the
    dictionaries hold strings that need escaping; nothing inside gives the 42-byte empty body"""
    from positions_ref import run
    from mobheat import readside
    eng = _engine()
    try:
        far = readside.zones_from_geojson({"type": "Polygon", "coordinates": [[[10.0, 10.0], [11.0, 10.0], [10.5, 11.0], [10.0, 10.0]]]})
        assert eng.positions_within_geojson(wc.mesh()) == EMPTY and eng.window_within_geojson(wc.mesh()) == EMPTY   # no state at all
        for epoch, b in enumerate(_batches()):
            run(eng, epoch, b)
        for name in ("triangle", "square_with_hole", "overlapping_squares", "mesh", "circles"):
            zones = wc.zone_set(name)
            want = readside.positions_within_from_engine(eng, zones)
            body = readside.positions_within_body(eng, zones)
            assert _sorted_features(json.loads(body)) == _sorted_features(want), name
            assert 0 < len(want["features"]) and body.startswith(b'{"type":"FeatureCollection","features":[{') and b"zone" not in body
            b2, recs, offs = eng.positions_within_geojson(zones, with_records=True)
            assert recs.size == len(want["features"]) == offs.size - 1 and len(b2) == len(body)
            assert sorted(bytes(b2[offs[i]: offs[i + 1] - 1]) for i in range(recs.size)) == _sorted_features(want), name   # the bytes themselves
            for res in (8, 5):
                want = readside.tiles_within_from_engine(eng, zones, res)
                body = readside.tiles_within_body(eng, zones, res)
                got = json.loads(body)
                key = lambda c: sorted((f["properties"]["cellId"], f["properties"]["count"], f["properties"]["windowStart"],
                                        gc.dumps(f["geometry"])) for f in c["features"])
                assert key(got) == key(want) and len(want["features"]) > 0, f"{name} res {res}"
                b2, recs, offs = eng.window_within_geojson(zones, None, res, with_records=True)
                assert recs.size == len(want["features"]) == offs.size - 1
                assert sorted(recs["cell"].tolist()) == sorted(eng.window_within(zones, None, res)[0]["cell"].tolist())
        assert b'"provider":"q\\"\\\\"' in readside.positions_within_body(eng, wc.mesh())
        assert eng.positions_within_geojson(far) == EMPTY and eng.window_within_geojson(far) == EMPTY and len(EMPTY) == 42
        ws = int(eng.live_windows()[0][-1])
        assert eng.window_within_geojson(wc.mesh(), ws + 7) == EMPTY   # a window that is not live
        # the unfiltered bodies keep their bytes after a within body used the encoder's buffers
        whole = json.loads(eng.positions_geojson())
        assert len(whole["features"]) == eng.positions()[0].size
    finally:
        eng.close()


def test_errors():
    from mobheat import _lib
    Z = _lib.Zones
    tri = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.5)]
    bad = [Z.from_rings([[tri]] * (_lib.HM_ZONES_MAX + 1)), Z.from_rings([[tri[:2]]]), Z.from_rings([[[(0.0, 0.0), (np.nan, 1.0), (1.0, 0.5)]]]),
           Z.from_rings([[[(0.0, 0.0), (91.0, 1.0), (1.0, 0.5)]]]), Z([0, 0, 1], [0, 3], *zip(*tri))]
    eng = _window_engine(True)
    try:
        dc.load(eng, dc.boston(300))
        for z in bad:
            for call in (lambda: eng.positions_within(z), lambda: eng.window_within(z), lambda: eng.positions_within_geojson(z),
                         lambda: eng.window_within_geojson(z), lambda: _lib.points_in_zones_selftest(z, [0.5], [0.5], device=0)):
                assert _code(call) == _lib.HM_E_INVALID
        assert "HM_ZONES_MAX" in str(pytest.raises(_lib.MobheatError, lambda: eng.positions_within(bad[0])).value)
        assert _code(lambda: eng.window_within(wc.mesh(), res=9)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.window_within_geojson(wc.mesh(), res=-1)) == _lib.HM_E_INVALID
        none = Z.from_rings([])   # no zone: nothing is inside
        r, z, t = eng.positions_within(none)
        assert r.size == 0 and z.size == 0 and t.size == 0 and eng.window_within(none)[0].size == 0
        assert eng.positions_within(wc.mesh())[0].size > 0   # and the engine works on
    finally:
        eng.close()
    empty = _engine()
    try:   # no positions state, no window
        r, z, t = empty.positions_within(wc.mesh())
        assert r.size == 0 and not t["n"].any() and np.all(t["newest_us"] == dc.INT64_MIN)
        assert empty.window_within(wc.mesh())[0].size == 0
    finally:
        empty.close()
    shard = _engine(shard=(0, 2))
    try:
        for call in (lambda: shard.positions_within(wc.mesh()), lambda: shard.window_within(wc.mesh()),
                     lambda: shard.positions_within_geojson(wc.mesh()), lambda: shard.window_within_geojson(wc.mesh())):
            assert _code(call) == _lib.HM_E_UNSUPPORTED
    finally:
        shard.close()
