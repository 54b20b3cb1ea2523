"""GPU: the positions state aggregated into H3 density cells (hm_positions_density*, k_density.h).  Device == host
execution (hm_selftest_positions_density) == the oracle's restatement (tests/density_cases.py), with that file's bars: cell
set, count, newest ts and the zero fields bit-equal, averages within REL = 1e-9 / ABS_DEG = 1e-12, sums bit-equal on
dyadic coordinates.  tests/test_density_host.py proves on the CPU that the cases reach the regimes they claim."""
import ctypes
import json

import numpy as np
import pytest

import density_cases as dc
import raster_cases as rc
import view_cases as vc

pytestmark = pytest.mark.gpu
EMPTY = b'{"type":"FeatureCollection","features":[]}'
# csrc/k_rollup.h's and csrc/dev_table.h's constants, which the library does not export: a change there must be made here
RU_THREADS, DUMP_PER, RU_SLOTS = 1024, 8, 2048
TILE_SLOTS = RU_THREADS * DUMP_PER   # the slots one group-by workgroup takes per iteration
RU_FILL = RU_SLOTS // 2              # the keys a workgroup's LDS front table takes before it spills


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _engine(recs=None, **kw):
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, **kw)
    if recs is not None:
        dc.load(eng, recs)
    return eng


def _check(eng, recs, res, since=None, dyadic=False, what=""):
    """device == host execution == oracle; returns (device records, info)"""
    from mobheat import _lib
    want, bad = dc.expected(recs, res, since)
    got = eng.positions_density(res, since)
    info = eng.positions_density_info()
    host, host_bad = _lib.positions_density_selftest(recs, res, since)
    dc.check(got, want, dyadic, f"{what} res {res} since {since}: device against the oracle")
    dc.check(host, want, dyadic, f"{what} res {res} since {since}: host execution against the oracle")
    kept = int((recs["ts_us"] >= (dc.INT64_MIN if since is None else since)).sum())
    assert (info["keys"], info["kept"], info["unsnapped"], info["groups"], info["returned"]) == (recs.size, kept, bad, want.size, want.size)
    assert host_bad == bad
    return got, info


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2048, 4096, 4097])
def test_sizes(n):
    """2048 / 4096 / 4097 keys: a pair table of 4096, 8192 and 16384 slots -- below, exactly and twice one workgroup tile
    (a capacity is a power of two, so one slot more than a tile is the next power)"""
    recs = dc.sized(n)
    eng = _engine(recs)
    try:
        cap = eng.positions_info()["capacity"]
        if n >= 2048:
            assert cap == {2048: TILE_SLOTS // 2, 4096: TILE_SLOTS, 4097: 2 * TILE_SLOTS}[n]
        assert eng.positions_density_info() == dict.fromkeys(eng.positions_density_info(), 0)   # all 0 before the first call
        for res in (8, 0):
            _, info = _check(eng, recs, res, what=f"n {n}")
            if n:
                assert info["workgroups"] == max(1, cap // TILE_SLOTS) and info["device_us"] > 0
                assert info["table_slots"] >= 1024
        if n == 0:
            assert eng.positions_density(8).size == 0 and eng.positions_density_geojson(8) == EMPTY
    finally:
        eng.close()


def test_one_hot_cell():
    recs = dc.hot_cell()
    eng = _engine(recs)
    try:
        got, info = _check(eng, recs, 0, dyadic=True, what="hot cell")
        assert got.size == 1 and int(got["count"][0]) == 50_000
        # each workgroup adds the one cell to the global table once: the pre-aggregation works
        assert 0 < info["global_adds"] <= info["workgroups"], info
        got, info = _check(eng, recs, 15, dyadic=True, what="hot cell")
        assert got.size > 40_000 and info["global_adds"] > RU_FILL, info   # the spill regime, far beyond the LDS table
    finally:
        eng.close()


def test_exact_path_and_cell_zero():
    from mobheat import _lib
    recs = dc.edges()
    eng = _engine(recs)
    try:
        for res in (9, 5, 0):
            _, info = _check(eng, recs, res, what="edges")
            _, fb = _lib.latlng_to_cell_fast_host_selftest(recs["lat"], recs["lon"], res)
            assert info["exact_keys"] == int(fb.sum()) > 0 and info["unsnapped"] == 7
    finally:
        eng.close()
    recs, at = dc.with_bad()
    eng = _engine(recs)
    try:
        for res in (8, 3):
            got, info = _check(eng, recs, res, what="with bad")
            assert info["unsnapped"] == 4
            dc.check(got, dc.expected(np.delete(recs, at), res)[0], what="the rest unchanged")
    finally:
        eng.close()


def test_since_edges_ties_and_negatives():
    recs, since = dc.since_edges()
    eng = _engine(recs)
    try:
        for res in (8, 15, 0):
            for s in (since - 1, since, since + 1, since + 2, None):
                _check(eng, recs, res, s, what="since edges")
        assert eng.positions_density(8, since + 2).size == 0
        assert eng.positions_density_geojson(8, since + 2) == EMPTY
    finally:
        eng.close()
    recs = dc.ts_extremes()
    eng = _engine(recs)
    try:
        got, _ = _check(eng, recs, 8, what="INT64_MIN")
        assert sorted(got["window_start_us"].tolist()) == [dc.INT64_MIN, -3, dc.INT64_MAX]
        got, info = _check(eng, recs, 8, dc.INT64_MAX, what="INT64_MAX")
        assert got.size == 1 and int(got["count"][0]) == 2 and info["kept"] == 2
        _check(eng, recs, 8, dc.INT64_MIN, what="explicit INT64_MIN")
        _check(eng, recs, 8, -3, what="since -3")
        _check(eng, recs, 0, what="one res-0 cell")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def sphere_engine():
    rng = np.random.default_rng(77)
    la, lo = dc.sphere(rng, 20_000)
    b = dc.boston(50)   # (so that the Boston view meets something)
    recs = dc.records(np.r_[la, 90.0, -90.0, b["lat"]], np.r_[lo, 0.0, 0.0, b["lon"]], dc.T0 + rng.integers(0, 900, la.size + 52) * dc.SEC)
    eng = _engine(recs)
    yield eng, recs
    eng.close()


VIEWS = [vc.BOSTON, (170.0, -60.0, -170.0, 60.0), (-180.0, 90.0, 180.0, 90.0), (-180.0, -90.0, 180.0, -90.0)]


@pytest.mark.parametrize("view", VIEWS)
def test_view(sphere_engine, view):
    eng, recs = sphere_engine
    want, _ = dc.expected(recs, 3)
    kept = dc.in_view(want, 3, view)
    assert 0 < kept.size < want.size
    got = eng.positions_density(3, None, view)
    info = eng.positions_density_info()
    dc.check(got, kept, what=f"view {view}")
    assert info["groups"] == want.size and info["returned"] == kept.size
    dc.check(eng.positions_density(3, None, vc.WORLD), want, what="the whole world")


def test_view_errors_and_nothing_in_view():
    from mobheat import _lib
    recs = dc.boston(2000)
    eng = _engine(recs)
    try:
        before = eng.positions_density_info()
        for v in vc.INVALID_VIEWS:
            assert _code(lambda: eng.positions_density(8, None, v)) == _lib.HM_E_INVALID, v
        assert eng.positions_density_info() == before   # nothing touched
        assert eng.positions_density(8, None, vc.ATHENS).size == 0
        info = eng.positions_density_info()
        assert info["returned"] == 0 and info["groups"] == dc.expected(recs, 8)[0].size
        assert eng.positions_density_geojson(8, view=vc.ATHENS) == EMPTY and len(EMPTY) == 42
    finally:
        eng.close()


def test_geojson_body_is_the_collection():
    import datetime as dt

    from mobheat import readside
    recs = dc.boston(5000)
    eng = _engine(recs)
    tz = dt.timezone(dt.timedelta(hours=-4))
    since, as_of = dc.T0 + 50 * dc.SEC, dc.T0 + 200 * dc.SEC
    try:
        for view in (None, vc.BOSTON):
            body, brecs, offs = eng.positions_density_geojson(8, since, tz, as_of, with_records=True, view=view)
            other = json.loads(readside.positions_density_body(eng, 8, since, tz, as_of, view=view))   # (another call: another order)
            fc = readside.positions_density_from_engine(eng, 8, since, tz, as_of, view=view)
            want, _ = dc.expected(recs, 8, since)
            if view is not None:
                want = dc.in_view(want, 8, view)
                assert 0 < want.size < dc.expected(recs, 8, since)[0].size
            dc.check(brecs, want, what=f"body records, view {view}")
            # the specification in the body's feature order
            by = {int(f["properties"]["cellId"], 16): f for f in fc["features"]}
            assert len(by) == len(fc["features"]) == brecs.size
            ordered = {"type": "FeatureCollection", "features": [by[int(c)] for c in brecs["cell"]]}
            assert bytes(body) == json.dumps(ordered, separators=(",", ":")).encode()
            by_cell = lambda c: sorted((f["properties"]["cellId"], f["properties"]["count"], json.dumps(f["geometry"])) for f in c["features"])
            assert by_cell(other) == by_cell(ordered)
            assert int(offs[0]) == 40 and len(offs) == brecs.size + 1
            p = ordered["features"][0]["properties"]
            assert p["windowStart"] == "2025-10-04T06:00:50" and p["windowEnd"] == "2025-10-04T06:03:20" and p["avgSpeedKmh"] == 0.0
        # no texts: empty strings
        body, brecs, _ = eng.positions_density_geojson(8, with_records=True)
        fc = readside.positions_density_from_engine(eng, 8)
        by = {int(f["properties"]["cellId"], 16): f for f in fc["features"]}
        ordered = {"type": "FeatureCollection", "features": [by[int(c)] for c in brecs["cell"]]}
        assert bytes(body) == json.dumps(ordered, separators=(",", ":")).encode() and b'"windowStart":""' in bytes(body)
    finally:
        eng.close()


def _grids():
    from mobheat import readside
    world = (np.linspace(89.5, -89.5, 90), np.linspace(-179.0, 179.0, 180))
    tile = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12))
    return {"world": world, "boston tile": tile, "1 x 65": (tile[0][:1], tile[1][:65]), "65 x 1": (tile[0][:65], tile[1][:1])}


@pytest.mark.parametrize("res", [8, 2])
def test_raster(res):
    from mobheat import _lib, readside
    rng = np.random.default_rng(31)
    la, lo = dc.sphere(rng, 5000)
    b = dc.boston(5000)
    recs = dc.records(np.r_[b["lat"], la], np.r_[b["lon"], lo], dc.T0 + rng.integers(0, 900, 10_000) * dc.SEC)
    since = dc.T0 + 300 * dc.SEC
    eng = _engine(recs)
    thr = readside.COUNT_THRESHOLDS
    try:
        dens = eng.positions_density(res, since)
        for name, (lat, lon) in _grids().items():
            counts, classes = eng.positions_density_raster(lat, lon, res, since, thr)
            info = eng.raster_info()
            assert info["pixels"] == counts.size and info["records"] == dens.size
            hc, hk = _lib.window_raster_selftest(dens, res, lat, lon, thr)
            np.testing.assert_array_equal(counts, hc, err_msg=name)
            np.testing.assert_array_equal(classes, hk, err_msg=name)
            ec, ek = rc.expected(dc.expected(recs, res, since)[0], res, lat, lon, thr)
            np.testing.assert_array_equal(counts, ec, err_msg=name)
            np.testing.assert_array_equal(classes, ek, err_msg=name)
            np.testing.assert_array_equal(eng.positions_density_raster(lat, lon, res, since), counts)
            if name == "boston tile" or (name == "world" and res == 2):   # (a 2-degree pixel rarely hits an occupied res-8 cell)
                assert counts.any(), name
        if res == 8:
            tx, ty = rc.tile_of(42.33, -71.07, 12)
            png = readside.positions_density_png(eng, 12, tx, ty, res=8, since_us=since)
            lat, lon = _grids()["boston tile"]
            _, hk = _lib.window_raster_selftest(dens, 8, lat, lon, thr)
            assert png == readside.png_from_classes(hk) and hk.any()
        assert not eng.positions_density_raster(*_grids()["world"], res, dc.INT64_MAX).any()   # nothing kept: zeros
        assert eng.positions_density_raster(np.zeros(0), np.zeros(4), res).shape == (0, 4)
        assert _code(lambda: eng.positions_density_raster(np.zeros(16385), np.zeros(1), res)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.positions_density_raster(np.zeros(2), np.zeros(2), res, None, (5, 2))) == _lib.HM_E_INVALID
    finally:
        eng.close()


def test_reads_only_and_allocates_nothing_twice():
    """density, density + view, the raster and the body leave the positions state, state_version and a live window's
    raster (the roll-up's table is not the density's) as they were; a repeated call of the same size allocates nothing"""
    from mobheat import readside, synth
    eng = _engine()
    try:
        b = synth.c1_boston(n=4000)
        eng.process_batch(0, **b)
        recs = dc.boston(3000)
        dc.load(eng, recs)
        lat, lon = _grids()["boston tile"]
        ws = eng.live_windows()[0].tolist()[-1]
        raster0 = eng.window_raster(lat, lon, ws, 8, readside.COUNT_THRESHOLDS)
        assert raster0[0].any()
        pos0, version = eng.positions()[0], eng.state_version()
        keep = []
        for _ in range(2):
            c0 = eng.last_counts()
            keep.append((np.sort(eng.positions_density(8), order="cell"), np.sort(eng.positions_density(8, None, vc.BOSTON), order="cell"),
                         eng.positions_density_raster(lat, lon, 8, None, readside.COUNT_THRESHOLDS),
                         len(eng.positions_density_geojson(8, view=vc.BOSTON))))
            c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        for f in ("cell", "count", "window_start_us"):
            np.testing.assert_array_equal(keep[0][0][f], keep[1][0][f])
            np.testing.assert_array_equal(keep[0][1][f], keep[1][1][f])
        np.testing.assert_array_equal(keep[0][2][0], keep[1][2][0])
        assert keep[0][3] == keep[1][3] > 42
        pos1 = eng.positions()[0]
        assert np.sort(pos0, order="vehicle").tobytes() == np.sort(pos1, order="vehicle").tobytes()
        assert eng.state_version() == version
        raster1 = eng.window_raster(lat, lon, ws, 8, readside.COUNT_THRESHOLDS)
        np.testing.assert_array_equal(raster0[0], raster1[0])
        np.testing.assert_array_equal(raster0[1], raster1[1])
        dc.check(eng.positions_density(8), dc.expected(recs, 8)[0], what="after the window raster")
    finally:
        eng.close()


def test_growth_across_folds():
    """two process_batch + update_positions rounds, the second moving half the vehicles to other cells and adding new
    ones: after each the density equals the oracle on positions()"""
    from positions_ref import Batch, run
    rng = np.random.default_rng(12)
    eng = _engine()
    try:
        n = 3000
        la, lo = rng.uniform(42.20, 42.45, n), rng.uniform(-71.20, -70.95, n)
        run(eng, 0, Batch([("p", f"v{k}", dc.T0 + k % 60 * dc.SEC, la[k], lo[k]) for k in range(n)]))
        cap0 = eng.positions_info()["capacity"]
        for res in (8, 4):
            dc.check(eng.positions_density(res), dc.expected(eng.positions()[0], res)[0], what="round 1")
        la2, lo2 = rng.uniform(42.20, 42.45, 2 * n), rng.uniform(-71.20, -70.95, 2 * n)
        rows = [("p", f"v{k}", dc.T0 + (100 + k % 60) * dc.SEC, la2[k], lo2[k]) for k in range(0, n, 2)]
        rows += [("p", f"v{k}", dc.T0 + (100 + k % 60) * dc.SEC, la2[k], lo2[k]) for k in range(n, 2 * n)]
        run(eng, 1, Batch(rows))
        pos = eng.positions()[0]
        assert pos.size == 2 * n and eng.positions_info()["capacity"] > cap0
        for res in (8, 4):
            got = eng.positions_density(res)
            dc.check(got, dc.expected(pos, res)[0], what="round 2")
            assert int(got["count"].sum()) == 2 * n
        moved = dc.expected(pos, 8, dc.T0 + 100 * dc.SEC)[0]
        dc.check(eng.positions_density(8, dc.T0 + 100 * dc.SEC), moved, what="round 2, the moved and the new")
        assert int(moved["count"].sum()) == n // 2 + n
    finally:
        eng.close()


def test_contract():
    from mobheat import _lib
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, HmBatchIn
    from mobheat import synth
    recs = dc.boston(500)
    eng = _engine(recs)
    try:
        assert _code(lambda: eng.positions_density(-1)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.positions_density(16)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.positions_density_raster(np.zeros(2), np.zeros(2), 16)) == _lib.HM_E_INVALID
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        rc_ = eng._lib.hm_positions_density(eng._ctx, 8, 0, None, 7, ctypes.byref(p), ctypes.byref(n))
        assert rc_ == _lib.HM_E_INVALID
        assert eng.positions_density(15).size == dc.expected(recs, 15)[0].size > 490   # res 15: a cell per vehicle
        # device records feed the tile encoder on the same context
        pd, nd = eng._density_device(8, None, None, _lib.HM_MEM_DEVICE)
        back = np.zeros(nd, _lib.STATE_REC_DTYPE)
        _lib.check(eng._lib.hm_memcpy(back.ctypes.data, pd, back.nbytes, 1), None, "hm_memcpy")
        dc.check(back, dc.expected(recs, 8)[0], what="device records")
        # between stage calls (a world of one, left after its ingest)
        k = {kk: np.ascontiguousarray(v) for kk, v in synth.c1_boston(n=2000).items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(eng._lib.hm_stage_ingest(eng._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), eng._ctx, "hm_stage_ingest")
        assert _code(lambda: eng.positions_density(8)) == _lib.HM_E_STATE
        assert _code(lambda: eng.positions_density_raster(np.zeros(2), np.zeros(2), 8)) == _lib.HM_E_STATE
        assert _code(lambda: eng.positions_density(16)) == _lib.HM_E_INVALID   # the argument errors come first
    finally:
        eng.close()
    shard = _engine(shard=(0, 2))
    try:
        assert _code(lambda: shard.positions_density(8)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.positions_density_raster(np.zeros(2), np.zeros(2), 8)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.positions_density_geojson(8)) == _lib.HM_E_UNSUPPORTED
    finally:
        shard.close()
