"""GPU: top-k hotspots (hm_top_records, hm_window_top, hm_window_geojson_top, hm_positions_density_top; csrc/k_top.h).
Device == host execution (hm_selftest_top_records) == numpy (readside.top_of) == Python's sorted (tests/top_cases.py) on
every case, whole records bit for bit, no tolerance; the window, GeoJSON and density forms against window_records /
positions_density + readside.top_of; what hm_top_info must show per case; state preservation and the contract.
tests/test_top_host.py proves on the CPU that the cases are what they claim."""
import ctypes
import json

import numpy as np
import pytest

import density_cases as dc
import raster_cases as rc
import top_cases as tc
import view_cases as vc

pytestmark = pytest.mark.gpu
EMPTY = b'{"type":"FeatureCollection","features":[]}'
ANTIMERIDIAN = (170.0, -60.0, -170.0, 60.0)
CASES = tc.cases()


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _dumps(collection):
    return json.dumps(collection, separators=(",", ":")).encode()


@pytest.fixture(scope="module")
def engine():
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def window(oracle_h3):
    """an engine whose one live window holds tc.window_records_case (counts up to 2^32 + 2) and whose positions state
    holds 3000 vehicles in Boston and 3000 on the sphere, all at multiples of 1/1024 degree (the density's coordinate sums
    are then exact in any order of addition, so two calls give the same bytes)"""
    import mobheat
    recs = tc.window_records_case(oracle_h3)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    eng.import_state(tc.state_info(recs.size), recs)
    rng = np.random.default_rng(8)
    la, lo = dc.sphere(rng, 3000)
    b = dc.boston(3000)
    la, lo = np.round(np.r_[b["lat"], la] * 1024) / 1024, np.round(np.r_[b["lon"], lo] * 1024) / 1024
    dc.load(eng, dc.records(la, lo, dc.T0 + rng.integers(0, 900, 6000) * dc.SEC))
    assert eng.live_windows()[0].tolist() == [tc.WS]
    yield eng, recs
    eng.close()


def _check_info(case, k, info):
    n = case["recs"].size
    m = min(k, n)
    assert (info["candidates"], info["returned"]) == (n, m), (case["name"], k, info)
    if m:
        assert info["device_us"] > 0
    if case["distinct"]:
        assert info["index_passes"] == 0, (case["name"], k, info)
    if 0 < k < n:
        assert info["tied"] >= 1
        for name, want in case["expect"].items():
            if want == "0":
                assert info[name] == 0, (case["name"], k, name, info)
            elif want == ">0":
                assert info[name] > 0, (case["name"], k, name, info)
            else:
                assert info[name] == want, (case["name"], k, name, info)
    else:   # nothing to select, or everything is taken: no pass
        assert info["count_passes"] == info["cell_passes"] == info["index_passes"] == 0


def _check_case(eng, case):
    from mobheat import _lib, readside
    recs = case["recs"]
    for k in case["ks"]:
        want = tc.ref_top(recs, k)
        got = eng.top_records(recs, k)
        info = eng.top_info()
        tc.same(got, want, f"{case['name']} k {k}: device against sorted")
        tc.same(_lib.top_records_selftest(recs, k), got, f"{case['name']} k {k}: host execution against the device")
        tc.same(readside.top_of(recs, k), got, f"{case['name']} k {k}: numpy against the device")
        _check_info(case, k, info)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_top_records(engine, case):
    _check_case(engine, case)


def test_every_workgroup_iterates_twice(monkeypatch):
    """a grid of tc.TEST_GRID workgroups: the keys, every pass and the compaction stride over the records several times"""
    import mobheat
    monkeypatch.setenv("MOBHEAT_TEST_TOP_GRID", str(tc.TEST_GRID))
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        for case in CASES:
            if case["recs"].size in (tc.SECOND_ITERATION, tc.TILE + 1, 257) or not case["distinct"]:
                _check_case(eng, case)
    finally:
        eng.close()


def test_k_limits_and_arguments(engine):
    from mobheat import _lib
    recs = CASES[5]["recs"]
    assert engine.top_info()["candidates"] >= 0
    assert _code(lambda: engine.top_records(recs, tc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.top_records(recs, -1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.window_top(tc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.window_top(-1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.window_top(5, res=9)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.window_geojson(top=tc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.positions_density(8, top=tc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: engine.positions_density(16, top=5)) == _lib.HM_E_INVALID
    for view in vc.INVALID_VIEWS[:3] + vc.INVALID_VIEWS[8:10]:
        assert _code(lambda: engine.window_top(5, view=view)) == _lib.HM_E_INVALID
        assert _code(lambda: engine.window_geojson(view=view, top=5)) == _lib.HM_E_INVALID
        assert _code(lambda: engine.positions_density(8, view=view, top=5)) == _lib.HM_E_INVALID
    p, n = ctypes.c_void_p(1), ctypes.c_int64(-7)
    rc_ = engine._lib.hm_top_records(engine._ctx, recs.ctypes.data, recs.size, 0, 3, 7, ctypes.byref(p), ctypes.byref(n))
    assert rc_ == _lib.HM_E_INVALID and n.value == -7 and p.value == 1   # nothing touched
    # device records in, device records out
    got = engine.top_records(recs, 3)
    rc_ = engine._lib.hm_top_records(engine._ctx, recs.ctypes.data, recs.size, 0, 3, _lib.HM_MEM_DEVICE, ctypes.byref(p), ctypes.byref(n))
    assert rc_ == 0 and n.value == 3
    back = np.zeros(3, _lib.STATE_REC_DTYPE)
    _lib.check(engine._lib.hm_memcpy(back.ctypes.data, p, back.nbytes, 1), None, "hm_memcpy")
    tc.same(back, got, "device output")


# ---- a live window ----
VIEWS = [None, vc.BOSTON, ANTIMERIDIAN]


@pytest.mark.parametrize("res", [8, 5])
def test_window_top(window, res):
    from mobheat import readside
    eng, recs = window
    for view in VIEWS:
        cand = eng.window_records(tc.WS, res)
        if res == 8:
            assert np.array_equal(np.sort(cand["cell"]), np.sort(recs["cell"])) and int(cand["count"].max()) >= 1 << 32
        if view is not None:
            cand = cand[readside.cells_in_view(cand["cell"], view, eng.device)]
            assert 0 < cand.size
        for k in (1, 7, 100, cand.size - 1, cand.size, cand.size + 1):
            got = eng.window_top(k, tc.WS, res, view)
            info = eng.top_info()
            tc.same(got, readside.top_of(cand, k), f"res {res} view {view} k {k}")
            tc.same(got, tc.ref_top(cand, k), f"res {res} view {view} k {k}: against sorted")
            assert (info["candidates"], info["returned"], info["index_passes"]) == (cand.size if k else 0, min(k, cand.size), 0)
        assert eng.window_top(0, tc.WS, res, view).size == 0
        tc.same(eng.window_top(9, None, res, view), readside.top_of(cand, 9), "the newest window by default")


@pytest.mark.parametrize("res", [8, 5])
def test_window_geojson_top(window, res):
    from mobheat import readside
    eng, _ = window
    for view in VIEWS:
        for k in (1, 50):
            body, brecs, offs = eng.window_geojson(tc.WS, res, with_records=True, view=view, top=k)
            want = readside.tiles_top_from_engine(eng, k, res, view=view)
            assert 0 < len(want["features"]) == brecs.size <= k
            assert bytes(body) == _dumps(want), f"res {res} view {view} k {k}"
            tc.same(brecs, eng.window_top(k, tc.WS, res, view), "with_records")
            assert int(offs[0]) == 40 and offs.size == brecs.size + 1
            assert readside.tiles_latest_body(eng, res, view=view, top=k) == bytes(body)
            counts = [f["properties"]["count"] for f in json.loads(bytes(body))["features"]]
            assert counts == sorted(counts, reverse=True)
    assert eng.window_geojson(tc.WS, res, top=0) == EMPTY
    assert eng.window_geojson(tc.WS, res, view=vc.ATHENS, top=5) == EMPTY


# ---- the positions density ----
@pytest.mark.parametrize("res", [8, 3])
def test_positions_density_top(window, res):
    from mobheat import _lib, readside
    eng, _ = window
    since = dc.T0 + 300 * dc.SEC
    for view in (None, vc.BOSTON):
        cand = eng.positions_density(res, since, view)
        assert cand.size > 0
        for k in (1, 20, cand.size, cand.size + 5):
            got = eng.positions_density(res, since, view, top=k)
            tc.same(got, readside.top_of(cand, k), f"density res {res} view {view} k {k}")
            assert eng.top_info()["index_passes"] == 0 and eng.positions_density_info()["returned"] == cand.size
        k = min(20, cand.size)
        body, brecs, offs = eng.positions_density_geojson(res, since, None, dc.T0 + 900 * dc.SEC, with_records=True, view=view, top=k)
        tc.same(brecs, readside.top_of(cand, k), "the body's records")
        want = readside.positions_density_from_engine(eng, res, since, None, dc.T0 + 900 * dc.SEC, view, top=k)
        assert bytes(body) == _dumps(want), f"density body res {res} view {view}"   # feature order included
        assert readside.positions_density_body(eng, res, since, None, dc.T0 + 900 * dc.SEC, view, top=k) == bytes(body)
        assert offs.size == k + 1
    late = dc.T0 + 10_000 * dc.SEC   # newer than every vehicle
    assert eng.positions_density(res, late, top=5).size == 0 and eng.positions_density(res, dc.INT64_MAX, top=5).size == 0
    assert eng.positions_density_geojson(res, late, top=5) == EMPTY
    # the ranked device records feed the tile encoder on the same context
    pd, nd = eng._density_device(res, since, None, _lib.HM_MEM_DEVICE, 10)
    back = np.zeros(nd, _lib.STATE_REC_DTYPE)
    _lib.check(eng._lib.hm_memcpy(back.ctypes.data, pd, back.nbytes, 1), None, "hm_memcpy")
    tc.same(back, readside.top_of(eng.positions_density(res, since), 10), "device records")


def test_nothing_live():
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert eng.top_info() == dict.fromkeys(eng.top_info(), 0)   # all 0 before the first call
        assert eng.window_top(5).size == 0 and eng.window_geojson(top=5) == EMPTY and len(EMPTY) == 42
        assert eng.positions_density(8, top=5).size == 0 and eng.positions_density_geojson(8, top=5) == EMPTY
        assert eng.top_records(np.zeros(0, mobheat._lib.STATE_REC_DTYPE), 5).size == 0
        recs = tc.records([1, 2, 3], tc.cells_of(3))
        eng.import_state(tc.state_info(3), recs)
        assert eng.window_top(5).size == 3
        assert eng.window_top(5, tc.WS + 5 * tc.MINUTE).size == 0                      # a window that is not live
        assert eng.window_geojson(tc.WS + 5 * tc.MINUTE, top=5) == EMPTY
        assert eng.top_info()["candidates"] == 0
    finally:
        eng.close()


def test_reads_only_and_allocates_nothing_twice(window):
    """the top calls leave state_version, the window's records, the positions state and the roll-up's table (window_raster)
    as they were; a repeated call of the same size allocates nothing"""
    from mobheat import readside
    eng, _ = window
    lat, lon = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12))
    version, pos0 = eng.state_version(), eng.positions()[0]
    win0 = np.sort(eng.window_records(tc.WS, 8), order="cell")
    raster0 = eng.window_raster(lat, lon, tc.WS, 8)
    assert raster0.any()
    recs = CASES[8]["recs"]
    keep = []
    for _ in range(2):
        c0 = eng.last_counts()
        keep.append((eng.top_records(recs, 100).tobytes(), eng.window_top(100, tc.WS, 5, vc.BOSTON).tobytes(),
                     eng.window_top(100, tc.WS, 8).tobytes(), bytes(eng.window_geojson(tc.WS, 8, view=vc.BOSTON, top=100)),
                     eng.positions_density(8, top=100).tobytes(), bytes(eng.positions_density_geojson(8, view=vc.BOSTON, top=100))))
        c1 = eng.last_counts()
    assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
    assert keep[0] == keep[1]   # the response bytes do not differ from call to call
    assert eng.state_version() == version
    assert np.sort(eng.window_records(tc.WS, 8), order="cell").tobytes() == win0.tobytes()
    assert np.sort(eng.positions()[0], order="vehicle").tobytes() == np.sort(pos0, order="vehicle").tobytes()
    # the raster directly after a density top answers from the roll-up's table
    eng.window_top(10, tc.WS, 8)
    eng.positions_density(8, top=10)
    np.testing.assert_array_equal(eng.window_raster(lat, lon, tc.WS, 8), raster0)
    eng.window_records(tc.WS, 8)
    eng.positions_density(3, top=10)
    assert np.array_equal(eng.window_raster(lat, lon, tc.WS, 8), raster0)


def test_contract():
    import mobheat
    from mobheat import _lib, synth
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, HmBatchIn
    recs = CASES[5]["recs"]
    shard = mobheat.HeatmapEngine(h3_res=8, device=0, shard=(0, 2))
    try:
        assert _code(lambda: shard.window_top(5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_geojson(top=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.positions_density(8, top=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_top(tc.TOP_MAX + 1)) == _lib.HM_E_INVALID   # the argument errors come first
        tc.same(shard.top_records(recs, 9), tc.ref_top(recs, 9), "top_records on a shard context")
    finally:
        shard.close()
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        # between stage calls (a world of one, left after its ingest)
        k = {kk: np.ascontiguousarray(v) for kk, v in synth.c1_boston(n=2000).items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(eng._lib.hm_stage_ingest(eng._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), eng._ctx, "hm_stage_ingest")
        assert _code(lambda: eng.top_records(recs, 5)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_top(5)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_geojson(top=5)) == _lib.HM_E_STATE
        assert _code(lambda: eng.positions_density(8, top=5)) == _lib.HM_E_STATE
        assert _code(lambda: eng.top_records(recs, -1)) == _lib.HM_E_INVALID
    finally:
        eng.close()
