"""GPU: the read side for a map viewport (csrc/k_view.h, csrc/api_view.h) -- the device's verdicts against the host
execution of the same code (which tests/test_view_host.py ties to the rule), and the two filtered GeoJSON bodies against
json.dumps of what Python keeps by the tests' own statement of the rule (tests/view_cases.py).  No tolerance anywhere."""
import ctypes
import json
import math

import numpy as np
import pytest

import geojson_cases as gc
import view_cases as vc
from positions_ref import Batch, run

pytestmark = pytest.mark.gpu
MINUTE = 60_000_000
EMPTY = b'{"type":"FeatureCollection","features":[]}'


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


# ---- hm_cells_in_view ----
@pytest.fixture(scope="module")
def cs():
    return vc.case_set()


def test_cells_in_view_device_equals_host_on_every_case(cs):
    from mobheat import _lib, readside
    for i, v in enumerate(cs.views):
        got = vc.device_cells_in_view(cs.cells, v, _lib.HM_MEM_HOST)
        np.testing.assert_array_equal(got, _lib.cells_in_view_selftest(cs.cells, v), err_msg=str(v))
        np.testing.assert_array_equal(got, cs.expect[i], err_msg=str(v))
    np.testing.assert_array_equal(readside.cells_in_view(cs.cells, vc.BOSTON), cs.expect[cs.views.index(vc.BOSTON)].astype(bool))
    with pytest.raises(ValueError):
        readside.cells_in_view(cs.cells, vc.INVALID_VIEWS[0])


def _patterns(kept, dropped, n):
    """the five keep patterns over n cells, built by ordering kept / dropped cells of one view"""
    k, d = np.resize(kept, max(n, 1)), np.resize(dropped, max(n, 1))
    alt = np.where(np.arange(max(n, 1)) % 2 == 0, k, d)
    first, last = d.copy(), d.copy()
    first[0], last[-1] = kept[0], kept[-1]
    return {"all": k[:n], "none": d[:n], "first": first[:n], "last": last[:n], "alternating": alt[:n]}


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70_001])   # on and around one compaction block, past one scan block
def test_cells_in_view_sizes_and_patterns(cs, n):
    from mobheat import _lib
    view = vc.BOSTON
    host = _lib.cells_in_view_selftest(cs.cells, view)   # the host execution, once per distinct cell
    verdict = dict(zip(cs.cells.tolist(), host.tolist()))
    kept, dropped = cs.cells[host == 1], cs.cells[host == 0]
    assert kept.size > 3 and dropped.size > 3
    for name, cells in _patterns(kept, dropped, n).items():
        want = np.array([verdict[c] for c in cells.tolist()], np.uint8)
        if n:
            assert {"all": want.all(), "none": not want.any(), "first": want[0] == 1 and want[1:].sum() == 0,
                    "last": want[-1] == 1 and want[:-1].sum() == 0,
                    "alternating": (want[::2] == 1).all() and (want[1::2] == 0).all()}[name], name
        for memory in (_lib.HM_MEM_HOST, _lib.HM_MEM_DEVICE):
            got = vc.device_cells_in_view(cells, view, memory)
            np.testing.assert_array_equal(got, want, err_msg=f"n {n} pattern {name} memory {memory}")


# ---- window_geojson(view=...) ----
def _boston(seed, shift_us):
    from mobheat import synth
    b = synth.c1_boston(seed=seed, n=20_000)
    b["ts_us"] = b["ts_us"] + shift_us
    return b


def _window_collection(eng, recs, ws):
    from mobheat import readside
    from mobheat.stream import _spark_datetime
    on_gpu = readside.cells_to_boundary
    return gc.tile_collection(recs, _spark_datetime(ws).isoformat(), _spark_datetime(ws + eng.tile_us).isoformat(),
                              lambda cells: on_gpu(cells, eng.device))


def _ref_filter(recs, res, view):
    """the records the tests' rule keeps: boundaries from the host execution, the pole cells from the oracle"""
    from mobheat import _lib
    from oracle import h3_oracle
    north, south = (int(c) for c in h3_oracle.latlng_to_cell(np.array([90.0, -90.0]), np.array([0.0, 0.0]), res))
    la, lo, nv = _lib.cells_to_boundary_host_selftest(recs["cell"])
    keep = [vc.ref_ring(la[k, :nv[k]].tolist(), lo[k, :nv[k]].tolist(), view,
                        1 if int(recs["cell"][k]) == north else -1 if int(recs["cell"][k]) == south else 0)
            for k in range(recs.size)]
    return recs[np.array(keep, bool)]


def _features(body, offs):
    body = bytes(body)
    return sorted(body[offs[i]: offs[i + 1] - 1] for i in range(len(offs) - 1))


@pytest.fixture(scope="module")
def engine():
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    eng.process_batch(0, **_boston(0, 0))
    eng.process_batch(1, **_boston(1, 0))   # (C1's 60 s straddle 10:25: two windows)
    yield eng
    eng.close()


@pytest.mark.parametrize("res", [8, 5, 0])
def test_window_geojson_view(engine, res):
    """[Boston view, res 8]: the data box is 0.25 x 0.25 degrees (~780 occupied res-8 cells) and the view a sixth of it, so
    0 < kept < candidates by construction; one res-0 cell covers the whole city, so res 5 and 0 only ask for kept >= 1"""
    eng = engine
    wins = eng.live_windows()[0].tolist()
    assert len(wins) == 2
    version = eng.state_version()
    for ws in wins:
        cand = eng.window_records(ws, res)
        body, recs, offs = eng.window_geojson(ws, res, with_records=True, view=vc.BOSTON)
        info = eng.geojson_info()
        assert info["candidates"] == cand.size and info["view_kernel_us"] > 0 and info["body_bytes"] == len(body)
        gc.check_body(body, offs, _window_collection(eng, recs, ws))
        want = _ref_filter(cand, res, vc.BOSTON)
        key = lambda r: sorted(zip(r["cell"].tolist(), r["count"].tolist(), r["n_speed"].tolist()))   # (two roll-ups: the sums' order of addition may differ)
        assert key(recs) == key(want)
        if res == 8:
            assert 0 < recs.size < cand.size
        assert recs.size >= 1
        assert eng.window_geojson(ws, res, view=vc.ATHENS) == EMPTY
        assert eng.geojson_info()["candidates"] == cand.size
        # the whole world keeps every candidate: the unfiltered body's features
        wbody, wrecs, woffs = eng.window_geojson(ws, res, with_records=True, view=vc.WORLD)
        gc.check_body(wbody, woffs, _window_collection(eng, wrecs, ws))
        assert wrecs.size == cand.size and key(wrecs) == key(cand)
    assert eng.state_version() == version


def test_window_geojson_view_none_is_todays_call(engine):
    """view=None takes hm_window_geojson: the same bytes as the call without the keyword.  Each call rolls the window up
    again -- its records come in the order that call's compaction gave them, their speed sums in that call's order of
    addition -- so the bytes are compared where the two calls' records are the same bytes, and both bodies are held to
    their own records, which are the same set, in every case."""
    from mobheat import readside
    eng = engine
    ws = eng.live_windows()[0].tolist()[-1]
    for res in (8, 5):
        a, ra, oa = eng.window_geojson(ws, res, with_records=True, view=None)
        info = eng.geojson_info()
        b, rb, ob = eng.window_geojson(ws, res, with_records=True)
        gc.check_body(a, oa, _window_collection(eng, ra, ws))
        gc.check_body(b, ob, _window_collection(eng, rb, ws))
        assert sorted(zip(ra["cell"].tolist(), ra["count"].tolist())) == sorted(zip(rb["cell"].tolist(), rb["count"].tolist()))
        if ra.tobytes() == rb.tobytes():
            assert a == b
        elif np.array_equal(np.sort(ra), np.sort(rb)):
            assert _features(a, oa) == _features(b, ob)
        assert info["body_bytes"] == len(a)
    # readside's two forms agree under a view, feature order apart
    fc = json.loads(readside.tiles_latest_body(eng, res=8, view=vc.BOSTON))
    ref = readside.tiles_latest_from_engine(eng, res=8, view=vc.BOSTON)
    by_cell = lambda c: sorted((f["properties"]["cellId"], f["properties"]["count"], f["properties"]["windowStart"],
                                gc.dumps(f["geometry"])) for f in c["features"])
    assert by_cell(fc) == by_cell(ref) and 0 < len(ref["features"]) < eng.window_records(None, 8).size


def test_window_geojson_view_edges():
    """a window that is not live, no window at all, a repeated call, an invalid view, between stage calls"""
    import mobheat
    from mobheat import _lib
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, HmBatchIn
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert eng.window_geojson(view=vc.BOSTON) == EMPTY   # no window at all
        eng.process_batch(0, **_boston(0, 0))
        wins = eng.live_windows()[0].tolist()
        version = eng.state_version()
        assert eng.window_geojson(wins[0] - 5 * MINUTE, 5, view=vc.BOSTON) == EMPTY
        assert eng.geojson_info()["candidates"] == 0
        assert _code(lambda: eng.window_geojson(wins[0], 9, view=vc.BOSTON)) == _lib.HM_E_INVALID
        eng.window_geojson(wins[-1], 8, view=vc.BOSTON)
        c0 = eng.last_counts()
        first = eng.window_geojson(wins[-1], 8, copy=False, view=vc.BOSTON)
        assert isinstance(first, memoryview) and len(first) > 1000
        c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        for v in vc.INVALID_VIEWS:
            assert _code(lambda: eng.window_geojson(wins[-1], 8, view=v)) == _lib.HM_E_INVALID, v
            assert _code(lambda: eng.positions_geojson(view=v)) == _lib.HM_E_INVALID, v
        assert len(eng.window_geojson(wins[-1], 8, view=vc.BOSTON)) == len(first)   # a working engine afterwards
        assert eng.state_version() == version
        # between stage calls (a world of one, left after its ingest)
        bt = _boston(20, 12 * MINUTE)
        k = {kk: np.ascontiguousarray(v) for kk, v in bt.items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(eng._lib.hm_stage_ingest(eng._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), eng._ctx, "hm_stage_ingest")
        assert _code(lambda: eng.window_geojson(wins[-1], 8, view=vc.BOSTON)) == _lib.HM_E_STATE
        assert _code(lambda: eng.positions_geojson(view=vc.BOSTON)) == _lib.HM_E_STATE
    finally:
        eng.close()


# ---- positions_geojson(view=...) ----
POS_VIEW = vc.BOSTON
ANTI_VIEW = (170.0, -60.0, -170.0, 60.0)
NORTH_POLE_VIEW = (-180.0, 90.0, 180.0, 90.0)
SOUTH_POLE_VIEW = (-180.0, -90.0, 180.0, -90.0)


def _vehicle_rows():
    """a few hundred vehicles: on every edge of POS_VIEW, one ulp inside and outside it, the same around ANTI_VIEW's two
    longitude edges, lon 180.0 and -180.0, both poles, and a random cloud around Boston"""
    up, down = math.inf, -math.inf
    w, s, e, n = POS_VIEW
    mid_lat, mid_lon = 0.5 * (s + n), 0.5 * (w + e)
    pts = []
    for lat in (s, math.nextafter(s, up), math.nextafter(s, down), n, math.nextafter(n, down), math.nextafter(n, up)):
        pts += [(lat, mid_lon), (lat, w), (lat, e)]
    for lon in (w, math.nextafter(w, up), math.nextafter(w, down), e, math.nextafter(e, down), math.nextafter(e, up)):
        pts += [(mid_lat, lon), (s, lon), (n, lon)]
    aw, a_s, ae, an = ANTI_VIEW
    for lon in (aw, math.nextafter(aw, up), math.nextafter(aw, down), ae, math.nextafter(ae, down), math.nextafter(ae, up),
                180.0, -180.0, math.nextafter(180.0, down), math.nextafter(-180.0, up), 0.0, -0.0):
        pts += [(0.0, lon), (a_s, lon), (an, lon), (math.nextafter(an, up), lon)]
    pts += [(90.0, 0.0), (-90.0, 0.0), (90.0, 180.0), (-90.0, -180.0), (math.nextafter(90.0, down), 10.0), (math.nextafter(-90.0, up), 10.0)]
    rng = np.random.default_rng(31)
    pts += list(zip(rng.uniform(42.2, 42.5, 200).tolist(), rng.uniform(-71.3, -70.9, 200).tolist()))
    T0 = 1_759_572_000_000_000
    return [(f"prov{k % 3}", f"veh-{k:04d}", T0 + k * 1_000_000, la, lo) for k, (la, lo) in enumerate(pts)]


def test_positions_geojson_view():
    import mobheat
    from mobheat import readside
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert eng.positions_geojson(view=POS_VIEW) == EMPTY   # no state
        rows = _vehicle_rows()
        run(eng, 0, Batch(rows))
        version = eng.state_version()
        _, providers, vehicles = eng.positions()
        ref = readside.positions_latest_from_engine(eng)
        assert len(ref["features"]) == len(rows)
        by_key = {(f["properties"]["provider"], f["properties"]["vehicleId"]): f for f in ref["features"]}
        for view in (POS_VIEW, ANTI_VIEW, NORTH_POLE_VIEW, SOUTH_POLE_VIEW, vc.WORLD):
            body, recs, offs = eng.positions_geojson(with_records=True, view=view)
            info = eng.geojson_info()
            assert info["candidates"] == len(rows) and info["view_kernel_us"] > 0
            want = {k for k, f in by_key.items() if vc.ref_point(f["geometry"]["coordinates"][1], f["geometry"]["coordinates"][0], view)}
            got = [(providers[int(r["provider"])], vehicles[int(r["vehicle"])]) for r in recs]
            assert set(got) == want and len(got) == len(want), view
            gc.check_body(body, offs, {"type": "FeatureCollection", "features": [by_key[k] for k in got]})
            mine = readside.positions_latest_from_engine(eng, view=view)
            assert sorted(gc.dumps(f) for f in mine["features"]) == sorted(gc.dumps(by_key[k]) for k in got)
            if view != vc.WORLD:
                assert 0 < len(got) < len(rows), view
            else:
                assert len(got) == len(rows)
        # the antimeridian view keeps lon 180.0 and -180.0; the pole views keep exactly the vehicles at their pole
        body = json.loads(eng.positions_geojson(view=ANTI_VIEW))
        lons = {f["geometry"]["coordinates"][0] for f in body["features"]}
        assert 180.0 in lons and -180.0 in lons and 0.0 not in lons
        assert all(f["geometry"]["coordinates"][1] == 90.0 for f in json.loads(eng.positions_geojson(view=NORTH_POLE_VIEW))["features"])
        assert eng.positions_geojson(view=(10.0, 10.0, 11.0, 11.0)) == EMPTY   # a view with nobody in it
        assert json.loads(readside.positions_latest_body(eng, view=POS_VIEW))["features"]
        eng.positions_geojson(view=POS_VIEW)
        c0 = eng.last_counts()
        eng.positions_geojson(view=POS_VIEW)
        c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        assert eng.state_version() == version
    finally:
        eng.close()
