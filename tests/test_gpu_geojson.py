"""GPU: the read side's GeoJSON bodies encoded on the device (csrc/float_repr.h, csrc/geojson_docs.h, csrc/k_geojson.h)
against the host execution of the same encoders -- which tests/test_float_repr_host.py and tests/test_geojson_host.py tie
to repr() and json.dumps -- and against json.dumps of what mobheat/readside.py builds from the engine.  Bytes equal;
no tolerance anywhere."""
import ctypes
import json

import numpy as np
import pytest

import geojson_cases as gc
from positions_ref import Batch, run

pytestmark = pytest.mark.gpu
MINUTE = 60_000_000


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def test_float_repr_device_equals_host():
    """the constant-memory table and __umul64hi: the special set and 2^20 random bit patterns"""
    from mobheat import _lib
    rng = np.random.default_rng(20250609)
    x = np.concatenate([gc.special_doubles(), rng.integers(0, 1 << 64, size=1 << 20, dtype=np.uint64).view(np.float64)])
    ht, hl = _lib.float_repr_selftest(x)
    dt, dl = _lib.float_repr_selftest(x, device=0)
    np.testing.assert_array_equal(dl, hl)
    keep = np.arange(24)[None, :] < hl[:, None]
    np.testing.assert_array_equal(np.where(keep, dt, 0), np.where(keep, ht, 0))
    gc.check_float_texts(x[:20000], dt[:20000], dl[:20000])


@pytest.fixture(scope="module")
def tile_recs():
    from mobheat import _lib
    cells = gc.tile_cells(_lib.cells_to_boundary_host_selftest)
    return gc.tile_records(np.resize(cells, 70_001))


@pytest.fixture(scope="module")
def engine():
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    yield eng
    eng.close()


@pytest.mark.parametrize("n", [0, 1, 257, 70_001])   # past one workgroup (64), past one scan block (4096)
def test_encode_tile_features_equals_host(engine, tile_recs, n):
    from mobheat import _lib
    recs = tile_recs[:n]
    hb, ho = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    for memory in (_lib.HM_MEM_HOST, _lib.HM_MEM_DEVICE):
        body, offs = engine.encode_tile_features(recs, gc.WS_TEXT, gc.WE_TEXT, memory)
        np.testing.assert_array_equal(offs, ho)
        assert body == hb.tobytes(), f"n {n} memory {memory}"
    if n:
        info = engine.geojson_info()
        assert info["body_bytes"] == len(hb) and info["sizes_kernel_us"] > 0 and info["write_kernel_us"] > 0
    assert _code(lambda: engine.encode_tile_features(recs, 'a"b', gc.WE_TEXT)) == _lib.HM_E_INVALID


def _boston(seed, shift_us):
    from mobheat import synth
    b = synth.c1_boston(seed=seed, n=20_000)
    b["ts_us"] = b["ts_us"] + shift_us
    return b


def _window_collection(eng, recs, ws):
    from mobheat import readside
    from mobheat.stream import _spark_datetime
    on_gpu = readside.cells_to_boundary   # (bound now: tile_collection swaps the module's attribute while it runs)
    return gc.tile_collection(recs, _spark_datetime(ws).isoformat(), _spark_datetime(ws + eng.tile_us).isoformat(),
                              lambda cells: on_gpu(cells, eng.device))


def test_window_geojson():
    """two batches of 20,000 C1 events in two windows: both windows at h3_res, h3_res - 3 and 0, and a window that is not
    live; the body = json.dumps of the collection built in Python from the records the same call returned"""
    import mobheat
    from mobheat import _lib, readside
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert eng.window_geojson() == b'{"type":"FeatureCollection","features":[]}'   # no window at all
        eng.process_batch(0, **_boston(0, 0))
        eng.process_batch(1, **_boston(1, 0))   # (C1's 60 s straddle 10:25: the same two windows again)
        wins = eng.live_windows()[0].tolist()
        assert len(wins) == 2
        version = eng.state_version()
        for ws in wins:
            for res in (8, 5, 0):
                body, recs, offs = eng.window_geojson(ws, res, with_records=True)
                gc.check_body(body, offs, _window_collection(eng, recs, ws))
                want = eng.window_records(ws, res)
                assert sorted(zip(recs["cell"].tolist(), recs["count"].tolist())) == \
                    sorted(zip(want["cell"].tolist(), want["count"].tolist())) and recs.size > 0
        # the newest window by default = readside's comparison form, feature order apart
        fc = json.loads(readside.tiles_latest_body(eng, res=5))
        ref = readside.tiles_latest_from_engine(eng, res=5)
        by_cell = lambda c: sorted(c["features"], key=lambda f: f["properties"]["cellId"])
        got, exp = by_cell(fc), by_cell(ref)
        assert len(got) == len(exp) > 3
        for g, e in zip(got, exp):
            assert g["geometry"] == e["geometry"] and g["properties"]["count"] == e["properties"]["count"]
            assert g["properties"]["windowStart"] == e["properties"]["windowStart"]
        # a window that is not live
        assert eng.window_geojson(wins[0] - 5 * MINUTE, 5) == b'{"type":"FeatureCollection","features":[]}'
        assert _code(lambda: eng.window_geojson(wins[0], 9)) == _lib.HM_E_INVALID
        # a repeated call allocates nothing; the state's version is unchanged
        eng.window_geojson(wins[1], 5)
        c0 = eng.last_counts()
        first = eng.window_geojson(wins[1], 5, copy=False)
        assert isinstance(first, memoryview) and len(first) > 1000
        c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        assert eng.state_version() == version
    finally:
        eng.close()


def test_window_geojson_reads_only():
    """Two engines fed the same batches, one encoding every live window between the batches: the same tiles per batch
    and final state; an encode between hm_state_export_begin and the copy of its dump leaves the checkpoint's records as
    they were; between stage calls HM_E_STATE."""
    import mobheat
    from mobheat import _lib
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, STATE_REC_DTYPE, HmBatchIn
    a, b = mobheat.HeatmapEngine(h3_res=8, device=0), mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        for epoch in range(3):
            bt = _boston(10 + epoch, epoch * 4 * MINUTE)
            ra, rb = a.process_batch(epoch, **bt), b.process_batch(epoch, **bt)
            ta, tb = ra.tiles, rb.tiles
            oa, ob = np.lexsort((ta.window_start_us, ta.cell)), np.lexsort((tb.window_start_us, tb.cell))
            for f in ("cell", "window_start_us", "count", "speed_null"):
                np.testing.assert_array_equal(getattr(ta, f)[oa], getattr(tb, f)[ob], err_msg=f"epoch {epoch}: {f}")
            assert ra.n_state == rb.n_state
            v = a.state_version()
            for ws in a.live_windows()[0].tolist():
                for r in (8, 4):
                    assert len(a.window_geojson(ws, r)) > 100
            assert a.state_version() == v
        _, ea = a.export_state()
        _, eb = b.export_state()
        for f in ("cell", "window_start_us", "count", "n_speed"):
            np.testing.assert_array_equal(np.sort(ea, order=["cell", "window_start_us"])[f],
                                          np.sort(eb, order=["cell", "window_start_us"])[f])
        info, n, recs, raw, fill = a.export_begin(touched_only=False)
        assert n == ea.size
        ws = a.live_windows()[0]
        assert len(a.window_geojson(ws[0], 2)) > 100 and len(a.window_geojson(ws[-1], 8)) > 100
        sync = np.zeros(n, STATE_REC_DTYPE)
        _lib.check(a._lib.hm_state_export_copy(a._ctx, sync.ctypes.data, 0, n), a._ctx, "hm_state_export_copy")
        fill(0, n)
        np.testing.assert_array_equal(np.sort(sync), np.sort(ea))
        np.testing.assert_array_equal(np.sort(recs), np.sort(ea))
        # between stage calls (a world of one, left after its ingest)
        bt = _boston(20, 12 * MINUTE)
        k = {kk: np.ascontiguousarray(v) for kk, v in bt.items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(b._lib.hm_stage_ingest(b._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), b._ctx, "hm_stage_ingest")
        assert _code(lambda: b.window_geojson(int(ws[0]), 8)) == _lib.HM_E_STATE
        assert _code(lambda: b.encode_tile_features(ea[:3], gc.WS_TEXT, gc.WE_TEXT)) == _lib.HM_E_STATE
        assert _code(lambda: b.positions_geojson()) == _lib.HM_E_STATE
    finally:
        a.close()
        b.close()


def _position_batches():
    """three batches, 1,000 vehicles in all, the strings of the host test among them"""
    rng = np.random.default_rng(77)
    T0 = 1_759_572_000_000_000
    # (years 1900..2100 and finite coordinates here: the engine's row filter drops a NaN latitude, and
    # datetime.fromtimestamp, which builds the comparison form, refuses the very ends of years 1 and 9999 -- both are the
    # host test's ground)
    lo_us, hi_us = -2_208_988_800 * 1_000_000, 4_102_444_800 * 1_000_000
    special = [(p, v, min(max(ts, lo_us), hi_us), la if la == la else 12.5, lo) for p, v, ts, la, lo in gc.position_rows()]
    out = []
    for b in range(3):
        n = 600
        veh = (np.arange(n) + 300 * b) % (1000 - len(special))   # overlapping thirds: every vehicle, most of them twice
        rows = [(f"prov{int(v) % 3}", f"veh-{int(v):04d}", T0 + int(rng.integers(0, 3000)) * 1_000_000 + int(rng.integers(0, 2)) * 123_456,
                 float(rng.uniform(-80, 80)), float(rng.uniform(-170, 170))) for v in veh]
        if b == 2:   # (last: their year-2100 timestamp moves the watermark past everything else)
            rows += special
        out.append(Batch(rows))
    return out


def _check_positions(eng):
    from mobheat import readside
    before = eng.positions(strings=False)
    ts = before[0]["ts_us"]
    np.testing.assert_array_equal(eng.positions_buckets(), np.unique(ts // 1_000_000 // 900))
    body, recs, offs = eng.positions_geojson(with_records=True)
    _, providers, vehicles = eng.positions()
    # the collection readside builds, its features matched through the records the call returned
    ref = readside.positions_latest_from_engine(eng)
    key = lambda f: (f["properties"]["provider"], f["properties"]["vehicleId"])
    by_key = {key(f): f for f in ref["features"]}
    assert len(by_key) == len(ref["features"]) == recs.size
    ordered = [by_key[(providers[int(r["provider"])], vehicles[int(r["vehicle"])])] for r in recs]
    gc.check_body(body, offs, {"type": "FeatureCollection", "features": ordered})
    again = json.loads(readside.positions_latest_body(eng))["features"]   # (feature order may differ between calls)
    assert sorted(gc.dumps(f) for f in again) == sorted(gc.dumps(f) for f in ordered)
    after = eng.positions(strings=False)
    np.testing.assert_array_equal(np.sort(before[0]), np.sort(after[0]))
    for x, y in zip(before[1:], after[1:]):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2][:int(x[1][-1])], y[2][:int(y[1][-1])])
    return recs.size


def test_positions_geojson():
    import mobheat
    from mobheat import _lib
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert eng.positions_buckets().size == 0                                   # a state with 0 vehicles
        assert eng.positions_geojson() == b'{"type":"FeatureCollection","features":[]}'
        run(eng, 0, Batch([("p", "only", 1_759_572_000_000_001, 42.0, -71.0)]))      # and with 1
        assert _check_positions(eng) == 1
        assert eng.positions_geojson() == (b'{"type":"FeatureCollection","features":[{"type":"Feature","geometry":{"type":"Point",'
                                           b'"coordinates":[-71.0,42.0]},"properties":{"provider":"p","vehicleId":"only",'
                                           b'"ts":"2025-10-04T10:00:00.000001"}}]}')
        for e, b in enumerate(_position_batches()):
            run(eng, 1 + e, b)
        version = eng.state_version()
        n = _check_positions(eng)
        assert n == 1001   # 951 plain vehicles, the 49 string pairs, the first one
        # a bucket missing from the caller's table fails the call
        ids = eng.positions_buckets()
        cfg, keep = _lib.bucket_cfg(ids[1:])
        pb, po, cnt = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        assert eng._lib.hm_positions_geojson(eng._ctx, ctypes.byref(cfg), _lib.HM_MEM_HOST, ctypes.byref(pb), ctypes.byref(po),
                                             ctypes.byref(cnt), None) == _lib.HM_E_INVALID
        c0 = eng.last_counts()
        eng.positions_geojson()
        c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        assert eng.state_version() == version
    finally:
        eng.close()
