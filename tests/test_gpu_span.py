"""GPU: a trailing span of live windows as one heatmap with per-window counts (hm_span_rollup, hm_span_geojson,
hm_span_raster; csrc/k_span.h).  The reference of every test is the engine's own per-window window_records at H3_RES
fed to readside.span_of, which tests/test_span_host.py checks against a plain dict loop; the inputs are dyadic
(tests/span_cases.py), so "equal" is bit-equal, but for the one uniform-random input, whose sums are held to
tests/test_gpu_rollup.py's closeness of averages."""
import ctypes
import json

import numpy as np
import pytest

import span_cases as sc

pytestmark = pytest.mark.gpu
KNOB = "MOBHEAT_TEST_READ_GRID"
W0 = sc.wstart(0)


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _engine(batch=None, grid=None, **kw):
    import mobheat
    with pytest.MonkeyPatch.context() as mp:
        if grid is None:
            mp.delenv(KNOB, raising=False)
        else:
            mp.setenv(KNOB, str(grid))
        eng = mobheat.HeatmapEngine(h3_res=sc.H3_RES, device=0, watermark_delay_ms=sc.DELAY_MS, **kw)
    if batch is not None:
        eng.process_batch(0, **batch)
    return eng


@pytest.fixture(scope="module")
def three():
    """an engine holding the membership batch: windows 0, 1, 2 live, every cell in a random non-empty subset of them"""
    eng = _engine(sc.membership_batch()[0])
    assert eng.live_windows()[0].tolist() == [sc.wstart(j) for j in (0, 1, 2)]
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def sparse():
    """an engine whose live windows are 3, 5 and 18"""
    eng = _engine(sc.sparse_batch()[0])
    assert eng.live_windows()[0].tolist() == [sc.wstart(j) for j in sc.SPARSE]
    yield eng
    eng.close()


def _want(eng, end_j, windows, res):
    """the span by readside.span_of from the engine's per-window records at H3_RES (a window that is not live: none)"""
    from mobheat import readside
    first_j = end_j - windows + 1
    per = [eng.window_records(sc.wstart(j), sc.H3_RES) for j in range(first_j, end_j + 1)]
    return readside.span_of(per, sc.wstart(first_j), sc.TILE, res), per


def _check(eng, end_j, windows, res, what):
    """the unranked, unviewed call against the reference; returns (records sorted by cell, series)"""
    want, per = _want(eng, end_j, windows, res)
    got = eng.window_span(sc.wstart(end_j), windows, res)
    assert np.unique(got[0]["cell"]).size == got[0].size, f"{what}: a cell appears twice"
    sc.same(sc.by_cell(*got), want, f"{what}: device against span_of")
    info = eng.span_info()
    live = [r for r in per if r.size]
    assert (info["live_windows"], info["keys"], info["parents"], info["in_view"], info["returned"]) == \
        (len(live), sum(r.size for r in live), want[0].size, want[0].size, want[0].size), (what, info)
    if live:
        assert info["table_slots"] >= 2 * want[0].size and info["device_us"] > 0
    return want


@pytest.mark.parametrize("res", [sc.H3_RES, 5, 0])
def test_one_window_is_the_roll_up(three, res):
    for j in (0, 1, 2):
        recs, series = sc.by_cell(*three.window_span(sc.wstart(j), 1, res))
        roll = three.window_records(sc.wstart(j), res)
        assert recs.tobytes() == np.sort(roll, order="cell").tobytes(), f"window {j} res {res}"
        assert series.shape == (recs.size, 1) and (series[:, 0] == recs["count"]).all()


@pytest.mark.parametrize("res", [sc.H3_RES, 5, 3, 0])
def test_membership(three, res):
    """three windows over ~4,500 cells: at res 8 more parents than the LDS table takes, so the direct path runs"""
    recs, series = _check(three, 2, 3, res, f"res {res}")
    if res == sc.H3_RES:
        cells_of = sc.membership_batch()[1]
        np.testing.assert_array_equal(recs["cell"], np.unique(np.concatenate(list(cells_of.values()))))
        assert recs.size > 1024
        for j in (0, 1, 2):
            np.testing.assert_array_equal(recs["cell"][series[:, j] > 0], cells_of[j])
        assert ((series > 0).sum(axis=1) >= 1).all() and len({tuple(r) for r in (series > 0).tolist()}) == 7   # every subset
    if res == 0:
        assert recs.size <= 122
    _check(three, 2, 2, res, f"res {res}: two of the three")
    _check(three, 1, 2, res, f"res {res}: the older two")


@pytest.mark.parametrize("res", [sc.H3_RES, 3, 1, 0])
def test_keys_under_pentagons(res):
    eng = _engine(sc.pentagon_batch()[0])
    try:
        _check(eng, 2, 3, res, f"pentagons res {res}")
    finally:
        eng.close()


@pytest.mark.parametrize("res", [sc.H3_RES, 5, 0])
def test_gaps_and_edges(sparse, res):
    lo, mid, hi = sc.SPARSE
    recs, series = _check(sparse, mid, 3, res, "a gap in the middle")           # windows 3, 4, 5
    assert recs.size and not series[:, 1].any() and series[:, 0].any() and series[:, 2].any()
    recs, series = _check(sparse, mid, 6, res, "reaching before the oldest")    # windows 0..5
    assert not series[:, :3].any() and series[:, 3].any()
    recs, series = _check(sparse, hi + 2, 3, res, "ending after the newest")    # windows 18, 19, 20
    assert series[:, 0].any() and not series[:, 1:].any()
    recs, series = _check(sparse, hi, sc.MAX_WINDOWS, res, "sixteen windows, three live")   # windows 3..18
    assert sparse.span_info()["live_windows"] == 3
    assert [j for j in range(16) if series[:, j].any()] == [0, mid - lo, hi - lo]
    for end_j, w in ((hi + 20, 4), (lo - 1, 3), (hi - 1, 12)):                  # wholly outside, or only gaps
        got = sparse.window_span(sc.wstart(end_j), w, res)
        assert got[0].size == 0 and got[1].shape == (0, w)
        assert sparse.span_info() == dict.fromkeys(sparse.span_info(), 0)
        assert sparse.window_span_geojson(sc.wstart(end_j), w, res) == sc.EMPTY
        assert sparse.window_span(sc.wstart(end_j), w, res, k=5)[0].size == 0


@pytest.mark.parametrize("res", [sc.H3_RES, 5, 0])
def test_unequal_tables(res):
    """a window of ~4,000 keys next to one of 3 -- a table smaller than one tile of the scan -- and one that is not live"""
    eng = _engine(sc.unequal_batch()[0])
    try:
        assert eng.live_windows()[1].tolist() == [4000, 3]
        recs, series = _check(eng, 2, 3, res, "4000 keys, 3 keys, none")
        assert series[:, 1].sum() == eng.window_records(sc.wstart(1), sc.H3_RES)["count"].sum() and not series[:, 2].any()
        assert np.count_nonzero(series[:, 1]) <= 3
        _check(eng, 1, 1, res, "the 3-key window alone")
        _check(eng, 1, 2, res, "both")
    finally:
        eng.close()


def _close(a, b):
    return np.abs(a - b) <= np.maximum(sc.REL * np.maximum(np.abs(a), np.abs(b)), sc.ABS_DEG)


@pytest.mark.parametrize("res", [sc.H3_RES, 5])
def test_non_dyadic(res):
    """uniform-random coordinates and speeds: cells, count, n_speed and the series exact; the sums by the closeness of the
    averages (the span and the per-window roll-ups add in different orders)"""
    eng = _engine(sc.random_batch()[0])
    try:
        (w, ws), _ = _want(eng, 2, 3, res)
        g, gs = sc.by_cell(*eng.window_span(sc.wstart(2), 3, res))
        assert g.size == w.size > 20
        for f in ("cell", "window_start_us", "count", "n_speed", "reserved"):
            np.testing.assert_array_equal(g[f], w[f], err_msg=f)
        np.testing.assert_array_equal(gs, ws)
        cnt = w["count"].astype(np.float64)
        for f in ("sum_lat", "sum_lon"):
            assert _close(g[f] / cnt, w[f] / cnt).all(), f"averages of {f} differ"
        sp = w["n_speed"] > 0
        ns = w["n_speed"][sp].astype(np.float64)
        assert _close(g["sum_speed"][sp] / ns, w["sum_speed"][sp] / ns).all() and not g["sum_speed"][~sp].any()
    finally:
        eng.close()


@pytest.mark.parametrize("res", [sc.H3_RES, 5])
def test_view_and_top(three, res):
    from mobheat import _lib, readside
    (recs, series), _ = _want(three, 2, 3, res)
    keep = readside.cells_in_view(recs["cell"], sc.VIEW)
    assert 0 < keep.sum() < recs.size                                # the viewport cuts the set
    inside = recs[keep], series[keep]
    sc.same(sc.by_cell(*three.window_span(W0 + 2 * sc.TILE, 3, res, sc.VIEW)), inside, f"res {res}: view")
    info = three.span_info()
    assert (info["parents"], info["in_view"], info["returned"]) == (recs.size, inside[0].size, inside[0].size)
    if res == sc.H3_RES:
        assert np.unique(recs["count"]).size < 12 < recs.size        # many ties: the cell decides
    for cand, view in (((recs, series), None), (inside, sc.VIEW)):
        for k in sc.ks_of(cand[0].size):
            o = readside.top_order(cand[0]["count"], cand[0]["cell"], k)
            got = three.window_span(W0 + 2 * sc.TILE, 3, res, view, k)
            sc.same(got, (cand[0][o], cand[1][o]), f"res {res} view {view} k {k}")
            assert got[0].tobytes() == readside.top_of(cand[0], k).tobytes()
            assert three.span_info()["returned"] == min(k, cand[0].size)
    far = (100.0, -10.0, 101.0, -9.0)
    if not readside.cells_in_view(recs["cell"], far).any():
        assert three.window_span(W0 + 2 * sc.TILE, 3, res, far)[0].size == 0
        assert three.window_span_geojson(W0 + 2 * sc.TILE, 3, res, far) == sc.EMPTY


@pytest.mark.parametrize("res", [sc.H3_RES, 5])
def test_geojson(three, res):
    from mobheat import _lib, readside
    end = W0 + 2 * sc.TILE
    ws_text, we_text = _lib.wall_iso(W0), _lib.wall_iso(end + sc.TILE)
    (recs, series), _ = _want(three, 2, 3, res)
    # ranked: the features in rank order, against a host-built collection and the host execution of the encoder
    for view, k in ((None, 25), (sc.VIEW, 400), (None, sc.TOP_MAX), (None, 0)):
        r, s = (recs, series) if view is None else (lambda m: (recs[m], series[m]))(readside.cells_in_view(recs["cell"], view))
        o = readside.top_order(r["count"], r["cell"], k)
        fc = sc.host_collection(r[o], s[o], ws_text, we_text)
        body = three.window_span_geojson(end, 3, res, view, k)
        assert bytes(body) == sc.dumps(fc), f"res {res} view {view} k {k}"
        assert bytes(body) == _lib.span_features_selftest(r[o], s[o], ws_text, we_text)[0].tobytes()
        assert fc == readside.tiles_span_from_engine(three, windows=3, res=res, view=view, k=k)
        assert bytes(readside.tiles_span_body(three, minutes=15, res=res, view=view, k=k)) == bytes(body)
    # unranked: the same features in the aggregation's order
    body = three.window_span_geojson(end, 3, res)
    got = json.loads(bytes(body))
    want = sc.host_collection(recs, series, ws_text, we_text)
    assert sorted(got["features"], key=lambda f: int(f["properties"]["cellId"], 16)) == want["features"]
    assert len(bytes(body)) == len(sc.dumps(want))
    assert want == readside.tiles_span_from_engine(three, minutes=11, res=res)
    for f in got["features"][:20]:
        assert f["properties"]["windows"] == 3 and sum(f["properties"]["counts"]) == f["properties"]["count"]


@pytest.mark.parametrize("res", [sc.H3_RES, 5, 0])
def test_raster(three, res):
    """the span's raster against a numpy lookup of the grid's cells in the span's records"""
    import mobheat
    import raster_cases as rc
    from mobheat import readside
    (recs, _), _ = _want(three, 2, 3, res)
    lat, lon = readside.tile_grid(11, *rc.tile_of(42.33, -71.07, 11), size=64)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    cells = mobheat.latlng_to_cell(la.ravel(), lo.ravel(), res)
    at = np.minimum(np.searchsorted(recs["cell"], cells), recs.size - 1)
    want = np.where(recs["cell"][at] == cells, recs["count"][at], 0).astype(np.uint32).reshape(64, 64)
    assert want.any()
    thr = readside.COUNT_THRESHOLDS
    counts, classes = three.window_span_raster(lat, lon, W0 + 2 * sc.TILE, 3, res, thr)
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(classes, (want[..., None] > np.asarray(thr)).sum(axis=-1).astype(np.uint8))
    np.testing.assert_array_equal(three.window_span_raster(lat, lon, W0 + 2 * sc.TILE, 3, res), want)
    one = three.window_span_raster(lat, lon, W0 + sc.TILE, 1, res)
    np.testing.assert_array_equal(one, three.window_raster(lat, lon, W0 + sc.TILE, res))
    assert not three.window_span_raster(lat, lon, W0 + 40 * sc.TILE, 2, res).any()
    png = readside.tiles_span_png(three, 11, *rc.tile_of(42.33, -71.07, 11), minutes=15, res=res, size=64)
    assert png == readside.png_from_classes(classes)


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_past_the_first_grid_iteration(three, grid):
    """MOBHEAT_TEST_READ_GRID: every output is the knob-unset engine's byte for byte.  The three tables are one tile of the
    scan each: with grid 1 one workgroup crosses both window boundaries, with grid 2 one crosses the first -- the flush
    path -- and with grid 3 every workgroup has one window."""
    import raster_cases as rc
    from mobheat import readside
    eng = _engine(sc.membership_batch()[0], grid)
    end = W0 + 2 * sc.TILE
    lat, lon = readside.tile_grid(11, *rc.tile_of(42.33, -71.07, 11), size=64)
    try:
        before = eng.read_grid_info()["launches_lowered"]
        launches = 0
        for res in (sc.H3_RES, 5, 0):
            for w in (3, 2):
                a, b = sc.by_cell(*eng.window_span(end, w, res)), sc.by_cell(*three.window_span(end, w, res))
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"res {res} {w} windows"
                # k_span over w one-tile tables; k_span_emit over thousands of slots (at res 0 the table is one tile)
                launches += (grid < w) + (res > 0)
            a, b = eng.window_span(end, 3, res, sc.VIEW, 500), three.window_span(end, 3, res, sc.VIEW, 500)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"res {res} view and top"
            assert bytes(eng.window_span_geojson(end, 3, res, k=300)) == bytes(three.window_span_geojson(end, 3, res, k=300))
            np.testing.assert_array_equal(eng.window_span_raster(lat, lon, end, 3, res), three.window_span_raster(lat, lon, end, 3, res))
            launches += 3 * ((grid < 3) + (res > 0))
        info = eng.read_grid_info()
        assert info["launches_lowered"] >= before + launches, info
        assert info["least_iterations"] >= 2, info
        assert three.read_grid_info()["launches_lowered"] == 0
    finally:
        eng.close()


def test_reads_only_and_allocates_nothing_twice(three):
    """the span calls leave state_version and the exported state as they were; window_records, window_raster and
    window_change right after one return what they returned before; a repeated identical call allocates nothing; the tile
    body without a span is the host execution's, byte for byte"""
    import raster_cases as rc
    from mobheat import _lib, readside
    eng = three
    end = W0 + 2 * sc.TILE
    lat, lon = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12))
    version = eng.state_version()
    state0 = np.sort(eng.export_state()[1]).tobytes()
    before = {ws: (np.sort(eng.window_records(ws, 8), order="cell").tobytes(), eng.window_raster(lat, lon, ws, 8).tobytes(),
                   eng.window_top(50, ws, 5).tobytes()) for ws in (W0, end)}
    change0 = eng.window_change(end, W0, 5, order="abs", k=100).tobytes()
    body0, recs0, offs0 = eng.window_geojson(end, 5, with_records=True)
    keep = []
    for _ in range(2):
        c0 = eng.last_counts()
        a, b = eng.window_span(end, 3), eng.window_span(end, 3, 5, sc.VIEW, 100)
        keep.append((sc.by_cell(*a)[0].tobytes(), b[0].tobytes(), b[1].tobytes(),
                     bytes(eng.window_span_geojson(end, 2, 5, sc.VIEW, 100)), eng.window_span_raster(lat, lon, end, 3, 5).tobytes()))
        c1 = eng.last_counts()
    assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
    assert keep[0] == keep[1]
    assert eng.state_version() == version and np.sort(eng.export_state()[1]).tobytes() == state0
    for ws in (W0, end):
        eng.window_span(end, 3, 5, k=10)
        assert np.sort(eng.window_records(ws, 8), order="cell").tobytes() == before[ws][0]
        eng.window_span(end, 3, 5)
        assert eng.window_raster(lat, lon, ws, 8).tobytes() == before[ws][1]
        eng.window_span(end, 2, 8, sc.VIEW)
        assert eng.window_top(50, ws, 5).tobytes() == before[ws][2]
    eng.window_span(end, 3, 3)
    assert eng.window_change(end, W0, 5, order="abs", k=100).tobytes() == change0
    # the tile body without a span: unchanged by the encoder's option
    eng.window_span_geojson(end, 3, 5)
    body, recs, offs = eng.window_geojson(end, 5, with_records=True)
    assert np.sort(recs, order="cell").tobytes() == np.sort(recs0, order="cell").tobytes() and len(body) == len(body0)
    text = (_lib.wall_iso(end), _lib.wall_iso(end + sc.TILE))
    assert bytes(body) == _lib.tile_features_selftest(recs, *text)[0].tobytes()
    # a checkpoint export in two halves with a span call in between
    info, n, recs, raw, fill = eng.export_begin(touched_only=False)
    assert eng.window_span(end, 3, 3, k=5)[0].size == 5
    fill(0, n)
    assert np.sort(recs).tobytes() == state0


def test_errors(three):
    from mobheat import _lib
    end = W0 + 2 * sc.TILE
    for w in (0, 17, -1):
        assert _code(lambda: three.window_span(end, w)) == _lib.HM_E_INVALID
        assert _code(lambda: three.window_span_geojson(end, w)) == _lib.HM_E_INVALID
        assert _code(lambda: three.window_span_raster([42.0], [-71.0], end, w)) == _lib.HM_E_INVALID
    for bad_end in (end + 1, end - sc.MINUTE, W0 + sc.TILE // 2):
        assert _code(lambda: three.window_span(bad_end, 2)) == _lib.HM_E_INVALID
        assert _code(lambda: three.window_span_geojson(bad_end, 2)) == _lib.HM_E_INVALID
        assert _code(lambda: three.window_span_raster([42.0], [-71.0], bad_end, 2)) == _lib.HM_E_INVALID
    for res in (sc.H3_RES + 1, -1, 16):
        assert _code(lambda: three.window_span(end, 3, res)) == _lib.HM_E_INVALID
        assert _code(lambda: three.window_span_raster([42.0], [-71.0], end, 3, res)) == _lib.HM_E_INVALID
    assert _code(lambda: three.window_span(end, 3, k=sc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: three.window_span_geojson(end, 3, k=sc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    assert _code(lambda: three.window_span(end, 3, view=(10.0, 50.0, 20.0, 40.0))) == _lib.HM_E_INVALID
    assert _code(lambda: three.window_span(end, 3, view=(10.0, 0.0, float("nan"), 40.0))) == _lib.HM_E_INVALID
    p, s, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()   # an out_memory that is neither
    assert three._lib.hm_span_rollup(three._ctx, end, 3, 8, None, -1, 7, ctypes.byref(p), ctypes.byref(s), ctypes.byref(n)) == _lib.HM_E_INVALID
    empty = _engine()
    try:
        assert empty.span_info() == dict.fromkeys(empty.span_info(), 0)   # all 0 before the first call
        assert empty.window_span(windows=4)[0].size == 0 and empty.window_span(windows=4, k=3)[0].size == 0
        assert empty.window_span_geojson(windows=2) == sc.EMPTY
        assert not empty.window_span_raster([42.0, 42.1], [-71.0], windows=2).any()
    finally:
        empty.close()
    # the trailing span's default end is the newest live window
    sc.same(sc.by_cell(*three.window_span(None, 3, 5)), sc.by_cell(*three.window_span(end, 3, 5)), "default end")


def test_shard_context():
    from mobheat import _lib
    shard = _engine(shard=(0, 2))
    try:
        assert shard.window_span(W0, 3)[0].size == 0                              # allowed: the rank's partial
        assert shard.window_span_geojson(W0, 3) == sc.EMPTY
        assert _code(lambda: shard.window_span(W0, 3, k=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_span_geojson(W0, 3, k=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_span_raster([42.0], [-71.0], W0, 3)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_span(W0, 3, k=sc.TOP_MAX + 1)) == _lib.HM_E_INVALID    # arguments first
        assert _code(lambda: shard.window_span(W0, 17, k=5)) == _lib.HM_E_INVALID
        assert _code(lambda: shard.window_span(W0, 3, 9, k=5)) == _lib.HM_E_INVALID               # then the resolution
    finally:
        shard.close()


def test_between_stage_calls():
    from mobheat import _lib, synth
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, HmBatchIn
    eng = _engine()
    try:
        # a world of one, left after its ingest (as tests/test_gpu_top.py's contract test)
        k = {kk: np.ascontiguousarray(v) for kk, v in synth.c1_boston(n=2000).items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(eng._lib.hm_stage_ingest(eng._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), eng._ctx, "hm_stage_ingest")
        assert _code(lambda: eng.window_span(W0, 3)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_span(W0, 3, k=5)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_span_geojson(W0, 3)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_span_raster([42.0], [-71.0], W0, 3)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_span(W0, 0)) == _lib.HM_E_INVALID    # arguments first
    finally:
        eng.close()
