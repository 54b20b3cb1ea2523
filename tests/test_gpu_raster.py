"""GPU: a live window as a raster (hm_window_raster: k_raster + k_raster_exact, csrc/k_raster.h) -- the device's grids
against the host execution of the same per-pixel code on the window's own roll-up records (hm_selftest_window_raster, which
tests/test_raster_host.py ties to the oracle) and against the rule restated with the oracle (tests/raster_cases.py).
No tolerance: counts and classes are integers, and a pixel's cell is bit-exact."""
import ctypes

import numpy as np
import pytest

import raster_cases as rc

pytestmark = pytest.mark.gpu
MINUTE = 60_000_000
BOSTON = (42.36, -71.06)
REL = 1e-9   # tests/test_gpu_parity.py's bound on averages of fp64 atomic sums (two engines add in different orders)


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _batch(seed=0, shift_us=0, edges=True):
    """a C1 Boston batch, with the UDF's edge points as rows of its newest window"""
    from mobheat import synth
    b = synth.c1_boston(seed=seed, n=20_000)
    b["ts_us"] = b["ts_us"] + shift_us
    if edges:
        el, eo = synth.edge_points()
        m = el.size
        b = dict(lat=np.r_[b["lat"], el], lon=np.r_[b["lon"], eo], ts_us=np.r_[b["ts_us"], np.full(m, b["ts_us"].max())],
                 speed=np.r_[b["speed"], np.zeros(m)], speed_valid=np.r_[b["speed_valid"], np.zeros(m, bool)],
                 vkey=np.r_[b["vkey"], np.arange(m, dtype=np.uint64) + np.uint64(1 << 40)],
                 row_valid=np.r_[b["row_valid"], np.ones(m, bool)])
    return b


def _check(eng, lat, lon, ws, res, what):
    """window_raster == the host execution on window_records(res) == the rule; returns the count grid"""
    from mobheat import _lib, readside
    thr = readside.COUNT_THRESHOLDS
    recs = eng.window_records(ws, res)
    counts, classes = eng.window_raster(lat, lon, ws, res, thr)
    info = eng.raster_info()
    assert info["pixels"] == counts.size and info["records"] == recs.size and info["kernel_us"] > 0
    hc, hk = _lib.window_raster_selftest(recs, res, lat, lon, thr)
    ec, ek = rc.expected(recs, res, lat, lon, thr)
    for name, c, k in (("host execution", hc, hk), ("oracle", ec, ek)):
        np.testing.assert_array_equal(counts, c, err_msg=f"{what}: counts differ from the {name}")
        np.testing.assert_array_equal(classes, k, err_msg=f"{what}: classes differ from the {name}")
    np.testing.assert_array_equal(eng.window_raster(lat, lon, ws, res), counts)   # counts alone
    return counts


def _raster_on_device(eng, lat, lon, ws, res, thresholds):
    """hm_window_raster with HM_MEM_DEVICE, the two grids copied back from the device pointers"""
    from mobheat import _lib
    lat, lon, thr = _lib.raster_args(lat, lon, thresholds)
    pc, pk = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(eng._lib.hm_window_raster(eng._ctx, int(ws), res, _lib.ptr(lat), lat.size, _lib.ptr(lon), lon.size, _lib.ptr(thr),
                                         thr.size, _lib.HM_MEM_DEVICE, ctypes.byref(pc), ctypes.byref(pk)), eng._ctx)
    counts, classes = np.zeros((lat.size, lon.size), np.uint32), np.zeros((lat.size, lon.size), np.uint8)
    _lib.check(eng._lib.hm_memcpy(counts.ctypes.data, pc, counts.nbytes, 1), None, "hm_memcpy")
    _lib.check(eng._lib.hm_memcpy(classes.ctypes.data, pk, classes.nbytes, 1), None, "hm_memcpy")
    return counts, classes


@pytest.fixture(scope="module")
def engine():
    import mobheat
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    eng.process_batch(0, **_batch())
    yield eng
    eng.close()


# ---- device == host execution == oracle ----
@pytest.mark.parametrize("res", [0, 1, 2])
def test_whole_world(engine, res):
    from mobheat import readside
    ws = int(engine.live_windows()[0][-1])
    lat, lon = readside.tile_grid(0, 0, 0)
    counts = _check(engine, lat, lon, ws, res, f"world res {res}")
    assert np.count_nonzero(counts) > 0


@pytest.mark.parametrize("z,res", [(12, 8), (12, 6), (18, 8), (10, 8)])
def test_boston_tiles(engine, z, res):
    """the tile over central Boston: at zoom 12 some ninety res-8 cells, every pixel on a tile of the batch; at zoom 18 one
    or two cells in all; at zoom 10 the tile is wider than the batch's box, so pixels with and without a tile"""
    from mobheat import readside
    ws = int(engine.live_windows()[0][-1])
    x, y = rc.tile_of(*BOSTON, z)
    if z == 12:
        assert (x, y) == (1239, 1514)
    lat, lon = readside.tile_grid(z, x, y)
    assert lat[-1] < BOSTON[0] < lat[0] and lon[0] < BOSTON[1] < lon[-1]
    counts = _check(engine, lat, lon, ws, res, f"zoom {z} res {res}")
    cells = np.unique(rc.pixel_cells(res, lat, lon))
    have = set(engine.window_records(ws, res)["cell"].tolist())
    assert have & set(cells.tolist()), "the tile covers no cell of the batch"
    assert np.count_nonzero(counts) > 0
    if z == 18:
        assert cells.size <= 3
    if z == 10:
        assert 0 < np.count_nonzero(counts) < counts.size
    if (z, res) == (12, 8):
        assert cells.size > 50 and np.unique(counts).size > 5   # many cells, many different counts


# ---- the edge grid ----
def test_edge_grid_on_the_device():
    """A window holding one record per distinct res-8 cell of the edge grid (counts 1..k), rastered over that grid at res 8
    (every in-range pixel has its record), 7 and 0 (the roll-up's parents): the face centres go through k_raster_exact, the
    NaN / out-of-range pixels have cell 0 and stay 0 although the table has free slots."""
    import mobheat
    lat, lon, nf = rc.edge_grid()
    cells = np.unique(rc.pixel_cells(8, lat, lon))
    cells = cells[cells != 0]
    ws = 1_759_572_000_000_000
    recs = rc.records(cells, np.arange(1, cells.size + 1), ws)
    info = dict(epoch_id=0, n_keys=recs.size, watermark_ms=0, prev_watermark_ms=0, tile_us=5 * MINUTE, watermark_delay_ms=600_000,
                h3_res=8)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        eng.import_state(info, recs)
        assert eng.live_windows()[0].tolist() == [ws]
        bad_r, bad_c = ~(np.abs(lat) <= 90.0), ~(np.abs(lon) <= 180.0)
        for res in (8, 7, 0):
            counts = _check(eng, lat, lon, ws, res, f"edge grid res {res}")
            ri = eng.raster_info()
            assert ri["exact_pixels"] >= 20, "the face centres did not reach k_raster_exact"
            # (the parent table has at least twice as many slots as records: a cell-0 probe would meet a free one at once)
            assert not counts[bad_r].any() and not counts[:, bad_c].any()
            assert np.count_nonzero(np.diag(counts)[:nf]) == nf
            if res == 8:
                assert counts[np.ix_(~bad_r, ~bad_c)].all()
    finally:
        eng.close()


# ---- sizes: on and around one wave and one 256-thread block, a ragged last segment; both memories ----
@pytest.fixture(scope="module")
def boston257(engine):
    from mobheat import readside
    ws = int(engine.live_windows()[0][-1])
    lat, lon = readside.tile_grid(12, *rc.tile_of(*BOSTON, 12), size=257)
    recs = engine.window_records(ws, 8)
    return ws, lat, lon, rc.expected(recs, 8, lat, lon, readside.COUNT_THRESHOLDS)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 63), (1, 64), (1, 65), (255, 3), (3, 257), (256, 256), (257, 65)])
def test_sizes_and_memories(engine, boston257, rows, cols):
    from mobheat import readside
    ws, lat, lon, (ec, ek) = boston257
    thr = readside.COUNT_THRESHOLDS
    counts, classes = engine.window_raster(lat[:rows], lon[:cols], ws, 8, thr)
    assert counts.shape == classes.shape == (rows, cols)
    np.testing.assert_array_equal(counts, ec[:rows, :cols])
    np.testing.assert_array_equal(classes, ek[:rows, :cols])
    dc, dk = _raster_on_device(engine, lat[:rows], lon[:cols], ws, 8, thr)
    np.testing.assert_array_equal(dc, ec[:rows, :cols])
    np.testing.assert_array_equal(dk, ek[:rows, :cols])
    # the grid's other end: the last rows and columns (another alignment of the same pixels)
    counts, classes = engine.window_raster(lat[-rows:], lon[-cols:], ws, 8, thr)
    np.testing.assert_array_equal(counts, ec[-rows:, -cols:])
    np.testing.assert_array_equal(classes, ek[-rows:, -cols:])


# ---- saturation and classes ----
def test_saturation_and_classes_on_the_device(oracle_h3):
    import mobheat
    from mobheat import readside
    rng = np.random.default_rng(4301)
    n = len(rc.EDGE_COUNTS)
    lat, lon = rng.uniform(42.20, 42.45, n), rng.uniform(-71.20, -70.95, n)
    cells = oracle_h3.latlng_to_cell(lat, lon, 8)   # pixel (k, k) in cell k
    assert np.unique(cells).size == n
    ws = 1_759_572_000_000_000
    recs = rc.records(cells, rc.EDGE_COUNTS, ws)
    info = dict(epoch_id=0, n_keys=n, watermark_ms=0, prev_watermark_ms=0, tile_us=5 * MINUTE, watermark_delay_ms=600_000, h3_res=8)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        eng.import_state(info, recs)
        for thr in (readside.COUNT_THRESHOLDS, (2 ** 33,), (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40)):
            counts, classes = eng.window_raster(lat, lon, ws, 8, thr)
            ec, ek = rc.expected(recs, 8, lat, lon, thr)
            np.testing.assert_array_equal(counts, ec)
            np.testing.assert_array_equal(classes, ek)
            assert np.diag(counts).tolist() == rc.EDGE_COUNTS[:11] + [0xFFFFFFFF] * 3
        assert np.diag(eng.window_raster(lat, lon, ws, 8, readside.COUNT_THRESHOLDS)[1]).tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6]
        assert np.diag(eng.window_raster(lat, lon, ws, 8, (2 ** 33,))[1]).tolist() == [0] * 13 + [1]
    finally:
        eng.close()


# ---- the contract ----
def test_contract():
    """a window that is not live, a resolution above h3_res, bad grids and thresholds, a repeated call's memory, between
    stage calls"""
    import mobheat
    from mobheat import _lib, readside
    from mobheat._lib import HM_MEM_HOST, HM_STAGE_SUMMARY_WORDS, HmBatchIn
    lat, lon = readside.tile_grid(12, *rc.tile_of(*BOSTON, 12))
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        assert not eng.window_raster(lat, lon).any()   # no window at all
        eng.process_batch(0, **_batch())
        wins = eng.live_windows()[0].tolist()
        for dead in (wins[0] - 5 * MINUTE, wins[-1] + 5 * MINUTE, wins[-1] + 1):
            counts, classes = eng.window_raster(lat, lon, dead, 8, readside.COUNT_THRESHOLDS)
            assert counts.shape == (256, 256) and not counts.any() and not classes.any()
            assert eng.raster_info()["records"] == 0
        assert eng.window_raster(lat, lon, wins[-1], 8).any()
        assert _code(lambda: eng.window_raster(lat, lon, wins[-1], 9)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.window_raster(lat, lon, wins[-1], -1)) == _lib.HM_E_INVALID
        for thr in ((5, 2), (2, 2), (-1, 3), tuple(range(16))):
            assert _code(lambda: eng.window_raster(lat, lon, wins[-1], 8, thr)) == _lib.HM_E_INVALID, thr
        assert _code(lambda: eng.window_raster(np.zeros(16385), lon, wins[-1], 8)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.window_raster(np.zeros(16384), np.zeros(8192), wins[-1], 8)) == _lib.HM_E_INVALID
        assert eng.window_raster(lat, lon[:0], wins[-1], 8).shape == (256, 0)
        # a second identical call leaves the device's free memory as it was
        free0, free1, total = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        first = eng.window_raster(lat, lon, wins[-1], 8, readside.COUNT_THRESHOLDS)
        _lib.check(eng._lib.hm_device_memory(0, ctypes.byref(free0), ctypes.byref(total)))
        c0 = eng.last_counts()
        again = eng.window_raster(lat, lon, wins[-1], 8, readside.COUNT_THRESHOLDS)
        _lib.check(eng._lib.hm_device_memory(0, ctypes.byref(free1), ctypes.byref(total)))
        c1 = eng.last_counts()
        assert free0.value == free1.value and (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        np.testing.assert_array_equal(first[0], again[0])
        np.testing.assert_array_equal(first[1], again[1])
        # between stage calls (a world of one, left after its ingest)
        k = {kk: np.ascontiguousarray(v) for kk, v in _batch(20, 12 * MINUTE, edges=False).items()}
        k["sv"], k["rv"] = k["speed_valid"].astype(np.uint8), k["row_valid"].astype(np.uint8)
        bi = HmBatchIn(n=k["lat"].size, memory=HM_MEM_HOST, lat=k["lat"].ctypes.data, lon=k["lon"].ctypes.data,
                       ts_us=k["ts_us"].ctypes.data, speed=k["speed"].ctypes.data, speed_valid=k["sv"].ctypes.data,
                       vkey=k["vkey"].ctypes.data, row_valid=k["rv"].ctypes.data)
        summ = np.zeros((1, HM_STAGE_SUMMARY_WORDS), np.int64)
        _lib.check(eng._lib.hm_stage_ingest(eng._ctx, 3, ctypes.byref(bi), 1, 0, summ.ctypes.data), eng._ctx, "hm_stage_ingest")
        assert _code(lambda: eng.window_raster(lat, lon, wins[-1], 8)) == _lib.HM_E_STATE
    finally:
        eng.close()


def test_raster_reads_only_and_follows_the_state():
    """Two engines fed the same batches, one rastering in between: state_version unchanged by a raster, the next batch's
    result the twin's (integers equal; averages within the suite's bound for sums added in another order), and a raster
    after that batch shows the new counts."""
    import mobheat
    from mobheat import readside
    lat, lon = readside.tile_grid(12, *rc.tile_of(*BOSTON, 12))
    a, b = mobheat.HeatmapEngine(h3_res=8, device=0), mobheat.HeatmapEngine(h3_res=8, device=0)
    try:
        a.process_batch(0, **_batch(0))
        b.process_batch(0, **_batch(0))
        v = a.state_version()
        ws = int(a.live_windows()[0][-1])
        before = a.window_raster(lat, lon, ws, 8)
        a.window_raster(lat, lon, ws, 5, readside.COUNT_THRESHOLDS)
        assert a.state_version() == v
        ra, rb = a.process_batch(1, **_batch(1)), b.process_batch(1, **_batch(1))
        ta, tb = ra.tiles, rb.tiles
        oa, ob = np.lexsort((ta.window_start_us, ta.cell)), np.lexsort((tb.window_start_us, tb.cell))
        for f in ("cell", "window_start_us", "count", "speed_null"):
            np.testing.assert_array_equal(getattr(ta, f)[oa], getattr(tb, f)[ob], err_msg=f)
        for f in ("avg_speed", "avg_lon", "avg_lat"):
            np.testing.assert_allclose(getattr(ta, f)[oa], getattr(tb, f)[ob], rtol=REL, atol=0, err_msg=f)
        assert ra.n_state == rb.n_state and (ra.n_valid, ra.n_late) == (rb.n_valid, rb.n_late)
        np.testing.assert_array_equal(np.sort(ra.latest_rows), np.sort(rb.latest_rows))
        after = _check(a, lat, lon, ws, 8, "after a further batch")
        assert (after >= before).all() and int(after.astype(np.int64).sum()) > int(before.astype(np.int64).sum())
        np.testing.assert_array_equal(after, b.window_raster(lat, lon, ws, 8))
    finally:
        a.close()
        b.close()


# ---- shard contexts ----
def test_shard_grids_add_up(engine):
    """The newest window's keys split over W shard contexts on this GPU by their owner rank (each imports its own; the
    stage API's exchange is tested elsewhere): the ranks' count grids add up to the single engine's; classes are refused."""
    import mobheat
    from mobheat import _lib, readside
    from mobheat.distributed import tile_owner
    W = 3
    ws = int(engine.live_windows()[0][-1])
    recs = engine.window_records(ws, 8)
    own = np.asarray(tile_owner(recs["cell"], recs["window_start_us"], W))
    lat, lon = readside.tile_grid(12, *rc.tile_of(*BOSTON, 12))
    info = dict(epoch_id=0, watermark_ms=0, prev_watermark_ms=0, tile_us=5 * MINUTE, watermark_delay_ms=600_000, h3_res=8)
    for res in (8, 6):
        total = np.zeros((256, 256), np.uint64)
        for r in range(W):
            mine = np.ascontiguousarray(recs[own == r])
            assert mine.size > 0
            sh = mobheat.HeatmapEngine(h3_res=8, device=0, shard=(r, W))
            try:
                sh.import_state(dict(info, n_keys=mine.size), mine)
                part = sh.window_raster(lat, lon, ws, res)
                assert part.any()
                total += part
                assert _code(lambda: sh.window_raster(lat, lon, ws, res, readside.COUNT_THRESHOLDS)) == _lib.HM_E_INVALID
            finally:
                sh.close()
        np.testing.assert_array_equal(np.minimum(total, 0xFFFFFFFF).astype(np.uint32), engine.window_raster(lat, lon, ws, res))


# ---- end to end ----
def test_tiles_latest_png(engine):
    from mobheat import readside
    z = 10   # (wider than the batch's box: pixels with and without a tile, test_boston_tiles)
    x, y = rc.tile_of(*BOSTON, z)
    png = readside.tiles_latest_png(engine, z, x, y)
    classes, plte, trns = rc.decode_png(png)
    lat, lon = readside.tile_grid(z, x, y)
    _, want = engine.window_raster(lat, lon, None, None, readside.COUNT_THRESHOLDS)
    np.testing.assert_array_equal(classes, want)
    assert classes.shape == (256, 256) and 0 < np.count_nonzero(classes) < classes.size
    assert plte == [p[:3] for p in readside.COUNT_PALETTE] and list(trns) == [p[3] for p in readside.COUNT_PALETTE]
    small, _, _ = rc.decode_png(readside.tiles_latest_png(engine, z, x, y, res=6, size=64))
    np.testing.assert_array_equal(small, engine.window_raster(*readside.tile_grid(z, x, y, 64), None, 6, readside.COUNT_THRESHOLDS)[1])
