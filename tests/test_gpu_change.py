"""GPU: the change between two live windows (hm_window_change, hm_window_change_top, hm_window_geojson_change;
csrc/k_change.h).  Every result is compared -- sorted by cell, or in rank order -- with the host execution
(hm_selftest_window_change) and with readside.change_of / change_top_of, both fed by window_records of the same engine;
the inputs are dyadic (tests/change_cases.py), so "equal" is bit-equal, but for the one uniform-random input, whose sums
are held to tests/test_gpu_rollup.py's closeness of averages.  tests/test_change_host.py proves on the CPU that the
batches are what they claim and that the two references agree with a plain dict join."""
import ctypes

import numpy as np
import pytest

import change_cases as cc

pytestmark = pytest.mark.gpu
KNOB = "MOBHEAT_TEST_READ_GRID"
SUMS = ("sum_speed", "sum_lat", "sum_lon")


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
        eng = mobheat.HeatmapEngine(h3_res=cc.H3_RES, device=0, **kw)
    if batch is not None:
        eng.process_batch(0, **batch)
    return eng


@pytest.fixture(scope="module")
def overlap():
    """an engine holding the overlap batch: both windows live, cells in A only, in B only and in both"""
    b, a_cells, b_cells = cc.shape_batch("overlap")
    eng = _engine(b)
    assert eng.live_windows()[0].tolist() == [cc.WB, cc.WA]
    yield eng, a_cells, b_cells
    eng.close()


def _references(eng, res, wa=cc.WA, wb=cc.WB):
    """the pairs sorted by cell from window_records of the engine: numpy's, checked against the host execution's"""
    from mobheat import _lib, readside
    cur, base = eng.window_records(wa, res), eng.window_records(wb, res)
    want = readside.change_of(cur, base, wa, wb)
    cc.same(_lib.window_change_selftest(cur, base, wa, wb), want, "host execution against numpy")
    return cur, base, want


def _check_all(eng, res, what, wa=cc.WA, wb=cc.WB):
    """the unranked call at res against both references; returns the pairs sorted by cell"""
    cur, base, want = _references(eng, res, wa, wb)
    got = eng.window_change(wa, wb, res)
    info = eng.change_info()
    assert np.unique(got["cur"]["cell"]).size == got.size, f"{what}: a cell appears twice"
    cc.same(cc.by_cell(got), want, f"{what}: device against the references")
    both = np.intersect1d(cur["cell"], base["cell"]).size
    assert (info["cur_cells"], info["base_cells"], info["both"], info["in_view"], info["returned"]) == \
        (cur.size, base.size, both, want.size, want.size), (what, info)
    return want


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_cell_set_shapes(shape):
    b, a_cells, b_cells = cc.shape_batch(shape)
    eng = _engine(b)
    try:
        want = _check_all(eng, cc.H3_RES, shape)
        np.testing.assert_array_equal(want["cur"]["cell"], np.union1d(a_cells, b_cells))
        in_a, in_b = np.isin(want["cur"]["cell"], a_cells), np.isin(want["cur"]["cell"], b_cells)
        assert (want["cur"]["count"][in_a] > 0).all() and not want["cur"]["count"][~in_a].any()
        assert (want["base"]["count"][in_b] > 0).all() and not want["base"]["count"][~in_b].any()
        assert (want["cur"]["window_start_us"] == cc.WA).all() and (want["base"]["window_start_us"] == cc.WB).all()
        for order in cc.ORDERS:   # a window that is not live ranks as zeros
            cc.same(eng.window_change(cc.WA, cc.WB, order=order, k=300), cc.ref_order(want, order, 300), f"{shape} {order}")
    finally:
        eng.close()


def test_neither_live_and_the_same_window(overlap):
    from mobheat import _lib
    eng, _, _ = overlap
    far = cc.WA + 50 * cc.MINUTE
    assert eng.window_change(far, far - 5 * cc.MINUTE).size == 0
    assert eng.change_info()["returned"] == 0
    assert eng.window_change(far, far - 5 * cc.MINUTE, order="abs", k=10).size == 0
    assert eng.window_change_geojson(far, far - 5 * cc.MINUTE) == cc.EMPTY
    assert _code(lambda: eng.window_change(cc.WA, cc.WA)) == _lib.HM_E_INVALID
    assert _code(lambda: eng.window_change(cc.WA, cc.WA, order="rising", k=5)) == _lib.HM_E_INVALID
    assert _code(lambda: eng.window_change_geojson(cc.WA, cc.WA)) == _lib.HM_E_INVALID
    for bad in (cc.H3_RES + 1, -1, 16):
        assert _code(lambda: eng.window_change(cc.WA, cc.WB, bad)) == _lib.HM_E_INVALID
    empty = _engine()
    try:
        assert empty.change_info() == dict.fromkeys(empty.change_info(), 0)   # all 0 before the first call
        assert empty.window_change().size == 0 and empty.window_change(order="falling", k=3).size == 0
        assert empty.window_change_geojson() == cc.EMPTY
    finally:
        empty.close()


def test_defaults_are_the_newest_window_and_the_one_before(overlap):
    eng, _, _ = overlap
    cc.same(cc.by_cell(eng.window_change()), cc.by_cell(eng.window_change(cc.WA, cc.WB)), "defaults")
    # the windows swapped: the halves swap
    fwd, rev = cc.by_cell(eng.window_change(cc.WA, cc.WB, 5)), cc.by_cell(eng.window_change(cc.WB, cc.WA, 5))
    assert fwd["cur"].tobytes() == rev["base"].tobytes() and fwd["base"].tobytes() == rev["cur"].tobytes()


@pytest.mark.parametrize("res", [cc.H3_RES, 5, 0])
def test_resolutions(overlap, res):
    eng, a_cells, b_cells = overlap
    want = _check_all(eng, res, f"res {res}")
    if res == cc.H3_RES:
        assert want.size == np.union1d(a_cells, b_cells).size
    else:   # children merge
        assert 0 < want.size < np.union1d(a_cells, b_cells).size // 2
    if res == 0:
        assert want.size <= 122
    for order in cc.ORDERS:
        for k in (1, 7, cc.TOP_MAX):
            cc.same(eng.window_change(cc.WA, cc.WB, res, order=order, k=k), cc.ref_order(want, order, k), f"res {res} {order} k {k}")


@pytest.mark.parametrize("res", [cc.H3_RES, 3, 1, 0])
def test_keys_under_pentagons(res):
    eng = _engine(cc.pentagon_batch()[0])
    try:
        want = _check_all(eng, res, f"pentagons res {res}")
        cc.same(eng.window_change(cc.WA, cc.WB, res, order="abs", k=50), cc.ref_order(want, "abs", 50), f"pentagons res {res}")
    finally:
        eng.close()


@pytest.mark.parametrize("n_base", [512, 4096])
def test_base_table_at_its_load_limit(n_base):
    b, a_cells, b_cells = cc.load_limit_batch(n_base)
    eng = _engine(b)
    try:
        assert eng.live_windows()[1].tolist() == [n_base, n_base // 2]
        want = _check_all(eng, cc.H3_RES, f"{n_base} base cells")
        assert eng.change_info()["base_cells"] == n_base and want.size == np.union1d(a_cells, b_cells).size
        for order in cc.ORDERS:
            cc.same(eng.window_change(cc.WA, cc.WB, order=order, k=100), cc.ref_order(want, order, 100), f"{n_base} {order}")
    finally:
        eng.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_past_the_first_grid_iteration(overlap, grid):
    """MOBHEAT_TEST_READ_GRID=1 and =3 with a few thousand cells per window: every lowered launch iterates at least twice,
    and the results are the knob-unset engine's byte for byte"""
    plain, _, _ = overlap
    eng = _engine(cc.shape_batch("overlap")[0], grid)
    try:
        before = eng.read_grid_info()["launches_lowered"]
        for res in (cc.H3_RES, 5):
            assert cc.by_cell(eng.window_change(cc.WA, cc.WB, res)).tobytes() == cc.by_cell(plain.window_change(cc.WA, cc.WB, res)).tobytes()
            for order in cc.ORDERS:
                assert eng.window_change(cc.WA, cc.WB, res, cc.VIEW, order, 500).tobytes() == \
                    plain.window_change(cc.WA, cc.WB, res, cc.VIEW, order, 500).tobytes()
            assert bytes(eng.window_change_geojson(cc.WA, cc.WB, res, order="abs", k=300)) == \
                bytes(plain.window_change_geojson(cc.WA, cc.WB, res, order="abs", k=300))
        info = eng.read_grid_info()
        # the join's two kernels, the view, the keys and the scatter over thousands of pairs: all on lowered grids
        assert info["launches_lowered"] >= before + 10 and info["least_iterations"] >= 2, info
        assert plain.read_grid_info()["launches_lowered"] == 0
    finally:
        eng.close()


def test_ranking(overlap):
    from mobheat import _lib, readside
    eng, _, _ = overlap
    cur, base, want = _references(eng, cc.H3_RES)
    n = want.size
    d = want["cur"]["count"] - want["base"]["count"]
    assert (d > 0).any() and (d < 0).any() and (d == 0).any() and np.unique(d).size < 12   # ties: the cell decides
    assert np.intersect1d(d[d > 0], -d[d < 0]).size > 0                                  # +c and -c tie in "abs"
    for order in cc.ORDERS:
        for k in cc.ks_of(n):
            got = eng.window_change(cc.WA, cc.WB, order=order, k=k)
            assert eng.change_info()["returned"] == min(k, n) == got.size
            cc.same(got, cc.ref_order(want, order, k), f"{order} k {k}: device against sorted")
            cc.same(readside.change_top_of(want, order, k), got, f"{order} k {k}: numpy against the device")
            cc.same(_lib.window_change_selftest(cur, base, cc.WA, cc.WB, order, k), got, f"{order} k {k}: host execution")
    assert eng.change_info()["device_us"] > 0
    for k in (cc.TOP_MAX + 1, -1):
        assert _code(lambda: eng.window_change(cc.WA, cc.WB, order="rising", k=k)) == _lib.HM_E_INVALID
    assert _code(lambda: eng.window_change_geojson(cc.WA, cc.WB, order="rising", k=cc.TOP_MAX + 1)) == _lib.HM_E_INVALID
    p, m = ctypes.c_void_p(), ctypes.c_int64()   # an order that is none of the three
    assert eng._lib.hm_window_change_top(eng._ctx, cc.WA, cc.WB, cc.H3_RES, None, 3, 5, _lib.HM_MEM_HOST, ctypes.byref(p),
                                         ctypes.byref(m)) == _lib.HM_E_INVALID


@pytest.mark.parametrize("res", [cc.H3_RES, 5])
def test_view_before_ranking(overlap, res):
    from mobheat import readside
    eng, _, _ = overlap
    _, _, want = _references(eng, res)
    keep = readside.cells_in_view(want["cur"]["cell"], cc.VIEW)
    assert 0 < keep.sum() < want.size                        # the viewport cuts the set
    inside = want[keep]
    cc.same(cc.by_cell(eng.window_change(cc.WA, cc.WB, res, cc.VIEW)), inside, f"res {res}: view")
    assert eng.change_info()["in_view"] == inside.size
    for order in cc.ORDERS:
        for k in (1, 40, inside.size + 1):
            cc.same(eng.window_change(cc.WA, cc.WB, res, cc.VIEW, order, k), cc.ref_order(inside, order, k), f"res {res} view {order} k {k}")
    from mobheat import _lib
    assert _code(lambda: eng.window_change(cc.WA, cc.WB, res, (10.0, 50.0, 20.0, 40.0))) == _lib.HM_E_INVALID
    far = (100.0, -10.0, 101.0, -9.0)
    if res == cc.H3_RES and not readside.cells_in_view(want["cur"]["cell"], far).any():
        assert eng.window_change(cc.WA, cc.WB, res, far).size == 0 and eng.window_change_geojson(cc.WA, cc.WB, res, far) == cc.EMPTY


@pytest.mark.parametrize("res", [cc.H3_RES, 5])
def test_geojson(overlap, res):
    from mobheat import readside
    from mobheat.stream import _spark_datetime
    eng, _, _ = overlap
    _, _, want = _references(eng, res)
    when = (_spark_datetime(cc.WA), _spark_datetime(cc.WA + eng.tile_us))
    # every pair, in the join's order: the features of the returned pairs, which are the references' pairs
    body, pairs, offs = eng.window_change_geojson(cc.WA, cc.WB, res, with_records=True)
    cc.same(cc.by_cell(pairs), want, f"res {res}: the pairs in feature order")
    cc.check_body(body, offs, readside.tiles_change_collection(pairs, *when))
    # ranked, with and without a view: the readside collection built from two window_records calls
    for view, order, k in ((None, "rising", 25), (cc.VIEW, "abs", 400), (None, "falling", 0)):
        body, pairs, offs = eng.window_change_geojson(cc.WA, cc.WB, res, view, order, k, with_records=True)
        fc = readside.tiles_change_from_engine(eng, cc.WA, cc.WB, res, view, order, k)
        assert len(fc["features"]) == pairs.size == (min(k, want.size) if view is None else pairs.size)
        cc.check_body(body, offs, fc)
        assert bytes(readside.tiles_change_body(eng, cc.WA, cc.WB, res, view, order, k)) == cc.dumps(fc)
    assert len(cc.EMPTY) == 42 and eng.window_change_geojson(cc.WA, cc.WB, res, order="abs", k=0) == cc.EMPTY


def _close(a, b):
    return np.abs(a - b) <= np.maximum(cc.REL * np.maximum(np.abs(a), np.abs(b)), cc.ABS_DEG)


@pytest.mark.parametrize("res", [cc.H3_RES, 5])
def test_non_dyadic(res):
    """uniform-random coordinates and speeds: cells, count and n_speed exact in both halves; the sums by the closeness of
    the averages (two roll-ups of one window add in different orders)"""
    from mobheat import readside
    eng = _engine(cc.random_batch()[0])
    try:
        want = readside.change_of(eng.window_records(cc.WA, res), eng.window_records(cc.WB, res), cc.WA, cc.WB)
        got = cc.by_cell(eng.window_change(cc.WA, cc.WB, res))
        assert got.size == want.size > 20   # (the box holds a few dozen res-5 parents)
        for half in ("cur", "base"):
            g, w = got[half], want[half]
            for f in ("cell", "window_start_us", "count", "n_speed", "reserved"):
                np.testing.assert_array_equal(g[f], w[f], err_msg=f"{half} {f}")
            has = w["count"] > 0
            cnt = w["count"][has].astype(np.float64)
            for f in ("sum_lat", "sum_lon"):
                assert _close(g[f][has] / cnt, w[f][has] / cnt).all(), f"{half}: averages of {f} differ"
                assert not g[f][~has].any()
            sp = w["n_speed"] > 0
            ns = w["n_speed"][sp].astype(np.float64)
            assert _close(g["sum_speed"][sp] / ns, w["sum_speed"][sp] / ns).all(), f"{half}: average speeds differ"
            assert not g["sum_speed"][~sp].any()
        ranked = eng.window_change(cc.WA, cc.WB, res, order="rising", k=30)
        np.testing.assert_array_equal(ranked["cur"]["cell"], cc.ref_order(want, "rising", 30)["cur"]["cell"])
    finally:
        eng.close()


def test_reads_only_and_allocates_nothing_twice(overlap):
    """the change calls leave state_version and the exported state as they were; hm_window_rollup, hm_window_raster and
    hm_window_top right after one return what a fresh engine returns; a repeated call of the same size allocates nothing"""
    import raster_cases as rc
    from mobheat import readside
    eng, _, _ = overlap
    fresh = _engine(cc.shape_batch("overlap")[0])
    try:
        lat, lon = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12))
        version = eng.state_version()
        state0 = np.sort(eng.export_state()[1]).tobytes()
        keep = []
        for _ in range(2):
            c0 = eng.last_counts()
            keep.append((cc.by_cell(eng.window_change(cc.WA, cc.WB)).tobytes(), eng.window_change(cc.WA, cc.WB, 5, cc.VIEW, "abs", 100).tobytes(),
                         eng.window_change(cc.WA, cc.WB, order="rising", k=100).tobytes(),
                         bytes(eng.window_change_geojson(cc.WA, cc.WB, 5, cc.VIEW, "falling", 100))))
            c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated call allocated"
        assert keep[0] == keep[1]
        assert eng.state_version() == version and np.sort(eng.export_state()[1]).tobytes() == state0
        for ws in (cc.WA, cc.WB):
            eng.window_change(cc.WA, cc.WB, 5, order="abs", k=10)
            assert np.sort(eng.window_records(ws, 8), order="cell").tobytes() == np.sort(fresh.window_records(ws, 8), order="cell").tobytes()
            eng.window_change(cc.WA, cc.WB, 5)
            np.testing.assert_array_equal(eng.window_raster(lat, lon, ws, 8), fresh.window_raster(lat, lon, ws, 8))
            eng.window_change(cc.WA, cc.WB, 8, cc.VIEW)
            assert eng.window_top(50, ws, 5).tobytes() == fresh.window_top(50, ws, 5).tobytes()
        assert fresh.window_raster(lat, lon, cc.WA, 8).any()
        # a checkpoint export in two halves with a change call in between
        from mobheat import _lib
        info, n, recs, raw, fill = eng.export_begin(touched_only=False)
        assert eng.window_change(cc.WA, cc.WB, 3, order="rising", k=5).size == 5
        fill(0, n)
        assert np.sort(recs).tobytes() == state0
    finally:
        fresh.close()


def test_shard_context():
    from mobheat import _lib
    shard = _engine(shard=(0, 2))
    try:
        assert shard.window_change(cc.WA, cc.WB).size == 0                       # allowed: the rank's own cells
        assert shard.window_change_geojson(cc.WA, cc.WB) == cc.EMPTY
        assert _code(lambda: shard.window_change(cc.WA, cc.WB, order="abs", k=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_change_geojson(cc.WA, cc.WB, order="abs", k=5)) == _lib.HM_E_UNSUPPORTED
        assert _code(lambda: shard.window_change(cc.WA, cc.WB, order="abs", k=cc.TOP_MAX + 1)) == _lib.HM_E_INVALID   # arguments first
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
        assert _code(lambda: eng.window_change(cc.WA, cc.WB)) == _lib.HM_E_STATE
        assert _code(lambda: eng.window_change(cc.WA, cc.WB, order="abs", k=5)) == _lib.HM_E_STATE
    finally:
        eng.close()
