"""CPU: a trailing span of windows -- readside.span_of against a plain dict loop (tests/span_cases.py), the host
execution of the library's span (hm_selftest_span) against both at several resolutions, the host execution of the
encoder (hm_selftest_span_features) against json.dumps of the readside collection, the tile encoder's bytes without a
span, the minutes -> windows rounding, and that the event batches of tests/test_gpu_span.py are what they claim."""
import numpy as np
import pytest

import span_cases as sc

CASES = sc.record_cases()


@pytest.mark.parametrize("res", [8, 5, 0])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_span_of_and_host_execution(case, res):
    from mobheat import _lib, readside
    name, per, first = case
    want = sc.ref_span(per, first, res)
    sc.same(readside.span_of(per, first, sc.TILE, res), want, f"{name} res {res}: numpy against the dict loop")
    sc.same(_lib.span_selftest(per, first, sc.TILE, res), want, f"{name} res {res}: host execution against the dict loop")
    recs, series = want
    assert series.shape == (recs.size, len(per))
    assert (recs["window_start_us"] == first).all() and not recs["reserved"].any()
    for j, r in enumerate(per):   # a column is the window's own roll-up
        assert series[:, j].sum() == r["count"].sum()
        assert np.count_nonzero(series[:, j]) == np.unique(readside.cell_to_parent(r["cell"], res)).size
    if res == 8 and recs.size:
        np.testing.assert_array_equal(recs["cell"], np.unique(np.concatenate([r["cell"] for r in per])))
    if res == 0:
        assert recs.size <= 122


def test_cell_to_parent_is_the_library_s():
    from mobheat import _lib, readside
    cells = np.concatenate([r["cell"] for r in CASES[1][1]])
    for res in range(0, 9):
        out = np.zeros(cells.size, np.uint64)
        _lib.check(_lib.load().hm_selftest_cell_to_parent(_lib.ptr(cells), cells.size, res, _lib.ptr(out)), None, "parent")
        np.testing.assert_array_equal(readside.cell_to_parent(cells, res), out)
        assert [sc.parent(c, res) for c in cells[:50]] == out[:50].tolist()


def test_one_window_is_the_roll_up_and_a_gap_is_a_zero_column():
    from mobheat import _lib
    _, per, first = next(c for c in CASES if c[0] == "one window")
    recs, series = _lib.span_selftest(per, first, sc.TILE, 8)
    o = np.argsort(per[0]["cell"])
    assert recs.tobytes() == per[0][o].tobytes() and (series[:, 0] == recs["count"]).all()
    _, per, first = next(c for c in CASES if c[0] == "a gap")
    recs, series = _lib.span_selftest(per, first, sc.TILE, 5)
    assert recs.size and not series[:, 1].any() and series[:, 0].any() and series[:, 2].any()
    _, per, first = next(c for c in CASES if c[0] == "all empty")
    recs, series = _lib.span_selftest(per, first, sc.TILE, 5)
    assert recs.size == 0 and series.shape[0] == 0


def test_host_execution_arguments():
    from mobheat import _lib
    _, per, first = CASES[1]
    for bad in ([], [per[0]] * 17):
        with pytest.raises(_lib.MobheatError) as e:
            _lib.span_selftest(bad, first, sc.TILE, 5)
        assert e.value.code == _lib.HM_E_INVALID
    for res in (-1, 16):
        with pytest.raises(_lib.MobheatError) as e:
            _lib.span_selftest(per, first, sc.TILE, res)
        assert e.value.code == _lib.HM_E_INVALID
    coarse = _lib.span_selftest(per, first, sc.TILE, 3)[0]
    with pytest.raises(_lib.MobheatError) as e:   # records coarser than the target resolution have no parent there
        _lib.span_selftest([coarse], first, sc.TILE, 5)
    assert e.value.code == _lib.HM_E_INVALID


@pytest.mark.parametrize("name", ["three overlapping", "sixteen", "all empty"])
def test_feature_bytes(name):
    from mobheat import _lib
    _, per, first = next(c for c in CASES if c[0] == name)
    for res in (8, 5):
        recs, series = sc.ref_span(per, first, res)
        body, offs = _lib.span_features_selftest(recs, series, sc.WS_TEXT, sc.WE_TEXT)
        fc = sc.host_collection(recs, series)
        sc.check_body(body, offs, fc)
        for f, row in zip(fc["features"], series):
            keys = list(f["properties"])
            assert keys[-3:] == ["windowEnd", "windows", "counts"] and f["properties"]["counts"] == row.tolist()
            assert f["properties"]["windows"] == len(per) and sum(f["properties"]["counts"]) == f["properties"]["count"]


def test_large_counts_in_the_series():
    from mobheat import _lib
    _, per, first = CASES[0]
    recs, series = sc.ref_span(per, first, 8)
    recs, series = recs[:5].copy(), np.repeat(series[:5], 16, axis=1)
    series[0] = (1 << 62) + 12345
    series[1, ::2] = 0
    body, offs = _lib.span_features_selftest(recs, series, sc.WS_TEXT, sc.WE_TEXT)
    sc.check_body(body, offs, sc.host_collection(recs, series))


def test_the_tile_body_without_a_span_is_unchanged():
    """the encoder takes the span as an option: without one, the bytes are json.dumps of the plain tile collection"""
    import geojson_cases as gc
    from mobheat import _lib, readside
    _, per, first = CASES[1]
    recs, _ = sc.ref_span(per, first, 8)
    body, offs = _lib.tile_features_selftest(recs, sc.WS_TEXT, sc.WE_TEXT)
    fc = sc.host_collection(recs, np.zeros((recs.size, 1), np.int64))
    for f in fc["features"]:
        del f["properties"]["windows"], f["properties"]["counts"]
        assert list(f["properties"])[-1] == "windowEnd"
    gc.check_body(body, offs, fc)
    assert readside.SPAN_MAX_WINDOWS == _lib.HM_SPAN_MAX_WINDOWS == sc.MAX_WINDOWS


def test_minutes_round_up_to_windows():
    from mobheat import readside
    five = 5 * sc.MINUTE
    for minutes, want in ((15, 3), (14, 3), (10.5, 3), (10, 2), (5, 1), (1, 1), (0.01, 1), (80, 16), (75.5, 16)):
        assert readside.span_windows(five, minutes=minutes) == want, minutes
    assert readside.span_windows(sc.MINUTE, minutes=15) == 15 and readside.span_windows(sc.MINUTE, minutes=0.5) == 1
    assert readside.span_windows(five, windows=7) == 7
    for bad in (dict(minutes=81), dict(windows=0), dict(windows=17), dict(), dict(minutes=5, windows=1)):
        with pytest.raises(ValueError):
            readside.span_windows(five, **bad)


def test_the_batches_are_what_they_claim():
    from mobheat import _lib
    b, cells_of = sc.membership_batch()
    allc = np.unique(np.concatenate(list(cells_of.values())))
    assert 4000 < allc.size < 5500 and sorted(cells_of) == [0, 1, 2]                    # more parents than RU_FILL = 1024
    for j in cells_of:
        assert 1024 < cells_of[j].size < allc.size                                     # every window on the direct path; none holds all
    assert np.intersect1d(cells_of[0], cells_of[1]).size and np.setdiff1d(cells_of[0], cells_of[1]).size
    cell = _lib.latlng_to_cell_host_selftest(b["lat"], b["lon"], sc.H3_RES)
    w = (b["ts_us"] - sc.T0) // sc.TILE
    for j in cells_of:
        np.testing.assert_array_equal(np.unique(cell[w == j]), cells_of[j])
        _, per_cell = np.unique(cell[w == j], return_counts=True)
        assert per_cell.min() >= 1 and per_cell.max() <= 3
    assert (b["lat"] * 1024 == np.round(b["lat"] * 1024)).all() and (b["speed"] * 2 == np.round(b["speed"] * 2)).all()
    _, cells_of = sc.unequal_batch()
    assert cells_of[0].size == 4000 and cells_of[1].size == 3
    _, cells_of = sc.sparse_batch()
    assert sorted(cells_of) == list(sc.SPARSE) and sc.SPARSE[-1] - sc.SPARSE[0] + 1 == sc.MAX_WINDOWS
    b, _ = sc.random_batch()
    assert (b["lat"] * 1024 != np.round(b["lat"] * 1024)).any()
    _, cells_of = sc.pentagon_batch()
    parents0 = {sc.parent(c, 0) for c in cells_of[0]}
    assert parents0 & {sc.parent(int(c), 0) for c in _lib.latlng_to_cell_host_selftest(*_pentagons(), 0)}


def _pentagons():
    import raster_cases as rc
    pla, plo = rc.pentagon_centres()
    return np.asarray(pla, np.float64), np.asarray(plo, np.float64)
