"""CPU: the change between two windows -- readside.change_of / change_order against a plain dict join and Python's
sorted (tests/change_cases.py), the host execution of the library's join, key and ordering (hm_selftest_window_change)
against both for every order, the host execution of the encoder (hm_selftest_change_features) against json.dumps of
the readside collection, and that the event batches of tests/test_gpu_change.py are what they claim."""
import numpy as np
import pytest

import change_cases as cc

CASES = cc.record_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_join_and_orders(case):
    from mobheat import _lib, readside
    name, cur, base = case
    want = cc.ref_change(cur, base)
    assert want.size == np.union1d(cur["cell"], base["cell"]).size
    cc.same(readside.change_of(cur, base, cc.WA, cc.WB), want, f"{name}: numpy against the dict join")
    cc.same(_lib.window_change_selftest(cur, base, cc.WA, cc.WB), want, f"{name}: host execution against the dict join")
    d = want["cur"]["count"] - want["base"]["count"]
    for order in cc.ORDERS:
        for k in cc.ks_of(want.size):
            ranked = cc.ref_order(want, order, k)
            idx = readside.change_order(d, want["cur"]["cell"], order, k)
            cc.same(want[idx], ranked, f"{name} {order} k {k}: numpy against sorted")
            cc.same(readside.change_top_of(want, order, k), ranked, f"{name} {order} k {k}: change_top_of")
            cc.same(_lib.window_change_selftest(cur, base, cc.WA, cc.WB, order, k), ranked, f"{name} {order} k {k}: host execution")


def test_the_cases_tie_and_change_both_ways():
    _, cur, base = next(c for c in CASES if c[0] == "overlap")
    p = cc.ref_change(cur, base)
    d = p["cur"]["count"] - p["base"]["count"]
    assert (d > 0).any() and (d < 0).any() and (d == 0).any()
    assert np.unique(d).size < 10 < d.size                     # many ties: the cell decides
    assert np.intersect1d(d[d > 0], -d[d < 0]).size > 0        # +c and -c tie in "abs"
    ab = cc.ref_order(p, "abs", p.size)
    dd = np.abs(ab["cur"]["count"] - ab["base"]["count"])
    assert (np.diff(dd) <= 0).all()
    same_d = np.diff(dd) == 0
    assert (np.diff(ab["cur"]["cell"].astype(object))[same_d] > 0).all()


def test_zero_halves_and_arguments():
    from mobheat import _lib, readside
    _, cur, base = next(c for c in CASES if c[0] == "disjoint")
    p = _lib.window_change_selftest(cur, base, cc.WA, cc.WB)
    only_b = ~np.isin(p["cur"]["cell"], cur["cell"])
    assert only_b.sum() == base.size
    z = p["cur"][only_b]
    assert (z["window_start_us"] == cc.WA).all() and (p["base"]["window_start_us"][~only_b] == cc.WB).all()
    for f in ("count", "n_speed", "sum_speed", "sum_lat", "sum_lon", "reserved"):
        assert not z[f].any() and not p["base"][f][~only_b].any()
    assert (p["cur"]["cell"] == p["base"]["cell"]).all()
    with pytest.raises(_lib.MobheatError) as e:
        _lib.window_change_selftest(cur, base, cc.WA, cc.WA)
    assert e.value.code == _lib.HM_E_INVALID
    with pytest.raises(_lib.MobheatError) as e:
        _lib.window_change_selftest(cur, base, cc.WA, cc.WB, "rising", cc.TOP_MAX + 1)
    assert e.value.code == _lib.HM_E_INVALID
    # k < 0 on the host execution: every pair, sorted by cell
    cc.same(_lib.window_change_selftest(cur, base, cc.WA, cc.WB, "rising", -1), cc.ref_change(cur, base), "k < 0")
    with pytest.raises(ValueError):
        readside.change_order([1], [2], "sideways", 1)
    with pytest.raises(ValueError):
        readside.change_order([1], [2], "abs", cc.TOP_MAX + 1)
    with pytest.raises(ValueError):
        readside.change_of(cur, base, cc.WA, cc.WA)


def _real_cells(pairs, seed):
    """the pairs on real cells (the encoder draws their boundaries): a few of every resolution class of the GeoJSON cases"""
    import geojson_cases as gc
    from mobheat import _lib
    cells = gc.tile_cells(_lib.cells_to_boundary_host_selftest)
    pick = np.random.default_rng(seed).choice(cells, pairs.size, replace=False)
    out = pairs.copy()
    out["cur"]["cell"] = out["base"]["cell"] = pick
    return out


@pytest.mark.parametrize("name", ["overlap", "large counts", "neither", "one cell each, equal"])
def test_change_features_equal_json_dumps(name):
    from mobheat import _lib
    _, cur, base = next(c for c in CASES if c[0] == name)
    pairs = _real_cells(cc.ref_change(cur, base)[:250], 9)
    body, offs = _lib.change_features_selftest(pairs, cc.WS_TEXT, cc.WE_TEXT)
    fc = cc.host_collection(pairs)
    cc.check_body(body, offs, fc)
    for f, p in zip(fc["features"], pairs):
        pr = f["properties"]
        assert list(pr)[-3:] == ["baseCount", "baseAvgSpeedKmh", "countChange"] and list(pr)[-4] == "windowEnd"
        assert pr["countChange"] == int(p["cur"]["count"]) - int(p["base"]["count"]) == pr["count"] - pr["baseCount"]
        if p["base"]["n_speed"] == 0:
            assert pr["baseAvgSpeedKmh"] == 0.0


def test_features_without_a_base_are_unchanged():
    """the same records through the tile encoder and, as cur halves, through the change encoder: the change's features are
    the tile's with the three properties spliced in before the closing braces"""
    from mobheat import _lib
    _, cur, base = next(c for c in CASES if c[0] == "identical")
    pairs = _real_cells(cc.ref_change(cur, base)[:100], 10)
    tb, to = _lib.tile_features_selftest(pairs["cur"], cc.WS_TEXT, cc.WE_TEXT)
    cb, co = _lib.change_features_selftest(pairs, cc.WS_TEXT, cc.WE_TEXT)
    tb, cb = bytes(tb), bytes(cb)
    for i in range(pairs.size):
        t, c = tb[to[i]:to[i + 1] - 1], cb[co[i]:co[i + 1] - 1]
        assert t.endswith(b'"}}') and c.startswith(t[:-2]) and c[len(t) - 2:].startswith(b',"baseCount":')
        assert len(c) - len(t) <= 111   # GJ_BASE_MAX


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_shape_batches_are_what_they_claim(shape):
    b, a_cells, b_cells = cc.shape_batch(shape)
    assert b["lat"].size <= cc.MAX_EVENTS
    a, bb = set(a_cells.tolist()), set(b_cells.tolist())
    assert {"disjoint": not (a & bb) and a and bb, "identical": a == bb and len(a) > 2000, "a_in_b": a < bb, "b_in_a": bb < a,
            "overlap": (a & bb) and (a - bb) and (bb - a), "a_only": a and not bb, "b_only": bb and not a}[shape]
    assert max(len(a), len(bb)) > 2000   # a few thousand cells: several workgroups, several tiles of a compaction
    in_a = b["ts_us"] >= cc.WA
    assert ((b["ts_us"] >= cc.WB) & (b["ts_us"] < cc.WA + 5 * cc.MINUTE)).all()
    assert in_a.any() == bool(a) and (~in_a).any() == bool(bb)
    assert (b["lat"] * 1024 == np.round(b["lat"] * 1024)).all() and (b["speed"] * 2 == np.round(b["speed"] * 2)).all()


@pytest.mark.parametrize("n_base", [512, 4096])
def test_load_limit_batches(n_base):
    b, a_cells, b_cells = cc.load_limit_batch(n_base)
    assert b_cells.size == n_base == np.unique(b_cells).size and a_cells.size == n_base // 2
    both = np.intersect1d(a_cells, b_cells).size
    assert 0 < both < a_cells.size and b["lat"].size <= cc.MAX_EVENTS


def test_pentagon_batch_has_keys_under_pentagons():
    import geojson_cases as gc
    _, a_cells, b_cells = cc.pentagon_batch()
    for cells in (a_cells, b_cells):
        bc = (cells >> np.uint64(45)) & np.uint64(127)
        assert np.isin(bc, gc.PENTAGON_BASE_CELLS).sum() > 100
