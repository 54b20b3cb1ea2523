"""GPU: the read side's and the sink's streaming kernels past their first grid-stride iteration.  MOBHEAT_TEST_READ_GRID=G
(read at hm_create) runs them on at most G workgroups, so that the few thousand items of a test are several iterations of
every workgroup: what a workgroup carries from one iteration to the next -- totals in LDS, a staging buffer, compaction
bases, counters in registers -- is then exercised.  G = 1: one workgroup runs every iteration; G = 3: uneven counts.

Every call is held to (a) the reference its own feature test uses (the host executions hm_selftest_*, the restatements in
within_cases / density_cases / geojson_cases / view_cases / raster_cases, test_gpu_rollup's group-by, the Spark oracle's
state) and (b) the same call on an engine with the same contents and the knob unset.  The inputs are dyadic
(read_grid_cases), so records and bodies are equal byte for byte; there is no tolerance.  Around every call
hm_test_read_grid_info must show that the call's streaming kernels ran on lowered grids (read_grid_cases.LAUNCHES)."""
import json

import numpy as np
import pytest

import density_cases as dc
import geojson_cases as gc
import raster_cases as rc
import read_grid_cases as rg
import view_cases as vc
import within_cases as wc

pytestmark = pytest.mark.gpu
KNOB = "MOBHEAT_TEST_READ_GRID"
ZONE_SETS = ("mesh", "overlapping_squares", "circles") + wc.STAGED
SINCE = dc.T0 + 100 * dc.SEC
WEST = (-125.0, 25.0, -95.0, 49.0)   # a view that keeps thousands of the wide rows
_REF = {}


def _ref(key, make):
    """a reference computed once for both grids (never modified afterwards)"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _engine(grid=None):
    import mobheat
    with pytest.MonkeyPatch.context() as mp:
        if grid is None:
            mp.delenv(KNOB, raising=False)
        else:
            mp.setenv(KNOB, str(grid))
        return mobheat.HeatmapEngine(h3_res=8, device=0)


@pytest.fixture(scope="module")
def plain():
    eng = _engine()
    rg.load(eng)
    yield eng
    assert eng.read_grid_info() == {"launches_lowered": 0, "least_iterations": 0, "most_iterations": 0}
    eng.close()


@pytest.fixture(scope="module", params=rg.GRIDS)
def pair(request, plain):
    eng = _engine(request.param)
    assert eng.read_grid_info() == {"launches_lowered": 0, "least_iterations": 0, "most_iterations": 0}
    rg.load(eng)
    yield request.param, eng, plain
    eng.close()


def _counted(eng, grid, call, fn, **sizes):
    """fn() on the engine: exactly those of its launches (read_grid_cases.LAUNCHES[call] lists every one) whose items are
    more than `grid` workgroup iterations must have run on a lowered grid -- one fewer: a site ignored the knob; one more:
    the table misses a launch that could hide such a site.  Returns (fn's result, the kernels that had to be lowered)."""
    want = rg.lowered(call, grid, **sizes)
    before = eng.read_grid_info()["launches_lowered"]
    out = fn()
    got = eng.read_grid_info()["launches_lowered"] - before
    assert got == len(want), f"{call} at grid {grid}: {got} launches on a lowered grid, expected {len(want)}: {want} ({sizes})"
    return out, want


def _done(eng, grid):
    info = eng.read_grid_info()
    assert info["launches_lowered"] > 0 and info["least_iterations"] >= 2 and info["most_iterations"] >= info["least_iterations"], info


def _sizes(plain, res=8):
    """the items the world's kernels run over (wslots: a lower bound, a window table's load is at most 1/2)"""
    keys = int(plain.live_windows()[1][-1])
    cells = 2 + 120 * 7 ** res
    return dict(cap=plain.positions_info()["capacity"], wslots=rg.next_pow2(2 * keys),
                pslots=rg.next_pow2(max(2 * min(keys, cells), 1024)), keys=keys,
                bslots=rg.next_pow2(max(2 * len(rg.world().rows), 1024)))


def _pos(plain):
    return _ref("pos", lambda: plain.positions()[0])


def _dicts(eng):
    """the engine's positions dictionaries (its codes are its own: the order its state took the strings in)"""
    if not hasattr(eng, "_world_dicts"):
        eng._world_dicts = eng.positions()[1:]
    return eng._world_dicts


def _by_key(eng, recs, zone=None):
    """position records of `eng` (and their labels) in the order of their string pair, the codes replaced by the strings'
    ranks among the world's -- the same bytes from any engine that holds the world"""
    providers, vehicles = _dicts(eng)
    prank = {s: k for k, s in enumerate(sorted(set(r[0] for r in rg.world().rows)))}
    vrank = _ref("vrank", lambda: {s: k for k, s in enumerate(sorted(set(r[1] for r in rg.world().rows)))})
    r = recs.copy()
    r["provider"] = np.array([prank[s] for s in providers], np.int64)[recs["provider"].astype(np.int64)]
    r["vehicle"] = np.array([vrank[s] for s in vehicles], np.int64)[recs["vehicle"].astype(np.int64)]
    o = np.argsort((r["provider"].astype(np.uint64) << np.uint64(32)) | r["vehicle"].astype(np.uint64), kind="stable")
    return r[o].tobytes() if zone is None else (r[o].tobytes(), zone[o].tolist())


def _by_cell(recs, zone=None):
    o = np.argsort(recs["cell"], kind="stable")
    return recs[o].tobytes() if zone is None else (recs[o].tobytes(), zone[o].tolist())


def _features(body, offs):
    body = bytes(body)
    return sorted(body[offs[i]: offs[i + 1] - 1] for i in range(len(offs) - 1))


def test_the_state_spans_several_tiles(pair):
    """the fixture's claims: four group-by tiles of pair-table slots, live slots and in-zone vehicles of both kinds past the
    first scan tile, a window of more roll-up records than three scan tiles; both engines hold the same dictionaries"""
    from mobheat import _lib
    grid, eng, plain = pair
    s = _sizes(plain)
    assert s["cap"] >= 4 * rg.GROUP and eng.positions_info()["capacity"] == s["cap"]
    assert s["keys"] > 3 * rg.SCAN and s["wslots"] >= 4 * rg.GROUP
    (recs, prov, veh), _ = _counted(eng, grid, "positions", eng.positions, **s)
    precs, pprov, pveh = plain.positions()
    assert sorted(prov) == sorted(pprov) and sorted(veh) == sorted(pveh) and _by_key(eng, recs) == _by_key(plain, precs)
    assert recs.size == len(rg.world().rows) > 2 * rg.SCAN   # (more live slots than two tiles hold)
    if grid == 1:   # one workgroup: the emission is in slot order, so a record at index >= SCAN lies in a later tile
        late = recs[rg.SCAN:]
        for name in ("mesh", "stage_span", "triangles1025"):
            assert _lib.points_in_zones_selftest(wc.zone_set(name), late["lat"], late["lon"])[1].any(), name
    # the records are the rows
    rows = rg.world()
    want = {(p, v): (ts, np.float64(la).tobytes(), np.float64(lo).tobytes()) for p, v, ts, la, lo in rows.rows}
    got = {(prov[int(r["provider"])], veh[int(r["vehicle"])]): (int(r["ts_us"]), r["lat"].tobytes(), r["lon"].tobytes()) for r in recs}
    assert got == want
    _done(eng, grid)


@pytest.mark.parametrize("name", ZONE_SETS)
def test_positions_within(pair, name):
    from mobheat import _lib
    grid, eng, plain = pair
    zones, pos, s = wc.zone_set(name), _pos(plain), _sizes(plain)
    for since in (None, SINCE):
        what = f"{name} since {since} grid {grid}"
        want, wz, wt = _ref(("pw", name, since), lambda: _lib.positions_within_selftest(zones, pos, since))
        (got, gz, gt), n = _counted(eng, grid, "positions_within", lambda: eng.positions_within(zones, since), **s)
        info = eng.within_info()
        assert n == ["k_pos_within"] and _by_key(eng, got, gz) == _by_key(plain, want, wz), what
        wc.same_totals(gt, wt, what)
        (none, nz, only), _ = _counted(eng, grid, "positions_within", lambda: eng.positions_within(zones, since, records=False), **s)
        assert none is None and nz is None
        wc.same_totals(only, wt, what + ", totals only")
        kept = pos.size if since is None else int((pos["ts_us"] >= since).sum())
        assert (info["scanned"], info["kept_since"], info["in_zone"], info["zones"], info["vertices"]) == \
            (s["cap"], kept, want.size, zones.n_zones, zones.lat.size), info
        assert eng.within_info()["in_zone"] == want.size and 0 < want.size < kept
        pgot, pz, pt = plain.positions_within(zones, since)
        assert _by_key(plain, pgot, pz) == _by_key(eng, got, gz) and pt.tobytes() == gt.tobytes(), what + ": the knob unset"
        if name == "overlapping_squares":
            assert gt["n"].sum() > got.size
    _done(eng, grid)


@pytest.mark.parametrize("name", wc.STAGED)
def test_staged_sets_with_the_knob_unset(name):
    """the three new sets on ordinary grids: device == host execution on random, vertex and on-edge points, and == the exact
    rule wherever it decides"""
    from mobheat import _lib
    zones = wc.zone_set(name)
    la, lo = wc.random_points(wc.TILE + 1, 9)
    ela, elo = wc.edge_points(zones, stride=3)
    lat, lon = np.r_[la, zones.lat[::5], ela], np.r_[lo, zones.lon[::5], elo]
    first, hits = _lib.points_in_zones_selftest(zones, lat, lon, device=0)
    hfirst, hhits = _lib.points_in_zones_selftest(zones, lat, lon)
    assert np.array_equal(first, hfirst) and np.array_equal(hits, hhits) and hhits.any(), name
    xla, xlo = wc.random_points(60 if name.startswith("triangles") else 150, seed=23)
    efirst, ehits, decided = wc.exact(zones, xla, xlo)
    xfirst, xhits = _lib.points_in_zones_selftest(zones, xla, xlo, device=0)
    assert decided.mean() > 0.9
    assert np.array_equal(xfirst[decided], efirst[decided]) and np.array_equal(xhits[decided], ehits[decided])


@pytest.mark.parametrize("grid", rg.GRIDS)
def test_points_in_zones_and_cells_in_view(monkeypatch, grid):
    """the two context-free kernels: the knob is read by every call, the counts are the process's"""
    from mobheat import _lib
    monkeypatch.setenv(KNOB, str(grid))
    n = rg.iterating(rg.SCAN)
    lat, lon = wc.random_points(n, 31)
    for name in ZONE_SETS:
        zones = wc.zone_set(name)
        before = _lib.read_grid_info()["launches_lowered"]
        first, hits = _lib.points_in_zones_selftest(zones, lat, lon, device=0)
        assert _lib.read_grid_info()["launches_lowered"] == before + 1, name
        hfirst, hhits = _ref(("pz", name), lambda: _lib.points_in_zones_selftest(zones, lat, lon))
        assert np.array_equal(first, hfirst) and np.array_equal(hits, hhits), f"{name}: {int((hits != hhits).sum())} differ"
        assert hhits[grid * rg.SCAN:].any(), name   # a point of a later iteration is inside
    cs = vc.case_set()
    n = rg.iterating(256)
    cells = np.resize(cs.cells, n)
    for view, cells in ((vc.BOSTON, cells), (vc.BOSTON, cells[::-1].copy())):
        want = _lib.cells_in_view_selftest(cells, view)
        assert 0 < int(want[grid * 256:].sum()) < n - grid * 256
        for memory in (_lib.HM_MEM_HOST, _lib.HM_MEM_DEVICE):
            before = _lib.read_grid_info()["launches_lowered"]
            got = vc.device_cells_in_view(cells, view, memory)
            assert _lib.read_grid_info()["launches_lowered"] == before + 1
            np.testing.assert_array_equal(got, want, err_msg=f"{view} memory {memory}")
    info = _lib.read_grid_info()
    assert info["least_iterations"] >= 2
    monkeypatch.delenv(KNOB)
    before = info["launches_lowered"]
    np.testing.assert_array_equal(vc.device_cells_in_view(cells, vc.BOSTON, _lib.HM_MEM_HOST), _lib.cells_in_view_selftest(cells, vc.BOSTON))
    assert _lib.read_grid_info()["launches_lowered"] == before   # unset: the grid as without the knob


@pytest.mark.parametrize("res", (8, 5))
def test_window_within(pair, res):
    from mobheat import _lib
    grid, eng, plain = pair
    ws = int(plain.live_windows()[0][-1])
    recs = _ref(("wr", res), lambda: plain.window_records(ws, res))
    s = dict(_sizes(plain, res), g=recs.size)
    assert recs.size > 3 * rg.SCAN   # (k_within_tiles iterates at either grid, at res 5 too)
    for name in ZONE_SETS:
        zones, what = wc.zone_set(name), f"{name} res {res} grid {grid}"
        want, wz, wt = _ref(("ww", name, res), lambda: _lib.tiles_within_selftest(zones, recs))
        (got, gz, gt), n = _counted(eng, grid, "window_within", lambda: eng.window_within(zones, ws, res), **s)
        info = eng.within_info()
        assert n == ["k_rollup", "k_rollup_emit", "k_within_tiles"] and _by_cell(got, gz) == _by_cell(want, wz), what
        wc.same_totals(gt, wt, what)
        assert not gt["newest_us"].any() and want.size > 0
        assert (info["scanned"], info["kept_since"], info["in_zone"], info["zones"], info["vertices"]) == \
            (recs.size, recs.size, want.size, zones.n_zones, zones.lat.size), info
        (_, _, only), _ = _counted(eng, grid, "window_within", lambda: eng.window_within(zones, ws, res, records=False), **s)
        wc.same_totals(only, wt, what + ", totals only")
        pgot, pz, pt = plain.window_within(zones, ws, res)
        assert _by_cell(pgot, pz) == _by_cell(got, gz) and pt.tobytes() == gt.tobytes(), what + ": the knob unset"
    if grid == 1 and res == 8:   # one workgroup: ru_out is in slot order, and a tile of a later iteration is inside
        late = eng.window_records(ws, 8)[rg.SCAN:]
        for name in ("mesh", "stage_end"):
            assert _lib.tiles_within_selftest(wc.zone_set(name), late)[0].size > 0, name
    _done(eng, grid)


def test_within_bodies(pair):
    from mobheat import readside
    grid, eng, plain = pair
    zones, s = wc.mesh(), _sizes(plain)
    want = _ref("pwb", lambda: sorted(gc.dumps(f) for f in readside.positions_within_from_engine(plain, zones)["features"]))
    (body, recs, offs), n = _counted(eng, grid, "positions_within_geojson", lambda: eng.positions_within_geojson(zones, with_records=True),
                                     kept=len(want), **s)
    assert n[-4:] == ["k_pos_within", "k_gj_pos_sizes", "k_scan_add", "k_gj_pos_write"] and len(n) == 8
    assert _features(body, offs) == want and recs.size == len(want) > 3 * 256
    assert bytes(body).startswith(gc.PREFIX + b"{") and bytes(body).count(gc.PREFIX) == 1 and bytes(body).endswith(b"}]}")
    pbody, precs, poffs = plain.positions_within_geojson(zones, with_records=True)
    assert _features(pbody, poffs) == want and len(pbody) == len(body)
    assert b'"provider":"q\\"\\\\"' in bytes(body) and b"w\\n" in bytes(body)
    ws = int(plain.live_windows()[0][-1])
    for res in (8, 5):
        pbody, precs, poffs = plain.window_within_geojson(zones, ws, res, with_records=True)
        sw = dict(_sizes(plain, res), g=_ref(("wr", res), lambda: plain.window_records(ws, res)).size, kept=precs.size)
        (body, recs, offs), n = _counted(eng, grid, "window_within_geojson",
                                         lambda: eng.window_within_geojson(zones, ws, res, with_records=True), **sw)
        assert n[:3] == ["k_rollup", "k_rollup_emit", "k_within_tiles"] and (res != 8 or ("k_gj_tile_write" in n and precs.size > 3 * rg.GJ_THREADS))
        assert _features(body, offs) == _features(pbody, poffs) and _by_cell(recs) == _by_cell(precs) and recs.size > 0
        want = readside.tiles_within_from_engine(plain, zones, res)
        key = lambda c: sorted((f["properties"]["cellId"], f["properties"]["count"], f["properties"]["windowStart"],
                                gc.dumps(f["geometry"])) for f in c["features"])
        assert key(json.loads(bytes(body))) == key(want), f"res {res}"
    _done(eng, grid)


@pytest.mark.parametrize("res", (8, 2))
def test_density(pair, res):
    """res 8: more cells than a workgroup's LDS table takes (it spills); res 2: a few dozen cells, each held in LDS across
    every iteration of its workgroup and added to the global table once per workgroup"""
    from mobheat import _lib, readside
    grid, eng, plain = pair
    pos, s = _pos(plain), _sizes(plain)
    for since in (None, SINCE):
        what = f"res {res} since {since} grid {grid}"
        want, bad = _ref(("de", res, since), lambda: dc.expected(pos, res, since))
        host, _ = _ref(("dh", res, since), lambda: _lib.positions_density_selftest(pos, res, since))
        dslots = rg.next_pow2(max(2 * min(pos.size, 2 + 120 * 7 ** res), 1024))
        got, n = _counted(eng, grid, "positions_density", lambda: eng.positions_density(res, since), dslots=dslots, **s)
        info = eng.positions_density_info()
        assert n == ["k_density_cells", "k_density_group", "k_density_emit"]
        dc.check(got, want, True, what + ": device against the oracle")
        dc.check(host, want, True, what + ": host execution against the oracle")
        kept = int((pos["ts_us"] >= (dc.INT64_MIN if since is None else since)).sum())
        assert (info["keys"], info["kept"], info["unsnapped"], info["groups"], info["returned"]) == (pos.size, kept, bad, want.size, want.size)
        assert _by_cell(plain.positions_density(res, since)) == _by_cell(got), what + ": the knob unset"
        assert info["workgroups"] == min(grid, s["cap"] // rg.GROUP)
        if res == 8:
            assert want.size > rg.RU_FILL and info["global_adds"] > rg.RU_FILL, info   # the LDS table spills
        else:
            assert want.size < rg.RU_FILL // 4
            assert want.size <= info["global_adds"] <= info["workgroups"] * want.size, info   # held across the iterations
            if grid == 1:
                assert info["global_adds"] == want.size, info
    # with a view
    want, _ = _ref(("de", res, None), lambda: dc.expected(pos, res, None))
    for view in (vc.BOSTON, WEST):
        kept = _ref(("dv", res, view), lambda: dc.in_view(want, res, view))
        dslots = rg.next_pow2(max(2 * min(pos.size, 2 + 120 * 7 ** res), 1024))
        got, n = _counted(eng, grid, "positions_density_view", lambda: eng.positions_density(res, None, view), dslots=dslots,
                          groups=want.size, **s)
        assert ("k_view_tiles" in n) == (res == 8)   # (res 2: fewer groups than one iteration takes)
        dc.check(got, kept, True, f"res {res} view {view} grid {grid}")
        assert 0 < kept.size < want.size and eng.positions_density_info()["returned"] == kept.size
        assert _by_cell(plain.positions_density(res, None, view)) == _by_cell(got)
    # the raster of the density
    lat, lon = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12))
    thr = readside.COUNT_THRESHOLDS
    dens = eng.positions_density(res, SINCE)
    (counts, classes), n = _counted(eng, grid, "positions_density_raster", lambda: eng.positions_density_raster(lat, lon, res, SINCE, thr),
                                    units=lat.size * ((lon.size + 63) // 64), dslots=dslots, **s)
    hc, hk = _lib.window_raster_selftest(dens, res, lat, lon, thr)
    np.testing.assert_array_equal(counts, hc)
    np.testing.assert_array_equal(classes, hk)
    pc, pk = plain.positions_density_raster(lat, lon, res, SINCE, thr)
    assert n[-1] == "k_raster" and len(n) == 4 and counts.any() and np.array_equal(pc, counts) and np.array_equal(pk, classes)
    _done(eng, grid)


def test_views_of_the_bodies(pair):
    from test_gpu_view import _ref_filter, _window_collection
    from mobheat import readside
    grid, eng, plain = pair
    ws = int(plain.live_windows()[0][-1])
    cand = _ref(("wr", 8), lambda: plain.window_records(ws, 8))
    for view in (vc.BOSTON, WEST):
        want = _ref(("vf", view), lambda: _ref_filter(cand, 8, view))
        s = dict(_sizes(plain), g=cand.size, kept=want.size)
        (body, recs, offs), n = _counted(eng, grid, "window_geojson_view", lambda: eng.window_geojson(ws, 8, with_records=True, view=view), **s)
        assert n[:3] == ["k_rollup", "k_rollup_emit", "k_view_tiles"] and _by_cell(recs) == _by_cell(want) and 0 < recs.size < cand.size, view
        assert len(n) == 6 or view != WEST   # (the encoders iterate on what the wide view kept)
        assert eng.geojson_info()["candidates"] == cand.size
        gc.check_body(body, offs, _window_collection(eng, recs, ws))
        pbody, precs, poffs = plain.window_geojson(ws, 8, with_records=True, view=view)
        assert _features(body, offs) == _features(pbody, poffs), view
    assert _ref(("vf", WEST), lambda: None).size > 3 * 256   # the encoders iterate on what the view kept
    # the positions body with a view
    ref = _ref("plf", lambda: readside.positions_latest_from_engine(plain))
    by_key = _ref("plk", lambda: {(f["properties"]["provider"], f["properties"]["vehicleId"]): f for f in ref["features"]})
    providers, vehicles = _dicts(eng)
    for view in (vc.BOSTON, WEST):
        want = {k for k, f in by_key.items() if vc.ref_point(f["geometry"]["coordinates"][1], f["geometry"]["coordinates"][0], view)}
        s = dict(_sizes(plain), kept=len(want))
        (body, recs, offs), n = _counted(eng, grid, "positions_geojson_view", lambda: eng.positions_geojson(with_records=True, view=view), **s)
        assert n[4] == "k_pos_emit_view" and (len(n) == 8 or view != WEST)
        got = [(providers[int(r["provider"])], vehicles[int(r["vehicle"])]) for r in recs]
        assert set(got) == want and len(got) == len(want) and 0 < len(got) < len(by_key), view
        gc.check_body(body, offs, {"type": "FeatureCollection", "features": [by_key[k] for k in got]})
        pbody, _, poffs = plain.positions_geojson(with_records=True, view=view)
        assert _features(body, offs) == _features(pbody, poffs), view
    _done(eng, grid)


def test_rollup_records_and_exports(pair):
    from oracle.spark_oracle import SparkHeatmapOracle
    from test_gpu_rollup import check_rollup, expected
    grid, eng, plain = pair
    ws = int(plain.live_windows()[0][-1])
    (dinfo, touched), n = _counted(eng, grid, "export_state_delta", eng.export_state_delta, **_sizes(plain))
    ptouched = plain.export_state_delta()[1].copy()
    assert n == ["k_dump_gen"]
    (info, recs), n = _counted(eng, grid, "export_state", eng.export_state, **_sizes(plain))
    pinfo, precs = plain.export_state()
    assert n == ["k_dump_gen"] and info == pinfo and _by_cell(recs) == _by_cell(precs) and recs.size == _sizes(plain)["keys"]

    def oracle_state():
        ora = SparkHeatmapOracle(h3_res=8)
        ora.process_batch(**rg.batch_columns())
        return ora.state
    state = _ref("ora", oracle_state)
    assert len(state) == recs.size and not recs["reserved"].any()
    for r in recs:   # dyadic inputs: the sums themselves
        assert tuple(state[(int(r["cell"]), int(r["window_start_us"]))]) == (int(r["count"]), int(r["n_speed"]), float(r["sum_speed"]),
                                                                      float(r["sum_lat"]), float(r["sum_lon"]))
    assert _by_cell(touched) == _by_cell(recs) == _by_cell(ptouched)   # the one batch touched every key
    for res in (8, 5, 0):
        got, n = _counted(eng, grid, "window_records", lambda: eng.window_records(ws, res), **_sizes(plain, res))
        assert n == ["k_rollup", "k_rollup_emit"][:1 + (res > 0)]
        check_rollup(got, expected(recs, ws, res), exact_sums=True, what=f"res {res} grid {grid}")
        assert _by_cell(plain.window_records(ws, res)) == _by_cell(got)
        assert int(got["count"].sum()) == len(rg.world().rows)
    _done(eng, grid)


def test_geojson_bodies(pair):
    from test_gpu_view import _window_collection
    from mobheat import _lib, readside
    grid, eng, plain = pair
    n = rg.iterating(rg.GJ_THREADS)
    recs = gc.tile_records(np.resize(gc.tile_cells(_lib.cells_to_boundary_host_selftest), n))
    hb, ho = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    for memory in (_lib.HM_MEM_HOST, _lib.HM_MEM_DEVICE):
        (body, offs), k = _counted(eng, grid, "encode_tile_features", lambda: eng.encode_tile_features(recs, gc.WS_TEXT, gc.WE_TEXT, memory), n=n)
        np.testing.assert_array_equal(offs, ho)
        assert "k_gj_tile_write" in k and (len(k) == 3) == (grid == 1) and body == hb.tobytes(), f"memory {memory}"
        # the prefix once, in front of the first feature; the closing bytes behind the last one, a later iteration's
        assert int(offs[0]) == len(gc.PREFIX) and body[:offs[0]] == gc.PREFIX and body.count(gc.PREFIX) == 1
        assert int(offs[-1]) == len(body) - 1 and body.endswith(b"}]}") and n - 1 >= grid * rg.GJ_THREADS
        pbody, poffs = plain.encode_tile_features(recs, gc.WS_TEXT, gc.WE_TEXT, memory)
        assert pbody == body and np.array_equal(poffs, offs)
    ws = int(plain.live_windows()[0][-1])
    for res in (8, 5):
        cand = _ref(("wr", res), lambda: plain.window_records(ws, res))
        s = dict(_sizes(plain, res), g=cand.size)
        (body, wrecs, offs), k = _counted(eng, grid, "window_geojson", lambda: eng.window_geojson(ws, res, with_records=True), **s)
        assert len(k) == 5 and cand.size > 3 * 256 and _by_cell(wrecs) == _by_cell(cand)
        gc.check_body(body, offs, _window_collection(eng, wrecs, ws))
        pbody, _, poffs = plain.window_geojson(ws, res, with_records=True)
        assert _features(body, offs) == _features(pbody, poffs), f"res {res}"
    # the positions body: dictionaries with strings that need escaping
    ref = _ref("plf", lambda: readside.positions_latest_from_engine(plain))
    by_key = _ref("plk", lambda: {(f["properties"]["provider"], f["properties"]["vehicleId"]): f for f in ref["features"]})
    providers, vehicles = _dicts(eng)
    s = dict(_sizes(plain), kept=len(by_key))
    ids, k = _counted(eng, grid, "positions_buckets", eng.positions_buckets, **s)
    np.testing.assert_array_equal(ids, np.unique(_pos(plain)["ts_us"] // 1_000_000 // 900))
    assert k == 2 * ["k_fill_i64", "k_gj_pos_buckets"]
    (body, precs, offs), k = _counted(eng, grid, "positions_geojson", lambda: eng.positions_geojson(with_records=True), **s)
    assert k[4:] == ["k_pos_emit", "k_gj_pos_sizes", "k_scan_add", "k_gj_pos_write"] and precs.size == len(by_key)
    ordered = [by_key[(providers[int(r["provider"])], vehicles[int(r["vehicle"])])] for r in precs]
    gc.check_body(body, offs, {"type": "FeatureCollection", "features": ordered})
    assert b'"provider":"q\\"\\\\"' in bytes(body) and b'"vehicleId":"w\\n1' in bytes(body)
    pbody, _, poffs = plain.positions_geojson(with_records=True)
    assert _features(body, offs) == _features(pbody, poffs)
    _done(eng, grid)


def test_window_raster(pair):
    from mobheat import _lib, readside
    grid, eng, plain = pair
    ws = int(plain.live_windows()[0][-1])
    lat, lon = readside.tile_grid(12, *rc.tile_of(42.33, -71.07, 12), size=257)
    lon = lon[:65]
    thr = readside.COUNT_THRESHOLDS
    for res in (8, 5):
        recs = _ref(("wr", res), lambda: plain.window_records(ws, res))
        (counts, classes), n = _counted(eng, grid, "window_raster", lambda: eng.window_raster(lat, lon, ws, res, thr), units=257 * 2,
                                        **_sizes(plain, res))
        hc, hk = _lib.window_raster_selftest(recs, res, lat, lon, thr)
        ec, ek = rc.expected(recs, res, lat, lon, thr)
        for what, c, k in (("host execution", hc, hk), ("oracle", ec, ek), ("knob unset", *plain.window_raster(lat, lon, ws, res, thr))):
            np.testing.assert_array_equal(counts, c, err_msg=f"res {res}: counts differ from the {what}")
            np.testing.assert_array_equal(classes, k, err_msg=f"res {res}: classes differ from the {what}")
        assert n == ["k_rollup", "k_rollup_emit", "k_raster"] and counts.shape == (257, 65) and counts.any()
    _done(eng, grid)


@pytest.mark.parametrize("grid", rg.GRIDS)
def test_sink_statements(grid):
    """the batch's tile and position statements at 2 * 3 * TD_THREADS - 5 and 2 * 3 * 256 - 5 of them; a CITY of 330 bytes
    takes the unstaged encoder (k_tile_docs_direct)"""
    from mobheat import _lib
    eng, plain = _engine(grid), _engine()
    try:
        for epoch, n in enumerate((rg.iterating(rg.TD_THREADS), rg.iterating(256))):
            b = rg.spaced_batch(n, seed=epoch)
            b["ts_us"] = b["ts_us"] + epoch * 3600 * dc.SEC
            res, pres = eng.process_batch(epoch, **b), plain.process_batch(epoch, **b)
            assert len(res.tiles) == n == res.latest_rows.size
            for city in ("ath", "greater-" * 40 + "αθήνα"):
                call = "tile_updates" if city == "ath" else "tile_updates_direct"
                (buf, offs), k = _counted(eng, grid, call, lambda: eng.encode_tile_updates(city, 45, copy=True), n=n)
                hb, ho = _lib.tile_statements_selftest(res.tiles, city, 8, 45, eng.tile_us)
                np.testing.assert_array_equal(offs, ho)
                np.testing.assert_array_equal(buf, hb)
                assert (len(k) == 3 if n > 3 * 256 or grid == 1 else k == ["k_tile_docs"][:city == "ath"]) and offs.size == n + 1
                pbuf, poffs = plain.encode_tile_updates(city, 45, copy=True)
                split = lambda x, o: sorted(x[o[i]:o[i + 1]].tobytes() for i in range(o.size - 1))
                assert split(buf, offs) == split(pbuf, poffs)
            providers, vehicles = ["p"], [f"v{k}" for k in range(n)]
            rows = res.latest_rows
            (buf, offs), k = _counted(eng, grid, "position_updates", lambda: eng.encode_position_updates(providers, vehicles, b["ts_us"][rows], copy=True), n=n)
            hb, ho = _lib.position_statements_selftest(providers, vehicles, b["vkey"][rows], b["ts_us"][rows], b["lat"][rows], b["lon"][rows])
            np.testing.assert_array_equal(offs, ho)
            np.testing.assert_array_equal(buf, hb)
            assert (len(k) == 3) == (n > 3 * 256 or grid == 1) and offs.size == n + 1
            pbuf, poffs = plain.encode_position_updates(providers, vehicles, b["ts_us"][pres.latest_rows], copy=True)
            assert np.array_equal(pres.latest_rows, rows) and pbuf.tobytes() == buf.tobytes() and np.array_equal(poffs, offs)
        _done(eng, grid)
        assert plain.read_grid_info()["launches_lowered"] == 0
    finally:
        eng.close()
        plain.close()
