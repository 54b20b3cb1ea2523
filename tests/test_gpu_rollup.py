"""GPU: a live window's tiles rolled up to any coarser H3 resolution (hm_live_windows / hm_window_rollup, k_rollup +
k_rollup_emit) against a numpy group-by over export_state()'s records of that window -- the checkpoint export is older,
separately tested code that shares nothing with the roll-up's kernels.

Bar: parent sets, count and n_speed bit-equal; averages within test_gpu_parity's REL = 1e-9 / ABS_DEG = 1e-12 (fp64
atomic sums in arrival order); on dyadic inputs (lat / lon / speed on binary grids: every fp64 sum is exact) the sums
bit-equal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-9
ABS_DEG = 1e-12
T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
SUMS = ("sum_speed", "sum_lat", "sum_lon")


def parent_rule(c, r):
    c = np.asarray(c, dtype=np.uint64)
    return (c & ~np.uint64(0xF << 52)) | np.uint64(r << 52) | np.uint64((1 << 3 * (15 - r)) - 1)


def expected(recs, ws, r):
    """the numpy group-by: export records of window ws grouped by their parent at resolution r, sorted by parent"""
    from mobheat._lib import STATE_REC_DTYPE
    w = recs[recs["window_start_us"] == ws]
    u, inv = np.unique(parent_rule(w["cell"], r), return_inverse=True)
    out = np.zeros(u.size, STATE_REC_DTYPE)
    out["cell"] = u
    out["window_start_us"] = ws
    for f in ("count", "n_speed"):
        a = np.zeros(u.size, np.int64)
        np.add.at(a, inv, w[f])
        out[f] = a
    for f in SUMS:
        out[f] = np.bincount(inv, weights=w[f], minlength=u.size)
    return out


def _close(a, b):
    return np.abs(a - b) <= np.maximum(REL * np.maximum(np.abs(a), np.abs(b)), ABS_DEG)


def check_rollup(got, exp, exact_sums, what=""):
    got = np.sort(got, order="cell")
    assert got.size == np.unique(got["cell"]).size, f"{what}: a parent appears twice"
    gs, es = set(got["cell"].tolist()), set(exp["cell"].tolist())
    assert gs == es, f"{what}: parent sets differ: roll-up only {len(gs - es)}, expected only {len(es - gs)}"
    for f in ("window_start_us", "count", "n_speed"):
        np.testing.assert_array_equal(got[f], exp[f], err_msg=f"{what}: {f}")
    assert not got["reserved"].any()
    if exact_sums:
        for f in SUMS:
            np.testing.assert_array_equal(got[f], exp[f], err_msg=f"{what}: {f}")
        return
    cnt = exp["count"].astype(np.float64)
    for f in ("sum_lat", "sum_lon"):
        bad = ~_close(got[f] / cnt, exp[f] / cnt)
        assert not bad.any(), f"{what}: {bad.sum()} averages of {f} differ"
    has = exp["n_speed"] > 0
    ns = exp["n_speed"][has].astype(np.float64)
    assert _close(got["sum_speed"][has] / ns, exp["sum_speed"][has] / ns).all(), f"{what}: average speeds differ"
    assert not got["sum_speed"][~has].any()


def _sphere(rng, n):
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


def _batch(rng, lat, lon, ts, null_frac=0.1, dyadic=False):
    n = lat.size
    speed = rng.integers(0, 160, n) * 0.5 if dyadic else rng.uniform(0.0, 90.0, n)
    return dict(lat=lat, lon=lon, ts_us=ts, speed=speed, speed_valid=rng.random(n) >= null_frac,
                vkey=rng.integers(0, 5000, n).astype(np.uint64), row_valid=np.ones(n, bool))


def test_every_target_resolution():
    """Engine at res 9, uniform-sphere rows plus the UDF's edge points, two windows, each rolled up to 9 (the window's
    own keys), 8, 6 (nearly one parent per key), 3, 1 and 0 (<= 122 parents: everything in the LDS tables)."""
    from mobheat import HeatmapEngine, synth
    rng = np.random.default_rng(3101)
    n = 200_000
    lat, lon = _sphere(rng, n)
    el, eo = synth.edge_points()
    lat, lon = np.r_[lat, el, el], np.r_[lon, eo, eo]
    ts = T0 + rng.integers(0, 10 * MINUTE, lat.size)
    ts[n:n + el.size] = T0 + 1_000_000            # the edge points in both windows
    ts[n + el.size:] = T0 + 5 * MINUTE + 1_000_000
    eng = HeatmapEngine(h3_res=9)
    try:
        eng.process_batch(0, **_batch(rng, lat, lon, ts))
        _, recs = eng.export_state()
        wins, keys = eng.live_windows()
        assert wins.tolist() == [T0, T0 + 5 * MINUTE]
        for ws, k in zip(wins.tolist(), keys.tolist()):
            own = recs[recs["window_start_us"] == ws]
            assert k == own.size > 90_000
            for r in (9, 8, 6, 3, 1, 0):
                got = eng.window_records(ws, r)
                exp = expected(recs, ws, r)
                check_rollup(got, exp, exact_sums=(r == 9), what=f"window {ws} res {r}")
                assert int(got["count"].sum()) == int(own["count"].sum())
                print(f"window {ws} res {r}: {own.size} keys -> {got.size} parents")
                if r == 9:   # the window's export, record for record
                    np.testing.assert_array_equal(np.sort(got, order="cell"), np.sort(own, order="cell"))
                if r == 0:
                    assert got.size <= 122
                if r == 6:
                    assert got.size > 0.9 * own.size
        # res None = h3_res, window None = the newest
        np.testing.assert_array_equal(np.sort(eng.window_records(), order="cell"),
                                      np.sort(recs[recs["window_start_us"] == T0 + 5 * MINUTE], order="cell"))
    finally:
        eng.close()


def test_lds_spill_regime_dyadic():
    """Engine at res 8, 300k rows of one window on a 1/1024-degree lattice over the sphere, rolled up to res 3: tens of
    thousands of parents (far beyond a workgroup's LDS table, far fewer than the keys) -- most records bypass the LDS
    level; every sum is exact, so the sums are bit-equal."""
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(3102)
    n = 300_000
    lat = rng.integers(-90 * 1024, 90 * 1024 + 1, n) / 1024.0
    lon = rng.integers(-180 * 1024, 180 * 1024 + 1, n) / 1024.0
    eng = HeatmapEngine(h3_res=8)
    try:
        eng.process_batch(0, **_batch(rng, lat, lon, T0 + rng.integers(0, 5 * MINUTE, n), dyadic=True))
        _, recs = eng.export_state()
        got = eng.window_records(T0, 3)
        exp = expected(recs, T0, 3)
        print(f"{recs.size} keys -> {exp.size} parents at res 3")
        assert 20_000 < exp.size < recs.size // 4
        check_rollup(got, exp, exact_sums=True, what="res 8 -> 3")
    finally:
        eng.close()


def test_output_cap_met_exactly_dyadic():
    """A window of a few thousand distinct res-8 cells rolled up at res == h3_res: every key is its own parent, so the
    output cap equals the record count and the last record lands on the last place (at < out_cap with nothing to
    spare); then at res 0, where a handful of records leave the same compaction."""
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(3108)
    n = 5000
    lat = rng.integers(-90 * 1024, 90 * 1024 + 1, n) / 1024.0
    lon = rng.integers(-180 * 1024, 180 * 1024 + 1, n) / 1024.0
    eng = HeatmapEngine(h3_res=8)
    try:
        eng.process_batch(0, **_batch(rng, lat, lon, T0 + rng.integers(0, 5 * MINUTE, n), dyadic=True))
        _, recs = eng.export_state()
        wins, keys = eng.live_windows()
        assert wins.tolist() == [T0] and keys.tolist() == [recs.size] and 3000 < recs.size <= n
        for r in (8, 0):
            got = eng.window_records(T0, r)
            exp = expected(recs, T0, r)
            assert got.size == exp.size
            check_rollup(got, exp, exact_sums=True, what=f"res 8 -> {r}")
        assert eng.window_records(T0, 8).size == recs.size and eng.window_records(T0, 0).size <= 122
    finally:
        eng.close()


def test_hot_parents_dyadic(oracle_h3):
    """300k rows on a 1/4096-degree lattice inside ONE res-2 cell (a box around the cell's centre, well inside its
    inradius), engine at res 10 (~2.6e5 keys, a table scanned by > 100 workgroups): rolled up to 2, 1 and 0 every
    record lands on one parent -- every LDS add of a workgroup on one slot, every workgroup's flush on one global slot."""
    import mobheat
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(3103)
    n = 300_000
    c2 = parent_rule(mobheat.latlng_to_cell(np.array([42.36]), np.array([-71.06]), 8), 2)
    cla, clo = oracle_h3.cell_to_latlng(c2)
    cla, clo = np.round(cla[0] * 4096) / 4096, np.round(clo[0] * 4096) / 4096
    lat = cla + rng.integers(-3072, 3073, n) / 4096.0   # +-0.75 degrees: <= 104 km from the centre, inradius ~158 km
    lon = clo + rng.integers(-3072, 3073, n) / 4096.0
    eng = HeatmapEngine(h3_res=10)
    try:
        eng.process_batch(0, **_batch(rng, lat, lon, T0 + rng.integers(0, 5 * MINUTE, n), dyadic=True))
        _, recs = eng.export_state()
        assert recs.size > 200_000 and np.unique(parent_rule(recs["cell"], 2)).tolist() == c2.tolist()
        for r in (2, 1, 0):
            got = eng.window_records(T0, r)
            assert got.size == 1 and int(got["count"][0]) == n
            check_rollup(got, expected(recs, T0, r), exact_sums=True, what=f"hot parent res {r}")
    finally:
        eng.close()


def test_null_speeds():
    """30% null speeds, and one parent (a far-away cluster) none of whose children has a speed: n_speed 0, speed_null."""
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(3104)
    n, m = 50_000, 500
    lat = np.r_[rng.uniform(42.20, 42.45, n), -30.0 + rng.uniform(0.0, 0.01, m)]
    lon = np.r_[rng.uniform(-71.20, -70.95, n), 100.0 + rng.uniform(0.0, 0.01, m)]
    b = _batch(rng, lat, lon, T0 + rng.integers(0, 5 * MINUTE, n + m), null_frac=0.3)
    b["speed_valid"][n:] = False
    eng = HeatmapEngine(h3_res=8)
    try:
        eng.process_batch(0, **b)
        _, recs = eng.export_state()
        for r in (8, 5):
            exp = expected(recs, T0, r)
            check_rollup(eng.window_records(T0, r), exp, exact_sums=(r == 8), what=f"null speeds res {r}")
            t = eng.window_tiles(T0, r)
            o = np.argsort(t.cell)
            np.testing.assert_array_equal(t.cell[o], exp["cell"])
            np.testing.assert_array_equal(t.count[o], exp["count"])
            np.testing.assert_array_equal(t.speed_null[o], exp["n_speed"] == 0)
            np.testing.assert_array_equal(t.window_end_us, t.window_start_us + eng.tile_us)
            assert not t.avg_speed[t.speed_null].any()
            has = exp["n_speed"] > 0
            assert _close(t.avg_speed[o][has], exp["sum_speed"][has] / exp["n_speed"][has]).all()
            assert _close(t.avg_lat[o], exp["sum_lat"] / exp["count"]).all()
            assert _close(t.avg_lon[o], exp["sum_lon"] / exp["count"]).all()
            far = parent_rule(recs["cell"][recs["sum_lat"] < 0], r)
            assert far.size and t.speed_null[np.isin(t.cell, far)].all() and 0 < t.speed_null.sum() < len(t)
        far5 = np.unique(parent_rule(recs["cell"][recs["sum_lat"] < 0], 5))
        exp5 = expected(recs, T0, 5)
        assert (exp5["n_speed"][np.isin(exp5["cell"], far5)] == 0).all() and far5.size <= 2
    finally:
        eng.close()


def test_table_reuse_and_growth():
    """test_gpu_parity.test_multi_batch_watermark_and_eviction's batches (eviction: released tables are reused without
    clearing; an empty batch; windows that grow into larger tables): after every batch every live window, at h3_res and
    at res 5, holds exactly the export's keys of that window -- no stale key of an evicted window, none missing."""
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(11)
    eng = HeatmapEngine(h3_res=9)
    try:
        seen = 0
        for epoch, (start_min, span_min, n) in enumerate([(0, 7, 20000), (5, 6, 20000), (0, 0, 0), (14, 9, 30000),
                                                          (1, 30, 30000), (40, 3, 5000), (0, 0, 0), (55, 2, 5000)]):
            lat = rng.uniform(37.90, 38.05, n)
            lon = rng.uniform(23.60, 23.85, n)
            ts = T0 + start_min * MINUTE + rng.integers(0, max(span_min, 1) * MINUTE, n)
            ts[: n // 50] = ts[n // 50: 2 * (n // 50)]
            eng.process_batch(epoch, lat=lat, lon=lon, ts_us=ts, speed=rng.uniform(0, 90, n), speed_valid=rng.random(n) > 0.2,
                              vkey=rng.integers(0, 500, n).astype(np.uint64), row_valid=rng.random(n) > 0.01)
            _, recs = eng.export_state()
            wins, keys = eng.live_windows()
            ew, ek = np.unique(recs["window_start_us"], return_counts=True)
            np.testing.assert_array_equal(wins, ew)
            np.testing.assert_array_equal(keys, ek)
            for ws in wins.tolist():
                for r in (9, 5):
                    check_rollup(eng.window_records(ws, r), expected(recs, ws, r), exact_sums=(r == 9),
                                 what=f"epoch {epoch} window {ws} res {r}")
            seen += wins.size
        assert seen > 8
    finally:
        eng.close()


def test_rollup_reads_only():
    """Two engines fed the same batches, one rolling every live window up between the batches: the same tiles per
    batch, n_state and final state; state_version unchanged by a roll-up; a roll-up between hm_state_export_begin and
    the copy of its dump leaves the checkpoint's records as they were."""
    from mobheat import HeatmapEngine, _lib
    from mobheat._lib import STATE_REC_DTYPE
    rng = np.random.default_rng(3106)
    a, b = HeatmapEngine(h3_res=8), HeatmapEngine(h3_res=8)
    try:
        for epoch in range(4):
            n = 40_000
            # dyadic (a 1/1024-degree lattice, half of it in a small box: keys with many rows): every sum is exact, so
            # two engines agree bit for bit whatever order their merges add in
            lat = rng.integers(-90 * 1024, 90 * 1024 + 1, n) / 1024.0
            lon = rng.integers(-180 * 1024, 180 * 1024 + 1, n) / 1024.0
            lat[: n // 2] = 42.25 + rng.integers(0, 256, n // 2) / 1024.0
            lon[: n // 2] = -71.25 + rng.integers(0, 256, n // 2) / 1024.0
            bt = _batch(rng, lat, lon, T0 + epoch * 4 * MINUTE + rng.integers(0, 4 * MINUTE, n), dyadic=True)
            ra, rb = a.process_batch(epoch, **bt), b.process_batch(epoch, **bt)

            ta, tb = ra.tiles, rb.tiles
            oa, ob = np.lexsort((ta.window_start_us, ta.cell)), np.lexsort((tb.window_start_us, tb.cell))
            for f in ("cell", "window_start_us", "count", "speed_null", "avg_speed", "avg_lon", "avg_lat"):
                np.testing.assert_array_equal(getattr(ta, f)[oa], getattr(tb, f)[ob], err_msg=f"epoch {epoch}: {f}")
            assert ra.n_state == rb.n_state
            np.testing.assert_array_equal(np.sort(ra.latest_rows), np.sort(rb.latest_rows))
            v = a.state_version()
            for ws in a.live_windows()[0].tolist():
                for r in (8, 3, 0):
                    assert a.window_records(ws, r).size > 0
            assert a.state_version() == v
        _, ea = a.export_state()
        _, eb = b.export_state()
        np.testing.assert_array_equal(np.sort(ea), np.sort(eb))
        # a checkpoint export in two halves with a roll-up in between
        info, n, recs, raw, fill = a.export_begin(touched_only=False)
        assert n == ea.size
        ws = a.live_windows()[0]
        assert a.window_records(ws[0], 2).size > 0 and a.window_records(ws[-1], 8).size > 0
        sync = np.zeros(n, STATE_REC_DTYPE)
        _lib.check(a._lib.hm_state_export_copy(a._ctx, sync.ctypes.data, 0, n), a._ctx, "hm_state_export_copy")
        fill(0, n)
        np.testing.assert_array_equal(np.sort(sync), np.sort(ea))
        np.testing.assert_array_equal(np.sort(recs), np.sort(ea))
    finally:
        a.close()
        b.close()


def test_edges():
    """An empty context, a window that is not live, resolutions outside 0..h3_res, and a repeated call's allocations."""
    from mobheat import HeatmapEngine
    from mobheat._lib import HM_E_INVALID, MobheatError
    rng = np.random.default_rng(3107)
    eng = HeatmapEngine(h3_res=7)
    try:
        ws, keys = eng.live_windows()
        assert ws.size == 0 and keys.size == 0 and ws.dtype == np.int64
        assert len(eng.window_tiles()) == 0 and len(eng.window_tiles(T0, 3)) == 0 and eng.window_records().size == 0
        n = 20_000
        lat, lon = _sphere(rng, n)
        eng.process_batch(0, **_batch(rng, lat, lon, T0 + rng.integers(0, 5 * MINUTE, n)))
        assert eng.live_windows()[0].tolist() == [T0]
        for ws_dead in (T0 - 5 * MINUTE, T0 + 5 * MINUTE, T0 + 1, 0):
            assert len(eng.window_tiles(ws_dead, 3)) == 0 and eng.window_records(ws_dead).size == 0
        for bad in (8, 16, -1):
            with pytest.raises(MobheatError) as e:
                eng.window_records(T0, bad)
            assert e.value.code == HM_E_INVALID
        first = eng.window_records(T0, 4)
        c0 = eng.last_counts()
        again = eng.window_records(T0, 4)
        c1 = eng.last_counts()
        assert (c0["allocs"], c0["frees"]) == (c1["allocs"], c1["frees"]), "a repeated roll-up allocated"
        check_rollup(again, np.sort(first, order="cell"), exact_sums=False, what="repeat")
    finally:
        eng.close()


@pytest.mark.parametrize("res", [8, 6])
def test_tiles_latest_from_engine(res):
    """The reference page's /api/tiles/latest collection served from the engine: the newest live window of the C1
    Boston batch at the engine's resolution and two levels up."""
    from mobheat import HeatmapEngine, readside, synth
    from mobheat.stream import _spark_datetime
    eng = HeatmapEngine(h3_res=8)
    try:
        eng.process_batch(0, **synth.c1_boston())
        _, recs = eng.export_state()
        newest = int(eng.live_windows()[0][-1])
        assert newest == int(recs["window_start_us"].max())
        exp = expected(recs, newest, res)
        fc = readside.tiles_latest_from_engine(eng, res=res, city="boston")
        assert fc["type"] == "FeatureCollection" and len(fc["features"]) == exp.size > 10
        feats = sorted(fc["features"], key=lambda f: int(f["properties"]["cellId"], 16))
        ids = [f["properties"]["cellId"] for f in feats]
        assert ids == [format(int(c), "x") for c in exp["cell"]]
        rings = readside.rings(ids)
        for f, ring, e in zip(feats, rings, exp):
            assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
            got = f["geometry"]["coordinates"]
            assert len(got) == 1 and got[0] == ring and ring[0] == ring[-1] and len(ring) >= 6
            p = f["properties"]
            assert p["count"] == int(e["count"])
            avg = e["sum_speed"] / e["n_speed"] if e["n_speed"] else 0.0
            assert abs(p["avgSpeedKmh"] - avg) <= max(REL * abs(avg), ABS_DEG)
            assert p["windowStart"] == _spark_datetime(newest).isoformat()
            assert p["windowEnd"] == _spark_datetime(newest + eng.tile_us).isoformat()
    finally:
        eng.close()
