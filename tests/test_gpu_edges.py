"""GPU: the aggregation paths pinned at their size, value and capacity edges (HeatmapEngine.process_batch against
oracle/spark_oracle.py on identical inputs; test_gpu_parity's assert_batch_equal, unchanged).

Sizes: every pinned path (MOBHEAT_INGEST_MODE unset / direct / table / binned in sub-bins / binned in whole bins) over
batches of n = 1 .. 8193 rows on and one off the kernels' tile constants (64, 256, 512, 1024, 4096, 8192), merging into
the same two windows, with every row valid, some invalid (the first and the last among them), none valid (every row a
gap), no speed column, no speed_valid column, and the dedup's three extremes (n vehicles, one vehicle with n tied rows,
one vehicle with one latest row).

Values: a hand-placed res-5 batch whose tiles hold +-Inf, a valid speed whose bits are the record's null sentinel
(SPEED_NULL_BITS), a payload NaN, -0.0, denormals, 1.7e308, nulls, and coordinates on +-90 / +-180 / -0.0 / 5e-324.
Tiles whose fp64 sums are exact in any order (single rows, equal rows, dyadic values) are compared bit for bit -- NaN
equal to NaN, the sign of a zero average disregarded (the sink writes `x or 0.0` for the three averages, reference
heatmap_stream.py:169-171) -- the others within the project's 1e-9 relative / 1e-12 degrees.  The same state then
through export -> import -> export, the roll-up (res 5 and 3) and the GPU-encoded statements; counts around 2^31 and
2^32 through the merge, the export, the roll-up and the statements' int32 / int64.

Capacity: WREG_SLOTS = 4095 windows per batch and GMAP_SLOTS / 2 = 2048 live windows per context are refused with
HM_E_OVERFLOW before the merge begins (state_version unchanged), and the engine goes on from the state it had.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_batch_equal
from test_gpu_rollup import expected as rollup_expected

pytestmark = pytest.mark.gpu
T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
TILE = 5 * MINUTE

# name -> (MOBHEAT_INGEST_MODE, MOBHEAT_SUBBINS)
MODES = {"adaptive": (None, None), "direct": ("direct", None), "table": ("table", None), "binned_sub": ("binned", "1"),
         "binned_whole": ("binned", "0")}
# (table_mode, binned) of eng.last_counts(), from csrc/host_batch.h: a pinned mode is honoured at every n > 0
# (choose_binned / choose_table return the pin before they look at n; last_binned = the ingest binned the batch and no
# slab overflowed -- about 100 keys of at most ~100 rows each never fill a slab of >= 256 records).  Unpinned, a batch
# below BIN_MIN_ROWS = 2^22 rows is not binned and one below 2^16 aggregated rows is not a table batch.
EXPECT_PATH = {"adaptive": (False, False), "direct": (False, False), "table": (True, False), "binned_sub": (False, True),
               "binned_whole": (False, True)}


@pytest.fixture
def pin(monkeypatch):
    def _pin(mode):
        for k, v in zip(("MOBHEAT_INGEST_MODE", "MOBHEAT_SUBBINS"), MODES[mode]):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    return _pin


def _bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _from_bits(b):
    return np.array([b], np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------------------
# 1. sizes
# ---------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)
SHAPES = ("all_valid", "some_invalid", "none_valid", "no_speed", "no_speed_valid", "vkeys_distinct", "one_vkey_tied",
          "one_vkey_distinct")
_SWEEP = {}


def _sweep_batches(shape):
    """The 20 batches of one input shape: ~50 res-9 cells x the windows [T0, +5 min) and [T0 + 5 min, +10 min), ts
    inside the first 4 minutes of either (never late: the watermark stays below T0), keys repeating within a batch."""
    rng = np.random.default_rng(7100 + SHAPES.index(shape))
    out = []
    for k, n in enumerate(SIZES):
        lat = 37.90 + rng.integers(0, 50, n) * 0.01 + rng.uniform(0, 1e-4, n)
        lon = 23.70 + rng.uniform(0, 1e-4, n)
        ts = T0 + rng.integers(0, 2, n) * TILE + rng.integers(0, 4 * MINUTE, n)
        speed = rng.uniform(0, 90, n)
        sv = rng.random(n) > 0.2
        vkey = rng.integers(0, 40, n).astype(np.uint64)
        rv = np.ones(n, bool)
        if shape == "some_invalid":
            rv = rng.random(n) >= 0.05
            rv[0] = rv[-1] = False
        elif shape == "none_valid":
            rv = np.zeros(n, bool)
        elif shape == "no_speed":
            speed = sv = None
        elif shape == "no_speed_valid":
            sv = None
        elif shape == "vkeys_distinct":
            vkey = rng.permutation(n).astype(np.uint64)
        elif shape == "one_vkey_tied":
            vkey = np.full(n, 7, np.uint64)
            ts = np.full(n, T0 + (k % 2) * TILE + MINUTE, np.int64)
        elif shape == "one_vkey_distinct":
            vkey = np.full(n, 7, np.uint64)
            p = rng.permutation(n)
            ts = T0 + (p % 2) * TILE + p * 1000
        out.append(dict(lat=lat, lon=lon, ts_us=ts.astype(np.int64), speed=speed, speed_valid=sv, vkey=vkey, row_valid=rv))
    return out


def _sweep(shape):
    """(batches, the oracle's result after each): computed once per shape, shared by the modes"""
    if shape not in _SWEEP:
        from oracle.spark_oracle import SparkHeatmapOracle
        ora = SparkHeatmapOracle(h3_res=9)
        batches = _sweep_batches(shape)
        _SWEEP[shape] = (batches, [ora.process_batch(**b) for b in batches])
    return _SWEEP[shape]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", list(MODES))
def test_size_sweep(mode, shape, pin):
    """n on and one off every tile constant of k_ingest, k_ev_hist / k_ev_scatter_rec, k_rp_scatter, k_agg /
    k_bin_reduce, k_merge_owned and the dedup compaction, 20 consecutive epochs merging into the same keys: the oracle's
    tiles, latest rows and statistics after every batch, on the path the mode pins."""
    from mobheat import HeatmapEngine
    pin(mode)
    batches, exps = _sweep(shape)
    eng = HeatmapEngine(h3_res=9)
    try:
        for epoch, (b, exp) in enumerate(zip(batches, exps)):
            n = b["lat"].size
            what = f"mode {mode}, shape {shape}, n {n}"
            res = eng.process_batch(epoch, **b)
            try:
                assert_batch_equal(res, exp)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from e
            c = eng.last_counts()
            assert (c["table_mode"], c["binned"]) == EXPECT_PATH[mode], f"{what}: path taken {c}"
            if shape == "none_valid":   # n > 0 rows and no key: every row a gap
                assert len(res.tiles) == 0 and res.latest_rows.size == 0 and res.n_valid == 0, what
            elif shape in ("vkeys_distinct", "one_vkey_tied"):
                assert res.latest_rows.size == n, what
            elif shape == "one_vkey_distinct":
                assert res.latest_rows.size == 1, what
            if shape == "no_speed":
                assert res.tiles.speed_null.all(), what
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 2. values
# ---------------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
SENTINEL_BITS = 0x7FF0000000000001     # csrc/kernels.h SPEED_NULL_BITS: here the bits of a VALID speed
PAYLOAD_NAN_BITS = 0xFFF8000000000123
# label -> the tile's speeds (None = null, an int = the bits); all rows of a tile on one dyadic point
SPEED_TILES = [("inf_both", [INF, -INF]), ("inf", [INF]), ("sentinel_nan", [SENTINEL_BITS, PAYLOAD_NAN_BITS]),
               ("neg_zero", [-0.0]), ("denormal", [5e-324, 5e-324]), ("huge", [1.7e308]), ("all_null", [None] * 3),
               ("null_nan", [None, NAN]), ("null_3", [None, 3.0])]
# what the oracle gives for the first batch (run on the CPU); "n_speed" where it matters
FIRST_AVG = {"inf_both": NAN, "inf": INF, "sentinel_nan": NAN, "neg_zero": 0.0, "denormal": 5e-324, "huge": 1.7e308,
             "all_null": None, "null_nan": NAN, "null_3": 3.0}
# label -> (lat, lon) of a single row with speed 1.0
COORD_TILES = [("north_east", 90.0, 180.0), ("south_west", -90.0, -180.0), ("lat_neg_zero", -0.0, 40.0),
               ("lon_neg_zero", 45.0, -0.0), ("lat_denormal", 5e-324, 50.0), ("lon_denormal", 50.0, 5e-324),
               ("antimeridian_e", 3.0, 180.0), ("antimeridian_w", -3.0, -180.0)]
DENORMAL = ("denormal", "lat_denormal", "lon_denormal")
_EDGE = {}


def _edge_case():
    """The value-edge batch (res 5, one window), its second instalment (the same values a minute later), the oracle's
    results, and label -> set of cells.  `loose`: the cells of the one tile whose sums depend on their order."""
    if _EDGE:
        return _EDGE
    from oracle import h3_oracle
    from oracle.spark_oracle import SparkHeatmapOracle
    rng = np.random.default_rng(7200)
    lat, lon, sp, sv, label = [], [], [], [], []
    for k, (name, speeds) in enumerate(SPEED_TILES):
        for s in speeds:
            lat.append(10.5 + 2 * k)
            lon.append(20.25)
            sv.append(s is not None)
            sp.append(0 if s is None else s if isinstance(s, int) else _bits(s))
            label.append(name)
    for name, la, lo in COORD_TILES:
        lat.append(la)
        lon.append(lo)
        sv.append(True)
        sp.append(_bits(1.0))
        label.append(name)
    # (240 and 200 rows of one key: below the 258 records of a bin's slab in a batch this small, csrc/host_batch.h
    # slab_cap_for -- a key with more rows overflows its slab and the batch leaves the binned path)
    for _ in range(240):   # dyadic: multiples of 2^-10, every sum exact in any order
        lat.append(30.0 + int(rng.integers(0, 8)) / 1024)
        lon.append(60.0 + int(rng.integers(0, 8)) / 1024)
        sv.append(bool(rng.random() > 0.2))
        sp.append(_bits(int(rng.integers(0, 1 << 17)) / 1024))
        label.append("dyadic")
    for _ in range(200):   # order-dependent sums: the 1e-9 bar
        lat.append(33.0 + rng.uniform(0, 0.01))
        lon.append(63.0 + rng.uniform(0, 0.01))
        sv.append(bool(rng.random() > 0.2))
        sp.append(_bits(rng.uniform(0, 90)))
        label.append("random")
    n = len(lat)
    lat, lon = np.array(lat, np.float64), np.array(lon, np.float64)
    speed = np.array(sp, np.uint64).view(np.float64)
    assert _bits(speed[label.index("sentinel_nan")]) == SENTINEL_BITS   # (the bits survive the way into the column)
    label = np.array(label)
    cells = h3_oracle.latlng_to_cell(lat, lon, 5)
    of = {name: set(cells[label == name].tolist()) for name in np.unique(label).tolist()}
    single = [name for name in of if name not in ("dyadic", "random")]
    assert all(len(of[name]) == 1 for name in single)
    allc = [c for name in of for c in of[name]]
    assert len(allc) == len(set(allc)), "two labelled tiles share a cell"
    batches = [dict(lat=lat, lon=lon, ts_us=np.full(n, T0 + (1 + e) * MINUTE, np.int64) + np.arange(n), speed=speed,
                    speed_valid=np.array(sv, bool), vkey=np.arange(n, dtype=np.uint64), row_valid=None) for e in range(2)]
    ora = SparkHeatmapOracle(h3_res=5)
    _EDGE.update(batches=batches, exps=[ora.process_batch(**b) for b in batches], cells=of, loose=of["random"],
                 denormal={c for name in DENORMAL for c in of[name]}, ora_state=dict(ora.state))
    # the table of the issue, from the oracle itself
    first = {t["cell"]: t for t in _EDGE["exps"][0]["tiles"]}
    for name, want in FIRST_AVG.items():
        got = first[next(iter(of[name]))]["avg_speed"]
        assert (got is None) == (want is None) and (want is None or _same(got, want)), (name, got, want)
    return _EDGE


def _same(a, b):
    """bit-equal averages: NaN equals NaN, the sign of zero disregarded (`x or 0.0`)"""
    a, b = float(a) or 0.0, float(b) or 0.0
    return (a != a and b != b) or _bits(a) == _bits(b)


def _assert_batch_equal_finite(res, exp):
    """assert_batch_equal on everything but the tiles whose expected averages hold an infinity (its tolerance takes
    a - b, NaN for two equal infinities): those must be present, and the caller compares them bit for bit."""
    import dataclasses
    from mobheat.engine import TileRows
    inf = {(x["cell"], x["window_start_us"]) for x in exp["tiles"]
           if any(v is not None and np.isinf(v) for v in (x["avg_speed"], x["avg_lon"], x["avg_lat"]))}
    t = res.tiles
    sel = np.array([k in inf for k in zip(t.cell.tolist(), t.window_start_us.tolist())], bool)
    assert int(sel.sum()) == len(inf), "a tile with an infinite average is missing"
    rest = TileRows(**{f.name: getattr(t, f.name)[~sel] for f in dataclasses.fields(TileRows)})
    assert_batch_equal(dataclasses.replace(res, tiles=rest),
                       dict(exp, tiles=[x for x in exp["tiles"] if (x["cell"], x["window_start_us"]) not in inf]))
    return {c for c, _ in inf}


def _assert_exact(res, exp, cells, what):
    """the tiles of `cells`: counts equal, null where the oracle's is null, the three averages bit-equal"""
    t = res.tiles
    g = {int(t.cell[k]): (int(t.count[k]), None if t.speed_null[k] else float(t.avg_speed[k]), float(t.avg_lon[k]),
                          float(t.avg_lat[k])) for k in range(len(t))}
    seen = 0
    for x in exp["tiles"]:
        if x["cell"] not in cells:
            continue
        seen += 1
        got, want = g[x["cell"]], (x["count"], x["avg_speed"], x["avg_lon"], x["avg_lat"])
        print(f"{what}: cell {x['cell']:x} gpu {got} oracle {want}")
        assert got[0] == want[0], f"{what}: cell {x['cell']:x} gpu {got} oracle {want}"
        assert (got[1] is None) == (want[1] is None), f"{what}: cell {x['cell']:x} gpu {got} oracle {want}"
        assert want[1] is None or _same(got[1], want[1]), f"{what}: cell {x['cell']:x} speed gpu {got} oracle {want}"
        assert _same(got[2], want[2]) and _same(got[3], want[3]), f"{what}: cell {x['cell']:x} gpu {got} oracle {want}"
    assert seen == len(cells)


def _edge_engine(mode, pin):
    """a res-5 engine after the two value-edge batches on the pinned path: (engine, results, case)"""
    from mobheat import HeatmapEngine
    case = _edge_case()
    pin(mode)
    eng = HeatmapEngine(h3_res=5)
    out = []
    for epoch, (b, exp) in enumerate(zip(case["batches"], case["exps"])):
        res = eng.process_batch(epoch, **b)
        c = eng.last_counts()
        assert (c["table_mode"], c["binned"]) == EXPECT_PATH[mode], f"mode {mode}: path taken {c}"
        out.append(res)
    return eng, out, case


@pytest.mark.parametrize("mode", list(MODES))
def test_value_edges_tiles(mode, pin):
    """The oracle's tiles after each of the two batches (the second merges the same values into existing state: Inf
    into Inf, 1.7e308 into 1.7e308 -> +Inf): assert_batch_equal, then bit for bit on every tile whose sums are exact.
    The valid speed with the null sentinel's bits counts as a (NaN) speed: n_speed 2, not null."""
    eng, results, case = _edge_engine(mode, pin)
    try:
        exact = {c for name, cs in case["cells"].items() for c in cs} - case["loose"] - case["denormal"]
        for epoch, (res, exp) in enumerate(zip(results, case["exps"])):
            what = f"mode {mode}, batch {epoch}"
            try:
                infinite = _assert_batch_equal_finite(res, exp)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from e
            assert infinite and infinite <= exact
            _assert_exact(res, exp, exact, what)
        _, recs = eng.export_state()
        (c,) = case["cells"]["sentinel_nan"]
        r = recs[recs["cell"] == c]
        assert r.size == 1 and int(r["count"][0]) == 4 and int(r["n_speed"][0]) == 4 and np.isnan(r["sum_speed"][0])
        (c,) = case["cells"]["all_null"]
        r = recs[recs["cell"] == c]
        assert r.size == 1 and int(r["count"][0]) == 6 and int(r["n_speed"][0]) == 0 and _bits(r["sum_speed"][0]) == 0
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_value_edges_denormal_sums(mode, pin):
    """Sums that stay denormal (5e-324 + 5e-324 as a speed, 5e-324 as a latitude and as a longitude) keep their bits
    through the LDS and global fp64 atomics (built with -munsafe-fp-atomics): bit for bit after both batches."""
    eng, results, case = _edge_engine(mode, pin)
    try:
        for epoch, (res, exp) in enumerate(zip(results, case["exps"])):
            _assert_exact(res, exp, case["denormal"], f"mode {mode}, batch {epoch}")
    finally:
        eng.close()


def _float_fields_identical(a, b, fields, what):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        nx, ny = np.isnan(x), np.isnan(y)
        assert np.array_equal(nx, ny), f"{what}: NaNs of {f} differ"
        bad = (x.view(np.uint64) != y.view(np.uint64)) & ~nx
        assert not bad.any(), f"{what}: {f} differs in {bad.sum()} records, e.g. {x[bad][:3]} / {y[bad][:3]}"


@pytest.mark.parametrize("mode", list(MODES))
def test_value_edges_state_rollup_statements(mode, pin):
    """The state after the two value-edge batches: export -> import into a fresh engine -> export gives the same
    records (count, n_speed, the sums' bits; NaN for NaN); window_records at res 5 is the export and at res 3 the numpy
    group-by of it; the GPU's statements decoded: NaN and +-Inf kept, -0.0 and null written as 0.0."""
    import bson
    from mobheat import HeatmapEngine
    from mobheat._lib import STATE_REC_DTYPE
    eng, results, case = _edge_engine(mode, pin)
    eng2 = HeatmapEngine(h3_res=5)
    try:
        order = ["cell", "window_start_us"]
        info, recs = eng.export_state()
        recs = recs[np.argsort(recs, order=order)]
        ora = case["ora_state"]
        assert recs.size == len(ora)
        for r in recs:   # the oracle's state: counts exact, exact sums bit-equal (the sign of a zero sum aside)
            c, nsp, ssp, sla, slo = ora[(int(r["cell"]), int(r["window_start_us"]))]
            assert (int(r["count"]), int(r["n_speed"])) == (c, nsp)
            if int(r["cell"]) not in case["loose"] | case["denormal"]:
                assert _same(r["sum_speed"], ssp) and _same(r["sum_lat"], sla) and _same(r["sum_lon"], slo), (r, ora)
        eng2.import_state(info, recs)
        info2, recs2 = eng2.export_state()
        recs2 = recs2[np.argsort(recs2, order=order)]
        assert info2 == info
        for f in ("cell", "window_start_us", "count", "n_speed", "reserved"):
            np.testing.assert_array_equal(recs[f], recs2[f], err_msg=f)
        _float_fields_identical(recs, recs2, ("sum_speed", "sum_lat", "sum_lon"), f"mode {mode}: import -> export")

        # the roll-up: at the engine's own resolution the window's records, at res 3 the group-by of them
        own = eng.window_records(T0, 5)
        own = own[np.argsort(own, order=order)]
        assert own.dtype == STATE_REC_DTYPE
        for f in ("cell", "window_start_us", "count", "n_speed", "reserved"):
            np.testing.assert_array_equal(own[f], recs[f], err_msg=f)
        _float_fields_identical(own, recs, ("sum_speed", "sum_lat", "sum_lon"), f"mode {mode}: roll-up res 5")
        got = np.sort(eng.window_records(T0, 3), order="cell")
        exp = rollup_expected(recs, T0, 3)
        np.testing.assert_array_equal(got["cell"], exp["cell"])
        for f in ("window_start_us", "count", "n_speed"):
            np.testing.assert_array_equal(got[f], exp[f], err_msg=f"roll-up res 3: {f}")
        from test_gpu_rollup import parent_rule
        loose = set(parent_rule(np.array(sorted(case["loose"] | case["denormal"]), np.uint64), 3).tolist())
        ex = np.array([int(c) not in loose for c in exp["cell"]])
        for f in ("sum_speed", "sum_lat", "sum_lon"):   # (NaN equal to NaN, exact elsewhere: the inputs are dyadic)
            np.testing.assert_array_equal(got[f][ex], exp[f][ex], err_msg=f"roll-up res 3: {f}")
            np.testing.assert_allclose(got[f][~ex], exp[f][~ex], rtol=1e-9, atol=1e-12, err_msg=f"roll-up res 3: {f}")

        # the statements of the last batch
        buf, offs = eng.encode_tile_updates("ath", 45, copy=True)
        docs = {}
        for k in range(offs.size - 1):
            d = bson.decode(bytes(buf[offs[k]:offs[k + 1]]))
            assert d["multi"] is False and d["upsert"] is True
            docs[int(d["u"]["$set"]["cellId"], 16)] = d["u"]["$set"]
        exp_tiles = {x["cell"]: x for x in case["exps"][1]["tiles"]}
        assert docs.keys() == exp_tiles.keys()
        skip = case["loose"] | case["denormal"]
        for c, x in exp_tiles.items():
            u = docs[c]
            assert u["count"] == x["count"]
            lon_, lat_ = u["centroid"]["coordinates"]
            for v in (u["avgSpeedKmh"], lon_, lat_):
                assert isinstance(v, float) and _bits(v) != _bits(-0.0), (hex(c), u)
            if x["avg_speed"] is None:
                assert _bits(u["avgSpeedKmh"]) == 0, (hex(c), u)
            if c in skip:
                continue
            want = x["avg_speed"] or 0.0
            assert (u["avgSpeedKmh"] != u["avgSpeedKmh"]) == (want != want), (hex(c), u, x)
            assert want != want or _bits(u["avgSpeedKmh"]) == _bits(want), (hex(c), u, x)
            assert _bits(lon_) == _bits(x["avg_lon"] or 0.0) and _bits(lat_) == _bits(x["avg_lat"] or 0.0), (hex(c), u, x)
        speeds = {name: docs[next(iter(case["cells"][name]))]["avgSpeedKmh"] for name in FIRST_AVG}
        assert np.isnan(speeds["inf_both"]) and np.isnan(speeds["sentinel_nan"]) and np.isnan(speeds["null_nan"])
        assert speeds["inf"] == INF and speeds["huge"] == INF and speeds["null_3"] == 3.0   # (1.7e308 twice: +Inf)
        assert _bits(speeds["neg_zero"]) == 0 and _bits(speeds["all_null"]) == 0
    finally:
        eng.close()
        eng2.close()


WIDE = (2**31 - 3, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**40)
ADD = (2, 1, 1, 1, 2, 1)   # rows the batch adds: 2^31 - 1 (the last int32), 2^31, 2^31 + 1, 2^32, 2^32 + 2, 2^40 + 1


def test_wide_counts_through_merge_export_rollup_and_statements(pin):
    """Imported keys whose counts straddle 2^31 and 2^32 (n_speed equal, sums dyadic), one or two rows added to each by
    a batch: the batch's tiles, the export, the roll-up to their common res-3 parent (its count exceeds 2^32) and the
    statements' count (int32 up to 2^31 - 1, int64 above) are exact."""
    import bson
    from bson.int64 import Int64
    from mobheat import HeatmapEngine
    from mobheat._lib import STATE_REC_DTYPE
    from oracle import h3_oracle
    from oracle.spark_oracle import SparkHeatmapOracle
    from test_gpu_rollup import parent_rule
    pin("adaptive")
    # six res-5 cells under one res-3 parent, each with a dyadic point inside
    g = np.arange(-24, 25) / 64.0
    la, lo = [a.ravel() for a in np.meshgrid(10.5 + g, 20.25 + g)]
    cells = h3_oracle.latlng_to_cell(la, lo, 5)
    par = parent_rule(cells, 3)
    u, inv = np.unique(par, return_inverse=True)
    sel = np.flatnonzero(par == u[np.bincount(inv.ravel()).argmax()])
    idx = sel[np.unique(cells[sel], return_index=True)[1][:len(WIDE)]]
    assert idx.size == len(WIDE)
    la, lo, cells = la[idx], lo[idx], cells[idx]
    recs = np.zeros(len(WIDE), STATE_REC_DTYPE)
    recs["cell"], recs["window_start_us"] = cells, T0
    recs["count"] = recs["n_speed"] = WIDE
    recs["sum_speed"] = np.array(WIDE, np.float64) * 0.5
    recs["sum_lat"] = np.array(WIDE, np.float64) * la      # (exact: < 2^53 on a 2^-6 grid)
    recs["sum_lon"] = np.array(WIDE, np.float64) * lo
    eng = HeatmapEngine(h3_res=5)
    ora = SparkHeatmapOracle(h3_res=5)
    try:
        info, _ = eng.export_state()
        eng.import_state(info, recs)
        for r in recs:
            ora.state[(int(r["cell"]), T0)] = [int(r["count"]), int(r["n_speed"]), float(r["sum_speed"]),
                                               float(r["sum_lat"]), float(r["sum_lon"])]
        rows = np.repeat(np.arange(len(WIDE)), ADD)
        n = rows.size
        b = dict(lat=la[rows], lon=lo[rows], ts_us=T0 + MINUTE + np.arange(n), speed=np.full(n, 0.5),
                 speed_valid=np.ones(n, bool), vkey=np.arange(n, dtype=np.uint64), row_valid=None)
        res = eng.process_batch(int(info["epoch_id"]) + 1, **b)
        exp = ora.process_batch(**b)
        assert_batch_equal(res, exp)
        want = {int(c): w + a for c, w, a in zip(cells, WIDE, ADD)}
        assert dict(zip(res.tiles.cell.tolist(), res.tiles.count.tolist())) == want
        _assert_exact(res, exp, set(want), "wide counts")
        _, out = eng.export_state()
        assert out.size == len(WIDE)
        for r in out:
            c, nsp, ssp, sla, slo = ora.state[(int(r["cell"]), T0)]
            assert (int(r["count"]), int(r["n_speed"])) == (c, nsp) == (want[int(r["cell"])],) * 2
            assert (float(r["sum_speed"]), float(r["sum_lat"]), float(r["sum_lon"])) == (ssp, sla, slo)
        up = eng.window_records(T0, 3)
        assert up.size == 1 and int(up["cell"][0]) == int(parent_rule(cells[:1], 3)[0])
        total = sum(want.values())
        assert total > 2**32 and int(up["count"][0]) == total and int(up["n_speed"][0]) == total
        e3 = rollup_expected(out, T0, 3)
        for f in ("sum_speed", "sum_lat", "sum_lon"):   # (each sum a multiple of 2^-7 below 2^53: exact in any order)
            assert float(up[f][0]) == float(e3[f][0]), f
        buf, offs = eng.encode_tile_updates("ath", 45, copy=True)
        assert offs.size - 1 == len(WIDE)
        for k in range(offs.size - 1):
            u = bson.decode(bytes(buf[offs[k]:offs[k + 1]]))["u"]["$set"]
            cnt = want[int(u["cellId"], 16)]
            assert u["count"] == cnt and isinstance(u["count"], Int64) == (cnt > 2**31 - 1), (u, cnt)
            assert u["avgSpeedKmh"] == 0.5
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 3. capacity
# ---------------------------------------------------------------------------------------------------------
def _windows_batch(first, count, rng):
    """one row in each of `count` consecutive windows from window `first` on"""
    return dict(lat=37.9 + rng.uniform(0, 0.1, count), lon=23.7 + rng.uniform(0, 0.1, count),
                ts_us=T0 + (first + np.arange(count, dtype=np.int64)) * TILE + rng.integers(0, TILE, count),
                speed=rng.uniform(0, 90, count), speed_valid=rng.random(count) > 0.2,
                vkey=rng.integers(0, 50, count).astype(np.uint64), row_valid=None)


def _normal_batch(first_window, rng, n=3000):
    return dict(lat=37.9 + rng.uniform(0, 0.1, n), lon=23.7 + rng.uniform(0, 0.1, n),
                ts_us=T0 + first_window * TILE + rng.integers(0, 2 * TILE, n), speed=rng.uniform(0, 90, n),
                speed_valid=rng.random(n) > 0.2, vkey=rng.integers(0, 50, n).astype(np.uint64), row_valid=None)


def _refused(eng, epoch, b):
    """process_batch must raise HM_E_OVERFLOW; returns whether the state was kept (state_version unchanged
    = the call failed before its merge began)"""
    from mobheat._lib import HM_E_OVERFLOW, MobheatError
    v0 = eng.state_version()
    with pytest.raises(MobheatError) as e:
        eng.process_batch(epoch, **b)
    assert e.value.code == HM_E_OVERFLOW, e.value
    return eng.state_version() == v0


@pytest.mark.parametrize("windows", [2048, 2049, 4095, 4096, 5000])
def test_windows_in_one_batch(windows):
    """One row in each of W windows: W = 2048 (GMAP_SLOTS / 2, the most a context holds) equals the oracle; more live
    windows than the context's window map (2049, 4095) or than the batch's window registry (4096, 5000) are refused
    with HM_E_OVERFLOW, and the engine then processes a normal batch from the state it reports."""
    from mobheat import HeatmapEngine
    from oracle.spark_oracle import SparkHeatmapOracle
    rng = np.random.default_rng(7300 + windows)
    delay = 10_000 * TILE // 1000   # (no window is evicted or late here)
    eng = HeatmapEngine(h3_res=9, watermark_delay_ms=delay)
    ora = SparkHeatmapOracle(h3_res=9, watermark_delay_ms=delay)
    try:
        b = _windows_batch(0, windows, rng)
        if windows == 2048:
            res = eng.process_batch(0, **b)
            assert_batch_equal(res, ora.process_batch(**b))
            assert len(res.tiles) == windows
        elif not _refused(eng, 0, b):
            ora = SparkHeatmapOracle(h3_res=9, watermark_delay_ms=delay)   # the state was reset
        nb = _normal_batch(1, rng)
        assert_batch_equal(eng.process_batch(1, **nb), ora.process_batch(**nb))
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["adaptive", "table"])
def test_windows_accumulated_over_batches(mode, pin):
    """1500 live windows, then 600 more: the second batch would pass GMAP_SLOTS / 2 = 2048 live windows and is refused
    with HM_E_OVERFLOW; the engine goes on from the state it reports (kept: the 1500 windows; reset: none), twice --
    on the direct path (the registry's census) and in table mode (k_agg's census)."""
    from mobheat import HeatmapEngine
    from oracle.spark_oracle import SparkHeatmapOracle
    pin(mode)
    rng = np.random.default_rng(7400)
    delay = 10_000 * TILE // 1000
    eng = HeatmapEngine(h3_res=9, watermark_delay_ms=delay)
    ora = SparkHeatmapOracle(h3_res=9, watermark_delay_ms=delay)
    try:
        b = _windows_batch(0, 1500, rng)
        assert_batch_equal(eng.process_batch(0, **b), ora.process_batch(**b))
        for attempt in range(2):
            if not _refused(eng, 1 + 2 * attempt, _windows_batch(1500, 600, rng)):
                ora = SparkHeatmapOracle(h3_res=9, watermark_delay_ms=delay)
            nb = _normal_batch(1499, rng)   # (an existing window and a new one)
            res = eng.process_batch(2 + 2 * attempt, **nb)
            assert_batch_equal(res, ora.process_batch(**nb))
    finally:
        eng.close()
