"""GPU: table-mode aggregation (csrc/k_table.h k_agg + k_bin_reduce, csrc/host_batch.h phase_table) pinned at its flush,
spill and bucket edges.  The cases are tests/table_mode_cases.py's (tests/test_table_mode_cases_host.py shows on the CPU
that each means what it claims); here every batch runs through HeatmapEngine.process_batch with the table path pinned,
MOBHEAT_TEST_AGG_GRID=1 (one k_agg workgroup streams the whole batch, 1024 rows a round) and, where the case says so,
MOBHEAT_TEST_AGG_CAP (the floor of the sub-bucket capacity); bin_reduce_emits alone runs on the production grid and
capacity.  After every batch: test_gpu_parity's assert_batch_equal,
all tiles bit for bit against the oracle (the inputs are dyadic, so every sum is exact in any order; test_gpu_edges'
_same), the path taken, no more partial records than aggregated rows (the partials buffer's size), and the regime the
case exists for, read from last_counts(): agg_flushes, agg_spill_probe, agg_spill_cap, bin_spill_probe, bin_emits,
agg_cap.

Which inserts fail the 64-probe bound is the device hash's business, so identities that need none to fail are asserted
when agg_spill_probe == 0 was observed (it was, on the committed seeds: DESIGN.md lists every case's counters); then
`evicted` must equal what table_mode_cases.simulate derives from the key ids alone -- the flush threshold, the count
classes and AG_KEEP_MAX, exactly.
"""
import numpy as np
import pytest

import table_mode_cases as tmc
from test_gpu_parity import assert_batch_equal

pytestmark = pytest.mark.gpu
_ORACLE = {}
SPILLS = ("agg_spill_probe", "agg_spill_cap", "bin_spill_probe")


def _expected(name):
    """the oracle's result after each batch of a case, computed once"""
    if name not in _ORACLE:
        from oracle.spark_oracle import SparkHeatmapOracle
        c = tmc.case(name)
        ora = SparkHeatmapOracle(h3_res=c["res"])
        _ORACLE[name] = [ora.process_batch(**b) for b in c["batches"]]
    return _ORACLE[name]


def _oracle_arrays(exp):
    """the oracle's tiles as columns sorted by (cell, window), kept with the result"""
    if "_columns" not in exp:
        t = exp["tiles"]
        cell = np.array([x["cell"] for x in t], np.int64)
        w = np.array([x["window_start_us"] for x in t], np.int64)
        null = np.array([x["avg_speed"] is None for x in t], bool)
        sp = np.array([0.0 if x["avg_speed"] is None else x["avg_speed"] for x in t], np.float64)
        cols = [cell, w, np.array([x["count"] for x in t], np.int64), null, sp,
                np.array([x["avg_lon"] for x in t], np.float64), np.array([x["avg_lat"] for x in t], np.float64)]
        o = np.lexsort((w, cell))
        exp["_columns"] = [c[o] for c in cols]
    return exp["_columns"]


def _assert_tiles_exact(tiles_list, exp, what):
    """every tile of the oracle, bit for bit, by test_gpu_edges._same's rule on whole columns: NaN equals NaN and the sign
    of a zero is disregarded, which is what == on two floats says otherwise (tiles_list: one TileRows per owner)"""
    cat = lambda f, dt: np.concatenate([np.asarray(getattr(t, f)) for t in tiles_list]).astype(dt)   # noqa: E731
    g = [cat("cell", np.int64), cat("window_start_us", np.int64), cat("count", np.int64), cat("speed_null", bool),
         cat("avg_speed", np.float64), cat("avg_lon", np.float64), cat("avg_lat", np.float64)]
    o = np.lexsort((g[1], g[0]))
    g = [c[o] for c in g]
    e = _oracle_arrays(exp)
    assert g[0].size == e[0].size, f"{what}: {g[0].size} tiles, the oracle has {e[0].size}"
    assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), f"{what}: key sets differ"
    same = lambda a, b: (a == b) | ((a != a) & (b != b))   # noqa: E731
    ok = (g[2] == e[2]) & (g[3] == e[3]) & (e[3] | same(g[4], e[4])) & same(g[5], e[5]) & same(g[6], e[6])
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} tiles differ, e.g. cell {int(g[0][k]):x} window {int(g[1][k])} "
                             f"gpu {[c[k] for c in g[2:]]} oracle {[c[k] for c in e[2:]]}")


def _run(name, monkeypatch, cap=None):
    """the case's batches through a fresh engine: [(counters, result, expected)] after the common assertions"""
    from mobheat import HeatmapEngine
    c = tmc.case(name)
    exps = _expected(name)
    for k, v in tmc.env_of(c, cap).items():
        monkeypatch.setenv(k, v)
    eng = HeatmapEngine(h3_res=c["res"])
    out = []
    try:
        for k, (b, exp) in enumerate(zip(c["batches"], exps)):
            res = eng.process_batch(k, **b)
            cnt = eng.last_counts()
            what = f"case {name}{'' if cap is None else f' (cap {cap})'}, batch {k}: counters {cnt}"
            print(what)
            try:
                assert_batch_equal(res, exp)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from e
            _assert_tiles_exact([res.tiles], exp, what)
            assert cnt["table_mode"] and not cnt["binned"], what
            assert cnt["partials"] <= res.n_valid - res.n_late, what
            assert res.n_late == 0, what
            out.append((cnt, res, exp, what))
    finally:
        eng.close()
    return out


def _distinct(name, k=0):
    ids = tmc.case(name)["ids"][k]
    return int(np.unique(ids[ids >= 0]).size)


def _simulated(name, k=0):
    return tmc.simulate(tmc.case(name)["ids"][k])


def test_resident(monkeypatch):
    """3000 keys never fill the table: one final flush, one record per key into the buckets, one partial per key out"""
    (c, _, _, what), = _run("resident", monkeypatch)
    assert c["agg_flushes"] == 0 and c["bin_emits"] == 0 and all(c[s] == 0 for s in SPILLS), what
    assert c["partials"] == c["evicted"] == _distinct("resident") == 3000, what
    assert c["agg_cap"] == 4096, what


def test_flush_keeps_hot(monkeypatch):
    """the 32 hot keys stay resident across the flushes (the keep threshold, the re-insertion, FC.occ = T.occ): each
    leaves the table once, at the final flush"""
    (c, _, _, what), = _run("flush_keeps_hot", monkeypatch)
    s = _simulated("flush_keeps_hot")
    assert c["agg_flushes"] >= 2 and c["agg_flushes"] == len(s["flushes"]), what
    assert c["partials"] == s["distinct"], what
    assert c["agg_spill_cap"] == 0 and c["bin_spill_probe"] == 0 and c["bin_emits"] == 0, what
    if c["agg_spill_probe"] == 0:
        assert c["evicted"] == s["distinct"] == s["evicted"], what


def test_keep_class_over_cap(monkeypatch):
    """hist[1] = 600 > AG_KEEP_MAX and nothing heavier: nothing is kept, the recurring keys are evicted again"""
    (c, _, _, what), = _run("keep_class_over_cap", monkeypatch)
    s = _simulated("keep_class_over_cap")
    assert c["agg_flushes"] >= 2 and c["agg_flushes"] == len(s["flushes"]), what
    assert c["evicted"] > s["distinct"] and c["partials"] == s["distinct"], what
    if c["agg_spill_probe"] == 0:
        assert c["evicted"] == s["evicted"], what


def test_keep_top_class_only(monkeypatch):
    """two classes of 300 keys, 600 > AG_KEEP_MAX together: the heavy class stays, the light one goes and recurs"""
    (c, _, _, what), = _run("keep_top_class_only", monkeypatch)
    s = _simulated("keep_top_class_only")
    assert c["agg_flushes"] >= 2 and s["distinct"] < c["evicted"], what
    if c["agg_spill_probe"] == 0:
        assert c["evicted"] == s["evicted"] and c["agg_flushes"] == len(s["flushes"]) and c["partials"] == s["distinct"], what


def test_round_overflows_table(monkeypatch):
    """the 4th round brings 1024 fresh keys to 3072 of 3833 slots: at least 263 rows reach the probe bound and go out
    as partial records of their own, counted for their windows"""
    (c, res, _, what), = _run("round_overflows_table", monkeypatch)
    assert c["agg_spill_probe"] >= tmc.AG_THREADS - (tmc.AG_SLOTS - 3 * tmc.AG_THREADS), what
    assert _distinct("round_overflows_table") <= c["partials"] <= res.n_valid - res.n_late, what
    assert c["evicted"] + c["agg_spill_probe"] == 8192, what   # (every key once: a singleton is evicted or spilled)
    assert c["agg_flushes"] >= 1 and c["agg_spill_cap"] == 0, what


_SWEEP = {}


def _sweep_all():
    """bucket_cap_sweep under every capacity floor, a fresh engine each, run once: floor -> (counters, result, what) or
    the exception its run raised"""
    if not _SWEEP:
        for cap in tmc.CAP_SWEEP:
            with pytest.MonkeyPatch.context() as mp:
                try:
                    (c, res, _, what), = _run("bucket_cap_sweep", mp, cap)
                    _SWEEP[cap] = (c, res, what)
                except Exception as e:   # (reported by that capacity's test and by the test across capacities)
                    _SWEEP[cap] = e
    return _SWEEP


@pytest.mark.parametrize("cap", tmc.CAP_SWEEP)
def test_bucket_cap_sweep(cap):
    """a sub-bucket capacity from 1 record up: what does not fit (pos >= cap) is spilled, k_bin_reduce reads no more
    than cap records of a sub-bucket, and the tiles are the oracle's at every capacity"""
    r = _sweep_all()[cap]
    if isinstance(r, Exception):
        raise r
    c, res, what = r
    s = _simulated("bucket_cap_sweep")
    assert c["agg_cap"] == cap, what
    assert c["partials"] <= res.n_valid - res.n_late, what
    if cap == 1:
        assert c["agg_spill_cap"] > 0, what
        assert c["agg_spill_cap"] >= c["evicted"] - tmc.AG_BINS * 8, what   # (the sub-buckets hold 2048 records in all)
    if cap == 4096:
        assert c["agg_spill_cap"] == 0, what
    if c["agg_spill_probe"] == 0:
        assert c["evicted"] == s["evicted"], what
        # one partial per key and one more per spilled aggregate of a key that has others
        assert s["distinct"] <= c["partials"] <= s["distinct"] + c["agg_spill_cap"], what
        if c["evicted"] == s["distinct"]:
            # every key was evicted once, by one workgroup, so into one sub-bucket of its bucket: exactly what exceeds
            # `cap` records there is spilled (an off-by-one in `pos < cap` changes this by the number of full buckets)
            nb = tmc.bucket_counts(*tmc.keys_of(tmc.case("bucket_cap_sweep")["batches"][0], 9))
            assert c["agg_spill_cap"] == int(np.maximum(nb - cap, 0).sum()), what


def test_bucket_cap_sweep_across_capacities():
    """the same batch under every floor: the same aggregates are evicted whatever the capacity, and a larger capacity
    never spills more"""
    runs = _sweep_all()
    for cap, r in runs.items():
        if isinstance(r, Exception):
            raise AssertionError(f"case bucket_cap_sweep (cap {cap}) did not run: {r}") from r
    assert list(runs) == list(tmc.CAP_SWEEP)
    seen = [(cap, runs[cap][0]) for cap in tmc.CAP_SWEEP]
    what = f"case bucket_cap_sweep: {[(cap, c['evicted'], c['agg_spill_cap']) for cap, c in seen]}"
    assert len({c["evicted"] for _, c in seen}) == 1, what
    assert all(a["agg_spill_cap"] >= b["agg_spill_cap"] for (_, a), (_, b) in zip(seen, seen[1:])), what
    assert seen[0][1]["agg_spill_cap"] > 0 and seen[-1][1]["agg_spill_cap"] == 0, what


def test_cap_adapts(monkeypatch):
    """one engine under a floor of 4: a batch that fits, one that overflows its sub-buckets, and the same a minute
    later with the capacity grown to twice the fullest sub-bucket; cumulative tiles after each"""
    (a, _, _, wa), (b, _, _, wb), (c, _, _, wc) = _run("cap_adapts", monkeypatch)
    assert a["agg_cap"] == 4 and all(a[s] == 0 for s in SPILLS), wa
    assert b["agg_cap"] == 4 and b["agg_spill_cap"] > 0, wb
    assert c["agg_cap"] > 4 and c["agg_spill_cap"] == 0, wc
    assert c["evicted"] == b["evicted"] or c["agg_spill_probe"] or b["agg_spill_probe"], wc


def test_bin_reduce_emits(monkeypatch):
    """937 000 keys of one window on the production grid and capacity, about 4500 records per bucket: every bucket holds
    more keys than the table and more than four rounds of records, so k_bin_reduce emits mid-stream, goes on
    inserting into the cleared table (FreshCount restarted: FC.occ = 0), and a key whose two records lie on either side
    of the emission leaves it twice and is merged again downstream; the same keys again a minute later (each re-read
    from the state)"""
    (a, ra, _, wa), (b, rb, _, wb) = _run("bin_reduce_emits", monkeypatch)
    rec = tmc.emit_bucket_records(tmc.case("bin_reduce_emits"))
    # an emission needs more than AG_FLUSH_AT keys inserted since the last one, a bucket gets at most rec[b] records
    most = int((rec // (tmc.AG_FLUSH_AT + 1)).sum())
    assert most == tmc.AG_BINS
    for c, res, what in ((a, ra, wa), (b, rb, wb)):
        assert c["agg_flushes"] >= 1, what
        assert 1 <= c["bin_emits"] <= most, what
        assert tmc.EMIT_DISTINCT <= c["partials"] <= res.n_valid - res.n_late, what
        # k_bin_reduce's own records (the partials that are no spill) outnumber the keys there are: some key left it
        # more than once
        assert c["partials"] - sum(c[s] for s in SPILLS) > tmc.EMIT_DISTINCT, what
        if c["agg_spill_probe"] == 0:   # then every bucket got all its records, more than four rounds: one emission each
            assert c["bin_emits"] == tmc.AG_BINS and c["evicted"] <= int(rec.sum()), what
        assert c["agg_cap"] == 4096, what
    assert a["tiles"] == b["tiles"] == tmc.EMIT_DISTINCT, wb


def test_many_windows_on_spill(monkeypatch):
    """8192 keys over 300 windows, most of them leaving as spilled partials (capacity floor 1, which 8192 aggregated
    rows make a capacity of max(1, 8192 / 4096) = 2: 4096 bucket records at the very most): the census that sizes the
    window tables counts every one of them for its window"""
    (c, res, exp, what), = _run("many_windows_on_spill", monkeypatch)
    assert c["agg_cap"] == 2, what
    assert c["agg_spill_cap"] > 0 and c["agg_spill_probe"] > 0, what
    assert res.n_state == exp["n_state"] == 8192, what


def test_stage_world2(monkeypatch):
    """the round_overflows_table batch, one half per rank, through the stage API: the owners' union is the single-shard
    oracle's, and either rank's counters show its spills"""
    import mobheat
    from test_gpu_stages import _stage_batch
    sw = tmc.STAGE_WORLD2
    c = tmc.case(sw["of"])
    exp = _expected(sw["of"])[0]
    for k, v in tmc.env_of(dict(c, grid=sw["grid"], cap=sw["cap"])).items():
        monkeypatch.setenv(k, v)
    lib = mobheat.load()
    engines = [mobheat.HeatmapEngine(h3_res=c["res"]) for _ in range(sw["world"])]
    try:
        b = c["batches"][0]
        n = b["lat"].size
        bounds = [i * n // sw["world"] for i in range(sw["world"] + 1)]
        shards = [{k: v[bounds[r]:bounds[r + 1]] for k, v in b.items()} for r in range(sw["world"])]
        outs, latest, tc, _, table = _stage_batch(engines, lib, shards, 0)
        counters = [e.last_counts() for e in engines]
        what = f"case stage_world2, batch 0: counters {counters}"
        print(what)
        assert table, what
        _assert_tiles_exact(outs, exp, what)
        rows = np.sort(np.concatenate([latest[r] + bounds[r] for r in range(sw["world"])]))
        np.testing.assert_array_equal(rows, exp["latest_rows"])
        for r, cnt in enumerate(counters):
            assert cnt["table_mode"] and cnt["agg_cap"] == sw["cap"], what
            assert cnt["agg_spill_probe"] > 0 or cnt["agg_spill_cap"] > 0, what
            assert bounds[r + 1] - bounds[r] == 4096 <= sum(tc[r]) <= 4096, what   # (all singletons: one record per row)
    finally:
        for e in engines:
            e.close()
