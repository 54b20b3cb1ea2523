"""GPU: event time pinned at the window, lateness and eviction edges -- the scripted boundary scenarios of
tests/event_time_cases.py (checked against the oracle alone in tests/test_event_time_cases_host.py) through
HeatmapEngine.process_batch, every batch against the oracle with test_gpu_parity's assert_batch_equal, unchanged, and
then bit for bit (the inputs are dyadic; the sign of a zero average aside, as in test_gpu_edges).

Seven (tile_us, watermark_delay_ms) configurations under both late rules on the unpinned path; the pinned aggregation
paths of test_gpu_edges.MODES (plus the binned ingest's fused kernel and a binned batch whose slabs overflow, which
re-derives every key with k_ingest's keys-only pass) on the default, the 1 000 001 us and the one-day configuration; one
pipelined case; one stage-API case with two ranks; the state exported after an evicting batch (and after an empty one)
and imported into a fresh engine; and a hand-written known-answer table that does not go through the oracle.  Every run
also checks the device's window division: the emitted window starts are ts - ts mod tile_us of the kept rows, among
them k * tile_us - 1, k * tile_us and k * tile_us + 1 for k around 0, around 2025 and at the largest valid k.

The invariant all of this pins: batch k's eviction test and batch k + 1's late test use the same watermark and the same
`<=`, so a window never returns once evicted (the state tables' reuse rule, csrc/kernels.h at GenDesc).
"""
import numpy as np
import pytest

import event_time_cases as etc
from test_event_time_cases_host import _scenario
from test_gpu_edges import EXPECT_PATH, MODES, _same
from test_gpu_parity import assert_batch_equal

pytestmark = pytest.mark.gpu

DEFAULT, ONE_DAY, ODD_US, OFF_HOUR, HOUR = 0, 3, 6, 4, 2   # indices into etc.CONFIGS


def _engine(ci, late_prev, **kw):
    from mobheat import HeatmapEngine
    tile, delay, _ = etc.CONFIGS[ci]
    return HeatmapEngine(h3_res=etc.RES, tile_us=tile, watermark_delay_ms=delay, late_uses_prev_watermark=late_prev, **kw)


def _assert_exact(tiles, exp, what):
    """every tile of the oracle: count equal, null where the oracle's is null, the three averages bit-equal"""
    g = {(int(tiles.cell[k]), int(tiles.window_start_us[k])):
         (int(tiles.count[k]), None if tiles.speed_null[k] else float(tiles.avg_speed[k]), float(tiles.avg_lon[k]),
          float(tiles.avg_lat[k])) for k in range(len(tiles))}
    assert len(g) == len(exp["tiles"]), what
    for x in exp["tiles"]:
        got, want = g[(x["cell"], x["window_start_us"])], (x["count"], x["avg_speed"], x["avg_lon"], x["avg_lat"])
        assert got[0] == want[0] and (got[1] is None) == (want[1] is None), f"{what}: gpu {got} oracle {want}"
        assert want[1] is None or _same(got[1], want[1]), f"{what}: speed gpu {got} oracle {want}"
        assert _same(got[2], want[2]) and _same(got[3], want[3]), f"{what}: gpu {got} oracle {want}"


def _check_batch(res, cols, exp, m, tile, what):
    try:
        assert_batch_equal(res, exp)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from e
    _assert_exact(res.tiles, exp, what)
    assert (res.n_valid, res.n_late) == (m["n_valid"], m["n_late"]), what          # the hand counts
    kept = [int(t) for t in cols["ts_us"][m["kind"] == "kept"]]
    assert set(res.tiles.window_start_us.tolist()) == {t - t % tile for t in kept}, what   # the device's division
    np.testing.assert_array_equal(res.tiles.window_end_us, res.tiles.window_start_us + tile)


def _run(eng, sc, tile, what, first=0, path=None, chunks=None):
    for k in range(first, len(sc)):
        name, cols, exp, m = sc[k]
        res = eng.process_batch(k, **cols)
        _check_batch(res, cols, exp, m, tile, f"{what}, batch {k} {name}")
        c = eng.last_counts()
        if cols["lat"].size:
            if path is not None:
                assert (c["table_mode"], c["binned"]) == path, f"{what}, batch {k} {name}: path taken {c}"
            if chunks is not None:
                assert c["pipe_chunks"] == chunks, f"{what}, batch {k} {name}: {c}"


@pytest.fixture
def pin(monkeypatch):
    def _pin(env):
        for k in ("MOBHEAT_INGEST_MODE", "MOBHEAT_SUBBINS", "MOBHEAT_INGEST_WRITERS", "MOBHEAT_TEST_SLAB_CAP", "MOBHEAT_PIPELINE"):
            if env.get(k) is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, env[k])
    return _pin


CASES = [(ci, lp) for ci in range(len(etc.CONFIGS)) for lp in (True, False)]
IDS = [f"{etc.CONFIG_IDS[ci]}-{'prev' if lp else 'cur'}" for ci, lp in CASES]


@pytest.mark.parametrize("ci,late_prev", CASES, ids=IDS)
def test_boundary_scenario_unpinned(ci, late_prev, pin):
    """every configuration under both late rules on the path the engine picks itself (neither table mode nor binned)"""
    pin({})
    tile = etc.CONFIGS[ci][0]
    eng = _engine(ci, late_prev)
    try:
        _run(eng, _scenario(ci, late_prev), tile, IDS[CASES.index((ci, late_prev))], path=(False, False))
    finally:
        eng.close()


# the pinned paths: test_gpu_edges.MODES, and the two other instantiations of k_ingest's late test -- the binned ingest
# without writer waves, and the keys-only pass that completes the keys of a binned batch whose slabs overflowed (slabs
# of 4 records: the batch re-partitions, so it is not reported as binned)
PINNED = {name: ({"MOBHEAT_INGEST_MODE": mode, "MOBHEAT_SUBBINS": sub}, EXPECT_PATH[name]) for name, (mode, sub) in MODES.items()}
PINNED["binned_fused"] = ({"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_INGEST_WRITERS": "0"}, (False, True))
PINNED["binned_overflow"] = ({"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_SLAB_CAP": "4"}, None)


@pytest.mark.parametrize("ci", [DEFAULT, ODD_US, ONE_DAY], ids=lambda ci: etc.CONFIG_IDS[ci])
@pytest.mark.parametrize("mode", list(PINNED))
def test_boundary_scenario_pinned_paths(mode, ci, pin):
    env, path = PINNED[mode]
    pin(env)
    tile = etc.CONFIGS[ci][0]
    eng = _engine(ci, True)
    try:
        _run(eng, _scenario(ci, True), tile, f"mode {mode}, {etc.CONFIG_IDS[ci]}", path=path)
        if mode == "binned_overflow":   # (every batch with aggregated rows overflowed: none stayed binned)
            assert not eng.last_counts()["binned"]
    finally:
        eng.close()


def test_boundary_scenario_pipelined(pin):
    """the pipelined batch (two chunks forced at any size) at the 420 s tile"""
    pin({"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_PIPELINE": "2", "MOBHEAT_SUBBINS": "0"})
    tile = etc.CONFIGS[OFF_HOUR][0]
    eng = _engine(OFF_HOUR, True)
    try:
        _run(eng, _scenario(OFF_HOUR, True), tile, "pipelined", chunks=2)
    finally:
        eng.close()


def test_boundary_scenario_stage_api_two_ranks(pin):
    """The stage API with two ranks on one device at the one-hour tile, each batch split in halves: the union of the
    owners' tiles (bit for bit), the ranks' latest rows, the sums of n_valid / n_late / n_state and every rank's
    watermarks equal the oracle's."""
    import dataclasses

    import mobheat
    from mobheat.engine import TileRows
    from test_gpu_stages import _stage_batch
    pin({})
    tile = etc.CONFIGS[HOUR][0]
    lib = mobheat.load()
    engines = [_engine(HOUR, True) for _ in range(2)]
    try:
        for k, (name, cols, exp, m) in enumerate(_scenario(HOUR, True)):
            n = cols["lat"].size
            bounds = [0, n // 2, n]
            shards = [{f: v[bounds[r]:bounds[r + 1]] for f, v in cols.items()} for r in range(2)]
            stats = []
            outs, latest, _, _, _ = _stage_batch(engines, lib, shards, k, stats)
            what = f"stage api, batch {k} {name}"
            union = TileRows(**{f.name: np.concatenate([getattr(t, f.name) for t in outs]) for f in dataclasses.fields(TileRows)})
            keys = list(zip(union.cell.tolist(), union.window_start_us.tolist()))
            assert len(set(keys)) == len(keys), f"{what}: a key emitted by two owners"
            _assert_exact(union, exp, what)
            rows = np.sort(np.concatenate([latest[r] + bounds[r] for r in range(2)]))
            np.testing.assert_array_equal(rows, exp["latest_rows"], err_msg=what)
            assert sum(s.n_valid for s in stats) == exp["n_valid"] == m["n_valid"], what
            assert sum(s.n_late for s in stats) == exp["n_late"] == m["n_late"], what
            assert sum(s.n_state for s in stats) == exp["n_state"], what
            for s in stats:
                assert (s.watermark_ms, s.late_watermark_ms, s.batch_max_event_ms) == \
                    (exp["watermark_ms"], exp["late_watermark_ms"], exp["batch_max_event_ms"]), what
            kept = [int(t) for t in cols["ts_us"][m["kind"] == "kept"]]
            assert set(union.window_start_us.tolist()) == {t - t % tile for t in kept}, what
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("late_prev", [True, False], ids=["prev", "cur"])
@pytest.mark.parametrize("after", ["step3", "all_invalid"])
def test_checkpoint_between_eviction_and_late_test(after, late_prev, pin):
    """export_state after a batch that evicted (and after the batch without valid rows, which shifts wm_prev), imported
    into a fresh engine of the same 420 s / 123 457 ms configuration: the watermarks are the oracle's two, and the rest of
    the scenario -- whose next batch replays the evicted rows as late ones -- equals the oracle's.  An engine of another
    tile_us or delay refuses the import."""
    from mobheat import HeatmapEngine
    from mobheat._lib import MobheatError
    pin({})
    tile, delay, _ = etc.CONFIGS[OFF_HOUR]
    sc = _scenario(OFF_HOUR, late_prev)
    cut = [name for name, _, _, _ in sc].index(after) + 1
    a, b = _engine(OFF_HOUR, late_prev), _engine(OFF_HOUR, late_prev)
    others = [HeatmapEngine(h3_res=etc.RES, tile_us=tile + 1, watermark_delay_ms=delay, late_uses_prev_watermark=late_prev),
              HeatmapEngine(h3_res=etc.RES, tile_us=tile, watermark_delay_ms=delay + 1, late_uses_prev_watermark=late_prev)]
    try:
        for k in range(cut):
            name, cols, exp, m = sc[k]
            _check_batch(a.process_batch(k, **cols), cols, exp, m, tile, f"before the export, batch {k} {name}")
        info, recs = a.export_state()
        nxt = sc[cut][3]
        assert (info["watermark_ms"], info["prev_watermark_ms"]) == (nxt["wm_cur"], nxt["wm_prev"])
        assert (info["tile_us"], info["watermark_delay_ms"]) == (tile, delay)
        assert nxt["wm_cur"] > nxt["wm_prev"] or after == "all_invalid"
        assert recs.size == sc[cut - 1][2]["n_state"]
        assert sorted(set(recs["window_start_us"].tolist())) == sc[cut - 1][3]["state_windows"]
        for o in others:
            with pytest.raises(MobheatError):
                o.import_state(info, recs)
        b.import_state(info, recs)
        _run(b, sc, tile, f"after the import ({after})", first=cut, path=(False, False))
    finally:
        for e in [a, b] + others:
            e.close()


@pytest.mark.parametrize("late_prev", [True, False], ids=["prev", "cur"])
def test_known_answers_default_configuration(late_prev, pin):
    """the hand-written table (literal timestamps, verdicts and watermarks): the device against it, not the oracle"""
    from mobheat import HeatmapEngine
    pin({})
    eng = HeatmapEngine(h3_res=etc.RES, late_uses_prev_watermark=late_prev)   # tile 5 min, delay 600 000 ms: the defaults
    col = 1 if late_prev else 2
    before = (0, 0)
    try:
        for k, (cols, b) in enumerate(etc.known_answer_batches()):
            res = eng.process_batch(k, **cols)
            verdicts = [r[col] for r in b["rows"]]
            assert (res.n_valid, res.n_late) == (len(verdicts), verdicts.count("late")), f"batch {k}"
            kept = sorted({r[0] - r[0] % etc.KNOWN_TILE_US for r in b["rows"] if r[col] == "kept"})
            assert sorted(res.tiles.window_start_us.tolist()) == kept, f"batch {k}"
            assert res.watermark_ms == before[1] and res.late_watermark_ms == before[0 if late_prev else 1], f"batch {k}"
            info, _ = eng.export_state()
            before = (info["prev_watermark_ms"], info["watermark_ms"])
            assert before == b["after"], f"batch {k}"
    finally:
        eng.close()
