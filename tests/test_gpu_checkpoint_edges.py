"""GPU: the tile-state checkpoint pinned at its size, order and restore edges (tests/checkpoint_cases.py; its cases are
checked against the oracle alone in tests/test_checkpoint_cases_host.py).

hm_state_export, hm_state_export_touched, hm_state_export_begin / _copy / _copy_async / _copy_wait and hm_state_import
(csrc/api_state.h), with k_dump_gen and the rehash merge under them, against oracle/spark_oracle.py fed the same batches:
the full state is the oracle's state, the delta the keys its batch result emits whose window outlives the batch's
eviction watermark, the info its epoch and watermarks.  Every comparison is exact -- records as key-sorted bytes, batch
results through assert_batch_equal on inputs whose fp64 sums are exact in any order.
"""
import ctypes

import numpy as np
import pytest

import checkpoint_cases as cc
from test_gpu_edges import EXPECT_PATH, MODES, pin  # noqa: F401  (pin: that file's fixture, used as it is)
from test_gpu_parity import assert_batch_equal

pytestmark = pytest.mark.gpu


def _engine(**kw):
    from mobheat import HeatmapEngine
    return HeatmapEngine(h3_res=cc.RES, **kw)


def _bytes(recs):
    return cc.keyed(recs).tobytes()


def _check_full(eng, ref, what=""):
    info, recs = eng.export_state()
    assert info == ref.info(), what
    assert not recs["reserved"].any() and _bytes(recs) == ref.full().tobytes(), f"{what}: full export"
    return info, recs


def _check_delta(eng, ref, what=""):
    info, recs = eng.export_state_delta()
    assert info == ref.info(), what
    assert not recs["reserved"].any() and _bytes(recs) == ref.delta().tobytes(), f"{what}: delta ({recs.size} records)"
    return info, recs


def _check_windows(eng, ref):
    ws, keys = eng.live_windows()
    assert ws.tolist() == sorted(ref.windows()) and dict(zip(ws.tolist(), keys.tolist())) == ref.windows()


def test_record_layout():
    from mobheat._lib import STATE_REC_DTYPE
    assert cc.REC_DTYPE == STATE_REC_DTYPE


# ---------------------------------------------------------------------------------------------------------
# 1. dump sizes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_window", "two_windows"])
@pytest.mark.parametrize("n", cc.SIZES)
def test_dump_sizes(n, two):
    """The 1024-slot minimum table, the 2048-slot dump tile and load 1/2: a window of 1, 511, 512, 513, 1024, 1025 and
    2049 keys (tables of 1024, 1024, 1024, 2048, 2048, 4096, 8192 slots: less than one k_dump_gen tile, one, two, four;
    512 and 1024 keys are their table's load-1/2 limit), alone and behind a second, smaller window in the same dump.
    The full export is the oracle's state, the delta of the one batch is every key, and the export imported into a fresh
    engine (whose tables import sizes for exactly these keys) exports the same bytes."""
    case = cc.sized_case(n, two)
    ref = cc.Reference()
    exp = ref.batch(case.batch)
    eng, eng2 = _engine(), _engine()
    try:
        assert_batch_equal(eng.process_batch(0, **case.batch), exp)
        info, recs = _check_full(eng, ref)
        assert recs.size == sum(case.windows.values())
        _check_windows(eng, ref)
        _check_delta(eng, ref)
        eng2.import_state(info, recs)
        info2, recs2 = eng2.export_state()
        assert info2 == info and _bytes(recs2) == _bytes(recs)
        _check_windows(eng2, ref)
    finally:
        eng.close()
        eng2.close()


# ---------------------------------------------------------------------------------------------------------
# 2. delta shapes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.DELTA_CASES, ids=cc.DELTA_IDS)
def test_delta_shapes(case):
    """Load 1/2 and the touched word through the regrow: no delta before any batch, none after an import, none after
    an empty batch; every live key; one key of a 513-key window; the 10 new and 5 re-touched keys of a 512-key window
    whose 1024-slot table the batch regrows (the other 507 go through k_dump_gen and the rehash merge with the touched
    word of an older batch, and stay out; the regrow runs before the batch's own merge, so no word of the current batch
    is moved here -- only a pipelined binned batch does that, past 10^6 keys of a window); the touched keys of the window the batch's watermark does not evict, with
    the post-eviction info.  After every batch the base export merged with the deltas since is the full export."""
    from mobheat.engine import merge_state
    ref = cc.Reference()
    eng = _engine()
    try:
        batches, first = case.batches, 0
        if case.start == "import":
            ref.batch(batches[0])
            eng.import_state(ref.info(), ref.full())
            ref.touched = []   # (no batch ran on this engine)
            batches, first = batches[1:], 1
        dinfo, drecs = _check_delta(eng, ref, "before any batch")
        assert drecs.size == 0
        base, deltas = _check_full(eng, ref, "base"), []
        for e, b in enumerate(batches, first):
            what = f"{case.name} batch {e}"
            exp = ref.batch(b)
            try:
                assert_batch_equal(eng.process_batch(e, **b), exp)
            except AssertionError as err:
                raise AssertionError(f"{what}: {err}") from err
            dinfo, drecs = _check_delta(eng, ref, what)
            deltas.append((dinfo, drecs))
            finfo, frecs = _check_full(eng, ref, what)
            minfo, mrecs = merge_state(base, deltas)
            assert minfo == finfo and _bytes(mrecs) == _bytes(frecs), f"{what}: base + deltas"
            _check_windows(eng, ref)
        assert drecs.size == case.n_delta
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 3. call orders on one state, slice edges
# ---------------------------------------------------------------------------------------------------------
ORDERS = {
    "full_begin_first": ("full", "delta", "begin_full", "delta", "begin_delta", "full"),
    "delta_begin_first": ("full", "delta", "begin_delta", "delta", "begin_full", "full"),
    "size_query_full_fetch": ("delta_size", "full", "delta_fetch", "begin_delta", "full", "delta"),
}


def _order_state():
    ref = cc.Reference()
    eng = _engine()
    for e, b in enumerate(cc.ORDER_CASE.batches):
        ref.batch(b)
        eng.process_batch(e, **b)
    return eng, ref


@pytest.mark.parametrize("order", list(ORDERS))
def test_export_call_orders(order):
    """The cached dump's bookkeeping (touched_dump_seq, export_dump_n, both dropped by state_dump) on the state of the
    load-1/2 regrow (522 keys, 15 in the delta): full and touched exports, whole and in two halves, in three orders --
    a delta after a full export dumps again, a delta sized (recs = NULL) before a full export and fetched after it
    too -- and every result is the reference's."""
    from mobheat import _lib
    from mobheat._lib import HmStateInfo, STATE_REC_DTYPE
    eng, ref = _order_state()
    lib = _lib.load()
    sized = None
    try:
        for k, op in enumerate(ORDERS[order]):
            what = f"{order} step {k} ({op})"
            if op == "full":
                _check_full(eng, ref, what)
            elif op == "delta":
                _check_delta(eng, ref, what)
            elif op in ("begin_full", "begin_delta"):
                touched = op == "begin_delta"
                info, n, recs, _, fill = eng.export_begin(touched_only=touched, slice_records=7)
                fill(0, n)
                want = ref.delta() if touched else ref.full()
                assert info == ref.info() and n == want.size and _bytes(recs) == want.tobytes(), what
            elif op == "delta_size":
                info, m = HmStateInfo(), ctypes.c_int64()
                _lib.check(lib.hm_state_export_touched(eng._ctx, ctypes.byref(info), None, 0, ctypes.byref(m)), eng._ctx, what)
                sized = int(m.value)
                assert sized == cc.ORDER_CASE.n_delta, what
            elif op == "delta_fetch":
                info, m = HmStateInfo(), ctypes.c_int64()
                recs = np.zeros(sized, STATE_REC_DTYPE)
                _lib.check(lib.hm_state_export_touched(eng._ctx, ctypes.byref(info), recs.ctypes.data, sized, ctypes.byref(m)),
                           eng._ctx, what)
                assert m.value == sized and _bytes(recs) == ref.delta().tobytes(), what
    finally:
        eng.close()


@pytest.mark.parametrize("touched", [False, True], ids=["full", "touched"])
def test_export_slice_edges(touched):
    """hm_state_export_begin's dump of n records (522, or the 15 of the delta) in slices of 1 (capped at 64 slices), n - 1,
    n and n + 1 records, and copied -- synchronously and queued -- as [0, 0), [n, 0), [n - 1, 1) and [0, n): every copy
    is that part of the dump, an empty one writes nothing."""
    from mobheat import _lib
    from mobheat._lib import STATE_REC_DTYPE
    eng, ref = _order_state()
    lib = _lib.load()
    want = ref.delta() if touched else ref.full()
    n = want.size
    try:
        for s in (1, n - 1, n, n + 1):
            info, m, recs, _, fill = eng.export_begin(touched_only=touched, slice_records=s)
            fill(0, m)
            assert info == ref.info() and m == n and _bytes(recs) == want.tobytes(), f"slices of {s}"
        dump = recs.copy()   # (the last begin's dump, in its own order: the copies below read the same one)
        for k, (first, count) in enumerate(((0, 0), (n, 0), (n - 1, 1), (0, n))):
            for queued in (False, True):
                buf = np.zeros(n + 1, STATE_REC_DTYPE)
                buf["reserved"] = -1   # (a guard: nothing but the copy writes here)
                if queued:
                    _lib.check(lib.hm_state_export_copy_async(eng._ctx, buf.ctypes.data, first, count, k), eng._ctx, "async")
                    _lib.check(lib.hm_state_export_copy_wait(eng._ctx, k), eng._ctx, "wait")
                else:
                    _lib.check(lib.hm_state_export_copy(eng._ctx, buf.ctypes.data, first, count), eng._ctx, "copy")
                assert buf[:count].tobytes() == dump[first: first + count].tobytes(), (first, count, queued)
                assert (buf["reserved"][count:] == -1).all(), (first, count, queued)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 4. import census
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", cc.CENSUS_ORDERS)
@pytest.mark.parametrize("W", cc.CENSUS_WINDOWS)
def test_import_census(W, order):
    """GMAP_SLOTS / 2 = 2048 windows: hm_state_import's host census (the `last` cache and its linear search) over W
    windows of 3 keys given grouped as an export leaves them, reversed, and round-robin with the window changing on
    every record; one window starts before 1970.  The export is the input as a set and live_windows() agrees."""
    info, recs = cc.census_records(W, order)
    eng = _engine()
    try:
        eng.import_state(info, recs)
        info2, back = eng.export_state()
        assert info2 == info and _bytes(back) == _bytes(recs)
        ws, keys = eng.live_windows()
        assert ws.tolist() == sorted(cc.census_window_starts(W).tolist()) and (keys == cc.CENSUS_KEYS).all()
        dinfo, drecs = eng.export_state_delta()
        assert dinfo == info and drecs.size == 0
    finally:
        eng.close()


@pytest.mark.parametrize("order", cc.CENSUS_ORDERS)
def test_import_of_2049_windows_is_refused(order):
    """GMAP_SLOTS / 2 = 2048: one window more is HM_E_OVERFLOW, and the same engine then imports the 2048-window set and
    exports it."""
    from mobheat._lib import HM_E_OVERFLOW, MobheatError
    info, recs = cc.census_records(cc.MAX_WINDOWS + 1, order)
    ginfo, good = cc.census_records(cc.MAX_WINDOWS, order)
    eng = _engine()
    try:
        with pytest.raises(MobheatError) as e:
            eng.import_state(info, recs)
        assert e.value.code == HM_E_OVERFLOW, e.value
        info0, recs0 = eng.export_state()
        assert info0["epoch_id"] == -1 and recs0.size == 0 and eng.live_windows()[0].size == 0
        eng.import_state(ginfo, good)
        info2, back = eng.export_state()
        assert info2 == ginfo and _bytes(back) == _bytes(good)
        assert eng.live_windows()[0].size == cc.MAX_WINDOWS
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 5. restore, then continue, in every ingest mode
# ---------------------------------------------------------------------------------------------------------
_RESTORE = {}


def _restore_reference():
    """the oracle through all three batches, once: (info and records engine A must export, the oracle after the batch
    on top, that batch's expected result)"""
    if not _RESTORE:
        ref = cc.Reference()
        for b in cc.RESTORE_BEFORE:
            ref.batch(b)
        _RESTORE["before"] = (ref.info(), ref.full())
        _RESTORE["exp"] = ref.batch(cc.RESTORE_AFTER)
        _RESTORE["ref"] = ref
    return _RESTORE["before"], _RESTORE["ref"], _RESTORE["exp"]


def _engine_a_export(pin):
    pin("adaptive")
    (info, recs), _, _ = _restore_reference()
    a = _engine()
    try:
        for e, b in enumerate(cc.RESTORE_BEFORE):
            a.process_batch(e, **b)
        ainfo, arecs = a.export_state()
    finally:
        a.close()
    assert ainfo == info and _bytes(arecs) == recs.tobytes()
    return ainfo, arecs


@pytest.mark.parametrize("mode", list(MODES))
def test_restore_then_continue(mode, pin):
    """Load 1/2 at the restore: import builds ordinary tables sized for exactly the imported keys, so engine B's first
    batch -- on the path the mode pins -- regrows the imported 512-key window it adds 20 keys to (and, binned, every
    window it touches, into range geometry: gens_prepare's misfit branch), re-touches imported keys, opens a window and
    has an imported window evicted by the restored watermark after emitting it.  The batch result, the full export and
    the delta are the oracle's."""
    ainfo, arecs = _engine_a_export(pin)
    _, ref, exp = _restore_reference()
    pin(mode)
    b = _engine()
    try:
        b.import_state(ainfo, arecs)
        res = b.process_batch(2, **cc.RESTORE_AFTER)
        assert_batch_equal(res, exp)
        c = b.last_counts()
        assert (c["table_mode"], c["binned"]) == EXPECT_PATH[mode], f"mode {mode}: path taken {c}"
        _check_full(b, ref, mode)
        _check_delta(b, ref, mode)
        _check_windows(b, ref)
    finally:
        b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_restore_then_continue_on_shards(mode, pin):
    """The same through shard contexts: engine A's export split by owner, each part imported into a context created as
    shard (r, 4) (range geometry from the start, sized for the shard's keys), the batch on top through the stage API of
    the four with the exchange routed on the host.  The owners' tiles together are the oracle's, and every shard --
    shard (1, 4) among them -- exports the oracle's records that it owns, in full and as the delta."""
    import mobheat
    from mobheat.distributed import tile_owner
    from mobheat.engine import BatchResult, TileRows
    from test_gpu_stages import _stage_batch
    import dataclasses
    W = 4
    ainfo, arecs = _engine_a_export(pin)
    _, ref, exp = _restore_reference()
    own = tile_owner(arecs["cell"], arecs["window_start_us"], W)
    assert all((own == r).any() for r in range(W))
    pin(mode)
    lib = mobheat.load()
    engines = [_engine(shard=(r, W)) for r in range(W)]
    try:
        for r, eng in enumerate(engines):
            mine = arecs[own == r]
            eng.import_state(dict(ainfo, n_keys=int(mine.size)), mine)
        n = cc.RESTORE_AFTER["lat"].size
        bounds = [r * n // W for r in range(W + 1)]
        shards = [{k: v[bounds[r]: bounds[r + 1]] for k, v in cc.RESTORE_AFTER.items()} for r in range(W)]
        stats = []
        outs, latest, _, _, table = _stage_batch(engines, lib, shards, 2, stats)
        assert table == EXPECT_PATH[mode][0]
        tiles = TileRows(**{f.name: np.concatenate([getattr(t, f.name) for t in outs]) for f in dataclasses.fields(TileRows)})
        rows = np.concatenate([latest[r] + bounds[r] for r in range(W)])
        s0 = stats[0]
        assert all((s.watermark_ms, s.late_watermark_ms, s.batch_max_event_ms) ==
                   (s0.watermark_ms, s0.late_watermark_ms, s0.batch_max_event_ms) for s in stats)
        union = BatchResult(tiles=tiles, latest_rows=rows, n_in=n, n_valid=sum(s.n_valid for s in stats),
                            n_late=sum(s.n_late for s in stats), n_state=sum(s.n_state for s in stats),
                            batch_max_event_ms=s0.batch_max_event_ms, watermark_ms=s0.watermark_ms,
                            late_watermark_ms=s0.late_watermark_ms, n_partials=0, n_tiles=len(tiles), n_latest=rows.size)
        assert_batch_equal(union, exp)
        full, delta = ref.full(), ref.delta()
        fown = tile_owner(full["cell"], full["window_start_us"], W)
        down = tile_owner(delta["cell"], delta["window_start_us"], W)
        for r, eng in enumerate(engines):
            info, recs = eng.export_state()
            assert info == dict(ref.info(), n_keys=int((fown == r).sum())), r
            assert _bytes(recs) == full[fown == r].tobytes(), f"shard {r}: full export"
            dinfo, drecs = eng.export_state_delta()
            assert dinfo == info and _bytes(drecs) == delta[down == r].tobytes(), f"shard {r}: delta"
    finally:
        for eng in engines:
            eng.close()


# ---------------------------------------------------------------------------------------------------------
# 6. refused records
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.REFUSED)
def test_import_refuses_and_stays_usable(name):
    """The 512-lane merge chunk: a (cell, window) key given twice -- next to its copy, where one chunk's claim set adds
    the two, and 600 records away, where the second finds the first in the table -- a cell of another resolution and a
    cell of another mode are HM_E_INVALID.  The refusal of a repeated key comes after the tables were acquired and
    merged into; after every refusal the same engine is fresh, imports the good set, exports it exactly and takes a
    batch on top."""
    from mobheat._lib import HM_E_INVALID, MobheatError
    info, good, bad = cc.refused_sets()
    eng = _engine()
    try:
        with pytest.raises(MobheatError) as e:
            eng.import_state(info, bad[name])
        assert e.value.code == HM_E_INVALID, e.value
        info0, recs0 = eng.export_state()
        assert info0["epoch_id"] == -1 and recs0.size == 0 and eng.live_windows()[0].size == 0
        eng.import_state(info, good)
        info2, back = eng.export_state()
        assert info2 == info and _bytes(back) == _bytes(good)
        ref = cc.Reference()
        ref.batch(cc.rows((np.arange(1300), 1, 1), seed=8))
        b = cc.rows((np.arange(1290, 1310), 1, 2), seed=11)
        assert_batch_equal(eng.process_batch(1, **b), ref.batch(b))
        _check_full(eng, ref)
        _check_delta(eng, ref)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 7. queued copies against the next batch
# ---------------------------------------------------------------------------------------------------------
def test_queued_export_copies_survive_the_next_batch():
    """Load 1/2 and hm_state_export_copy_async's fence: six slices of the 1536-record dump are queued and none waited
    for; the next batch regrows both windows, whose k_dump_gen rewrites all 1536 records of the buffer the slices read.
    The batch's stream waits for the last queued copy first (export_copies_fence), so the slices waited for afterwards
    hold the export of before the batch, and the batch is the one a twin engine that never exported computes.
    (Without the fence this is a race that the copies usually win: the test pins the contract, it does not prove the
    race.)"""
    ref = cc.Reference()
    ref.batch(cc.QUEUED_BUILD)
    eng, twin = _engine(), _engine()
    try:
        eng.process_batch(0, **cc.QUEUED_BUILD)
        twin.process_batch(0, **cc.QUEUED_BUILD)
        before_info, before = ref.info(), ref.full().tobytes()
        info, n, recs, _, fill = eng.export_begin(touched_only=False, slice_records=cc.QUEUED_SLICE)
        assert info == before_info and n == 1536
        exp = ref.batch(cc.QUEUED_BATCH)
        res = eng.process_batch(1, **cc.QUEUED_BATCH)
        fill(0, n)
        assert _bytes(recs) == before, "the queued slices hold something else than the export before the batch"
        ret = twin.process_batch(1, **cc.QUEUED_BATCH)
        assert_batch_equal(res, exp)
        ka, kb = np.lexsort((res.tiles.window_start_us, res.tiles.cell)), np.lexsort((ret.tiles.window_start_us, ret.tiles.cell))
        for f in ("cell", "window_start_us", "count", "speed_null", "avg_speed", "avg_lon", "avg_lat"):
            assert getattr(res.tiles, f)[ka].tobytes() == getattr(ret.tiles, f)[kb].tobytes(), f
        assert np.array_equal(res.latest_rows, ret.latest_rows) and res.n_state == ret.n_state == exp["n_state"]
        _check_full(eng, ref)
        _check_delta(eng, ref)
    finally:
        eng.close()
        twin.close()
