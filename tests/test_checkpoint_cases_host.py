"""Host: tests/checkpoint_cases.py's cases are the edges they claim (the oracle alone, no engine).

Each sized case holds exactly the intended number of distinct cells per window, by the oracle's own cells, and the
table the engine's sizing rule gives it has the slots the edge is about; every batch's per-key sums are the same bits in
two row orders; every delta case's expected touched set has its stated shape and size; the record sets an import is
given are what their names say.  A case that fails here is wrong and is fixed here.
"""
import numpy as np
import pytest

import checkpoint_cases as cc


def _cells(batch):
    from oracle import h3_oracle
    return h3_oracle.latlng_to_cell(batch["lat"], batch["lon"], cc.RES)


def _all_batches():
    out = []
    for n in cc.SIZES:
        for two in (False, True):
            out.append((f"sized {n} two={two}", cc.sized_case(n, two).batch))
    for c in cc.DELTA_CASES:
        out += [(f"delta {c.name} batch {e}", b) for e, b in enumerate(c.batches)]
    out += [(f"restore before {e}", b) for e, b in enumerate(cc.RESTORE_BEFORE)]
    out += [("restore after", cc.RESTORE_AFTER), ("queued build", cc.QUEUED_BUILD), ("queued batch", cc.QUEUED_BATCH)]
    return out


def test_sizes_are_the_stated_edges():
    """1024-slot minimum table, 2048-slot dump tile, load 1/2: the sweep's key counts and the tables they give"""
    assert cc.SIZES == (1, 511, 512, 513, 1024, 1025, 2049)
    assert [cc.slots_for(n) for n in cc.SIZES] == [1024, 1024, 1024, 2048, 2048, 4096, 8192] == \
        [cc.SIZE_SLOTS[n] for n in cc.SIZES]
    assert cc.MIN_SLOTS == 1024 and cc.DUMP_TILE == 2048
    # below one dump tile, exactly one, exactly two, more; and a window at its load-1/2 limit at two table sizes
    slots = [cc.slots_for(n) for n in cc.SIZES]
    assert min(slots) < cc.DUMP_TILE and cc.DUMP_TILE in slots and 2 * cc.DUMP_TILE in slots and max(slots) > 2 * cc.DUMP_TILE
    assert [n for n in cc.SIZES if 2 * n == cc.slots_for(n)] == [512, 1024]
    for n in cc.SIZES:
        assert cc.second_window_keys(n) not in (0, n)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", cc.SIZES)
def test_sized_case_holds_its_keys(n, two):
    """exactly the intended distinct cells per window, one row per key in the edge window (the census counts rows)"""
    case = cc.sized_case(n, two)
    ref = cc.Reference()
    exp = ref.batch(case.batch)
    assert ref.windows() == case.windows and len(case.windows) == 1 + two
    assert case.windows[cc.T0 + cc.TILE] == n
    ws = case.batch["ts_us"] - np.mod(case.batch["ts_us"], cc.TILE)
    assert int((ws == cc.T0 + cc.TILE).sum()) == n                       # rows of the edge window = its keys
    assert exp["n_late"] == 0 and exp["n_valid"] == case.batch["lat"].size and exp["n_state"] == sum(case.windows.values())
    if two:
        assert len({n, cc.second_window_keys(n)}) == 2
        assert max(t["count"] for t in exp["tiles"]) == 2                # (sums of more than one row are in the dump)


@pytest.mark.parametrize("what,batch", _all_batches(), ids=[w for w, _ in _all_batches()])
def test_sums_are_exact_in_any_order(what, batch):
    """dyadic points and speeds: every key's count and fp64 sums are the same bits added in the given order and in a
    fixed permutation of it -- and they are the oracle's"""
    if batch["lat"].size == 0:
        return
    assert np.array_equal(batch["lat"], cc.dyadic(batch["lat"])) and np.array_equal(batch["lon"], cc.dyadic(batch["lon"]))
    assert np.array_equal(batch["speed"] * 4, np.round(batch["speed"] * 4))
    a = cc.key_sums(batch, _cells(batch))
    p = cc.permuted(batch)
    assert not np.array_equal(p["ts_us"], batch["ts_us"]) or batch["lat"].size == 1
    assert cc.key_sums(p, _cells(p)) == a
    ref = cc.Reference()
    ref.batch(batch)
    got = {(int(r["cell"]), int(r["window_start_us"])): (int(r["count"]), int(r["n_speed"]), r["sum_speed"].tobytes(),
                                                         r["sum_lat"].tobytes(), r["sum_lon"].tobytes()) for r in ref.full()}
    late_free = {k: v for k, v in a.items() if k in got}
    assert late_free == got and len(got) == len(a)
    assert max(v[0] for v in a.values()) < 1 << 20


@pytest.mark.parametrize("case", cc.DELTA_CASES, ids=cc.DELTA_IDS)
def test_delta_case_has_its_shape(case):
    """the expected touched set of the last batch: empty, every live key, a strict non-empty subset, or such a subset
    with an untouched key in a window the batch regrows (load 1/2 crossed, by the engine's own rule)"""
    ref = cc.Reference()
    before, tables = {}, {}
    for e, b in enumerate(case.batches):
        before = ref.windows()
        ws = b["ts_us"] - np.mod(b["ts_us"], cc.TILE)
        census = {int(w): int((ws == w).sum()) for w in np.unique(ws)}
        last_tables = dict(tables)
        for w, c in census.items():   # the engine's sizing, batch after batch
            if w not in tables:
                tables[w] = cc.slots_for(c)
            elif cc.regrows(before[w], c, tables[w]):
                tables[w] = max(2 * tables[w], cc.slots_for(before[w] + c))
        exp = ref.batch(b)
        assert exp["n_late"] == 0, (case.name, e)
    if case.start == "import" or not case.batches:
        ref.touched = []   # (an imported state, or none: no batch ran on the engine under test)
    delta, live = set(ref.delta_keys()), set(ref.ora.state)
    assert len(delta) == case.n_delta and delta <= live
    if case.shape == "empty":
        assert not delta
    elif case.shape == "every":
        assert delta == live and live
    else:
        assert delta and delta < live
    regrown = tuple(sorted((w - cc.T0) // cc.TILE for w in tables if w in last_tables and tables[w] != last_tables[w]))
    assert regrown == case.regrown
    if case.shape == "subset_regrown":
        assert regrown
        for wi in regrown:
            w = cc.T0 + wi * cc.TILE
            assert any(k[1] == w for k in live - delta) and any(k[1] == w for k in delta)
    emitted_gone = {k[1] for k in ref.touched} - {k[1] for k in live}
    assert tuple(sorted((w - cc.T0) // cc.TILE for w in emitted_gone)) == case.evicted_touched
    if case.name == "regrow_15":   # the issue's numbers
        w = cc.T0 + cc.TILE
        assert before[w] == 512 and last_tables[w] == 1024 and ref.windows()[w] == 522 and tables[w] == 2048
        assert sum(1 for k in delta if k not in set(_state_keys(case.batches[0]))) == 10
    if case.name == "one_of_513":
        assert before[cc.T0 + cc.TILE] == 513 and tables[cc.T0 + cc.TILE] == 2048 and not regrown


def _state_keys(batch):
    ref = cc.Reference()
    ref.batch(batch)
    return list(ref.ora.state)


def test_order_case_state():
    assert cc.ORDER_CASE.name == "regrow_15" and cc.ORDER_CASE.n_delta == 15


@pytest.mark.parametrize("W", cc.CENSUS_WINDOWS + (cc.MAX_WINDOWS + 1,))
def test_census_records(W):
    """GMAP_SLOTS / 2 = 2048 windows: W windows of 3 keys, the same set in three orders; one window before 1970; the
    interleaved order changes window on every record, the grouped one never inside a window"""
    assert cc.CENSUS_WINDOWS == (1, 2, 7, 2048) and cc.MAX_WINDOWS == 2048
    sets = {o: cc.census_records(W, o) for o in cc.CENSUS_ORDERS}
    info, g = sets["grouped"]
    assert g.size == info["n_keys"] == 3 * W
    assert len({(int(r["cell"]), int(r["window_start_us"])) for r in g}) == g.size
    assert (g["window_start_us"] % cc.TILE == 0).all() and (g["window_start_us"] < 0).sum() == 3
    assert len(set(g["window_start_us"].tolist())) == W
    assert ((g["count"] >= 1) & (g["n_speed"] >= 0) & (g["n_speed"] <= g["count"]) & (g["reserved"] == 0)).all()
    assert ((g["cell"] >> np.uint64(52)) == np.uint64((1 << 7) | cc.RES)).all()
    # records an export could hold: no sum over no speeds (such keys exist from the seventh window on)
    assert (g["n_speed"] == 0).any() == (W >= 7) and not g["sum_speed"][g["n_speed"] == 0].any()
    for o in cc.CENSUS_ORDERS:
        assert cc.keyed(sets[o][1]).tobytes() == cc.keyed(g).tobytes(), o
    changes = {o: int((np.diff(sets[o][1]["window_start_us"]) != 0).sum()) for o in cc.CENSUS_ORDERS}
    assert changes["grouped"] == changes["reversed"] == W - 1
    assert changes["interleaved"] == (3 * W - 1 if W > 1 else 0)
    assert sets["reversed"][1].tobytes() == g[::-1].tobytes()


def test_restore_case():
    """load 1/2 at the restore: the imported 512-key window gets a 1024-slot table, and the batch after the restore
    does its four things -- re-touches imported keys, grows that window, opens a window, and has one evicted"""
    ref = cc.Reference()
    for b in cc.RESTORE_BEFORE:
        assert ref.batch(b)["n_late"] == 0
    T = lambda i: cc.T0 + i * cc.TILE   # noqa: E731
    before = ref.windows()
    assert before[T(cc.RESTORE_GROWN)] == 512 and cc.slots_for(512) == 1024      # import sizes it for its 512 keys
    assert T(cc.RESTORE_EVICTED) in before and T(cc.RESTORE_OPENED) not in before
    # the restored watermark lies past the evicted window's end, short of every other's
    assert T(cc.RESTORE_EVICTED) + cc.TILE <= ref.ora.wm_cur * 1000 < min(w for w in before if w != T(cc.RESTORE_EVICTED)) + cc.TILE
    old = set(ref.ora.state)
    ws = cc.RESTORE_AFTER["ts_us"] - np.mod(cc.RESTORE_AFTER["ts_us"], cc.TILE)
    assert cc.regrows(512, int((ws == T(cc.RESTORE_GROWN)).sum()), 1024)
    wm = ref.ora.wm_cur
    exp = ref.batch(cc.RESTORE_AFTER)
    after, emitted = ref.windows(), set(ref.touched)
    assert exp["n_late"] == 0
    assert emitted & old and emitted - old                                         # re-touched and new keys
    assert after[T(cc.RESTORE_GROWN)] == 532
    assert T(cc.RESTORE_OPENED) in after
    assert T(cc.RESTORE_EVICTED) not in after and any(k[1] == T(cc.RESTORE_EVICTED) for k in emitted)
    assert ref.ora.wm_cur > wm                                                     # and the watermark moves on
    assert set(ref.delta_keys()) < set(ref.ora.state)
    # a shard of four owns some of every window
    from mobheat.distributed import tile_owner
    keys = np.array(sorted(old), dtype=[("c", "<u8"), ("w", "<i8")])
    own = tile_owner(keys["c"], keys["w"], 4)
    for r in range(4):
        assert {int(w) for w in keys["w"][own == r]} == set(before), r


def test_refused_sets():
    """the 512-lane merge chunk: the good set is more than two chunks of distinct keys of the context's resolution; a
    repeated key sits next to its copy, or 600 records -- more than a chunk -- away; the two bad cells differ from the
    good ones in their resolution bits, or their mode bits, alone"""
    info, good, bad = cc.refused_sets()
    assert tuple(bad) == cc.REFUSED and cc.MERGE_CHUNK == 512
    assert good.size == info["n_keys"] == 1300 > 2 * cc.MERGE_CHUNK
    key = lambda r: list(zip(r["cell"].tolist(), r["window_start_us"].tolist()))   # noqa: E731
    assert len(set(key(good))) == good.size
    hi = np.uint64((1 << 7) | cc.RES)
    assert ((good["cell"] >> np.uint64(52)) == hi).all()
    for name in ("repeat_adjacent", "repeat_600_apart"):
        k = key(bad[name])
        assert len(set(k)) == good.size - 1 and bad[name].size == good.size
        i, j = [x for x in range(len(k)) if k.count(k[x]) == 2]
        assert j - i == (1 if name == "repeat_adjacent" else 600) and (j - i > cc.MERGE_CHUNK) == (name != "repeat_adjacent")
        assert bad[name][i].tobytes() == bad[name][j].tobytes()
    r = bad["other_resolution"]
    d = np.nonzero(r["cell"] != good["cell"])[0]
    assert d.tolist() == [20] and int(r["cell"][20] >> np.uint64(52)) == (1 << 7) | (cc.RES - 1)
    r = bad["other_mode"]
    d = np.nonzero(r["cell"] != good["cell"])[0]
    assert d.tolist() == [30] and int(r["cell"][30] >> np.uint64(59)) == 2 and int((r["cell"][30] >> np.uint64(52)) & np.uint64(15)) == cc.RES


def test_queued_case():
    """both windows at load 1/2 before the batch, both regrown by it: the regrow moves every record of the dump"""
    ref = cc.Reference()
    ref.batch(cc.QUEUED_BUILD)
    w1, w2 = cc.T0 + cc.TILE, cc.T0 + 2 * cc.TILE
    assert ref.windows() == {w1: 512, w2: 1024}
    n = len(ref.ora.state)
    assert n == 1536 and -(-n // cc.QUEUED_SLICE) == 6
    ws = cc.QUEUED_BATCH["ts_us"] - np.mod(cc.QUEUED_BATCH["ts_us"], cc.TILE)
    assert cc.regrows(512, int((ws == w1).sum()), cc.slots_for(512)) and cc.regrows(1024, int((ws == w2).sum()), cc.slots_for(1024))
    exp = ref.batch(cc.QUEUED_BATCH)
    assert exp["n_late"] == 0 and ref.windows() == {w1: 520, w2: 1032}
