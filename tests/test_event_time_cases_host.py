"""CPU: the event-time boundary scenarios of tests/event_time_cases.py against the oracle alone -- every boundary class is
populated for every configuration and rule (a populated class is a condition, not a measurement), the hand counts hold,
and the hand-written known-answer table of the default configuration equals the oracle.  The GPU runs the same scenarios
in tests/test_gpu_event_time.py."""
import numpy as np
import pytest

import event_time_cases as etc

_CACHE = {}


def _scenario(ci, late_prev):
    if (ci, late_prev) not in _CACHE:
        from oracle.spark_oracle import SparkHeatmapOracle
        tile, delay, _ = etc.CONFIGS[ci]
        _CACHE[ci, late_prev] = etc.scenario(tile, delay, late_prev, SparkHeatmapOracle)
    return _CACHE[ci, late_prev]


CASES = [(ci, lp) for ci in range(len(etc.CONFIGS)) for lp in (True, False)]
IDS = [f"{etc.CONFIG_IDS[ci]}-{'prev' if lp else 'cur'}" for ci, lp in CASES]


@pytest.mark.parametrize("ci,late_prev", CASES, ids=IDS)
def test_hand_counts_and_watermarks(ci, late_prev):
    """n_valid and n_late of every batch are the sums of the groups' sizes (verdicts fixed by construction); the watermark
    follows the batch maxima: truncated milliseconds, never back, unmoved by invalid rows."""
    tile, delay, _ = etc.CONFIGS[ci]
    sc = _scenario(ci, late_prev)
    assert len(sc) == 19
    wm = 0
    for name, cols, exp, m in sc:
        assert exp["n_valid"] == m["n_valid"], name
        assert exp["n_late"] == m["n_late"], name
        assert exp["watermark_ms"] == wm == m["wm_cur"], name
        assert exp["late_watermark_ms"] * 1000 == m["L"], name
        valid = m["kind"] != "invalid"
        if valid.any():
            mx = int(cols["ts_us"][valid].max())
            want = mx // 1000 if mx >= 0 else -(-mx // 1000)   # truncation toward zero
            assert exp["batch_max_event_ms"] == want, name
            wm = max(wm, want - delay)
        else:
            assert exp["batch_max_event_ms"] == etc.INT64_MIN, name
        if m["marker"] is not None:
            assert int(cols["ts_us"][valid].max()) == m["batch_max"] >= m["marker"], name
    by = {name: (cols, exp, m) for name, cols, exp, m in sc}
    assert by["negative_only"][1]["batch_max_event_ms"] == 0            # trunc(-1 / 1000); a floor gives -1
    assert by["negative_only"][2]["n_late"] == by["negative_only"][2]["n_valid"] > 0 and not by["negative_only"][1]["tiles"]
    assert by["late_only"][2]["n_late"] == by["late_only"][2]["n_valid"] > 0 and not by["late_only"][1]["tiles"]
    assert by["steady"][2]["wm_cur"] == by["lower_max"][2]["wm_cur"] > 0  # the lower maximum moved nothing
    assert by["first"][2]["marker"] % 1000 == 999 and by["step1"][2]["marker"] % 1000 == 999
    assert by["late_only"][2]["wm_cur"] == by["after_zero"][2]["wm_cur"]  # a millisecond short: no move
    advancing = [m["wm_cur"] for name, _, _, m in sc if name.startswith("step") or name == "all_invalid"]
    assert len(advancing) >= 7 and all(b > a for a, b in zip(advancing, advancing[1:]))
    steps = {(b - a) * 1000 for a, b in zip(advancing[1:], advancing[2:])}
    if tile % 1000 == 0:   # whole windows per batch
        assert steps == {etc.steps_per_batch(tile, delay) * tile}, steps


@pytest.mark.parametrize("ci,late_prev", CASES, ids=IDS)
def test_every_class_is_populated(ci, late_prev):
    tile, delay, _ = etc.CONFIGS[ci]
    sc = _scenario(ci, late_prev)
    want = etc.expectations(tile, late_prev)
    ordinary = [(name, cols, exp, m) for name, cols, exp, m in sc if "late_edge" in m["groups"] and m["tags"]]

    # classes 1 and 2
    for name, cols, exp, m in ordinary:
        assert m["groups"]["late_edge"].size == etc.GROUP_ROWS and m["groups"]["kept_edge"].size == etc.GROUP_ROWS, name
        ts = cols["ts_us"]
        assert m["L"] in ts[m["groups"]["kept_edge"]].tolist() and m["L"] - 1 in ts[m["groups"]["l_minus_1"]].tolist()
        # late and kept rows side by side: no run of 64 rows of one verdict
        k = (m["kind"] == "late").astype(int)
        assert all(0 < k[i:i + 64].sum() < 64 for i in range(0, k.size - 63, 64)), name
    assert any(m["tags"]["end_equals_L"] and m["L"] > 0 for _, _, _, m in ordinary) == want["end_equals_L"]
    assert any(not m["tags"]["end_equals_L"] for _, _, _, m in ordinary)       # L inside a window: that window is kept
    if want["decided_at_us"]:
        assert any(m["tags"]["kept_end_within_ms"] for _, _, _, m in ordinary)
        assert any(m["tags"]["late_end_within_ms"] for _, _, _, m in ordinary)

    # class 3: emitted and evicted by the same batch, late in the next
    hits = 0
    for (name, cols, exp, m), (name2, cols2, exp2, m2) in zip(sc, sc[1:]):
        w = m["tags"].get("evict_now_window") if m["tags"] else None
        if w is None:
            continue
        hits += 1
        assert m["L"] < w + tile <= m["E"], name
        assert any(t["window_start_us"] == w for t in exp["tiles"]), name      # emitted
        assert w not in m["state_windows"], name                               # evicted: n_state does not count it
        assert exp["n_state"] == m["n_state_keys"], name
        if "late_edge" in m2["groups"] and m2["tags"]:
            r = m2["groups"]["replay_evicted"]
            assert r.size == etc.GROUP_ROWS and (m2["kind"][r] == "late").all(), name2
            assert sorted(cols2["ts_us"][r].tolist()) == sorted(cols["ts_us"][m["groups"]["evict_now"]].tolist())
    assert (hits >= 6) == want["evict_now"] and (hits > 0) == want["evict_now"], hits

    # classes 4 and 5: a strict drop of n_state where windows go and nothing comes (the batch without valid rows)
    by = {name: k for k, (name, _, _, _) in enumerate(sc)}
    for name in ("all_invalid", "zero_rows"):
        k = by[name]
        before, now = sc[k - 1], sc[k]
        assert before[3]["tags"]["doomed_window"] in before[3]["state_windows"], name
        assert before[3]["tags"]["doomed_window"] not in now[3]["state_windows"], name
        assert now[2]["n_state"] < before[2]["n_state"] and not now[2]["tiles"], name
    assert sc[by["zero_rows"]][1]["lat"].size == 0 and sc[by["all_invalid"]][1]["lat"].size > 0
    assert sc[by["all_invalid"]][3]["n_valid"] == 0

    # class 4: a key created, updated by the next batch (cumulative count), evicted, and later windows created after
    life = 0
    for k in range(len(sc) - 2):
        m, m2 = sc[k][3], sc[k + 1][3]
        if "head" not in m["groups"] or "head_prev" not in m2["groups"]:
            continue
        x = int(sc[k][1]["ts_us"][m["groups"]["head"]].min()) // tile * tile
        c1 = {t["cell"]: t["count"] for t in sc[k][2]["tiles"] if t["window_start_us"] == x}
        c2 = {t["cell"]: t["count"] for t in sc[k + 1][2]["tiles"] if t["window_start_us"] == x}
        assert c1 and set(c2) & set(c1) and all(c2[c] > c1[c] for c in set(c2) & set(c1)), sc[k][0]
        gone = [j for j in range(k + 2, len(sc)) if x not in sc[j][3]["state_windows"]]
        if gone and any(max(sc[j][3]["state_windows"], default=x) > x for j in gone):
            life += 1
    assert life >= 6, life

    # class 5: rows made late by a batch without valid rows (previous-watermark rule only): the late_edge window of the
    # batch after it was still on time under the late bound in force during the empty batch
    made_late = 0
    for name in ("all_invalid", "zero_rows"):
        k = by[name]
        empty_L, after = sc[k][3]["L"], sc[k + 1][3]
        end = after["tags"]["late_edge_end"]
        if empty_L < end <= after["L"]:
            made_late += after["groups"]["late_edge"].size
    assert (made_late > 0) == want["late_by_empty_batch"], made_late

    # class 6: late rows among the latest rows
    for name, cols, exp, m in ordinary:
        latest = set(exp["latest_rows"].tolist())
        for g, rows in (("veh_late_only", 1), ("veh_tie_late", 2), ("veh_tie_kept", 2)):
            assert len(latest & set(m["groups"][g].tolist())) == rows, (name, g)
        g = m["groups"]["veh_late_newest"]
        assert [cols["ts_us"][r] for r in g if r in latest] == [cols["ts_us"][g].max()], name
        g = m["groups"]["veh_late_then_kept"]
        assert [m["kind"][r] for r in g if r in latest] == ["kept"], name

    # class 7: the range edge
    name, cols, exp, m = sc[by["range_edge"]]
    lo, hi = etc.valid_range(tile)
    ts = cols["ts_us"]
    assert sorted(ts[m["groups"]["edge_valid"]].tolist()) == [lo, hi]
    assert sorted(ts[m["groups"]["edge_invalid"]].tolist()) == [etc.INT64_MIN, lo - 1, hi + 1, etc.INT64_MAX]
    assert (lo, hi) == (etc.INT64_MIN + 2 * tile + 1, etc.INT64_MAX - 2 * tile - 1)
    assert any(t["window_start_us"] == hi - hi % tile for t in exp["tiles"])
    assert exp["batch_max_event_ms"] == hi // 1000
    last = sc[by["aftermath2"]]
    assert (last[3]["kind"][last[3]["groups"]["ordinary"]] == "late").all() and last[3]["groups"]["ordinary"].size == 5
    from oracle import h3_oracle
    c0 = int(h3_oracle.latlng_to_cell(np.array([37.5]), np.array([23.75]), etc.RES)[0])   # the cell of the edge rows
    counts = [[t["count"] for t in sc[by[n]][2]["tiles"] if (t["cell"], t["window_start_us"]) == (c0, hi - hi % tile)]
              for n in ("range_edge", "aftermath1", "aftermath2")]
    assert all(len(c) == 1 for c in counts) and counts[0][0] < counts[1][0] < counts[2][0], counts   # cumulative


@pytest.mark.parametrize("ci,late_prev", CASES, ids=IDS)
def test_window_starts_of_the_scenario(ci, late_prev):
    """The emitted window starts are ts - ts mod tile (Python integers) of the kept rows, among them k * tile - 1,
    k * tile and k * tile + 1 for k around 0, around today's date and at the largest valid k."""
    tile, delay, _ = etc.CONFIGS[ci]
    seen = set()
    for name, cols, exp, m in _scenario(ci, late_prev):
        kept = [int(t) for t in cols["ts_us"][m["kind"] == "kept"]]
        assert {t - t % tile for t in kept} == {t["window_start_us"] for t in exp["tiles"]}, name
        seen |= {(t // tile, t % tile) for t in kept}
    _, hi = etc.valid_range(tile)
    for k in (1, 2, hi // tile):
        assert (k, 0) in seen and (k - 1, tile - 1) in seen, k
    assert (0, 0) in seen and (0, 1) in seen and (1, 1) in seen   # (window -1 ends at L = 0: late from the start)
    assert any(q > 10**9 // (tile // 10**6) and r == 0 for q, r in seen)


@pytest.mark.parametrize("late_prev", [True, False])
def test_known_answer_table_equals_the_oracle(late_prev):
    from oracle.spark_oracle import SparkHeatmapOracle
    ora = SparkHeatmapOracle(h3_res=etc.RES, watermark_delay_ms=etc.KNOWN_DELAY_MS, late_uses_prev_watermark=late_prev,
                             tile_us=etc.KNOWN_TILE_US)
    col = 1 if late_prev else 2
    for cols, b in etc.known_answer_batches():
        exp = ora.process_batch(**cols)
        verdicts = [r[col] for r in b["rows"]]
        assert exp["n_late"] == verdicts.count("late") and exp["n_valid"] == len(verdicts)
        kept = sorted({r[0] - r[0] % etc.KNOWN_TILE_US for r in b["rows"] if r[col] == "kept"})
        assert sorted(t["window_start_us"] for t in exp["tiles"]) == kept
        assert (ora.wm_prev, ora.wm_cur) == b["after"]


def test_configurations_are_the_seven_of_the_issue():
    assert [(t, d) for t, d, _ in etc.CONFIGS] == [(300_000_000, 600_000), (60_000_000, 0), (3_600_000_000, 600_000),
                                                   (86_400_000_000, 1), (420_000_000, 123_457), (1_000_000, 1_500),
                                                   (1_000_001, 600_000)]
    assert np.iinfo(np.int64).max == etc.INT64_MAX and np.iinfo(np.int64).min == etc.INT64_MIN
