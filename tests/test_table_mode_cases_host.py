"""CPU: the table-mode cases of tests/table_mode_cases.py mean what they claim, from the oracle's cells and window starts
alone -- the distinct keys per span and per flush interval, the count classes the keep threshold reads at every flush,
sums that are exact in any order (summed in two orders, compared bit for bit), a key whose speeds are all null, and no
late row.  The GPU runs the same cases in tests/test_gpu_table_mode.py."""
import numpy as np
import pytest

import table_mode_cases as tmc

GRID1 = [n for n, s in tmc.SPECS.items() if s[3] == 1]


def _key_index(c, b):
    """row -> dense index of its (cell, window) key among the batch's valid rows, from the oracle's cells"""
    cells, ws = tmc.keys_of(b, c["res"])
    keys = np.rec.fromarrays([cells, ws], names="c,w")
    uniq, inv = np.unique(keys, return_inverse=True)
    return uniq, inv.ravel()


@pytest.mark.parametrize("name", list(tmc.SPECS))
def test_ids_are_the_oracles_keys(name, oracle_h3):
    """distinct key ids are distinct (cell, window) keys and equal ids equal keys, in every batch: what `simulate`
    says about the ids holds for the keys the device sees"""
    c = tmc.case(name)
    for ids, b in zip(c["ids"], c["batches"]):
        v = ids >= 0
        assert np.array_equal(v, b["row_valid"])
        uniq, inv = _key_index(c, b)
        _, id_inv = np.unique(ids[v], return_inverse=True)
        # a bijection between ids and keys: each pairing (id, key) is seen with one partner only
        pairs = np.unique(np.stack([id_inv.ravel(), inv]), axis=1)
        assert pairs.shape[1] == uniq.size == np.unique(ids[v]).size
        w = (b["ts_us"][v] - tmc.T0) // tmc.TILE
        assert w.min() >= 0 and w.max() < c["windows"] and np.unique(w).size == c["windows"]


@pytest.mark.parametrize("name", list(tmc.SPECS))
def test_sums_exact_nulls_and_no_late_row(name, oracle_h3):
    from oracle.spark_oracle import SparkHeatmapOracle
    c = tmc.case(name)
    ora = SparkHeatmapOracle(h3_res=c["res"])
    for k, b in enumerate(c["batches"]):
        v = b["row_valid"]
        for col in ("lat", "lon", "speed"):   # multiples of 2^-10 below 2^7
            x = b[col] * 1024.0
            assert np.array_equal(x, np.round(x)) and np.abs(b[col]).max() < 128
        uniq, inv = _key_index(c, b)
        sv = b["speed_valid"][v]
        for col, sel in (("lat", np.ones(inv.size, bool)), ("lon", np.ones(inv.size, bool)), ("speed", sv)):
            x, g = b[col][v][sel], inv[sel]
            fwd = np.bincount(g, weights=x, minlength=uniq.size)
            p = np.random.default_rng(5).permutation(x.size)
            rev = np.bincount(g[p][::-1], weights=x[p][::-1], minlength=uniq.size)
            assert np.array_equal(fwd.view(np.uint64), rev.view(np.uint64)), f"{name}, batch {k}: {col} sums inexact"
        nsp = np.bincount(inv, weights=sv, minlength=uniq.size)
        assert (nsp == 0).any(), f"{name}, batch {k}: no key with all speeds null"
        assert 0.15 < 1 - sv.mean() < 0.3
        if name == "bin_reduce_emits":
            # (the oracle's million-key batches are left to the GPU test's shared run.)  The late bound of batch k is
            # the watermark before batch k - 1 under the previous-watermark rule, at most the one after it: the
            # earlier batch's maximum less the 10-minute delay, in truncated milliseconds.  Every window ends above both.
            prev = c["batches"][k - 1] if k else None
            bound_us = 0 if prev is None else (int(prev["ts_us"][prev["row_valid"]].max()) // 1000 - 600_000) * 1000
            assert bound_us < tmc.T0 or prev is None
            assert ((b["ts_us"] - b["ts_us"] % tmc.TILE + tmc.TILE)[v] > max(bound_us, 0)).all(), f"{name}, batch {k}"
            continue
        exp = ora.process_batch(**b)
        assert exp["n_late"] == 0 and exp["n_valid"] == int(v.sum()), f"{name}, batch {k}"


def test_resident(oracle_h3):
    s = tmc.simulate(tmc.case("resident")["ids"][0])
    assert s["distinct"] == 3000 < tmc.AG_FLUSH_AT and not s["flushes"] and s["evicted"] == 3000
    assert tmc.case("resident")["ids"][0].size == 8192


def test_flush_keeps_hot(oracle_h3):
    ids = tmc.case("flush_keeps_hot")["ids"][0]
    s = tmc.simulate(ids)
    assert ids.size == tmc.HOT_ROUNDS * tmc.AG_THREADS and s["distinct"] == tmc.HOT_KEYS + tmc.HOT_ROUNDS * tmc.HOT_FRESH
    for r0 in range(0, ids.size, tmc.AG_THREADS):   # per round: 128 keys never seen before, the rest on the hot keys
        rnd = ids[r0:r0 + tmc.AG_THREADS]
        assert np.setdiff1d(rnd[rnd >= tmc.HOT_KEYS], ids[:r0]).size == tmc.HOT_FRESH
        assert (rnd < tmc.HOT_KEYS).sum() == tmc.AG_THREADS - tmc.HOT_FRESH
    assert len(s["flushes"]) >= 2
    for f in s["flushes"]:   # every hot key is kept (counts of hundreds: few classes, far fewer than AG_KEEP_MAX keys)
        assert f["kept"] == tmc.HOT_KEYS and f["kf"] == 1 and f["hist"][0] == f["evicted"]
        assert all(f["counts"][k] >= 256 for k in range(tmc.HOT_KEYS))
        assert f["occ"] <= tmc.AG_FLUSH_AT + tmc.HOT_FRESH   # 87% of the slots at most
    assert s["evicted"] == s["distinct"]   # each key leaves the table once
    assert s["max_occ"] <= 0.87 * tmc.AG_SLOTS


def test_keep_class_over_cap(oracle_h3):
    ids = tmc.case("keep_class_over_cap")["ids"][0]
    s = tmc.simulate(ids)
    assert [f["round"] for f in s["flushes"]] == [4, 8, 12]
    for f in s["flushes"]:   # 600 keys of count exactly 2, nothing heavier: the class alone exceeds the cap, nothing is kept
        assert f["hist"][1] == tmc.PAIR_KEYS > tmc.AG_KEEP_MAX and sum(f["hist"][2:]) == 0
        assert sorted(set(f["counts"].values())) == [1, 2]
        assert all(f["counts"][k] == 2 for k in range(tmc.PAIR_KEYS))
        assert f["kf"] == 2 and f["kept"] == 0 and f["occ"] == tmc.PAIR_KEYS + tmc.PAIR_SINGLES
    assert s["evicted"] > s["distinct"] == tmc.PAIR_KEYS + 3 * tmc.PAIR_SINGLES + 400
    assert s["max_occ"] <= 0.87 * tmc.AG_SLOTS


def test_keep_top_class_only(oracle_h3):
    ids = tmc.case("keep_top_class_only")["ids"][0]
    s = tmc.simulate(ids)
    assert [f["round"] for f in s["flushes"]] == [5, 10, 15]
    for n, f in enumerate(s["flushes"], 1):
        # the light keys (2-3 rows since the last flush) and the heavy ones (4-7 rows per interval, resident since the
        # first flush) are 600 together: only the heavy class fits under AG_KEEP_MAX
        assert f["hist"][1] == tmc.TOP_LIGHT and sum(f["hist"][2:]) == tmc.TOP_HEAVY
        assert all(4 * n <= f["counts"][k] <= 7 * n for k in range(tmc.TOP_HEAVY))
        assert all(2 <= f["counts"][k] <= 3 for k in range(tmc.TOP_HEAVY, tmc.TOP_HEAVY + tmc.TOP_LIGHT))
        assert f["kf"] == 2 and f["kept"] == tmc.TOP_HEAVY and tmc.TOP_HEAVY + tmc.TOP_LIGHT > tmc.AG_KEEP_MAX
    assert s["distinct"] < s["evicted"]
    assert s["max_occ"] <= 0.87 * tmc.AG_SLOTS


def test_round_overflows_table(oracle_h3):
    ids = tmc.case("round_overflows_table")["ids"][0]
    assert ids.size == 8192 == np.unique(ids).size
    # rounds 1-3 insert 3072 keys without a flush (<= AG_FLUSH_AT), the 4th brings 1024 more than the 761 free slots
    assert 3 * tmc.AG_THREADS <= tmc.AG_FLUSH_AT and tmc.AG_SLOTS - 3 * tmc.AG_THREADS < tmc.AG_THREADS
    for half in (ids[:4096], ids[4096:]):   # the stage case: either rank's span does the same
        assert np.unique(half).size == 4096


def test_bucket_cap_sweep(oracle_h3):
    c = tmc.case("bucket_cap_sweep")
    ids = c["ids"][0]
    s = tmc.simulate(ids)
    assert ids.size == 8192 and s["distinct"] == 6000
    n_agg = int((ids >= 0).sum())
    assert n_agg // (2 * tmc.AG_BINS * 8) == 1   # the first batch's capacity is max(floor, this): the floor from 1 on
    assert [f["round"] for f in s["flushes"]][:1] == [4]
    assert s["max_occ"] <= 0.87 * tmc.AG_SLOTS
    # 6000 or more evicted aggregates over 256 buckets: a floor of 1 must overflow (pigeonhole), one of 4096 cannot
    assert s["evicted"] >= 6000 > tmc.AG_BINS * 8 and s["evicted"] <= n_agg < 4096 * tmc.AG_BINS
    assert tmc.CAP_SWEEP == (1, 2, 8, 16, 24, 32, 64, 4096)


def test_cap_adapts(oracle_h3):
    c = tmc.case("cap_adapts")
    a, b, cc = c["ids"]
    assert np.unique(a).size == 50 and np.array_equal(b, tmc.case("bucket_cap_sweep")["ids"][0]) and np.array_equal(b, cc)
    assert (c["batches"][2]["ts_us"] - c["batches"][1]["ts_us"]).min() > -3 * tmc.MINUTE   # (a minute later, same windows)
    k1, k2 = tmc.keys_of(c["batches"][1], 9), tmc.keys_of(c["batches"][2], 9)
    assert np.array_equal(k1[0], k2[0]) and np.array_equal(k1[1], k2[1])


def test_bin_reduce_emits(oracle_h3):
    c = tmc.case("bin_reduce_emits")
    ids = c["ids"][0]
    assert ids.size == tmc.EMIT_ROWS >= 1_000_000 and np.unique(ids).size == tmc.EMIT_DISTINCT >= 900_000
    cells, ws = tmc.keys_of(c["batches"][0], c["res"])
    assert np.unique(cells).size == tmc.EMIT_DISTINCT and np.unique(ws).size == 1
    # every k_agg workgroup of a 256-CU device streams a span of 8 rounds: 640 fresh keys a round (520 never seen, 120
    # of another span), one flush after the 5th at 3200 keys (84% of the slots), none later
    span = tmc.emit_span()
    assert span == 8 * tmc.AG_THREADS and ids.size % span == 0
    rounds = ids.reshape(-1, tmc.AG_THREADS)
    for r in range(0, rounds.shape[0], 37):
        u = np.unique(rounds[r])
        assert tmc.EMIT_NEW + tmc.EMIT_OLD - 4 <= u.size <= tmc.EMIT_NEW + tmc.EMIT_OLD
        old = u[(u < r * tmc.EMIT_NEW)]
        assert (old < (r - 7) * tmc.EMIT_NEW).all()   # the keys seen before come from another span
    for i in range(0, ids.size, 29 * span):
        s = tmc.simulate(ids[i:i + span])
        assert [f["round"] for f in s["flushes"]] == [5] and s["max_occ"] <= 0.84 * tmc.AG_SLOTS
    # what the buckets receive: more than AG_FLUSH_AT keys and more than four rounds of records each -- the emission
    # at the end of the 4th round is followed by inserts into the cleared table -- and fewer than two emissions' worth
    rec = tmc.emit_bucket_records(c)
    assert rec.min() > 4 * tmc.AG_THREADS + 100 and rec.max() < 2 * (tmc.AG_FLUSH_AT + 1)
    assert tmc.bucket_counts(cells, ws).min() > tmc.AG_FLUSH_AT
    # keys with records in two spans: those whose records straddle a bucket's emission leave k_bin_reduce twice
    assert rec.sum() - tmc.EMIT_DISTINCT > 50_000
    k2 = tmc.keys_of(c["batches"][1], c["res"])
    assert np.array_equal(cells, k2[0]) and np.array_equal(ws, k2[1])


def test_many_windows_on_spill(oracle_h3):
    c = tmc.case("many_windows_on_spill")
    cells, ws = tmc.keys_of(c["batches"][0], c["res"])
    assert np.unique(ws).size == 300 and np.unique(np.rec.fromarrays([cells, ws], names="c,w")).size == 8192
