"""GPU: the tiles sink's update statements BSON-encoded on the MI355X.

Bar: bit-exact -- every statement equals the bytes pymongo encodes for the reference's UpdateOne
(reference heatmap_stream.py:164-196; pymongo/synchronous/bulk.py add_update builds {q, u, multi, upsert}).
"""
import os
import time

import numpy as np
import pytest

from test_stream_host import _reference_statements

pytestmark = pytest.mark.gpu


def _split(buf, offs):
    return [buf[offs[i]:offs[i + 1]].tobytes() for i in range(offs.size - 1)]


@pytest.mark.parametrize("city", ["ath", "greater-" * 40 + "αθήνα"])
def test_c1_batch_statements_match_pymongo(city):
    """C1 through the GPU encoder; a CITY of 330 bytes takes the unstaged encoder (k_tile_docs_direct)."""
    from mobheat import HeatmapEngine, synth
    eng = HeatmapEngine(h3_res=8)
    res = eng.process_batch(0, **synth.c1_boston())
    buf, offs = eng.encode_tile_updates(city, 45)
    assert offs.size == len(res.tiles) + 1 > 100
    assert _split(buf, offs) == _reference_statements(res.tiles, city, 8, 45)
    eng.close()


@pytest.mark.parametrize("tz", ["EET-2EEST,M3.5.0/3,M10.5.0/4", "UTC"])
def test_stream_statements_local_time_and_dst(tz):
    """Several batches around the EU DST change (2025-10-26 01:00 UTC), pyspark's naive local datetimes."""
    from mobheat import HeatmapEngine
    old = os.environ.get("TZ")
    os.environ["TZ"] = tz
    time.tzset()
    try:
        rng = np.random.default_rng(41)
        eng = HeatmapEngine(h3_res=10, tile_minutes=5)
        t0 = 1761440100 * 1_000_000 - 20 * 60_000_000
        for e in range(4):
            n = 30000
            b = dict(lat=rng.uniform(37.90, 38.05, n), lon=rng.uniform(23.60, 23.85, n),
                     ts_us=t0 + e * 10 * 60_000_000 + rng.integers(0, 15 * 60_000_000, n), speed=rng.uniform(0, 90, n),
                     speed_valid=rng.random(n) > 0.3, vkey=rng.integers(0, 300, n).astype(np.uint64), row_valid=None)
            res = eng.process_batch(e, **b)
            buf, offs = eng.encode_tile_updates("αθήνα", 45)
            assert _split(buf, offs) == _reference_statements(res.tiles, "αθήνα", 10, 45)
        eng.close()
    finally:
        if old is None:
            del os.environ["TZ"]
        else:
            os.environ["TZ"] = old
        time.tzset()


def test_large_batch_statements_and_device_copy():
    """2e6 events at res 8 (~2e6 tiles): every statement equals the host execution of the same encoder, a
    random sample equals pymongo's bytes, and the device-resident copy equals the host one."""
    import ctypes
    from mobheat import HeatmapEngine, _lib
    from mobheat.engine import TileRows
    rng = np.random.default_rng(42)
    n = 2_000_000
    eng = HeatmapEngine(h3_res=8)
    res = eng.process_batch(0, lat=np.degrees(np.arcsin(rng.uniform(-1, 1, n))), lon=rng.uniform(-180, 180, n),
                            ts_us=1759572000_000_000 + rng.integers(0, 15 * 60_000_000, n), speed=rng.uniform(0, 80, n),
                            speed_valid=rng.random(n) > 0.1, vkey=rng.integers(0, 50000, n).astype(np.uint64))
    buf, offs = eng.encode_tile_updates("ath", 45)
    hb, ho = _lib.tile_statements_selftest(res.tiles, "ath", 8, 45, eng.tile_us)
    np.testing.assert_array_equal(offs, ho)
    np.testing.assert_array_equal(buf, hb)
    pick = rng.choice(len(res.tiles), 2000, replace=False)
    sub = TileRows(**{f: getattr(res.tiles, f)[pick] for f in TileRows.__dataclass_fields__})
    assert [buf[offs[i]:offs[i + 1]].tobytes() for i in pick] == _reference_statements(sub, "ath", 8, 45)
    pb, po, nd = eng.encode_tile_updates_device("ath", 45)
    assert nd == len(res.tiles)
    dev_offs = np.zeros(nd + 1, np.int64)
    dev_buf = np.zeros(int(offs[-1]), np.uint8)
    _lib.check(_lib.load().hm_memcpy(dev_offs.ctypes.data, po, dev_offs.nbytes, 1))
    _lib.check(_lib.load().hm_memcpy(dev_buf.ctypes.data, pb, dev_buf.nbytes, 1))
    np.testing.assert_array_equal(dev_offs, offs)
    np.testing.assert_array_equal(dev_buf, buf)
    eng.close()
    del ctypes


def test_streamed_statements_land_in_pieces_and_feed_the_wire_sink():
    """HM_MEM_HOST_STREAM (hm_statements_wait): the offsets are there when the encode returns, the bytes land in pieces
    (>= 32 MiB, at most 64) -- after landed(offs[k]) statements [0, k) equal the synchronous encode's; a wait past the
    end or without a streamed encode is refused; a sink fed command by command as they land (wire.WireMongoSink, each
    command's bytes captured as send_statements is called) sends the synchronous encode's bytes."""
    from mobheat import HeatmapEngine
    rng = np.random.default_rng(44)
    n = 1_500_000
    eng = HeatmapEngine(h3_res=9)
    eng.process_batch(0, lat=np.degrees(np.arcsin(rng.uniform(-1, 1, n))), lon=rng.uniform(-180, 180, n),
                      ts_us=1759572000_000_000 + rng.integers(0, 15 * 60_000_000, n), speed=rng.uniform(0, 80, n),
                      speed_valid=rng.random(n) > 0.1, vkey=rng.integers(0, 50000, n).astype(np.uint64))
    ref_buf, ref_offs = eng.encode_tile_updates("ath", 45, copy=True)
    assert ref_buf.size > (64 << 20)   # (several pieces)
    buf, offs, landed = eng.encode_tile_updates_streamed("ath", 45)
    np.testing.assert_array_equal(offs, ref_offs)
    seen = []
    for k in np.linspace(0, offs.size - 1, 9).astype(int)[1:]:
        landed(int(offs[k]))
        seen.append(buf[: offs[k]].tobytes() == ref_buf[: ref_offs[k]].tobytes())
    assert all(seen)
    with pytest.raises(RuntimeError, match="bytes of"):
        landed(int(offs[-1]) + 1)
    # the wire sink, command by command: each command's bytes as send_statements sees them when it is called
    from mobheat import wire

    class Capture(wire.WireMongoSink):
        def __init__(self):
            self.sent = []

        def send_statements(self, collection, buf, lo, hi, n_statements, write_concern=None):
            self.sent.append(bytes(buf[lo:hi]))
            return {"ok": 1.0, "n": n_statements}
    buf, offs, landed = eng.encode_tile_updates_streamed("ath", 45)
    sink = Capture()
    sink.update_statements("tiles", buf, offs, landed=landed)
    assert len(sink.sent) > 10 and b"".join(sink.sent) == ref_buf.tobytes()
    eng.encode_tile_updates("ath", 45)   # (synchronous: nothing left to wait for)
    with pytest.raises(RuntimeError, match="without a streamed encode"):
        landed(1)
    eng.close()


def test_empty_batch_and_errors():
    from mobheat import HeatmapEngine
    eng = HeatmapEngine(h3_res=8)
    z = np.zeros(0)
    eng.process_batch(0, lat=z, lon=z, ts_us=np.zeros(0, np.int64))
    buf, offs = eng.encode_tile_updates("ath", 45)
    assert buf.size == 0 and offs.tolist() == [0]
    with pytest.raises(RuntimeError, match="city"):
        eng.encode_tile_updates("x" * (1 << 20 | 1), 45)   # (a CITY of more than 1 MiB)
    eng.close()


def test_position_statements_match_pymongo():
    """The positions half: a C5-like batch (vehicles with several updates and ties) through foreach's columns;
    the GPU statements equal pymongo's bytes for the reference's positions_latest UpdateOne ops."""
    import bson
    import pandas as pd
    from mobheat import HeatmapEngine, stream
    rng = np.random.default_rng(43)
    n = 200_000
    ts = 1759572000_000_000 + rng.integers(0, 60, n) * 1_000_000 + rng.integers(0, 3, n) * 1000
    df = pd.DataFrame({"provider": rng.choice(["mbta", "opensky"], n),
                       "vehicleId": [f"V{int(x)}" for x in rng.integers(0, 20000, n)],
                       "lat": rng.uniform(42.2, 42.45, n), "lon": rng.uniform(-71.2, -70.95, n),
                       "speedKmh": rng.uniform(0, 80, n), "eventTs": pd.to_datetime(ts, unit="us")})
    cols = stream.batch_columns(df)
    eng = HeatmapEngine(h3_res=8)
    res = eng.process_batch(0, cols["lat"], cols["lon"], cols["ts_us"], cols["speed"], cols["speed_valid"],
                            cols["vkey"], cols["row_valid"])
    rows = res.latest_rows
    assert rows.size > 20000   # ties: several rows for some vehicles
    t = cols["ts_us"][rows]
    buf, offs = eng.encode_position_updates(cols["provider_uniques"], cols["vehicle_uniques"], t)
    exp = [bson.encode({"q": op._filter, "u": op._doc, "multi": False, "upsert": True})
           for op in stream.position_ops(cols, rows)]
    assert _split(buf, offs) == exp
    with pytest.raises(RuntimeError, match="dictionaries"):
        eng.encode_position_updates(cols["provider_uniques"][:1], cols["vehicle_uniques"], t)
    eng.close()


DST_TZ = "EET-2EEST,M3.5.0/3,M10.5.0/4"
DST_CHANGE_US = 1761440400 * 1_000_000   # 2025-10-26 01:00:00 UTC: 04:00 EEST becomes 03:00 EET


@pytest.mark.parametrize("tile_minutes", [60, 1440])
def test_hour_and_day_windows_around_the_dst_change(tile_minutes):
    """Windows of 60 minutes (the DST change is exactly the end of the window [00:00, 01:00) UTC, whose local windowStart
    and windowEnd are both 03:00) and of one day (the change lies inside the window) under a local zone with DST, two
    batches: every statement equals pymongo's bytes."""
    import bson
    from mobheat import HeatmapEngine
    old = os.environ.get("TZ")
    os.environ["TZ"] = DST_TZ
    time.tzset()
    try:
        tile = tile_minutes * 60_000_000
        rng = np.random.default_rng(45 + tile_minutes)
        eng = HeatmapEngine(h3_res=9, tile_minutes=tile_minutes)
        first = DST_CHANGE_US // tile * tile - 2 * tile   # two windows before the one that holds or ends at the change
        seen = {}
        for e in range(2):
            n = 600
            b = dict(lat=37.90 + rng.integers(0, 40, n) / 256.0, lon=23.60 + rng.integers(0, 8, n) / 256.0,
                     ts_us=first + rng.integers(0, 5, n) * tile + rng.integers(0, tile, n), speed=rng.integers(0, 720, n) / 8.0,
                     speed_valid=rng.random(n) > 0.3, vkey=rng.integers(0, 50, n).astype(np.uint64), row_valid=None)
            res = eng.process_batch(e, **b)
            assert len(set(res.tiles.window_start_us.tolist())) == 5 and res.n_late == 0
            buf, offs = eng.encode_tile_updates("αθήνα", 45)
            docs = _split(buf, offs)
            assert docs == _reference_statements(res.tiles, "αθήνα", 9, 45)
            for d, ws in zip(docs, res.tiles.window_start_us.tolist()):
                u = bson.decode(d)["u"]["$set"]
                seen[ws] = (u["windowStart"], u["windowEnd"])
        eng.close()
        if tile_minutes == 60:   # the window that ends at the change: 03:00 EEST to 03:00 EET
            s, e = seen[DST_CHANGE_US - tile]
            assert s == e and (s.hour, s.minute) == (3, 0)
            s, e = seen[DST_CHANGE_US]
            assert (e - s).total_seconds() == 3600
        else:                    # the day that holds the change: 03:00 EEST to 02:00 EET the next day, 25 hours long
            s, e = seen[DST_CHANGE_US // tile * tile]
            assert (s.hour, e.hour) == (3, 2) and (e - s).total_seconds() == 23 * 3600
    finally:
        if old is None:
            del os.environ["TZ"]
        else:
            os.environ["TZ"] = old
        time.tzset()


def test_window_starts_off_the_second_are_refused():
    """tile_us = 1 000 001: the windows do not start on whole seconds, which the statements' datetimes cannot hold --
    encode_tile_updates refuses them, and the engine goes on working."""
    from mobheat import HeatmapEngine
    from oracle.spark_oracle import SparkHeatmapOracle
    from test_gpu_parity import assert_batch_equal
    eng = HeatmapEngine(h3_res=9, tile_us=1_000_001)
    ora = SparkHeatmapOracle(h3_res=9, tile_us=1_000_001)
    rng = np.random.default_rng(46)
    for e in range(2):
        n = 300
        b = dict(lat=37.90 + rng.integers(0, 40, n) / 256.0, lon=np.full(n, 23.625), ts_us=1759572000_000_000 + e * 1_000_000 +
                 rng.integers(0, 3_000_000, n), speed=rng.integers(0, 720, n) / 8.0, speed_valid=rng.random(n) > 0.3,
                 vkey=rng.integers(0, 50, n).astype(np.uint64), row_valid=None)
        res = eng.process_batch(e, **b)
        assert_batch_equal(res, ora.process_batch(**b))
        assert len(res.tiles) > 0
        with pytest.raises(RuntimeError, match="not a whole second"):
            eng.encode_tile_updates("ath", 45)
    eng.close()


def _city_of(nbytes):
    """a city of exactly nbytes UTF-8 bytes, two-byte letters first"""
    return "α" * (nbytes // 2) + "x" * (nbytes % 2)


def _max_doc(city, h3_res, tile_us, ws):
    """hm_encode_tile_updates' max_doc: the longest statement this city and resolution can produce (16 hex digits,
    an int64 count), from the host execution of the encoder"""
    from mobheat import _lib
    from mobheat.engine import TileRows
    one = TileRows(cell=np.array([0xFFFFFFFFFFFFFFFF], np.uint64), window_start_us=np.array([ws], np.int64),
                   window_end_us=np.array([ws + tile_us], np.int64), count=np.array([1 << 62], np.int64),
                   avg_speed=np.zeros(1), speed_null=np.ones(1, bool), avg_lon=np.zeros(1), avg_lat=np.zeros(1))
    _, offs = _lib.tile_statements_selftest(one, city, h3_res, 45, tile_us)
    return int(offs[1])


TD_THREADS, TD_MAX_DOC = 128, 576   # csrc/bson_docs.h


def _staging_lds(max_doc):
    return TD_THREADS * ((max_doc + 15) & ~15) + 32   # csrc/api_sink.h


@pytest.mark.parametrize("h3_res", [9, 10])
def test_city_lengths_on_both_sides_of_the_encoder_launch_thresholds(h3_res):
    """hm_encode_tile_updates stages the statements in LDS sized by the longest possible statement max_doc (3 bytes per
    city byte): up to 496 within 64 KiB of dynamic LDS, from 497 on with more (the launch raises the kernel's limit first),
    above TD_MAX_DOC = 576 by k_tile_docs_direct without staging.  The longest city on the near side of either threshold
    and the one a byte longer, n = 1, 128, 129 and 257 tiles (one workgroup, one full, one more, three): byte for byte
    pymongo's statements and the host execution of the encoder."""
    from mobheat import HeatmapEngine, _lib
    T0 = 1759572000_000_000
    tile = 300_000_000
    base = _max_doc("", h3_res, tile, T0)
    assert _max_doc("x", h3_res, tile, T0) == base + 3 and _max_doc("α", h3_res, tile, T0) == base + 6
    sides = []   # (city bytes, staged, lds above 64 KiB)
    for limit in (496, TD_MAX_DOC):
        c = (limit - base) // 3
        sides += [c, c + 1]
        assert base + 3 * c <= limit < base + 3 * (c + 1)
    lds = [_staging_lds(base + 3 * c) for c in sides]
    assert lds[0] <= 65536 < lds[1] and lds[2] > 65536 and base + 3 * sides[2] <= TD_MAX_DOC < base + 3 * sides[3]
    assert lds[2] == TD_THREADS * TD_MAX_DOC + 32   # the largest staging buffer any launch asks for: 73 760 bytes
    eng = HeatmapEngine(h3_res=h3_res)
    rng = np.random.default_rng(47 + h3_res)
    try:
        for e, n in enumerate((1, 128, 129, 257)):
            # n cells 1/128 degree apart, a few rows in each, one window
            idx = np.repeat(np.arange(n), 3)
            b = dict(lat=37.0 + idx / 128.0, lon=np.full(idx.size, 23.75), ts_us=T0 + e * 1_000_000 + np.arange(idx.size),
                     speed=rng.integers(0, 720, idx.size) / 8.0, speed_valid=rng.random(idx.size) > 0.3,
                     vkey=rng.integers(0, 50, idx.size).astype(np.uint64), row_valid=None)
            res = eng.process_batch(e, **b)
            assert len(res.tiles) == n
            for c in sides:
                city = _city_of(c)
                assert len(city.encode()) == c and _max_doc(city, h3_res, tile, T0) == base + 3 * c
                buf, offs = eng.encode_tile_updates(city, 45, copy=True)
                hb, ho = _lib.tile_statements_selftest(res.tiles, city, h3_res, 45, tile)
                np.testing.assert_array_equal(offs, ho, err_msg=f"n {n}, city of {c} bytes")
                np.testing.assert_array_equal(buf, hb, err_msg=f"n {n}, city of {c} bytes")
                assert _split(buf, offs) == _reference_statements(res.tiles, city, h3_res, 45), f"n {n}, city of {c} bytes"
    finally:
        eng.close()
