"""GPU: the input decode -- hm_decode_json (Kafka values) and hm_arrow_columns (Arrow frames) -- pinned at its size,
alignment and dictionary edges.  Every comparison is exact: bit patterns for doubles (NaN equal to NaN), equality for
everything else.  The inputs and the comparisons are in tests/input_edge_cases.py.

References: oracle/kafka_oracle.py (Python json + pandas) for decoded values; float(text) for number tokens (the
integer token -0 is +0.0, the double of the integer 0, as the oracle and Jackson have it); plain Python for the
dictionaries (exactly the distinct non-null strings, one code each, every valid row's vkey decoding to the row's two
strings); _lib.json_records_selftest (the same json_decode.h run on the host) where the oracle cannot speak: years outside
pandas' 1678-2261 and which records are flagged unsupported; stream.batch_columns for the Arrow forms.

1. numbers: the host test's 206k (significand, exponent) pairs in three spellings each, the zero / overflow / underflow /
   subnormal edge tokens, and tokens of 20-40 digits far from and exactly on a rounding boundary;
2. timestamps: ~2e4 strings (month ends, leap days, negative instants, fractions, zones, separators, blanks, escapes,
   blank padding past 64 bytes, and the invalid forms);
3. alignment: 40 records starting at every offset of a 16-byte window, as host input and as device input (pointer advanced
   / offsets[0] advanced), the buffer ending with the last record;
4. sizes: n = 0 .. 2^20 + 4097 on and off 64 / 256 / 4096 / the 2^20-thread grid cap, three id patterns, nulls placed so
   that a wave's first lane is not live and one wave holds a single live lane;
5. dictionary contents: "" against null, one-byte runs, strings differing in byte 7 / 8 / 15 / 16 / last, a against a\\0,
   64 KiB strings, escaped against raw spellings, scalars against their texts, an all-null column, 300-row splices;
6. dictionary sizing across batches of one engine (20 -> 50,000 -> 3 -> 70,000 -> 70,000 -> 0 -> 1 -> 2^20 distinct);
7. Arrow forms: validity bitmaps from bit 0..7, string / large_string, sliced offsets, absent columns;
8. decreasing offsets inside the buffer are refused with HM_E_INVALID and the engine goes on.
"""
import ctypes
import itertools
import random

import numpy as np
import pytest

import input_edge_cases as X
from mobheat import _lib

pytestmark = pytest.mark.gpu
STRIDE = X.STRIDE


def _d2h(ptr, n, dtype):
    out = np.zeros(max(n, 1), dtype)
    if n:
        _lib.check(_lib.load().hm_memcpy(out.ctypes.data, ptr, n * out.itemsize, 1), None, "hm_memcpy")
    return out[:n]


def _read(kb, n):
    """the KafkaBatch's device columns on the host"""
    b = kb.batch
    assert b.n == n and b.memory == _lib.HM_MEM_DEVICE
    return X.Decoded(lat=_d2h(b.lat, n, np.float64), lon=_d2h(b.lon, n, np.float64), ts=_d2h(b.ts_us, n, np.int64),
                     speed=_d2h(b.speed, n, np.float64), sv=_d2h(b.speed_valid, n, np.uint8),
                     rv=_d2h(b.row_valid, n, np.uint8), vkey=_d2h(b.vkey, n, np.uint64), providers=kb.providers,
                     vehicles=kb.vehicles)


def _decode(eng, buf, offs):
    """HeatmapEngine.decode_json (host input; unsupported records spliced) -> (Decoded, KafkaBatch)"""
    kb = eng.decode_json(buf, offs)
    return _read(kb, len(offs) - 1), kb


def _decode_values(eng, values):
    buf, offs = _lib.pack_values(values)
    return _decode(eng, buf, offs)


def _raw_decode(eng, n, memory, flags, bytes_ptr, offs_ptr):
    """lib.hm_decode_json on an HmJsonIn built by hand -> (rc, HmJsonOut)"""
    jin = _lib.HmJsonIn(n=n, memory=memory, flags=flags, bytes=bytes_ptr, offsets=offs_ptr)
    jout = _lib.HmJsonOut()
    return _lib.load().hm_decode_json(eng._ctx, ctypes.byref(jin), ctypes.byref(jout)), jout


def _unsupported_rows(eng, buf, offs):
    """the rows hm_decode_json lists for the host (HM_JSON_SPLICE), as it returns them"""
    rc, jout = _raw_decode(eng, len(offs) - 1, _lib.HM_MEM_HOST, _lib.HM_JSON_SPLICE, buf.ctypes.data, offs.ctypes.data)
    assert rc == 0
    m = int(jout.n_unsupported)
    if m == 0:
        return np.zeros(0, np.int64)
    return np.ctypeslib.as_array(ctypes.cast(jout.unsupported_rows, ctypes.POINTER(ctypes.c_int64)), shape=(m,)).copy()


def _arrow(eng, table):
    """HeatmapEngine.arrow_columns of an Arrow table -> (Decoded, KafkaBatch)"""
    from mobheat import stream
    cols = stream.ArrowColumns(table, table.num_rows)   # (keeps the buffers alive over the call)
    kb = eng.arrow_columns(cols.struct)
    return _read(kb, table.num_rows), kb


def _n_valid_and_latest(eng, kb):
    """hm_process_batch on the decoded device batch: (n_valid, n_latest)"""
    out = _lib.HmBatchOut()
    _lib.check(_lib.load().hm_process_batch(eng._ctx, 0, ctypes.byref(kb.batch), _lib.HM_MEM_HOST, ctypes.byref(out)),
               eng._ctx, "hm_process_batch")
    return int(out.n_valid), int(out.n_latest)


@pytest.fixture(scope="module")
def eng():
    from mobheat import HeatmapEngine
    e = HeatmapEngine(h3_res=8)
    yield e
    e.close()


@pytest.fixture
def fresh():
    from mobheat import HeatmapEngine
    e = HeatmapEngine(h3_res=8)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------
# 1. numbers on the device
# ---------------------------------------------------------------------------------------------------------
def test_numbers_of_up_to_19_digits_equal_float_of_their_text(eng):
    """decimal_to_double_bits on the device (__umul64hi, __clzll, the __constant__ table) over the host test's 206k
    (w, q), each as WeQ, with the point inside the digits and as 0.000W000E+Q, plus the edge tokens: no record is left to
    the host and every value has float(text)'s bits."""
    w, q = X.number_population()
    rng = random.Random(6)
    tokens = [s for a, b in zip(w, q) for s in X.spellings(a, b, rng)] + list(X.NUMBER_EDGES)
    vals, exp = X.number_records(tokens)
    d, kb = _decode_values(eng, vals)
    assert kb.n_spliced == 0 and kb.n_malformed == 0
    show = lambda k: vals[k]   # noqa: E731
    X._first_bad(X.same_f64(d.lat, exp[:, 0]), "lat", show)
    X._first_bad(X.same_f64(d.lon, exp[:, 1]), "lon", show)
    X._first_bad(X.same_f64(d.speed, exp[:, 2]), "speedKmh", show)
    assert d.sv.all() and d.rv.all()
    assert np.signbit(exp.reshape(-1)[len(tokens) - 7]) and not np.signbit(exp.reshape(-1)[len(tokens) - 8])   # -0.0, -0


def test_long_number_tokens_decode_or_are_spliced(eng):
    """Tokens of 20-40 digits: far from a rounding boundary the device decodes them (not listed); an exact halfway value
    of more than 19 digits, bare or followed by more digits, is listed -- exactly the rows the host run of the same code
    flags, ascending -- and after the splice still has float(text)'s bits.  Without HM_JSON_SPLICE the batch is refused."""
    far, half = X.long_tokens()
    vals_f, exp_f = X.number_records(far)
    vals_h, exp_h = X.number_records(half)
    order = np.random.default_rng(3).permutation(len(vals_f) + len(vals_h))
    vals = [(vals_f + vals_h)[k] for k in order]
    exp = np.concatenate([exp_f, exp_h])[order]
    want_rows = np.flatnonzero(order >= len(vals_f))
    buf, offs = _lib.pack_values(vals)
    rows = _unsupported_rows(eng, buf, offs)
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(rows, X.host_columns(_lib.json_records_selftest(vals))["unsupported"])
    d, kb = _decode(eng, buf, offs)
    assert kb.n_spliced == want_rows.size and kb.n_malformed == 0
    show = lambda k: vals[k]   # noqa: E731
    X._first_bad(X.same_f64(d.lat, exp[:, 0]), "lat", show)
    X._first_bad(X.same_f64(d.lon, exp[:, 1]), "lon", show)
    X._first_bad(X.same_f64(d.speed, exp[:, 2]), "speedKmh", show)
    assert d.rv.all() and d.sv.all()
    rc, jout = _raw_decode(eng, len(vals), _lib.HM_MEM_HOST, 0, buf.ctypes.data, offs.ctypes.data)
    assert rc == _lib.HM_E_UNSUPPORTED and jout.n_unsupported == want_rows.size


# ---------------------------------------------------------------------------------------------------------
# 2. timestamps on the device
# ---------------------------------------------------------------------------------------------------------
def test_timestamps_equal_the_oracle_and_the_host_run(eng):
    from oracle import kafka_oracle
    texts, in_range = X.timestamp_strings()
    vals = X.timestamp_records(texts)
    d, kb = _decode_values(eng, vals)
    assert kb.n_spliced == 0 and kb.n_malformed == 0 and 15_000 < len(vals) < 30_000
    show = lambda k: texts[k]   # noqa: E731
    host = X.host_columns(_lib.json_records_selftest(vals))
    X._first_bad(d.rv.astype(bool) == host["row_valid"], "eventTs is null (host run)", show)
    X._first_bad(d.ts == host["ts_us"], "eventTs (host run)", show)
    exp = kafka_oracle.decode_values(vals)
    X._first_bad((d.rv.astype(bool) == exp["row_valid"]) | ~in_range, "eventTs is null (oracle)", show)
    X._first_bad((d.ts == exp["ts_us"]) | ~in_range, "eventTs (oracle)", show)
    # the cases by name
    at = {s: k for k, s in enumerate(texts)}
    assert d.ts[at["1969-12-31T23:59:59.999999Z"]] == -1 and d.ts[at["1969-12-31T23:59:59.9999999"]] == -1
    assert d.ts[at["1900-01-01"]] == -2_208_988_800_000_000 and d.ts[at["0001-01-01"]] == -62_135_596_800_000_000
    assert d.rv[at["2024-02-29"]] and d.rv[at["2000-02-29"]] and not d.rv[at["2100-02-29"]] and not d.rv[at["1970-02-29"]]
    assert d.rv[at["2100-02-28T12:34:56.123456789+18:00"]] and d.rv[at["2024-02-29T12:34:56Z".ljust(64)]]
    t29 = 1_709_210_096_000_000   # 2024-02-29T12:34:56Z
    for pad in ("2024-02-29T12:34:56Z".ljust(65), "2024-02-29T12:34:56Z".rjust(65), "2024-02-29T12:34:56Z".center(65),
                "\\u0020" * 50 + "2024-02-29T12:34:56Z"):
        assert d.rv[at[pad]] and d.ts[at[pad]] == t29, pad
    assert d.rv[at[" " * 1000 + "2024-02-29"]] and d.rv[at["1600-02-29T12:00:00Z".rjust(80)]]
    assert not d.rv[at["2024-02-29T12:34:56" + " " * 50 + "Z"]] and not d.rv[at[" " * 65]]
    for bad in ("2024-13-01", "2024-02-30", "2024-02-29T24:34:56", "2024-02-29T12:34:60", "2024-02-29T12:34:56.1234567890",
                "1970-01-31Z", "1970-01-31+02:00", "2" * 65, "2024-02-29T12:34:56Z" + "x" * 45):
        assert not d.rv[at[bad]], bad
    assert 9_000 < int(d.rv.sum()) < len(vals) - 3_000


# ---------------------------------------------------------------------------------------------------------
# 3. alignment
# ---------------------------------------------------------------------------------------------------------
def _rows(d, sl):
    return X.Decoded(d.lat[sl], d.lon[sl], d.ts[sl], d.speed[sl], d.sv[sl], d.rv[sl], d.vkey[sl], d.providers, d.vehicles)


def test_records_at_every_offset_of_a_16_byte_window(eng):
    """ByteReader's aligned 16-byte loads: the 40 records behind a filler record of s = 0..15 blanks (malformed: an
    all-null row), as host input, as device input with the pointer advanced by s and offsets[0] = 0, and as device input
    with offsets[0] = s; the buffer is exactly offsets[n] bytes.  Every layout gives the oracle's columns and strings."""
    import torch
    from mobheat.engine import _device_batch
    from oracle import kafka_oracle
    recs = X.alignment_records()
    n = len(recs)
    assert n >= 40
    exp = kafka_oracle.decode_values(recs)
    assert exp["n_unsupported"] == 0 and exp["n_malformed"] == 4
    assert b"k" * 1024 in exp["vehicleId"] and b"?x" in exp["vehicleId"] and "😀x".encode() in exp["vehicleId"]
    for s in range(16):
        buf, offs = X.pack_exact([b" " * s] + recs)
        assert buf.size == offs[-1]
        d, kb = _decode(eng, buf, offs)
        assert kb.n_malformed == 5 and kb.n_spliced == 0
        assert not d.rv[0] and not d.sv[0] and np.isnan(d.lat[0]) and np.isnan(d.lon[0]) and d.vkey[0] == 0
        X.check_oracle(_rows(d, slice(1, None)), exp, recs)
        t = torch.from_numpy(buf).cuda()
        assert t.numel() == offs[-1] and t.data_ptr() % 16 == 0
        for o, ptr in ((offs[1:] - s, t.data_ptr() + s), (offs[1:], t.data_ptr())):
            to = torch.from_numpy(np.ascontiguousarray(o)).cuda()
            torch.cuda.synchronize()
            rc, jout = _raw_decode(eng, n, _lib.HM_MEM_DEVICE, _lib.HM_JSON_SPLICE, ptr, to.data_ptr())
            assert rc == 0, (s, _lib.load().hm_last_error(eng._ctx))
            assert jout.n_malformed == 4 and jout.n_unsupported == 0
            X.check_oracle(_read(_device_batch(jout), n), exp, recs)


# ---------------------------------------------------------------------------------------------------------
# 4. sizes
# ---------------------------------------------------------------------------------------------------------
def _sample_rows(n):
    rng = np.random.default_rng(n)
    pick = np.concatenate([np.arange(0, 300), np.arange(STRIDE - 100, STRIDE + 100), rng.integers(0, n, 500)])
    return np.unique(pick[pick < n])


def test_fixed_width_json_template_equals_the_oracle(eng):
    """~1000 records of the largest fixed-width batch (its first rows, the rows around the grid cap, random rows): the
    numpy-computed expectation equals the oracle's decode of the same bytes, and so does the device's."""
    from oracle import kafka_oracle
    n = X.SIZES[-1]
    buf, offs, e = X.json_fixed(X.pattern_ids("wrap", n))
    rows = _sample_rows(n)
    vals = X.fixed_sample_values(buf, rows)
    exp = kafka_oracle.decode_values(vals)
    es = X.sample_of(e, rows)
    prov, veh = X.fixed_strings(es)
    assert exp["provider"] == prov and exp["vehicleId"] == veh and exp["n_malformed"] == 0 and exp["n_unsupported"] == 0
    for k in ("lat", "lon", "speed"):
        assert X.same_f64(exp[k], es[k]).all(), k
    for k in ("speed_valid", "ts_us", "ts_valid", "row_valid"):
        assert np.array_equal(exp[k], es[k]), k
    d, _ = _decode_values(eng, vals)
    X.check_oracle(d, exp, vals)


def test_fixed_width_arrow_template_equals_batch_columns(eng):
    from mobheat import stream
    n = X.SIZES[-1]
    t, e = X.arrow_fixed(X.pattern_ids("wrap", n))
    rows = _sample_rows(n)
    ts = t.take(rows)
    h = stream.batch_columns(ts)
    es = X.sample_of(e, rows)
    prov, veh = X.fixed_strings(es)
    enc = lambda col: [None if x is None else x.encode() for x in col.to_pylist()]   # noqa: E731
    assert enc(h["provider"]) == prov and enc(h["vehicleId"]) == veh
    assert X.same_f64(h["lat"], es["lat"]).all() and X.same_f64(h["lon"], es["lon"]).all()
    assert np.array_equal(h["speed_valid"], es["speed_valid"]) and np.array_equal(h["row_valid"], es["row_valid"])
    assert X.same_f64(np.where(h["speed_valid"], h["speed"], 0.0), es["speed"]).all()
    assert np.array_equal(h["ts_us"], es["ts_us"])
    d, _ = _arrow(eng, ts)
    X.check_values(d, es)
    X.check_strings(d, prov, veh, es["row_valid"])


@pytest.mark.parametrize("n", X.SIZES)
@pytest.mark.parametrize("pattern", X.PATTERNS)
@pytest.mark.parametrize("entry", ("json", "arrow"))
def test_sizes(eng, entry, pattern, n):
    """n on and off the block constants and past the grid cap (rows i and i + 2^20 are one lane's two passes; in `wrap`
    the lane's cached slot is right for even i and wrong for odd i), every 7th vehicleId null, row 0 and row 64 among
    them, rows 128..191 null but one.  The largest all-distinct batch also goes through hm_process_batch."""
    ids = X.pattern_ids(pattern, n)
    if entry == "json":
        buf, offs, e = X.json_fixed(ids)
        d, kb = _decode(eng, buf, offs)
        assert kb.n_malformed == 0 and kb.n_spliced == 0
    else:
        t, e = X.arrow_fixed(ids, large=pattern == "mod3")
        d, kb = _arrow(eng, t)
    X.check_fixed(d, e)
    if n == X.SIZES[-1] and pattern == "distinct":
        from mobheat import HeatmapEngine
        one = HeatmapEngine(h3_res=8)   # (a state of its own: no row is late; the decoded columns stay eng's)
        try:
            out = _lib.HmBatchOut()
            _lib.check(_lib.load().hm_process_batch(one._ctx, 0, ctypes.byref(kb.batch), _lib.HM_MEM_DEVICE,
                                                    ctypes.byref(out)), one._ctx, "hm_process_batch")
            res = one._result_counts(out)
        finally:
            one.close()
        valid = e["row_valid"] & ~np.isnan(e["lat"]) & ~np.isnan(e["lon"])   # (every coordinate is in range)
        assert res.n_in == n and res.n_valid == int(valid.sum()) and res.n_late == 0
        assert res.n_latest == int(valid.sum())   # every vehicle holds one row: each valid row is a latest row


# ---------------------------------------------------------------------------------------------------------
# 5. dictionary contents
# ---------------------------------------------------------------------------------------------------------
_JS_CASES, _ARROW_CASES = X.dictionary_cases()


@pytest.mark.parametrize("name", sorted(_JS_CASES))
def test_dictionary_contents_json(eng, name):
    from oracle import kafka_oracle
    vals = X.pair_records(_JS_CASES[name])
    exp = kafka_oracle.decode_values(vals)
    assert exp["n_malformed"] == 0 and exp["n_unsupported"] == 0
    d, kb = _decode_values(eng, vals)
    assert kb.n_spliced == 0
    X.check_oracle(d, exp, vals)
    vehs = set(X.Decoded.strings(d.vehicles))
    if name == "spellings":   # every spelling of a string shares its code
        assert vehs == {b"a/b", "😀".encode(), "ώ".encode(), b"a\\b"} and X.Decoded.strings(d.providers) == [b"p"]
    elif name == "scalars":
        assert vehs == {b"12", b"0", b"true", b"false", b"-12", b"-0"}
        assert set(X.Decoded.strings(d.providers)) == {b"p", b"false", b"-12"}
    elif name == "nul_byte":
        assert vehs == {b"a", b"a\x00", b"a\x00\x00", b"\x00", b""}
    elif name == "empty_and_null":
        assert vehs == {b"", b"a"} and d.rv.tolist() == [1, 0, 1, 0, 1, 1, 0]
    elif name == "one_byte_runs":
        assert len(vehs) == 34 + 1 and d.providers[0] == 34 + 1
    elif name == "long_64k":
        assert sorted(len(v) for v in vehs) == [1, 65535, 65536, 65536]
    elif name == "three_providers":
        assert d.providers[0] == 3 and d.vehicles[0] == 5


@pytest.mark.parametrize("large", (False, True))
@pytest.mark.parametrize("name", sorted(_ARROW_CASES))
def test_dictionary_contents_arrow(eng, name, large):
    import pyarrow as pa
    rows = _ARROW_CASES[name]
    typ = pa.large_string() if large else pa.string()
    n = len(rows)
    t = pa.table({"provider": pa.array([p for p, _ in rows], typ), "vehicleId": pa.array([v for _, v in rows], typ),
                  "lat": pa.array(np.full(n, 42.5)), "lon": pa.array(np.full(n, -71.25)),
                  "eventTs": pa.array(np.full(n, X.TS0_US), pa.timestamp("us"))})
    d, kb = _arrow(eng, t)
    enc = lambda x: None if x is None else x.encode()   # noqa: E731
    prov, veh = [enc(p) for p, _ in rows], [enc(v) for _, v in rows]
    rv = np.array([p is not None and v is not None for p, v in rows])
    X.check_strings(d, prov, veh, rv)
    assert np.array_equal(d.rv.astype(bool), rv) and (d.ts == X.TS0_US).all() and not d.sv.any()
    assert (d.lat == 42.5).all() and (d.lon == -71.25).all()


@pytest.mark.parametrize("entry", ("json", "arrow"))
def test_column_null_in_every_row(fresh, entry):
    """vehicleId null in all 300 rows: no vehicle code, every vkey 0, no valid row through hm_process_batch."""
    n = 300
    if entry == "json":
        d, kb = _decode_values(fresh, X.pair_records([('"p%d"' % (k % 3), None) for k in range(n)]))
    else:
        import pyarrow as pa
        t = pa.table({"provider": pa.array(["p%d" % (k % 3) for k in range(n)]), "vehicleId": pa.array([None] * n, pa.string()),
                      "lat": pa.array(np.full(n, 42.5)), "lon": pa.array(np.full(n, -71.25)),
                      "eventTs": pa.array(np.full(n, X.TS0_US), pa.timestamp("us"))})
        d, kb = _arrow(fresh, t)
    assert kb.vehicles[0] == 0 and set(X.Decoded.strings(d.providers)) == {b"p0", b"p1", b"p2"}
    assert not d.vkey.any() and not d.rv.any()
    assert _n_valid_and_latest(fresh, kb) == (0, 0)


@pytest.mark.parametrize("new_vehicles", (False, True))
def test_splice_of_300_rows(eng, new_vehicles):
    """300 unsupported records (more than one workgroup of k_json_patch) among 1600: with every spliced string already in
    the dictionary (n_vehicles unchanged: no re-key), and adding 300 vehicles (k_json_rekey: every other valid row's
    vkey must still name its strings)."""
    vals, prov, veh, odd = X.splice_records(new_vehicles)
    buf, offs = _lib.pack_values(vals)
    assert np.array_equal(_unsupported_rows(eng, buf, offs), odd)
    rc, jout = _raw_decode(eng, len(vals), _lib.HM_MEM_HOST, _lib.HM_JSON_SPLICE, buf.ctypes.data, offs.ctypes.data)
    assert rc == 0 and jout.n_vehicles == (411 if new_vehicles else 300) and jout.n_providers == 3
    d, kb = _decode(eng, buf, offs)
    assert kb.n_spliced == 300 and kb.n_malformed == 0
    assert kb.vehicles[0] == (711 if new_vehicles else 300)
    X.check_strings(d, prov, veh, np.ones(len(vals), bool))
    assert d.rv.all() and (d.lat == 42.5).all() and (d.lon == -71.25).all() and (d.ts == X.TS0_US).all() and not d.sv.any()
    assert _n_valid_and_latest(eng, kb)[0] == len(vals)


# ---------------------------------------------------------------------------------------------------------
# 6. dictionary sizing across batches
# ---------------------------------------------------------------------------------------------------------
def test_dictionary_sizing_across_batches(fresh):
    """One engine, JSON and Arrow batches in turn (both build jd_prov / jd_veh and size the next table from last_codes):
    20 -> 50,000 -> 3 -> 70,000 -> 70,000 -> no row -> one row -> 2^20 distinct vehicles, the last with no null
    vehicleId so that the full-size table (2^21 slots) sits at load 0.5.  Every call succeeds, every dictionary is exact."""
    steps = [("json", 20, 60), ("arrow", 50_000, 110_003), ("json", 3, 4097), ("arrow", 70_000, 150_001),
             ("json", 70_000, 150_001), ("arrow", 0, 0), ("json", 1, 1), ("json", STRIDE, STRIDE), ("arrow", 1, 1),
             ("arrow", STRIDE, STRIDE), ("json", 0, 0)]
    for entry, k, n in steps:
        i = np.arange(n, dtype=np.int64)
        ids = (i + i // max(k, 1)) % max(k, 1)   # (an id's rows differ mod 7: never all among the null rows)
        kw = dict(first=1) if n == 1 else dict(vehicle_nulls=False) if k == STRIDE else {}
        if entry == "json":
            buf, offs, e = X.json_fixed(ids, **kw)
            d, kb = _decode(fresh, buf, offs)
        else:
            t, e = X.arrow_fixed(ids, **kw)
            d, kb = _arrow(fresh, t)
        X.check_fixed(d, e)
        assert kb.vehicles[0] == k, (entry, k, n)


# ---------------------------------------------------------------------------------------------------------
# 7. Arrow forms at the small sizes
# ---------------------------------------------------------------------------------------------------------
def _check_against_batch_columns(eng, t):
    from mobheat import stream
    h = stream.batch_columns(t)
    d, kb = _arrow(eng, t)
    exp = dict(lat=h["lat"], lon=h["lon"], speed=np.where(h["speed_valid"], h["speed"], 0.0),
               speed_valid=h["speed_valid"], ts_us=h["ts_us"], row_valid=h["row_valid"])
    X.check_values(d, exp)
    enc = lambda col: [None if x is None else x.encode() for x in col.to_pylist()]   # noqa: E731
    X.check_strings(d, enc(h["provider"]), enc(h["vehicleId"]), h["row_valid"])
    assert kb.providers[0] == len(h["provider_uniques"]) and kb.vehicles[0] == len(h["vehicle_uniques"])
    return d, kb


@pytest.mark.parametrize("large", (False, True))
def test_arrow_sliced_arrays(eng, large):
    """Arrays sliced at 1..9 (validity bitmaps starting at bit 1..7, 0 and 1 of the next byte; string offsets whose first
    entry is past 0), nulls in every column, string and large_string, at lengths on and off 64 and 256."""
    t, _ = X.arrow_fixed(np.arange(400, dtype=np.int64) % 23, large=large)
    for k, m in itertools.product(range(1, 10), (1, 63, 64, 65, 256, 257)):
        ts = t.slice(k, m)
        col = ts.column("provider").chunk(0)
        assert col.offset == k
        d, _ = _check_against_batch_columns(eng, ts)
        assert d.lat.size == m
    d, _ = _check_against_batch_columns(eng, t.slice(0, 300))   # (bit 0)
    assert np.isnan(d.lat).any() and np.isnan(d.lon).any() and not d.sv.all() and not d.rv.all() and d.rv.any()


@pytest.mark.parametrize("absent", ("speedKmh", "vehicleId", "provider", "lat"))
def test_arrow_absent_column(eng, absent):
    t, _ = X.arrow_fixed(np.arange(257, dtype=np.int64) % 23)
    d, kb = _check_against_batch_columns(eng, t.drop([absent]).slice(3, 200))
    if absent == "speedKmh":
        assert not d.sv.any() and not d.speed.any() and d.rv.any()
    elif absent == "lat":
        assert np.isnan(d.lat).all() and d.rv.any()
    else:
        assert not d.rv.any() and not d.vkey.any()
        assert (kb.vehicles[0] == 0) == (absent == "vehicleId") and (kb.providers[0] == 0) == (absent == "provider")


# ---------------------------------------------------------------------------------------------------------
# 8. refusals that cannot read out of range
# ---------------------------------------------------------------------------------------------------------
def test_decreasing_offsets_are_refused_and_the_engine_goes_on(fresh):
    import torch
    recs = X.alignment_records()[:4]
    buf = np.frombuffer((b"".join(recs) * 2)[:40], np.uint8).copy()
    offs = np.array([0, 30, 20, 40], np.int64)   # decreasing, every offset inside the 40 bytes
    with pytest.raises(_lib.MobheatError, match="offsets out of order") as err:
        fresh.decode_json(buf, offs)
    assert err.value.code == _lib.HM_E_INVALID
    t, to = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    torch.cuda.synchronize()
    rc, _ = _raw_decode(fresh, 3, _lib.HM_MEM_DEVICE, _lib.HM_JSON_SPLICE, t.data_ptr(), to.data_ptr())
    assert rc == _lib.HM_E_INVALID
    from oracle import kafka_oracle
    vals = X.alignment_records()
    d, kb = _decode_values(fresh, vals)
    X.check_oracle(d, kafka_oracle.decode_values(vals), vals)
