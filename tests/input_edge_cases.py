"""Inputs, expectations and comparisons of tests/test_gpu_input_edges.py (no test here, nothing here touches the GPU):
the number and timestamp populations, the alignment and dictionary records, the fixed-width million-row batches for
hm_decode_json and hm_arrow_columns with their expected columns computed by numpy, and the exact comparison of a decoded
batch (`Decoded`: the columns read back from the device and the two dictionaries) with those expectations."""
import calendar
import random
from dataclasses import dataclass

import numpy as np

STRIDE = 1 << 20   # grid_for's cap: 4096 workgroups x 256 threads; row i + STRIDE is the same lane's second pass
TS0 = "2025-10-04T10:00:00Z"
TS0_US = calendar.timegm((2025, 10, 4, 10, 0, 0)) * 1_000_000
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, STRIDE, STRIDE + 1, STRIDE + 4097)
PATTERNS = ("distinct", "mod3", "wrap")


@dataclass
class Decoded:
    """A decoded batch on the host: hm_batch_in's columns and the dictionaries' strings (bytes, in code order)."""
    lat: np.ndarray
    lon: np.ndarray
    ts: np.ndarray
    speed: np.ndarray
    sv: np.ndarray
    rv: np.ndarray
    vkey: np.ndarray
    providers: tuple   # (n, offsets, bytes)
    vehicles: tuple

    @staticmethod
    def strings(d):
        n, offs, raw = d
        return [raw[offs[k]:offs[k + 1]].tobytes() for k in range(n)]


def same_f64(a, e):
    """bit patterns, NaN matching NaN"""
    a, e = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(e, np.float64)
    return (a.view(np.uint64) == e.view(np.uint64)) | (np.isnan(a) & np.isnan(e))


def _first_bad(ok, what, show=None):
    bad = np.flatnonzero(~np.asarray(ok))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), None if show is None else [show(int(k)) for k in bad[:3]])


def check_values(d, exp, show=None):
    """lat / lon / speed / speed_valid / ts_us / row_valid of every row, exactly (exp: oracle.kafka_oracle.decode_values'
    layout; ts_us is compared on every row when exp holds ts_valid -- a null eventTs is 0 -- else on the valid rows)."""
    n = len(exp["row_valid"])
    assert d.lat.size == n
    _first_bad(same_f64(d.lat, exp["lat"]), "lat", show)
    _first_bad(same_f64(d.lon, exp["lon"]), "lon", show)
    _first_bad(d.sv.astype(bool) == np.asarray(exp["speed_valid"], bool), "speed_valid", show)
    _first_bad(same_f64(np.where(d.sv.astype(bool), d.speed, 0.0), exp["speed"]), "speed", show)
    rv = np.asarray(exp["row_valid"], bool)
    _first_bad(d.rv.astype(bool) == rv, "row_valid", show)
    if "ts_valid" in exp:
        _first_bad(d.ts == np.where(exp["ts_valid"], exp["ts_us"], 0), "ts_us", show)
    else:
        _first_bad(d.ts[rv] == np.asarray(exp["ts_us"])[rv], "ts_us of the valid rows")
    assert set(np.unique(d.sv).tolist()) <= {0, 1} and set(np.unique(d.rv).tolist()) <= {0, 1}


def check_strings(d, prov, veh, rv, extra_prov=(), extra_veh=()):
    """The dictionaries hold exactly the distinct non-null strings (bytes or None per row; extra_*: strings of rows the
    caller knows apart), one code each, and every valid row's vkey names the row's two strings; an invalid row's is 0."""
    provs, vehs = Decoded.strings(d.providers), Decoded.strings(d.vehicles)
    pcode = {s: k for k, s in enumerate(provs)}
    vcode = {s: k for k, s in enumerate(vehs)}
    assert len(pcode) == len(provs) and len(vcode) == len(vehs), "a string holds two codes"
    assert set(provs) == {p for p in prov if p is not None} | set(extra_prov)
    assert set(vehs) == {v for v in veh if v is not None} | set(extra_veh)
    nv = max(len(vehs), 1)
    rv = np.asarray(rv, bool)
    ep = np.array([-1 if p is None else pcode[p] for p in prov], np.int64)
    ev = np.array([-1 if v is None else vcode[v] for v in veh], np.int64)
    want = np.where(rv, ep * nv + ev, 0).astype(np.uint64)
    _first_bad(d.vkey == want, "vkey", lambda k: (prov[k], veh[k], int(d.vkey[k]), nv))


def check_oracle(d, exp, values=None):
    show = None if values is None else (lambda k: values[k][:120])
    check_values(d, exp, show)
    check_strings(d, exp["provider"], exp["vehicleId"], exp["row_valid"])


def host_columns(o):
    """_lib.json_records_selftest's per-record output (json_decode.h run on the host) in k_json_parse's column
    conventions: what the device must give row for row -- an unsupported record is an all-null row."""
    from mobheat._lib import JF
    fl = o["flags"].astype(np.int64)
    un = (fl & JF["UNSUPPORTED"]) != 0
    f = np.where(un, 0, fl)
    sv = (f & JF["SPEED"]) != 0
    tv = (f & JF["TS"]) != 0
    rv = ((f & JF["PROV"]) != 0) & ((f & JF["VEH"]) != 0) & tv
    keep = lambda s, bit: [x if (int(f[k]) & bit) else None for k, x in enumerate(s)]   # noqa: E731
    return dict(lat=np.where(f & JF["LAT"], o["lat"], np.nan), lon=np.where(f & JF["LON"], o["lon"], np.nan),
                speed=np.where(sv, o["speed"], 0.0), speed_valid=sv, ts_us=np.where(tv, o["ts_us"], 0), ts_valid=tv,
                row_valid=rv, provider=keep(o["provider"], JF["PROV"]), vehicleId=keep(o["vehicleId"], JF["VEH"]),
                unsupported=np.flatnonzero(un), n_malformed=int(((f & JF["MALFORMED"]) != 0).sum()))


def pack_exact(values):
    """values back to back with no spare byte (the last record ends at the buffer's end) + offsets int64[n + 1]"""
    offs = np.zeros(len(values) + 1, np.int64)
    np.cumsum([len(v) for v in values], out=offs[1:])
    return np.frombuffer(b"".join(values), np.uint8).copy(), offs


# ---------------------------------------------------------------------------------------------------------
# 1. numbers
# ---------------------------------------------------------------------------------------------------------
def number_population():
    """test_kafka_decode_host.test_decimal_to_double_is_correctly_rounded's population: (w, q) of w * 10^q"""
    rng = random.Random(5)
    w, q = [], []
    for _ in range(200_000):
        nd = rng.randint(1, 19)
        w.append(rng.randrange(10 ** (nd - 1), 10 ** nd))
        q.append(rng.randint(-360, 320))
    for j in range(2000):
        for t in (0, 3, 9):
            w.append((2 ** 53 + 2 * j + 1) << t)
            q.append(0)
    return w, q


def spellings(w, q, rng):
    """three texts of w * 10^q: WeQ, the point moved inside the digits, and 0.000...W000 with the exponent to match"""
    d = str(w)
    k = rng.randint(1, len(d) - 1) if len(d) > 1 else 1
    inside = f"{d[:k]}.{d[k:] or '0'}e{q + len(d) - k}"
    z, tz = rng.randint(0, 5), rng.randint(0, 4)
    small = f"0.{'0' * z}{d}{'0' * tz}E{q + z + len(d):+d}"
    return f"{w}e{q}", inside, small


NUMBER_EDGES = ("-0", "-0.0", "0e5", "1e400", "1e-400", "4.9e-324", "2.2250738585072014e-308", "1.7976931348623157e308")


def number_value(text):
    """float(text); an integer token is the double of its integer (Jackson's getDoubleValue of an int token, the
    oracle's float(int)), which differs from float(text) for the one token -0: +0.0"""
    return 0.0 if text == "-0" else float(text)


def number_records(tokens):
    """three tokens per record (padded with 1); returns (values, expected float64[n, 3])"""
    tokens = list(tokens) + ["1"] * (-len(tokens) % 3)
    vals = [('{"provider":"p","vehicleId":"v","lat":%s,"lon":%s,"speedKmh":%s,"ts":"2025-10-04"}'
             % (tokens[k], tokens[k + 1], tokens[k + 2])).encode() for k in range(0, len(tokens), 3)]
    exp = np.array([number_value(t) for t in tokens], np.float64).reshape(-1, 3)
    return vals, exp


def long_tokens():
    """(far, halfway): tokens of 20-40 digits.  far: the 19 leading digits W and W + 1 round to the same double, so the
    digits beyond cannot matter (the device decodes them); halfway: an exact halfway value (2^53 + 2j + 1) 2^t of more
    than 19 digits, alone and followed by more digits -- W lies below it and W + 1 above, so the device cannot decide."""
    rng = random.Random(77)
    far = []
    while len(far) < 300:
        nd = rng.randint(20, 40)
        digs = str(rng.randrange(10 ** (nd - 1), 10 ** nd))
        e = rng.randint(-330, 280)
        w19 = int(digs[:19])
        if float(f"{w19}e{e + nd - 19}") != float(f"{w19 + 1}e{e + nd - 19}"):
            continue
        k = rng.choice([0, 1, nd // 2, nd])   # the point before, inside or after the digits
        far.append((f"{digs[:k] or '0'}.{digs[k:]}" if k < nd else digs) + f"e{e + nd - k}")
    half = []
    for j in range(100):
        for t in (20, 40, 60):
            h = str((2 ** 53 + 2 * (j * 37) + 1) << t)
            assert 20 <= len(h) <= 40
            if int(h[19:]) == 0:   # (W would be the value itself)
                continue
            # (each in a record of its own, beside two short tokens: every spelling has to be listed itself)
            half += [h, "1", "2"]
            half += ["1", h + "." + "0" * rng.randint(0, 40 - len(h) - 1) + str(rng.randint(1, 9)), "2"]
            half += ["1", "2", "-" + h + ".5"]
    return far, half


# ---------------------------------------------------------------------------------------------------------
# 2. timestamps
# ---------------------------------------------------------------------------------------------------------
def _escaped(s, every=1):
    return "".join("\\u%04x" % ord(c) if k % every == 0 else c for k, c in enumerate(s))


def timestamp_strings():
    """(texts as they stand between the JSON quotes, oracle_ok: the year is inside pandas' range)"""
    out = []
    fracs = ["." + "123456789"[:k] for k in range(1, 10)]
    times = ["", "T00:00", " 23:59", "T23:59:59", " 00:00:00"] + [sep + "12:34:56" + f for sep in "T " for f in fracs]
    zones = ["", "Z", "+00", "-00", "+14", "-18", "+0530", "-0930", "+1800", "+05:30", "-12:00", "+18:00", "-18:00"]
    dim = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    dates = []
    for y in (1970, 1972, 2000, 2024, 2100):
        for m in range(1, 13):
            dates.append(f"{y:04d}-{m:02d}-{dim[m - 1]:02d}")
        dates += [f"{y:04d}-02-29", f"{y:04d}-02-30", f"{y:04d}-13-01", f"{y:04d}-04-31"]   # (02-29: valid in leap years)
    for dt in dates:
        for t in times:
            for z in zones:
                if t == "" and z != "":
                    continue
                out.append(dt + t + z)
    out += [dt + z for dt in dates[:20] for z in ("Z", "+02:00", "-05")]                      # a zone after a bare date
    early = ["1969-12-31T23:59:59.999999Z", "1969-12-31T23:59:59.9999999", "1969-12-31 23:59:59.000001+00:00",
             "1900-01-01", "1900-02-29", "1899-12-31T23:59:59.5-18:00", "1678-01-01T00:00:00Z", "1700-03-01 00:00",
             "2261-12-31T23:59:59.999999999+18:00",
             # outside pandas' datetime64[ns]: the host run is the reference
             "1677-09-20", "1600-02-29T12:00:00Z", "0001-01-01", "0000-01-01T00:00:00.5Z", "0400-02-29", "1500-02-29",
             "2262-04-12T00:00:00Z", "2300-02-29", "2400-02-29 10:00", "9999-12-31T23:59:59.999999999-18:00"]
    out += early
    sample = out[::41]
    out += [" " + s for s in sample] + [s + "  " for s in sample] + ["   " + s + " " for s in sample[::3]]
    out += [_escaped(s) for s in sample[:120] if len(s) <= 64] + [_escaped(s, 3) for s in sample]
    out += [_escaped(s, 2) for s in early]
    base = "2024-02-29T12:34:56"
    out += [base.replace("T12", "T24"), base.replace(":56", ":60"), base.replace(":34", ":60"), base + ".1234567890",
            base + ".", base + "+05:60", base + "z", base + " Z", "2024-2-29", "24-02-29", base + "+5",
            "2024-02-29T12", "2024-02-29T12:34:5", "2024-00-10", "2024-01-00", "2024-02-29X12:34", "", " ", "2024-02-29T",
            # 64 bytes (valid: blanks around a timestamp) and 65 bytes whose text is no timestamp
            (base + "Z").ljust(64), (base + ".123456789+05:30").rjust(64), base + "." + "1" * 45, "2" * 65,
            base + "Z" + "x" * 45]
    assert len(out[-1]) == 65 and len(out[-3]) == 65
    # a timestamp padded with blanks past 64 bytes is trimmed like any other (valid), before, behind and on both sides,
    # raw and escaped; blanks inside the text are not (invalid)
    full = base + ".123456789+05:30"
    out += [(base + "Z").ljust(65), (base + "Z").rjust(65), (base + "Z").center(65), full.ljust(65), full.rjust(66),
            " " * 64 + full + " " * 64, " " * 1000 + "2024-02-29", "2024-02-29" + " " * 1000, " " * 63 + full,
            "\\u0020" * 50 + base + "Z", base + "Z" + "\\t" * 50 + " " * 20, "\\u0020" * 70 + "\\u0032024-02-29\\u0020" + " " * 70,
            "1600-02-29T12:00:00Z".rjust(80), "1600-02-30".ljust(80),
            base + " " * 50 + "Z", "2024-02-29" + " " * 60 + "12:00", " " * 40 + base + " " * 30 + "x", " " * 65, "2024-02-30".rjust(65)]

    def year_ok(s):
        t = s.encode().decode("unicode_escape").strip()
        return not (t[:4].isdigit() and not 1678 <= int(t[:4]) <= 2261)
    return out, np.array([year_ok(s) for s in out])


def timestamp_records(texts):
    return [('{"provider":"p","vehicleId":"v","ts":"%s"}' % s).encode() for s in texts]


# ---------------------------------------------------------------------------------------------------------
# 3. alignment
# ---------------------------------------------------------------------------------------------------------
def alignment_records():
    import json
    rng = random.Random(40)
    vals = []
    for k in range(24):   # the producer's shape
        msg = {"provider": rng.choice(["mbta", "opensky"]), "vehicleId": f"y{rng.randrange(9)}ώ",
               "lat": rng.uniform(42.2, 42.45), "lon": rng.uniform(-71.2, -70.95),
               "speedKmh": rng.choice([None, rng.uniform(0, 30) * 3.6]), "bearing": rng.choice([None, 90]),
               "accuracyM": None, "ts": f"2025-10-04T10:{rng.randint(0, 14):02d}:{rng.randint(0, 59):02d}Z"}
        vals.append(json.dumps(msg, ensure_ascii=k % 2 == 0).encode())
    t = '"ts":"2025-10-04T10:00:01Z"'
    vals += [('{"provider":"Αθήνα","vehicleId":"ώ1",%s}' % t).encode(),
             ('{"provider":"\\u0391\\u03b8\\u03ae\\u03bd\\u03b1","vehicleId":"\\u03ce1",%s}' % t).encode(),
             ('{"provider":"p","vehicleId":"\\ud83d\\ude00x",%s}' % t).encode(),
             ('{"provider":"p","vehicleId":"😀x",%s}' % t).encode(),
             ('{"provider":"p","vehicleId":"\\ud83dx",%s}' % t).encode(),                       # a lone surrogate: '?'
             ('{"provider":"p","vehicleId":"a\\u0062c","vehicleId":"raw",%s}' % t).encode(),    # the raw repeat wins
             ('{"provider":"p\\t","provider":null,"vehicleId":"v",%s}' % t).encode(),
             ('{"provider":"p","vehicleId":"raw","vehicleId":"a\\/b",%s}' % t).encode(),
             ('{"provider":"p","vehicleId":"%s",%s}' % ("k" * 1024, t)).encode(),
             ('{"provider":"p","vehicleId":"%s\\n",%s}' % ("k" * 1023, t)).encode(),
             ('{"provider":"p","vehicleId":12,"lat":1e0,"lon":-0.0,"speedKmh":"NaN",%s}' % t).encode(),
             ('  {"provider" : "p" , "vehicleId" : true , "\\u0074s" : "2025-10-04 10:00:02" }  ').encode(),
             b'{"provider":"p","vehicleId":"v","ts":"\\u0032025-10-04T10:00:03+01:00"}',
             b'{"provider":"p","vehicleId":"v","lat":"x"}', b"[1,2]", b"", b'{"provider":"p"']
    return vals


# ---------------------------------------------------------------------------------------------------------
# 4. sizes: fixed-width batches filled by numpy
# ---------------------------------------------------------------------------------------------------------
def pattern_ids(pattern, n):
    i = np.arange(n, dtype=np.int64)
    if pattern == "distinct":
        return i
    if pattern == "mod3":
        return i % 3
    assert pattern == "wrap"   # rows i and i + STRIDE: the same id for even i, different ids for odd i
    return np.where((i >= STRIDE) & (i % 2 == 0), i - STRIDE, i)


def fixed_expected(ids, with_nulls_everywhere=False, first=0, vehicle_nulls=True):
    """The rows of a fixed-width batch: every 7th vehicleId null, row 0 and row 64 among them (a wave whose first lane is
    not live), rows 128..191 null but row 130 (a wave with a single live lane); every 11th provider null; every 5th
    speed null.  Arrow batches (with_nulls_everywhere) also hold null lat, lon and eventTs.  first: the pattern's index
    of the batch's row 0; vehicle_nulls=False: no vehicleId is null."""
    n = ids.size
    i = np.arange(n, dtype=np.int64) + first
    vnull = ((i % 7 == 0) | (i == 64) | ((i >= 128) & (i < 192) & (i != 130))) & vehicle_nulls
    pnull = i % 11 == 3
    snull = i % 5 == 2
    pcode = np.where(pnull, -1, (i // 5) % 2)
    flat, flon = (i * 7919) % 1_000_000, (i * 104_729) % 1_000_000
    e = dict(ids=ids, vnull=vnull, pnull=pnull, pcode=pcode, flat=flat, flon=flon, sd=i % 10, sec=i % 900,
             # (an integer / 1e6 is the correctly rounded quotient of two exact doubles: float() of the decimal text)
             lat=(42_000_000 + flat) / 1e6, lon=-((71_000_000 + flon) / 1e6),
             speed=np.where(snull, 0.0, 10.0 + i % 10 + 0.5), speed_valid=~snull,
             ts_us=TS0_US + (i % 900) * 1_000_000, ts_valid=np.ones(n, bool))
    if with_nulls_everywhere:
        e["lat"] = np.where(i % 13 == 5, np.nan, e["lat"])
        e["lon"] = np.where(i % 19 == 7, np.nan, e["lon"])
        e["ts_valid"] = i % 17 != 9
        e["ts_us"] = np.where(e["ts_valid"], e["ts_us"], 0)
    e["row_valid"] = ~vnull & ~pnull & e["ts_valid"]
    return e


_TEMPLATE = (b'{"provider":"pA","vehicleId":"v0000000","lat":42.000000,"lon":-71.000000,"speedKmh":10.5,'
             b'"ts":"2025-10-04T10:00:00Z"}')
WIDTH = len(_TEMPLATE)


def _digits(a, col, val, k):
    for j in range(k):
        a[:, col + j] = 48 + (val // 10 ** (k - 1 - j)) % 10


def json_fixed(ids, **kw):
    """(bytes uint8[n * WIDTH], offsets, expected) of the fixed-width records of ids"""
    e = fixed_expected(ids, **kw)
    n = ids.size
    a = np.tile(np.frombuffer(_TEMPLATE, np.uint8), (n, 1))
    pc, vc = _TEMPLATE.index(b'"pA"'), _TEMPLATE.index(b'"v0')
    _digits(a, vc + 2, ids, 7)
    a[e["vnull"], vc:vc + 10] = np.frombuffer(b"null      ", np.uint8)
    a[e["pcode"] == 1, pc + 2] = ord("B")
    a[e["pnull"], pc:pc + 4] = np.frombuffer(b"null", np.uint8)
    _digits(a, _TEMPLATE.index(b"42.") + 3, e["flat"], 6)
    _digits(a, _TEMPLATE.index(b"-71.") + 4, e["flon"], 6)
    sc = _TEMPLATE.index(b"10.5")
    _digits(a, sc + 1, e["sd"], 1)
    a[~e["speed_valid"], sc:sc + 4] = np.frombuffer(b"null", np.uint8)
    tc = _TEMPLATE.index(b"T10:") + 4
    _digits(a, tc, e["sec"] // 60, 2)
    _digits(a, tc + 3, e["sec"] % 60, 2)
    return a.reshape(-1), np.arange(n + 1, dtype=np.int64) * WIDTH, e


def _arrow_strings(pa, typ, present, rows):
    """an Arrow string array from a uint8 [m, w] matrix of the present rows' bytes"""
    n, w = present.size, rows.shape[1]
    ot = np.int64 if typ == pa.large_string() else np.int32
    offs = np.zeros(n + 1, ot)
    np.cumsum(np.where(present, w, 0), out=offs[1:])
    bits = np.packbits(present, bitorder="little")
    return pa.Array.from_buffers(typ, n, [pa.py_buffer(bits), pa.py_buffer(offs), pa.py_buffer(np.ascontiguousarray(rows).reshape(-1))],
                                 null_count=int(n - present.sum()))


def arrow_fixed(ids, large=False, **kw):
    """(Arrow table, expected) of the same rows: provider / vehicleId strings, lat / lon / speedKmh doubles and eventTs
    in microseconds, every column with nulls, built from numpy buffers"""
    import pyarrow as pa
    e = fixed_expected(ids, with_nulls_everywhere=True, **kw)
    n = ids.size
    typ = pa.large_string() if large else pa.string()
    v = np.empty((int((~e["vnull"]).sum()), 8), np.uint8)
    v[:, 0] = ord("v")
    _digits(v, 1, ids[~e["vnull"]], 7)
    p = np.empty((int((~e["pnull"]).sum()), 2), np.uint8)
    p[:, 0] = ord("p")
    p[:, 1] = ord("A") + e["pcode"][~e["pnull"]]

    def f64(x, valid):
        return pa.Array.from_buffers(pa.float64(), n, [pa.py_buffer(np.packbits(valid, bitorder="little")),
                                                       pa.py_buffer(np.where(valid, x, -7.25))], null_count=int(n - valid.sum()))
    ts = pa.Array.from_buffers(pa.timestamp("us"), n, [pa.py_buffer(np.packbits(e["ts_valid"], bitorder="little")),
                                                       pa.py_buffer(np.where(e["ts_valid"], e["ts_us"], 123))],
                               null_count=int(n - e["ts_valid"].sum()))
    t = pa.table({"provider": _arrow_strings(pa, typ, ~e["pnull"], p), "vehicleId": _arrow_strings(pa, typ, ~e["vnull"], v),
                  "lat": f64(e["lat"], ~np.isnan(e["lat"])), "lon": f64(e["lon"], ~np.isnan(e["lon"])),
                  "speedKmh": f64(e["speed"], e["speed_valid"]), "eventTs": ts})
    return t, e


def check_fixed(d, e):
    """A decoded fixed-width batch against its expectation, vectorised: the columns, the dictionaries (exactly the
    distinct non-null strings, one code each) and every valid row's vkey through them."""
    check_values(d, e)
    vn, vo, vb = d.vehicles
    want = np.unique(e["ids"][~e["vnull"]])
    assert vn == want.size, (vn, want.size)
    assert np.array_equal(vo, np.arange(vn + 1) * 8)
    raw = vb[:vn * 8].reshape(vn, 8)
    dig = raw[:, 1:].astype(np.int64) - 48
    assert (raw[:, 0] == ord("v")).all() and ((dig >= 0) & (dig <= 9)).all()
    got = dig @ (10 ** np.arange(6, -1, -1, dtype=np.int64))
    assert np.array_equal(np.sort(got), want)                       # exactly the distinct strings, none twice
    provs = Decoded.strings(d.providers)
    names = [b"pA", b"pB"]
    assert sorted(provs) == sorted(names[c] for c in np.unique(e["pcode"][~e["pnull"]]))
    pname = np.array([names.index(p) for p in provs] + [-9], np.int64)
    nv = max(vn, 1)
    rv = e["row_valid"]
    pc, vc = (d.vkey // np.uint64(nv)).astype(np.int64), (d.vkey % np.uint64(nv)).astype(np.int64)
    assert (d.vkey[~rv] == 0).all()
    assert (pc[rv] < len(provs)).all()
    _first_bad(pname[pc[rv]] == e["pcode"][rv], "vkey's provider")
    _first_bad(got[vc[rv]] == e["ids"][rv], "vkey's vehicle")


def fixed_sample_values(buf, rows):
    a = buf.reshape(-1, WIDTH)
    return [a[r].tobytes() for r in rows]


def sample_of(e, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in e.items()}


def fixed_strings(e):
    """the expectation's provider / vehicleId as lists of bytes or None (small samples only)"""
    prov = [None if c < 0 else (b"pA", b"pB")[c] for c in e["pcode"].tolist()]
    veh = [None if z else b"v%07d" % k for k, z in zip(e["ids"].tolist(), e["vnull"].tolist())]
    return prov, veh


# ---------------------------------------------------------------------------------------------------------
# 5. dictionary contents: name -> rows of (provider, vehicleId) as JSON text (None: null), and as Arrow values where the
# case has a meaning there (str or None)
# ---------------------------------------------------------------------------------------------------------
def _q(s):
    return '"%s"' % s


def dictionary_cases():
    big = "z" * 65535
    base = "abcdefghijklmnopqrstuvwxyz012345"[:25]
    flip = lambda s, k: s[:k] + "#" + s[k + 1:]   # noqa: E731
    pairs = [base] + [flip(base, k) for k in (7, 8, 15, 16, 24)] + [base[:17], flip(base[:17], 16), base[:9], flip(base[:9], 8),
                                                                      base[:8], flip(base[:8], 7), base[:16], flip(base[:16], 15)]
    runs = ["x" * k for k in range(34)]
    cases = {
        "empty_and_null": [("p", ""), ("p", None), ("", "a"), (None, ""), ("p", ""), ("", ""), (None, None)],
        "one_byte_runs": [("p", s) for s in runs + runs[::-1]] + [(s, "v") for s in runs],
        "pairs": [("p", s) for s in pairs * 2] + [(s, "v") for s in pairs],
        "nul_byte": [("p", "a"), ("p", "a\x00"), ("p", "a"), ("a\x00", "a\x00\x00"), ("a", "\x00"), ("a", "")],
        "long_64k": [("p", big + "a"), ("p", big + "b"), ("p", big + "a"), (big + "c", "v"), ("p", big)],
        "three_providers": [("p%d" % (k % 3), "v%d" % (k * 7 % 5)) for k in range(37)],
    }
    js = {k: [(None if p is None else _q(p.replace("\x00", "\\u0000")), None if v is None else _q(v.replace("\x00", "\\u0000")))
              for p, v in rows] for k, rows in cases.items()}
    js["spellings"] = [(_q("p"), _q("a/b")), (_q("p"), _q("a\\/b")), (_q("p"), _q("\\u0061\\u002fb")), (_q("p"), _q("a\\u002Fb")),
                       (_q("p"), _q("😀")), (_q("p"), _q("\\ud83d\\ude00")), (_q("p"), _q("\\uD83D\\uDE00")),
                       (_q("\\u0070"), _q("ώ")), (_q("p"), _q("\\u03ce")), (_q("p"), _q("a\\\\b")), (_q("p"), _q("a\\u005cb"))]
    js["scalars"] = [(_q("p"), "12"), (_q("p"), _q("12")), (_q("p"), "-0"), (_q("p"), _q("0")), (_q("p"), "true"),
                     (_q("p"), _q("true")), ("false", _q("false")), (_q("false"), "0"), ("-12", "-12"), (_q("-12"), _q("-0"))]
    return js, cases


def pair_records(rows, ts=TS0):
    tok = lambda x: "null" if x is None else x   # noqa: E731
    return [('{"provider":%s,"vehicleId":%s,"ts":"%s"}' % (tok(p), tok(v), ts)).encode() for p, v in rows]


def splice_records(new_vehicles):
    """1000 producer-shaped records and 300 whose vehicleId is a float (outside the device decoder: spliced from the host
    decode as the text k.5); new_vehicles: those texts are in no other record, else every one is.  Returns (values,
    provider, vehicleId (bytes per row), the 300 rows)."""
    rng = random.Random(300)
    n = 1600
    odd = np.sort(rng.sample(range(300, n), 300))   # (the first 300 rows hold every text of the first kind)
    is_odd = np.zeros(n, bool)
    is_odd[odd] = True
    vals, prov, veh = [], [], []
    k_odd = 0
    for k in range(n):
        p = "p%d" % (k % 3)
        if is_odd[k]:
            v = "%d.5" % k_odd
            tok = v
            k_odd += 1
        else:
            v = ("w%d" % (k % 411)) if new_vehicles else "%d.5" % (k % 300)
            tok = _q(v)
        vals.append(('{"provider":"%s","vehicleId":%s,"lat":42.5,"lon":-71.25,"ts":"%s"}' % (p, tok, TS0)).encode())
        prov.append(p.encode())
        veh.append(v.encode())
    return vals, prov, veh, odd
