"""Shared by the GeoJSON tests (tests/test_float_repr_host.py, tests/test_geojson_host.py, tests/test_gpu_geojson.py):
the value sets, the tile records and position rows they encode, and the Python statement of the expected bytes --
json.dumps(..., separators=(",", ":")) of what mobheat/readside.py builds."""
import datetime
import json

import numpy as np

PENTAGON_BASE_CELLS = [4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117]
PREFIX = b'{"type":"FeatureCollection","features":['
WS_TEXT, WE_TEXT = "2025-10-04T10:00:00", "2025-10-04T10:05:00"
INT64_MAX = (1 << 63) - 1


def py_json_float(v):
    v = float(v)
    return ("NaN" if v != v else "Infinity" if v == float("inf") else "-Infinity" if v == -float("inf") else repr(v)).encode()


def special_doubles():
    """powers of two and ten with both neighbours, the format's ends, the layout's thresholds, 0.1 * k"""
    vals = []
    for e in range(-1074, 1024):
        vals.append(float.fromhex(f"0x1p{e}"))
    for e in range(-323, 309):
        vals.append(float(f"1e{e}"))
    v = np.array(vals)
    v = np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])
    extra = [5e-324, float.fromhex("0x0.fffffffffffffp-1022"), float.fromhex("0x1p-1022"), float.fromhex("0x1.fffffffffffffp1023"),
             9007199254740993.0, 1e15, 1e16, 1e17, 9999999999999998.0, 0.0001, 0.00001, 1e22, 1e23, 0.0, -0.0,
             float("nan"), -float("nan"), float("inf"), -float("inf")] + [0.1 * k for k in range(1, 101)]
    v = np.concatenate([v, np.array(extra), -np.array(extra[:13])])
    nan_payload = np.array([0x7ff0000000000001, 0xfff8000000000123, 0x7fffffffffffffff], np.uint64).view(np.float64)
    return np.concatenate([v, nan_payload])


def check_float_texts(x, text, ln):
    raw = text.tobytes()
    bad = []
    for i in range(x.size):
        got, want = raw[24 * i: 24 * i + int(ln[i])], py_json_float(x[i])
        if got != want:
            bad.append((float(x[i]).hex(), got, want))
    assert not bad, f"{len(bad)} of {x.size} differ, e.g. {bad[:5]}"


# ---- tiles ----
def _pentagon(bc, res):
    return (1 << 59) | (res << 52) | (bc << 45) | ((1 << (3 * (15 - res))) - 1)


def tile_cells(boundary):
    """300 cells: res 0, 8 and 15, the 12 pentagons at an even and an odd resolution, Class III cells whose boundary
    crosses an icosahedron edge (7-9 vertices), one invalid index; boundary(cells) -> (lat, lng, nverts)."""
    from oracle import h3_oracle
    rng = np.random.default_rng(4242)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, 4000)))
    lon = rng.uniform(-180, 180, 4000)
    cross = np.concatenate([np.unique(h3_oracle.latlng_to_cell(lat, lon, r)) for r in (1, 3)])
    nv = boundary(cross)[2]
    cross = cross[(nv > 6) & (nv < 10)][:24]
    assert cross.size >= 8
    pent = [_pentagon(bc, r) for r in (2, 1) for bc in PENTAGON_BASE_CELLS]
    cells = [np.array([0x1234], np.uint64), np.array(pent, np.uint64), cross,
             h3_oracle.latlng_to_cell(lat[:20], lon[:20], 0), h3_oracle.latlng_to_cell(lat[:40], lon[:40], 15)]
    have = sum(c.size for c in cells)
    cells.append(h3_oracle.latlng_to_cell(rng.uniform(42.2, 42.5, 300 - have), rng.uniform(-71.3, -70.9, 300 - have), 8))
    cells = np.concatenate(cells).astype(np.uint64)
    nv = boundary(cells)[2]
    assert cells.size == 300 and nv[0] == 0 and set(nv[1:13]) == {5} and set(nv[13:25]) == {10}
    return cells


def tile_records(cells, seed=7):
    """records over `cells` (repeated to the size asked for by the caller): counts 0, -1, INT64_MAX, n_speed 0, a NaN sum"""
    from mobheat._lib import STATE_REC_DTYPE
    rng = np.random.default_rng(seed)
    n = cells.size
    r = np.zeros(n, STATE_REC_DTYPE)
    r["cell"] = cells
    r["window_start_us"] = 1_759_572_000_000_000
    r["count"] = rng.integers(1, 5000, n)
    r["n_speed"] = rng.integers(1, 50, n)
    r["sum_speed"] = rng.uniform(0, 90, n) * r["n_speed"]
    r["sum_lat"] = rng.uniform(-90, 90, n)
    r["sum_lon"] = rng.uniform(-180, 180, n)
    if n >= 8:
        r["count"][1:4] = [0, -1, INT64_MAX]
        r["n_speed"][4] = 0
        r["sum_speed"][5] = np.nan
        r["sum_speed"][6] = -0.0
        r["sum_speed"][7] = 1e-7
        r["n_speed"][7] = 3
    return r


def finite(recs):
    return recs[np.isfinite(recs["sum_speed"])]


def tile_collection(recs, ws_text, we_text, boundary):
    """readside.tiles_latest_collection of the records' documents, its rings from boundary(cells)"""
    from mobheat import readside

    class _Text:   # a datetime stand-in whose isoformat() is the caller's text
        def __init__(self, t):
            self.t = t

        def isoformat(self):
            return self.t
    docs = []
    for r in recs:
        avg = 0.0 if r["n_speed"] == 0 else float(np.float64(r["sum_speed"]) / np.float64(r["n_speed"]))
        docs.append({"cellId": format(int(r["cell"]), "x"), "count": int(r["count"]), "avgSpeedKmh": avg,
                     "windowStart": _Text(ws_text), "windowEnd": _Text(we_text)})
    saved = readside.cells_to_boundary
    readside.cells_to_boundary = lambda cells, device=0: boundary(cells)
    try:
        with np.errstate(all="ignore"):
            return readside.tiles_latest_collection(docs)
    finally:
        readside.cells_to_boundary = saved


def dumps(obj):
    return json.dumps(obj, separators=(",", ":")).encode()


def check_body(body, offs, collection):
    """the body and every feature slice against json.dumps of the collection"""
    body = bytes(body)
    feats = collection["features"]
    n = len(feats)
    assert len(offs) == n + 1 and offs[0] == len(PREFIX) and body[:len(PREFIX)] == PREFIX
    for i, f in enumerate(feats):
        got, want = body[offs[i]: offs[i + 1] - 1], dumps(f)
        assert got == want, f"feature {i}: {got!r} != {want!r}"
        assert body[offs[i + 1] - 1: offs[i + 1]] == (b"]" if i == n - 1 else b",")
    assert body == dumps(collection)
    assert len(body) == offs[n] + (1 if n else 2)


# ---- positions ----
ALL_ASCII = bytes(range(0x80)).decode("ascii")
POSITION_STRINGS = ["", ALL_ASCII, "é-ü", "日本バス", "🚌🚍", "a\"b\\c\n\r\t\b\f\x7f", "plain-42"]
Y1_S = -62135596800            # 0001-01-01T00:00:00
Y9999_S = 253402300799         # 9999-12-31T23:59:59
DST_BUCKET = 1_762_063_200 // 900   # 2025-11-02T06:00:00Z: US Eastern leaves daylight time


def position_rows():
    """(provider, vehicleId, ts_us, lat, lon): every string as provider and as vehicle; ts at 0, +-1 us, with
    microseconds, either side of an offset change, in year 1 and year 9999"""
    ts = [0, -1, 1, 1_759_572_000_123_456, DST_BUCKET * 900 * 1_000_000 - 1, DST_BUCKET * 900 * 1_000_000,
          Y1_S * 1_000_000, Y9999_S * 1_000_000 + 999_999, 1_759_572_000_000_000]
    rows = []
    rng = np.random.default_rng(99)
    for i, p in enumerate(POSITION_STRINGS):
        for j, v in enumerate(POSITION_STRINGS):
            rows.append((p, v, ts[(i * len(POSITION_STRINGS) + j) % len(ts)], float(rng.uniform(-80, 80)),
                         float(rng.uniform(-170, 170))))
    rows[3] = rows[3][:3] + (float("nan"), -0.0)
    return rows


def bucket_table(ts_us, offset_of=None):
    """the rows' distinct 900-s buckets and a local offset for each: -4 h before DST_BUCKET, -5 h from it on (unless
    offset_of(bucket) says otherwise)"""
    ids = np.unique(np.floor_divide(np.floor_divide(np.asarray(ts_us, np.int64), 1_000_000), 900))
    # (year 1 and year 9999 stay inside 1..9999 only with offset 0)
    offs = np.array([(offset_of(int(b)) if offset_of else
                      (0 if abs(int(b)) > 10 ** 7 else -14400 if b < DST_BUCKET else -18000)) for b in ids], np.int64)
    return ids, offs


def position_collection(rows, ids, offs):
    """readside.positions_latest_collection of the rows' documents (ts: the naive wall time shifted by the bucket's offset)"""
    from mobheat import readside
    off = dict(zip(ids.tolist(), offs.tolist()))
    docs = []
    for p, v, ts, lat, lon in rows:
        s, us = divmod(int(ts), 1_000_000)
        when = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=s + off[s // 900], microseconds=us)
        docs.append({"provider": p, "vehicleId": v, "ts": when, "loc": {"type": "Point", "coordinates": [float(lon), float(lat)]}})
    return readside.positions_latest_collection(docs)


def dictionary(strings):
    """(n, offsets, bytes) of a list of str / bytes (bytes: any byte string, valid UTF-8 or not)"""
    raw = [s if isinstance(s, bytes) else s.encode("utf-8") for s in strings]
    offs = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(b) for b in raw], out=offs[1:])
    data = np.frombuffer(b"".join(raw) + b"\0", np.uint8).copy()
    return len(raw), offs, data


def position_records(rows, providers, vehicles):
    from mobheat._lib import POSITION_REC_DTYPE
    pi, vi = {s: k for k, s in enumerate(providers)}, {s: k for k, s in enumerate(vehicles)}
    r = np.zeros(len(rows), POSITION_REC_DTYPE)
    for k, (p, v, ts, lat, lon) in enumerate(rows):
        r[k] = (pi[p], vi[v], ts, lat, lon)
    return r
