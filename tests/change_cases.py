"""Shared by the change tests (tests/test_change_host.py, tests/test_gpu_change.py): change(A, B) of include/mobheat.h's
hm_window_change* restated with a plain dict join and Python's sorted on Python ints -- on purpose none of the library's
code -- and the record sets and event batches the host execution and the device are held to.

The join.  One pair per cell of either window; a half a window does not have is {cell, that window's start, 0, ...}.
The orders.  rising: countChange = cur.count - base.count descending; falling: ascending; abs: |countChange| descending;
then cell ascending as uint64, then the pair's index.

Everything is dyadic: coordinates on a 1/1024-degree lattice, half-integer speeds, so every fp64 sum is exact in any
order of addition and "equal" means bit-equal.  The two windows are [T0, T0 + 5 min) -- the base, WB -- and
[T0 + 5 min, T0 + 10 min) -- the current one, WA."""
import functools
import json

import numpy as np

T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
WB, WA = T0, T0 + 5 * MINUTE
H3_RES = 8
TOP_MAX = 65536
ORDERS = ("rising", "falling", "abs")
EMPTY = b'{"type":"FeatureCollection","features":[]}'
MAX_EVENTS = 20_000
BOX = (42.0, 43.0, -71.5, -70.5)            # lat0, lat1, lon0, lon1: a few dozen res-5 parents, thousands of res-8 cells
VIEW = (-71.20, 42.20, -70.90, 42.50)       # west, south, east, north: cuts the box
WS_TEXT, WE_TEXT = "2025-10-04T10:05:00", "2025-10-04T10:10:00"
REL, ABS_DEG = 1e-9, 1e-12                  # tests/test_gpu_rollup.py's closeness of two averages


# ---- the reference ----
def _zero(cell, ws):
    from mobheat._lib import STATE_REC_DTYPE
    z = np.zeros((), STATE_REC_DTYPE)
    z["cell"], z["window_start_us"] = cell, ws
    return z


def ref_change(cur, base, wa=WA, wb=WB):
    """the pairs by a dict join, sorted by cell"""
    from mobheat._lib import CHANGE_REC_DTYPE
    a = {int(r["cell"]): r for r in cur}
    b = {int(r["cell"]): r for r in base}
    assert len(a) == cur.size and len(b) == base.size
    cells = sorted(set(a) | set(b))
    out = np.zeros(len(cells), CHANGE_REC_DTYPE)
    for i, c in enumerate(cells):
        out[i]["cur"] = a[c] if c in a else _zero(c, wa)
        out[i]["base"] = b[c] if c in b else _zero(c, wb)
    return out


def ref_order(pairs, order, k):
    """the first min(k, n) pairs of the order by Python's sorted"""
    assert 0 <= k <= TOP_MAX
    d = [int(p["cur"]["count"]) - int(p["base"]["count"]) for p in pairs]
    cell = pairs["cur"]["cell"].tolist()
    first = {"rising": lambda i: -d[i], "falling": lambda i: d[i], "abs": lambda i: -abs(d[i])}[order]
    idx = sorted(range(pairs.size), key=lambda i: (first(i), cell[i], i))[:k]
    return pairs[np.array(idx, np.int64)] if idx else pairs[:0]


def by_cell(pairs):
    return pairs[np.argsort(pairs["cur"]["cell"], kind="stable")]


def same(got, want, what=""):
    """whole pairs, bit for bit, in order"""
    assert got.size == want.size, f"{what}: {got.size} pairs, {want.size} expected"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(got, want)])
        raise AssertionError(f"{what}: {bad.size} of {got.size} pairs differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def ks_of(n):
    return sorted({k for k in (0, 1, n, n + 1, TOP_MAX) if 0 <= k <= TOP_MAX})


# ---- record sets (host tests: no engine) ----
def _records(cells, counts, ws, salt):
    from mobheat._lib import STATE_REC_DTYPE
    i = np.arange(len(cells)) + salt
    r = np.zeros(len(cells), STATE_REC_DTYPE)
    r["cell"], r["count"], r["window_start_us"] = cells, counts, ws
    r["n_speed"] = np.minimum(np.asarray(counts, np.int64), i % 3)
    r["sum_speed"] = np.where(r["n_speed"] > 0, (i % 320) / 2.0, 0.0)
    r["sum_lat"], r["sum_lon"] = (i % 2048) / 1024.0, -((i * 7) % 2048) / 1024.0
    return r


@functools.lru_cache(maxsize=None)
def record_cases():
    """(name, cur, base): the cell-set shapes with small counts -- many changes tie, +c and -c both occur, 0 too"""
    import top_cases as tc
    rng = np.random.default_rng(4101)
    cells = rng.permutation(tc.cells_of(900))

    def recs(sel, ws, salt):
        return _records(cells[sel], rng.integers(1, 5, len(sel)), ws, salt)
    i = np.arange(900)
    out = [("disjoint", recs(i[:300], WA, 0), recs(i[300:700], WB, 5)),
           ("identical", recs(i[:500], WA, 0), recs(rng.permutation(i[:500]), WB, 5)),
           ("A inside B", recs(i[100:300], WA, 0), recs(rng.permutation(i[:600]), WB, 5)),
           ("B inside A", recs(rng.permutation(i[:600]), WA, 0), recs(i[100:300], WB, 5)),
           ("overlap", recs(rng.permutation(i[:600]), WA, 0), recs(rng.permutation(i[300:900]), WB, 5)),
           ("only A", recs(i[:257], WA, 0), recs(i[:0], WB, 5)),
           ("only B", recs(i[:0], WA, 0), recs(i[:255], WB, 5)),
           ("neither", recs(i[:0], WA, 0), recs(i[:0], WB, 5)),
           ("one cell each, equal", recs(i[:1], WA, 0), recs(i[:1], WB, 5))]
    # counts that differ in a high byte, and a base far above the current count
    big_a = _records(cells[:40], (rng.integers(0, 3, 40) << 32) + 7, WA, 0)
    big_b = _records(cells[20:60], (rng.integers(0, 3, 40) << 33) + 7, WB, 5)
    out.append(("large counts", big_a, big_b))
    return out


# ---- event batches (GPU tests; the host tests prove their claims) ----
def lattice(rng, n, box=None):
    """n points on the 1/1024-degree lattice: inside box (lat0, lat1, lon0, lon1), or over the sphere"""
    la0, la1, lo0, lo1 = box or (-90.0, 90.0, -180.0, 180.0)
    return (rng.integers(int(la0 * 1024), int(la1 * 1024) + 1, n) / 1024.0,
            rng.integers(int(lo0 * 1024), int(lo1 * 1024) + 1, n) / 1024.0)


def pentagon_points(rng, n):
    """lattice points within half a degree of the 12 pentagon centres (keys under a pentagon at every resolution)"""
    import raster_cases as rc
    pla, plo = rc.pentagon_centres()
    j = rng.integers(0, len(pla), n)
    la = np.clip(np.round(np.asarray(pla)[j] * 1024) + rng.integers(-512, 513, n), -90 * 1024, 90 * 1024) / 1024.0
    lo = np.clip(np.round(np.asarray(plo)[j] * 1024) + rng.integers(-512, 513, n), -180 * 1024, 180 * 1024) / 1024.0
    return la, lo


SHAPES = ("disjoint", "identical", "a_in_b", "b_in_a", "overlap", "a_only", "b_only")


def membership(shape, n, rng):
    """(in A, in B) per cell"""
    j = rng.integers(0, 3, n)
    one = np.ones(n, bool)
    return {"disjoint": (j == 0, j != 0), "identical": (one, one), "a_in_b": (j == 0, one), "b_in_a": (one, j == 0),
            "overlap": (j != 1, j != 0), "a_only": (one, ~one), "b_only": (~one, one)}[shape]


def batch_of(lat, lon, shape, seed, n_a=None, n_b=None, dyadic=True):
    """One batch of events over the points' distinct res-8 cells (one point per cell), each cell in window A, B or both
    as `shape` says, 1..3 events per cell and window; n_a / n_b: exactly that many cells in A / B (the first ones).
    Returns (batch, cells in A, cells in B)."""
    from mobheat import _lib
    rng = np.random.default_rng(seed)
    cell = _lib.latlng_to_cell_host_selftest(lat, lon, H3_RES)
    ucell, first = np.unique(cell, return_index=True)
    first = first[ucell != 0]
    p = rng.permutation(first.size)
    lat, lon, cell = lat[first][p], lon[first][p], cell[first][p]
    in_a, in_b = (f.copy() for f in membership(shape, cell.size, rng))
    for flag, want in ((in_a, n_a), (in_b, n_b)):
        if want is not None:
            on = np.flatnonzero(flag)
            assert on.size >= want, f"{on.size} cells, {want} wanted"
            flag[on[want:]] = False
    ca = np.where(in_a, rng.integers(1, 4, cell.size), 0)
    cb = np.where(in_b, rng.integers(1, 4, cell.size), 0)
    rows = np.r_[np.repeat(np.arange(cell.size), ca), np.repeat(np.arange(cell.size), cb)]
    n, na = rows.size, int(ca.sum())
    assert n <= MAX_EVENTS, n
    ts = np.r_[np.full(na, WA), np.full(n - na, WB)] + rng.integers(0, 300, n) * 1_000_000
    speed = rng.integers(0, 160, n) * 0.5 if dyadic else rng.uniform(0.0, 90.0, n)
    la, lo = lat[rows], lon[rows]
    if not dyadic:   # off the lattice, inside the cell's neighbourhood or not: the test compares with the engine's own roll-ups
        la, lo = la + rng.uniform(-1e-4, 1e-4, n), lo + rng.uniform(-1e-4, 1e-4, n)
    o = rng.permutation(n)
    b = dict(lat=la[o], lon=lo[o], ts_us=ts[o], speed=speed[o], speed_valid=(rng.random(n) >= 0.2)[o],
             vkey=rng.integers(0, 5000, n).astype(np.uint64), row_valid=np.ones(n, bool))
    return b, np.sort(cell[in_a]), np.sort(cell[in_b])


@functools.lru_cache(maxsize=None)
def box_points(seed=4201, n=3600):
    rng = np.random.default_rng(seed)
    la, lo = lattice(rng, n, BOX)
    ga, go = lattice(rng, n // 4)
    return np.r_[la, ga], np.r_[lo, go]


@functools.lru_cache(maxsize=None)
def shape_batch(shape):
    """a few thousand cells in the box and over the sphere, in the given cell-set shape"""
    la, lo = box_points()
    return batch_of(la, lo, shape, 4300 + SHAPES.index(shape))


@functools.lru_cache(maxsize=None)
def pentagon_batch():
    rng = np.random.default_rng(4401)
    la, lo = pentagon_points(rng, 3000)
    return batch_of(la, lo, "overlap", 4402)


@functools.lru_cache(maxsize=None)
def load_limit_batch(n_base):
    """exactly n_base base cells (512, 4096: the base's parent table of next_pow2(max(2 n, 1024)) slots exactly half full)
    and about half as many current ones, two thirds of them among the base's"""
    rng = np.random.default_rng(4500 + n_base)
    la, lo = lattice(rng, 3 * n_base, BOX)
    return batch_of(la, lo, "overlap", 4501 + n_base, n_a=n_base // 2, n_b=n_base)


@functools.lru_cache(maxsize=None)
def random_batch():
    rng = np.random.default_rng(4601)
    la, lo = lattice(rng, 5000, BOX)
    return batch_of(la, lo, "overlap", 4602, dyadic=False)


# ---- GeoJSON ----
def dumps(obj):
    return json.dumps(obj, separators=(",", ":")).encode()


class Text:   # a datetime stand-in whose isoformat() is the caller's text
    def __init__(self, t):
        self.t = t

    def isoformat(self):
        return self.t


def host_collection(pairs, ws_text=WS_TEXT, we_text=WE_TEXT):
    """readside.tiles_change_collection of the pairs, its rings from the host execution of cellToBoundary (no GPU)"""
    from mobheat import _lib, readside
    saved = readside.cells_to_boundary
    readside.cells_to_boundary = lambda cells, device=0: _lib.cells_to_boundary_host_selftest(cells)
    try:
        return readside.tiles_change_collection(pairs, Text(ws_text), Text(we_text))
    finally:
        readside.cells_to_boundary = saved


def check_body(body, offs, collection):
    """the body and every feature slice against json.dumps of the collection; the offsets' consistency"""
    import geojson_cases as gc
    gc.check_body(body, offs, collection)
    if not collection["features"]:
        assert bytes(body) == EMPTY and len(EMPTY) == 42
