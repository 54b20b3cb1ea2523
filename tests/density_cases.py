"""Shared by the density tests (tests/test_density_host.py, tests/test_gpu_density.py): the contract of
include/mobheat.h's hm_positions_density restated with the CPU oracle and numpy -- on purpose none of the library's code --
and the states the host execution and the device are held to.

The rule.  A key is kept iff ts_us >= since_us.  A kept key's cell is the oracle's latLngToCell(lat, lon, res), or none
when a coordinate is NaN or outside [-90, 90] / [-180, 180] (the reference UDF's range guard): such a key is "unsnapped" and
in no group.  One record per distinct cell: count, the sums of lat / lon, window_start_us = the newest kept ts_us of the
group, n_speed 0, sum_speed +0.0, reserved 0.  With a view a group stays iff its cell's ring (the oracle's boundary) meets
the view by readside.ring_in_view, the pole cells as such.

Bars (tests/test_gpu_rollup.py's): the cell set, count, window_start_us, n_speed, sum_speed and reserved bit-equal;
averages sum / count within REL = 1e-9 / ABS_DEG = 1e-12 (fp64 sums of up to 50,000 terms below 180 in any order differ by
at most n * 2^-53 relative ~ 6e-12); on dyadic coordinates (multiples of 1/1024 degree: every partial sum below 2^24 is
exact in binary64) the sums themselves bit-equal."""
import functools

import numpy as np

import raster_cases as rc

REL = 1e-9
ABS_DEG = 1e-12
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0 = 1_759_572_000_000_000
SEC = 1_000_000
BOSTON_BOX = (42.20, 42.45, -71.20, -70.95)   # synth.c1_boston's coordinates


def dictionaries(n):
    """one provider "p" and n vehicles "v0000000".. as (n, offsets, bytes) tuples (no Arrow needed)"""
    prov = (1, np.array([0, 1], np.int64), np.frombuffer(b"p", np.uint8).copy())
    if n == 0:
        return prov, (0, np.zeros(1, np.int64), np.zeros(1, np.uint8))
    raw = np.frombuffer(b"".join(b"v%07d" % k for k in range(n)), np.uint8).copy()
    return prov, (n, np.arange(n + 1, dtype=np.int64) * 8, raw)


def records(lat, lon, ts):
    """POSITION_REC_DTYPE records of vehicles 0..n-1 of provider 0"""
    from mobheat._lib import POSITION_REC_DTYPE
    lat = np.asarray(lat, np.float64)
    r = np.zeros(lat.size, POSITION_REC_DTYPE)
    r["vehicle"], r["ts_us"], r["lat"], r["lon"] = np.arange(lat.size), ts, lat, lon
    return r


def load(eng, recs):
    """the records as the (empty) engine's positions state"""
    prov, veh = dictionaries(recs.size)
    eng.import_positions(recs, prov, veh)


def oracle_cells(res, lat, lon):
    """the oracle's cell per key, 0 where the range guard leaves none"""
    from oracle import h3_oracle
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(lat) <= 90.0) & (np.abs(lon) <= 180.0)   # (False on a NaN)
    cells = np.zeros(lat.size, np.uint64)
    if ok.any():
        cells[ok] = h3_oracle.latlng_to_cell(lat[ok], lon[ok], res)
    return cells


def expected(recs, res, since_us=None):
    """(STATE_REC_DTYPE records sorted by cell, unsnapped) by the rule"""
    from mobheat._lib import STATE_REC_DTYPE
    since = INT64_MIN if since_us is None else int(since_us)
    kept = recs[recs["ts_us"] >= since]
    cells = oracle_cells(res, kept["lat"], kept["lon"])
    has = cells != 0
    kept, cells = kept[has], cells[has]
    uniq, inv = np.unique(cells, return_inverse=True)
    out = np.zeros(uniq.size, STATE_REC_DTYPE)
    out["cell"] = uniq
    out["count"] = np.bincount(inv, minlength=uniq.size)
    out["sum_lat"] = np.bincount(inv, weights=kept["lat"], minlength=uniq.size)
    out["sum_lon"] = np.bincount(inv, weights=kept["lon"], minlength=uniq.size)
    newest = np.full(uniq.size, INT64_MIN, np.int64)
    np.maximum.at(newest, inv, kept["ts_us"])
    out["window_start_us"] = newest
    return out, int((~has).sum())


@functools.lru_cache(maxsize=None)
def _poles(res):
    from oracle import h3_oracle
    p = h3_oracle.latlng_to_cell(np.array([90.0, -90.0]), np.array([0.0, 0.0]), res)
    return int(p[0]), int(p[1])


def in_view(want, res, view):
    """the expected records whose cell is in view: readside.ring_in_view on the oracle's rings"""
    from mobheat import readside
    from oracle import h3_oracle
    la, lo, nv = h3_oracle.cell_to_boundary(want["cell"])
    north, south = _poles(res)
    keep = []
    for k in range(want.size):
        ring = [[float(lo[k, v]), float(la[k, v])] for v in range(max(int(nv[k]), 0))]
        c = int(want["cell"][k])
        keep.append(readside.ring_in_view(ring, view, "north" if c == north else "south" if c == south else None))
    return want[np.array(keep, bool)] if want.size else want


def close(a, b):
    return np.abs(a - b) <= np.maximum(REL * np.maximum(np.abs(a), np.abs(b)), ABS_DEG)


def check(got, want, dyadic=False, what=""):
    """got (any order) against expected()'s records by the bars above"""
    got = np.sort(got, order="cell")
    assert got.size == want.size, f"{what}: {got.size} groups, {want.size} expected"
    for f in ("cell", "count", "window_start_us", "n_speed", "reserved"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    assert got["sum_speed"].tobytes() == np.zeros(got.size).tobytes(), f"{what}: sum_speed is not +0.0"
    if got.size == 0:
        return
    for f in ("sum_lat", "sum_lon"):
        if dyadic:
            assert got[f].tobytes() == want[f].tobytes(), f"{what}: {f} on dyadic coordinates"
        else:
            assert close(got[f] / got["count"], want[f] / want["count"]).all(), f"{what}: avg of {f}"


# ---- the states ----
def dyadic(rng, n, box):
    """n points on the 1/1024-degree lattice inside box = (lat0, lat1, lon0, lon1)"""
    la = rng.integers(int(np.ceil(box[0] * 1024)), int(np.floor(box[1] * 1024)) + 1, n) / 1024.0
    lo = rng.integers(int(np.ceil(box[2] * 1024)), int(np.floor(box[3] * 1024)) + 1, n) / 1024.0
    return la, lo


def sphere(rng, n):
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


def boston(n, seed=0):
    """n vehicles in C1's box, ts over 200 s"""
    rng = np.random.default_rng(seed)
    return records(rng.uniform(BOSTON_BOX[0], BOSTON_BOX[1], n), rng.uniform(BOSTON_BOX[2], BOSTON_BOX[3], n),
                   T0 + rng.integers(0, 200, n) * SEC)


def sized(n, seed=3):
    """n vehicles uniform on the sphere with every tenth at a dyadic point of a ~1-km box in Boston (a handful of res-8
    cells: several keys per cell)"""
    rng = np.random.default_rng(seed + n)
    la, lo = sphere(rng, n)
    dl, do = dyadic(rng, n, (42.30, 42.31, -71.06, -71.05))
    la[::10], lo[::10] = dl[::10], do[::10]
    return records(la, lo, T0 + rng.integers(-50, 50, n) * SEC)


HOT_BOX = (5.0, 9.0, 5.0, 9.0)   # inside one res-0 cell (the tests assert it)


def hot_cell(n=50_000, seed=9):
    """n vehicles at DISTINCT points of the 1/1024-degree lattice inside one res-0 cell"""
    rng = np.random.default_rng(seed)
    side = int((HOT_BOX[1] - HOT_BOX[0]) * 1024)
    pick = rng.choice(side * side, n, replace=False)
    la, lo = HOT_BOX[0] + (pick // side) / 1024.0, HOT_BOX[2] + (pick % side) / 1024.0
    return records(la, lo, T0 + rng.integers(0, 3600, n) * SEC)


def edges(n_sphere=20_000, seed=21):
    """synth.edge_points() (poles, +-180, zeros, sub-normals, just-outside and non-finite values), the 12 pentagon and the
    20 face centres (a point that close to a face centre takes the exact path) and n_sphere uniform points"""
    from mobheat import synth
    rng = np.random.default_rng(seed)
    ela, elo = synth.edge_points()
    pla, plo = rc.pentagon_centres()
    fla, flo = rc.face_centres()
    sla, slo = sphere(rng, n_sphere)
    la, lo = np.r_[ela, pla, fla, sla], np.r_[elo, plo, flo, slo]
    return records(la, lo, T0 + rng.integers(0, 900, la.size) * SEC)


BAD_COORDS = [(np.nan, 10.0), (90.0000001, 10.0), (10.0, -180.0000001), (10.0, np.inf)]


def with_bad(n=300, seed=5):
    """n Boston vehicles with the four unsnappable records spread among them: (records, indices of the bad ones)"""
    r = boston(n, seed)
    at = [7, n // 3, n // 2, n - 1]
    for i, (la, lo) in zip(at, BAD_COORDS):
        r["lat"][i], r["lon"][i] = la, lo
    return r, at


def since_edges():
    """(records, since): keys at since - 1, since and since + 1 at one point (one cell at every res) and across three other
    cells.  The filter drops a group's OLDEST members, so a group's newest ts is always that of a kept key; what the compare
    can get wrong is the key at exactly `since` (kept), a group that loses some members (count 2 of 3) and a group that
    loses all of them (it vanishes)."""
    since = T0
    pa, pb, pc, pd = (42.25, -71.0), (42.40, -71.10), (42.30, -71.15), (42.35, -70.96)
    rows = [(pa, since - 1), (pa, since), (pa, since + 1),   # one cell: two of three kept, newest since + 1
            (pb, since - 1), (pc, since), (pd, since + 1),   # across cells: pb's cell vanishes
            (pc, since - 1), (pc, since - 1000)]             # pc's cell keeps exactly the key at since
    la = [p[0][0] for p in rows]
    lo = [p[0][1] for p in rows]
    return records(la, lo, [p[1] for p in rows]), since


def ts_extremes():
    """keys with ts INT64_MIN, negatives, 0, INT64_MAX (twice: a tied maximum) in one cell; a second cell all-negative
    with its maximum tied on three members; a third cell whose only key has ts INT64_MIN"""
    pa, pb, pc = (42.25, -71.0), (42.40, -71.10), (42.30, -71.15)
    rows = [(pa, INT64_MIN), (pa, -5), (pa, 0), (pa, INT64_MAX), (pa, INT64_MAX), (pa, 17),
            (pb, -9), (pb, -3), (pb, -3), (pb, -3), (pb, -1_000_000_000_000),
            (pc, INT64_MIN)]
    return records([p[0][0] for p in rows], [p[0][1] for p in rows], [p[1] for p in rows])
