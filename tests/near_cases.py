"""Shared cases of the radius queries (tests/test_near_host.py on the CPU, tests/test_gpu_near.py on the device): query
points, candidate sets, radii, k and since_us.  Everything is compared bit for bit: the distance has no tolerance."""
import math

import numpy as np

TOP_MAX = 65536
R = 6378100.0
PI_R_UP = math.nextafter(math.pi * R, math.inf)   # pi R, rounded up: no distance exceeds it
INT64_MIN = -(1 << 63)
T0 = 1_759_572_000_000_000
SEC = 1_000_000
DUMP_PER = 8                 # csrc/dev_table.h
TILE = 256 * DUMP_PER        # the slots one scan workgroup takes per iteration

QUERIES = [(0.0, 0.0), (42.3601, -71.0589), (89.999, 10.0), (-90.0, 0.0), (10.0, 179.95), (10.0, -180.0)]


def antipode(lat0, lon0):
    return -lat0, lon0 + 180.0 if lon0 <= 0.0 else lon0 - 180.0


def sphere(rng, n):
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


def candidates(lat0, lon0, seed=1, n_sphere=600, n_cluster=300):
    """(name, lat, lon, key) sets around one query point; key is word 1 of the order (distinct unless said otherwise)"""
    rng = np.random.default_rng(seed)
    out = []
    la, lo = sphere(rng, n_sphere)
    out.append(("sphere", la, lo))
    # a 1-km cluster: +-0.009 degrees of latitude, the longitude span widened by 1 / cos(lat) (capped near the poles)
    w = 0.009 / max(math.cos(math.radians(lat0)), 1e-3)
    cl = np.clip(lat0 + rng.uniform(-0.009, 0.009, n_cluster), -90.0, 90.0)
    out.append(("cluster", cl, lon0 + rng.uniform(-w, w, n_cluster)))
    a_lat, a_lon = antipode(lat0, lon0)
    special_lat = [lat0, a_lat, 90.0, -90.0, 90.0, -90.0, lat0, lat0]
    special_lon = [lon0, a_lon, 0.0, 0.0, 137.5, -42.0, 179.999, -179.999]
    out.append(("special", np.array(special_lat), np.array(special_lon)))
    # pairs on both sides of the antimeridian
    al = rng.uniform(-60.0, 60.0, 100)
    dx = rng.uniform(0.0, 0.5, 100)
    out.append(("antimeridian", np.r_[al, al], np.r_[180.0 - dx, -180.0 + dx]))
    sets = []
    for name, la, lo in out:
        key = rng.permutation(la.size).astype(np.uint64) + np.uint64(7)
        sets.append((name, np.asarray(la, np.float64), np.asarray(lo, np.float64), key))
    # exact duplicates of one coordinate under different keys: the tie is decided by word 1
    la, lo = sphere(rng, 40)
    la, lo = np.repeat(la, 5), np.repeat(lo, 5)
    sets.append(("duplicates", la, lo, rng.permutation(la.size).astype(np.uint64)))
    # one coordinate for every candidate: word 0 is constant, the select walks key bytes only
    sets.append(("one coordinate", np.full(700, 12.25), np.full(700, -33.5), rng.permutation(700).astype(np.uint64) << np.uint64(9)))
    # the same with repeated keys: the index decides
    sets.append(("one coordinate, one key", np.full(300, 12.25), np.full(300, -33.5), np.full(300, 5, np.uint64)))
    return sets


def mirror_pairs(seed=4, n=200):
    """(+-lat, lon0 +- x) around the equatorial query (0, 0): four candidates of one distance each, by the formula's symmetry"""
    rng = np.random.default_rng(seed)
    la, x = rng.uniform(0.0, 80.0, n), rng.uniform(0.0, 170.0, n)
    return np.r_[la, -la, la, -la], np.r_[x, x, -x, -x]


def ks(n):
    return sorted({0, 1, 255, 256, 257, max(n - 1, 0), n, n + 1, TOP_MAX})


def radii(dist):
    """0, inf, and one candidate's own distance with its predecessor (the closed comparison keeps it, nextafter drops it)"""
    d = np.sort(dist[dist == dist])
    own = float(d[d.size // 3]) if d.size else 1000.0
    return [0.0, math.inf, own, math.nextafter(own, 0.0)]


def position_records(lat, lon, key, ts=None):
    from mobheat._lib import POSITION_REC_DTYPE
    r = np.zeros(lat.size, POSITION_REC_DTYPE)
    key = np.asarray(key, np.uint64)
    r["provider"], r["vehicle"] = key >> np.uint64(32), key & np.uint64(0xffffffff)
    r["ts_us"] = T0 if ts is None else ts
    r["lat"], r["lon"] = lat, lon
    return r


def tile_records(lat, lon, key, seed=2):
    """records whose centroid sum / count is not the coordinate itself: count 1..9, sums = coordinate * count (rounded)"""
    from mobheat._lib import STATE_REC_DTYPE
    rng = np.random.default_rng(seed)
    r = np.zeros(lat.size, STATE_REC_DTYPE)
    r["cell"], r["window_start_us"] = key, T0
    r["count"] = rng.integers(1, 10, lat.size)
    r["sum_lat"], r["sum_lon"] = lat * r["count"], lon * r["count"]
    return r


def same(got, want, what=""):
    assert got.size == want.size, f"{what}: {got.size} records, {want.size} expected"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at rank {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")
