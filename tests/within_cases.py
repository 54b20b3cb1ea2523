"""Shared by the geofence tests (tests/test_within_host.py, tests/test_gpu_within.py): the zone sets and the point sets the
host execution, readside.points_in_zones and the device are held to, and an exact evaluation of the membership rule of
include/mobheat.h with fractions.Fraction -- on purpose none of the library's code.

The rule.  A point is in a zone iff it crosses an odd number of the zone's edges, all rings together.  Edge (a, b) with the
endpoints ordered so that a.lat < b.lat (a.lat == b.lat: never crossed) is crossed iff a.lat <= lat < b.lat and
(b.lon - a.lon) * (lat - a.lat) > (lon - a.lon) * (b.lat - a.lat).  Nothing has a tolerance: device, host execution and numpy
agree on every point, on-edge points and vertices included; the exact evaluation agrees wherever rounding cannot decide
(exact_margin_ok)."""
import functools
from fractions import Fraction

import numpy as np

import density_cases as dc

BOX = dc.BOSTON_BOX   # (lat0, lat1, lon0, lon1)
TILE = 256 * 8        # slots per workgroup iteration of the scans (256 lanes x DUMP_PER)
STAGE = 512           # edges per LDS stage (csrc/k_within.h WITHIN_STAGE)
ZLDS = 1024           # zones whose totals a workgroup keeps in LDS (WITHIN_ZLDS)


def _zones(rings):
    from mobheat._lib import Zones
    return Zones.from_rings(rings)


def _rect(lat0, lat1, lon0, lon1, reverse=False):
    r = [(lat0, lon0), (lat0, lon1), (lat1, lon1), (lat1, lon0)]
    return r[::-1] if reverse else r


@functools.lru_cache(maxsize=None)
def triangle():
    return _zones([[[(42.22, -71.18), (42.43, -71.05), (42.25, -70.97)]]])


@functools.lru_cache(maxsize=None)
def square_with_hole():
    return _zones([[_rect(42.25, 42.40, -71.15, -71.00), _rect(42.30, 42.35, -71.10, -71.05, reverse=True)]])


@functools.lru_cache(maxsize=None)
def concave_c():
    c = [(42.22, -71.18), (42.22, -71.00), (42.27, -71.00), (42.27, -71.13), (42.38, -71.13), (42.38, -71.00), (42.43, -71.00),
         (42.43, -71.18)]
    return _zones([[c]])


@functools.lru_cache(maxsize=None)
def overlapping_squares():
    return _zones([[_rect(42.25, 42.35, -71.15, -71.05)], [_rect(42.30, 42.40, -71.10, -71.00, reverse=True)]])


@functools.lru_cache(maxsize=None)
def mesh_vertices(nx=8, ny=8, seed=4):
    """the (ny + 1) x (nx + 1) vertices of the jittered mesh over BOX: the border's vertices stay on the border"""
    rng = np.random.default_rng(seed)
    la = np.linspace(BOX[0], BOX[1], ny + 1)[:, None] + np.zeros((1, nx + 1))
    lo = np.linspace(BOX[2], BOX[3], nx + 1)[None, :] + np.zeros((ny + 1, 1))
    dla, dlo = (BOX[1] - BOX[0]) / ny, (BOX[3] - BOX[2]) / nx
    la[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, (ny - 1, nx - 1)) * dla
    lo[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, (ny - 1, nx - 1)) * dlo
    return la, lo


@functools.lru_cache(maxsize=None)
def mesh(nx=8, ny=8):
    """2 nx ny triangles that tile BOX: every cell of the jittered grid cut along one of its diagonals (alternating), every
    other triangle clockwise"""
    la, lo = mesh_vertices(nx, ny)
    v = lambda i, j: (float(la[i, j]), float(lo[i, j]))
    tris = []
    for i in range(ny):
        for j in range(nx):
            a, b, c, d = v(i, j), v(i, j + 1), v(i + 1, j + 1), v(i + 1, j)
            pair = [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
            for t in pair:
                tris.append([t[::-1] if len(tris) % 2 else t])
    return _zones(tris)


@functools.lru_cache(maxsize=None)
def horizontal_edge():
    """a zone whose bottom and top edges are horizontal, at the latitudes of horizontal_points()"""
    return _zones([[_rect(42.30, 42.35, -71.10, -71.05)], [[(42.30, -71.05), (42.30, -71.00), (42.40, -71.02)]]])


def horizontal_points():
    lo = np.array([-71.12, -71.10, -71.075, -71.05, -71.03, -71.00, -70.99])
    return np.r_[np.full(lo.size, 42.30), np.full(lo.size, 42.35)], np.r_[lo, lo]


@functools.lru_cache(maxsize=None)
def degenerate():
    """a zero-area ring (three collinear vertices), a ring that goes out and back, and a real triangle after them"""
    return _zones([[[(42.25, -71.15), (42.30, -71.10), (42.35, -71.05)]], [[(42.25, -71.00), (42.40, -71.00), (42.25, -71.00)]],
                   [[(42.22, -71.18), (42.43, -71.05), (42.25, -70.97)]]])


@functools.lru_cache(maxsize=None)
def circles(n=64, verts=1024):
    """n circles of `verts` vertices each on a grid over BOX, neighbours overlapping: with 64 x 1024 the vertex limit, and
    every zone two LDS stages"""
    side = int(round(np.sqrt(n)))
    t = np.arange(verts) * (2.0 * np.pi / verts)
    rings = []
    for k in range(n):
        i, j = divmod(k, side)
        cla = BOX[0] + (i + 0.5) * (BOX[1] - BOX[0]) / side
        clo = BOX[2] + (j + 0.5) * (BOX[3] - BOX[2]) / side
        r = 0.7 * (BOX[1] - BOX[0]) / side
        la, lo = cla + r * np.sin(t), clo + r * np.cos(t) * (1 if k % 2 else -1)
        rings.append([list(zip(la.tolist(), lo.tolist()))])
    return _zones(rings)


@functools.lru_cache(maxsize=None)
def triangles4096(side=64):
    """HM_ZONES_MAX one-triangle zones, one per cell of a side x side grid over BOX (more zones than a workgroup totals in LDS)"""
    dla, dlo = (BOX[1] - BOX[0]) / side, (BOX[3] - BOX[2]) / side
    rings = []
    for k in range(side * side):
        i, j = divmod(k, side)
        a = (BOX[0] + i * dla, BOX[2] + j * dlo)
        rings.append([[a, (a[0], a[1] + dlo), (a[0] + dla, a[1] + 0.5 * dlo)]])
    return _zones(rings)


def _circle(cla, clo, r, verts):
    t = np.arange(verts) * (2.0 * np.pi / verts)
    return [list(zip((cla + r * np.sin(t)).tolist(), (clo + r * np.cos(t)).tolist()))]


def _regular(cla, clo, r, verts):
    """a regular polygon of `verts` vertices, none of its edges horizontal (every one of them is an edge of the packed set)"""
    t = (np.arange(verts) + 0.25) * (2.0 * np.pi / verts)
    return [list(zip((cla + r * np.sin(t)).tolist(), (clo + r * np.cos(t)).tolist()))]


_TRI_A = [[(42.22, -71.18), (42.43, -71.05), (42.25, -70.97)]]
_TRI_B = [[(42.40, -71.15), (42.24, -71.12), (42.30, -71.00)]]


@functools.lru_cache(maxsize=None)
def stage_span():
    """a 3-vertex zone, a 1500-vertex circle, a 3-vertex zone: the circle's edges are [3, 1503) of the set's, three LDS
    stages at unaligned offsets, and the last zone starts in the middle of a stage"""
    return _zones([_TRI_A, _circle(42.32, -71.08, 0.09, 1500), _TRI_B])


@functools.lru_cache(maxsize=None)
def stage_end():
    """zones of 509, 3 and 512 edges: the second ends exactly at the first stage's end, the third is the second stage"""
    return _zones([_regular(42.30, -71.10, 0.07, 509), _TRI_A, _regular(42.34, -71.04, 0.08, 512)])


def _triangles(n, side=33):
    dla, dlo = (BOX[1] - BOX[0]) / side, (BOX[3] - BOX[2]) / side
    rings = []
    for k in range(n):
        i, j = divmod(k, side)
        a = (BOX[0] + i * dla, BOX[2] + j * dlo)
        rings.append([[a, (a[0], a[1] + dlo), (a[0] + dla, a[1] + 0.5 * dlo)]])
    return _zones(rings)


@functools.lru_cache(maxsize=None)
def triangles1024():
    """exactly ZLDS one-triangle zones: the last set whose totals a workgroup keeps in LDS"""
    return _triangles(ZLDS)


@functools.lru_cache(maxsize=None)
def triangles1025():
    """ZLDS + 1 one-triangle zones: the first set whose totals go straight to memory"""
    return _triangles(ZLDS + 1)


# the sets at the LDS staging's and the LDS totals' edges (tests/test_gpu_read_grid.py runs them over several grid iterations)
STAGED = ("stage_span", "stage_end", "triangles1024", "triangles1025")
SMALL = ("triangle", "square_with_hole", "concave_c", "overlapping_squares", "mesh", "horizontal_edge", "degenerate")
LARGE = ("circles", "triangles4096")
ALL = SMALL + LARGE


def zone_set(name):
    return globals()[name]()


# ---- points ----
def random_points(n, seed=0, margin=0.02):
    rng = np.random.default_rng(seed)
    return rng.uniform(BOX[0] - margin, BOX[1] + margin, n), rng.uniform(BOX[2] - margin, BOX[3] + margin, n)


def edges_of(zones):
    """(a_lat, a_lon, b_lat, b_lon) of every edge, in ring order (not canonical)"""
    al, ao, bl, bo = [], [], [], []
    for z in range(zones.n_zones):
        for la, lo in zones.rings(z):
            al.append(la)
            ao.append(lo)
            bl.append(np.roll(la, -1))
            bo.append(np.roll(lo, -1))
    return tuple(np.concatenate(x) for x in (al, ao, bl, bo))


def edge_points(zones, seed=1, stride=1):
    """every `stride`-th edge's midpoint and a random point on it, computed in binary64 (so: on or beside the edge)"""
    rng = np.random.default_rng(seed)
    al, ao, bl, bo = (x[::stride] for x in edges_of(zones))
    t = rng.uniform(0.0, 1.0, al.size)
    return np.r_[(al + bl) * 0.5, al + t * (bl - al)], np.r_[(ao + bo) * 0.5, ao + t * (bo - ao)]


def box_points(zones):
    """per zone: the corners and side midpoints of its box (min / max latitude and longitude) and the points one ulp
    outside and inside each side"""
    la, lo = [], []
    for z in range(zones.n_zones):
        zla = np.concatenate([r[0] for r in zones.rings(z)])
        zlo = np.concatenate([r[1] for r in zones.rings(z)])
        a0, a1, o0, o1 = zla.min(), zla.max(), zlo.min(), zlo.max()
        lats = [a0, a1, (a0 + a1) * 0.5, np.nextafter(a0, -np.inf), np.nextafter(a0, np.inf), np.nextafter(a1, -np.inf), np.nextafter(a1, np.inf)]
        lons = [o0, o1, (o0 + o1) * 0.5, np.nextafter(o0, -np.inf), np.nextafter(o0, np.inf), np.nextafter(o1, -np.inf), np.nextafter(o1, np.inf)]
        for x in lats:
            for y in lons:
                la.append(x)
                lo.append(y)
    return np.array(la), np.array(lo)


def special_points():
    n, i = np.nan, np.inf
    return (np.array([n, 42.3, n, i, -i, 42.3, 42.3, 0.0, 1e300, 42.3]), np.array([-71.1, n, n, -71.1, -71.1, i, -i, 0.0, -71.1, -1e300]))


def point_sets(name, n_random=3000):
    """[(what, lat, lon)] for a zone set: random points, every vertex, points on the edges, the boxes' sides, non-finite"""
    zones = zone_set(name)
    stride = 1 if name in SMALL else 37
    sets = [("random", *random_points(n_random, seed=len(name))),
            ("vertices", zones.lat[::stride].copy(), zones.lon[::stride].copy()),
            ("on edges", *edge_points(zones, stride=stride)),
            ("special", *special_points())]
    if name in SMALL:
        sets.append(("box sides", *box_points(zones)))
    if name == "horizontal_edge":
        sets.append(("at the horizontal edges' latitude", *horizontal_points()))
    return sets


# ---- the rule, exactly ----
def exact(zones, lat, lon):
    """(first, hits, decided) by the rule in exact rational arithmetic; decided[i]: for every edge whose latitude range
    holds the point, the exact margin |L - R| exceeds 2^-48 (|L| + |R|) -- three roundings a side (relative 2^-53 each)
    cannot turn its sign, so the binary64 evaluation must agree there"""
    F = Fraction
    eps = F(1, 1 << 48)
    first, hits, decided = [], [], []
    zone_edges = []
    for z in range(zones.n_zones):
        e = []
        for la, lo in zones.rings(z):
            n = len(la)
            for k in range(n):
                a, b = (F(float(la[k])), F(float(lo[k]))), (F(float(la[(k + 1) % n])), F(float(lo[(k + 1) % n])))
                if a[0] == b[0]:
                    continue
                e.append((a, b) if a[0] < b[0] else (b, a))
        zone_edges.append(e)
    for y, x in zip(lat, lon):
        y, x = F(float(y)), F(float(x))
        f, h, ok = -1, 0, True
        for z, e in enumerate(zone_edges):
            c = 0
            for a, b in e:
                if not (a[0] <= y < b[0]):
                    continue
                L, R = (b[1] - a[1]) * (y - a[0]), (x - a[1]) * (b[0] - a[0])
                if abs(L - R) <= eps * (abs(L) + abs(R)):
                    ok = False
                c += L > R
            if c & 1:
                h += 1
                f = z if f < 0 else f
        first.append(f)
        hits.append(h)
        decided.append(ok)
    return np.array(first, np.int32), np.array(hits, np.uint32), np.array(decided, bool)


# ---- the two queries restated in numpy (readside.points_in_zones one zone at a time) ----
def positions_expected(zones, recs, since_us=None):
    """(kept records in input order, labels, totals) of hm_positions_within by the rule"""
    from mobheat import readside
    keep = np.ones(recs.size, bool) if since_us is None else recs["ts_us"] >= int(since_us)
    inside, tot = readside.zone_totals_of(zones, recs["lat"], recs["lon"], keep=keep, ts_us=recs["ts_us"])
    any_ = inside.any(axis=0) if zones.n_zones else np.zeros(recs.size, bool)
    label = np.where(any_, inside.argmax(axis=0), -1).astype(np.int32) if zones.n_zones else np.full(recs.size, -1, np.int32)
    return recs[any_], label[any_], tot


def tiles_expected(zones, recs):
    from mobheat import readside
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = recs["count"].astype(np.uint64).astype(np.float64)
        la, lo = recs["sum_lat"] / cnt, recs["sum_lon"] / cnt
    inside, tot = readside.zone_totals_of(zones, la, lo, count=recs["count"], n_speed=recs["n_speed"], sum_speed=recs["sum_speed"])
    any_ = inside.any(axis=0)
    label = np.where(any_, inside.argmax(axis=0), -1).astype(np.int32)
    return recs[any_], label[any_], tot


def same_totals(got, want, what="", dyadic=True):
    """counts, n, n_speed and newest_us exactly; sum_speed bit-equal on dyadic speeds, else its average within dc.REL"""
    for f in ("n", "count", "n_speed", "newest_us", "reserved"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    if dyadic:
        assert got["sum_speed"].tobytes() == want["sum_speed"].tobytes(), f"{what}: sum_speed on dyadic speeds"
    else:
        has = want["n_speed"] > 0
        a, b = got["sum_speed"][has] / got["n_speed"][has], want["sum_speed"][has] / want["n_speed"][has]
        assert np.all(np.abs(a - b) <= dc.REL * np.maximum(np.abs(a), np.abs(b))), f"{what}: avg speed"
        assert not got["sum_speed"][~has].any(), f"{what}: sum_speed of a zone without a speed"
