"""Shared by the viewport tests (tests/test_view_host.py, tests/test_gpu_view.py): the rule of DESIGN §5i restated on
Python floats -- on purpose not mobheat.readside's code -- and the (cell set, view) cases the host execution and the
device are held to.  No tolerance anywhere: every expectation is a verdict.

The rule.  A view (west, south, east, north) is valid when all four are finite, -90 <= south <= north <= 90 and
-180 <= west, east <= 180; its longitudes are [west, east], or [west, 180] and [-180, east] when west > east.  A
position is in view iff south <= lat <= north and lon is in one of those intervals.  A tile is in view iff its ring's
latitude range [min, max] intersects [south, north] and one of its longitude intervals intersects one of the view's:
[min, max], or -- max - min > 180 -- [least lng > 0, 180] and [-180, greatest lng <= 0]; the cell holding a pole has
every longitude and latitudes up to that pole; a cell without vertices is never in view.  All intervals closed."""
import functools
import math

import numpy as np

import geojson_cases as gc

WORLD = (-180.0, -90.0, 180.0, 90.0)
BOSTON = (-71.10, 42.30, -71.00, 42.40)
ATHENS = (23.60, 37.90, 23.85, 38.05)
FIXED_VIEWS = [
    (-71.05, 42.35, -71.05, 42.35),   # a point inside a res-0 cell
    WORLD,
    (180.0, -60.0, -180.0, 60.0),     # the antimeridian itself
    (170.0, -60.0, -170.0, 60.0),
    (-180.0, 90.0, 180.0, 90.0),      # the north pole alone
    (-180.0, -90.0, 180.0, -90.0),    # the south pole alone
    BOSTON,
]
NAN, INF = float("nan"), float("inf")
INVALID_VIEWS = [
    (NAN, 0.0, 1.0, 1.0), (0.0, NAN, 1.0, 1.0), (0.0, 0.0, NAN, 1.0), (0.0, 0.0, 1.0, NAN),
    (-INF, 0.0, 1.0, 1.0), (0.0, 0.0, INF, 1.0), (0.0, -INF, 1.0, 1.0), (0.0, 0.0, 1.0, INF),
    (0.0, 2.0, 1.0, 1.0),                                   # south > north
    (0.0, -90.5, 1.0, 1.0), (0.0, 0.0, 1.0, 90.0000001),     # |lat| > 90
    (-180.5, 0.0, 1.0, 1.0), (0.0, 0.0, 180.0000001, 1.0),   # |lon| > 180
]


# ---- the reference rule ----
def ref_valid(view):
    w, s, e, n = view
    if any(math.isnan(x) or math.isinf(x) for x in view):
        return False
    return s >= -90.0 and n <= 90.0 and s <= n and abs(w) <= 180.0 and abs(e) <= 180.0


def _intervals_of_view(view):
    w, _, e, _ = view
    if w <= e:
        return ((w, e),)
    return ((w, 180.0), (-180.0, e))


def _closed_meet(p, q):
    return p[0] <= q[1] and q[0] <= p[1]


def ref_point(lat, lon, view):
    _, s, _, n = view
    if lat < s or lat > n or lat != lat:
        return False
    for a, b in _intervals_of_view(view):
        if a <= lon <= b:
            return True
    return False


def ref_ring(lats, lngs, view, pole=0):
    """lats / lngs: the ring's vertices (any closing repeat is harmless); pole +1 / -1: the cell holds that pole"""
    if len(lats) == 0:
        return False
    _, s, _, n = view
    lat_lo, lat_hi = min(lats), max(lats)
    if pole > 0:
        lat_hi = 90.0
    if pole < 0:
        lat_lo = -90.0
    if not _closed_meet((lat_lo, lat_hi), (s, n)):
        return False
    if pole:
        own = ((-180.0, 180.0),)
    elif max(lngs) - min(lngs) > 180.0:
        own = ((min(x for x in lngs if x > 0.0), 180.0), (-180.0, max(x for x in lngs if x <= 0.0)))
    else:
        own = ((min(lngs), max(lngs)),)
    return any(_closed_meet(p, q) for p in own for q in _intervals_of_view(view))


# ---- the cases ----
def _pentagon(bc, res):
    return (1 << 59) | (res << 52) | (bc << 45) | ((1 << (3 * (15 - res))) - 1)


def _lng_ends(lngs):
    """(west end, east end) of the ring's longitude set: the bounds a view can touch from outside"""
    if max(lngs) - min(lngs) > 180.0:
        return min(x for x in lngs if x > 0.0), max(x for x in lngs if x <= 0.0)
    return min(lngs), max(lngs)


def _edge_views(lats, lngs, pole):
    """views built from the cell's own extremes: (view, expected verdict for this cell) -- the edge itself, one ulp away
    from the cell, one ulp toward it"""
    out = []
    up, down = math.inf, -math.inf
    if pole <= 0:    # the view's south edge against the cell's max lat
        t = max(lats)
        out += [((-180.0, t, 180.0, 90.0), True), ((-180.0, math.nextafter(t, up), 180.0, 90.0), False),
                ((-180.0, math.nextafter(t, down), 180.0, 90.0), True)]
    if pole >= 0:    # the view's north edge against the cell's min lat
        t = min(lats)
        out += [((-180.0, -90.0, 180.0, t), True), ((-180.0, -90.0, 180.0, math.nextafter(t, down)), False),
                ((-180.0, -90.0, 180.0, math.nextafter(t, up)), True)]
    if pole == 0:
        w_end, e_end = _lng_ends(lngs)
        if e_end < 179.0:   # the view's west edge against the cell's east end
            far = e_end + 1.0
            out += [((e_end, -90.0, far, 90.0), True), ((math.nextafter(e_end, up), -90.0, far, 90.0), False),
                    ((math.nextafter(e_end, down), -90.0, far, 90.0), True)]
        if w_end > -179.0:  # the view's east edge against the cell's west end
            far = w_end - 1.0
            out += [((far, -90.0, w_end, 90.0), True), ((far, -90.0, math.nextafter(w_end, down), 90.0), False),
                    ((far, -90.0, math.nextafter(w_end, up), 90.0), True)]
    return out


CLASSES = ("ordinary", "pentagon", "wrapping", "pole", "crossing")


class CaseSet:
    """cells (uint64[n]) with their rings (lats / lngs: lists per cell), pole (+1 / -1 / 0) and class; views; expect
    (uint8[len(views), n]): the reference's verdicts, computed once"""


@functools.lru_cache(maxsize=None)
def case_set():
    from mobheat import _lib
    from oracle import h3_oracle
    boundary = _lib.cells_to_boundary_host_selftest
    parts = [gc.tile_cells(boundary)]
    # cells that straddle +-180 degrees
    grid = np.linspace(-84.0, 84.0, 29)
    for r in (0, 2, 5, 8):
        c = np.unique(np.concatenate([h3_oracle.latlng_to_cell(grid, np.full(grid.size, lon), r) for lon in (179.9999, -179.9999)]))
        la, lo, nv = boundary(c)
        wraps = np.array([lo[k, :nv[k]].max() - lo[k, :nv[k]].min() > 180.0 for k in range(c.size)])
        assert wraps.sum() >= 4, f"res {r}: {int(wraps.sum())} wrapping cells"
        parts.append(c[wraps][:12])
    # both pole cells
    poles = {}
    for r in (0, 1, 8, 15):
        p = h3_oracle.latlng_to_cell(np.array([90.0, -90.0]), np.array([0.0, 0.0]), r)
        poles[int(p[0])], poles[int(p[1])] = 1, -1
        parts.append(p)
    parts.append(np.array([_pentagon(bc, r) for r in (1, 2) for bc in gc.PENTAGON_BASE_CELLS], np.uint64))
    parts.append(np.concatenate([h3_oracle.latlng_to_cell(np.array([42.35]), np.array([-71.05]), r) for r in (0, 5)]))   # around the point view
    cells = np.concatenate(parts).astype(np.uint64)
    la, lo, nv = boundary(cells)
    cs = CaseSet()
    cs.cells = cells
    cs.lats = [la[k, :nv[k]].tolist() for k in range(cells.size)]
    cs.lngs = [lo[k, :nv[k]].tolist() for k in range(cells.size)]
    cs.pole = [poles.get(int(c), 0) for c in cells]
    cs.cls = []
    for k in range(cells.size):
        if nv[k] == 0:
            cs.cls.append("invalid")
        elif cs.pole[k]:
            cs.cls.append("pole")
        elif nv[k] in (5, 10):
            cs.cls.append("pentagon")
        elif 7 <= nv[k] <= 9:
            cs.cls.append("crossing")
        elif max(cs.lngs[k]) - min(cs.lngs[k]) > 180.0:
            cs.cls.append("wrapping")
        else:
            cs.cls.append("ordinary")
    # views from the cells' own vertices: three cells of every class (every pole cell), each held to its own verdicts
    views, own = list(FIXED_VIEWS), {}
    taken = {c: 0 for c in CLASSES}
    for k in range(cells.size):
        c = cs.cls[k]
        if c == "invalid" or (c != "pole" and taken[c] >= 3):
            continue
        taken[c] += 1
        for v, want in _edge_views(cs.lats[k], cs.lngs[k], cs.pole[k]):
            assert ref_valid(v), v
            own[len(views)] = (k, want)
            views.append(v)
    cs.views = views
    cs.expect = np.array([[ref_ring(cs.lats[k], cs.lngs[k], v, cs.pole[k]) for k in range(cells.size)] for v in views], np.uint8)
    # an edge equal to the cell's extreme keeps it, one ulp away drops it, one ulp toward keeps it
    for i, (k, want) in own.items():
        assert bool(cs.expect[i, k]) == want, f"view {views[i]} cell {int(cells[k]):x}: {bool(cs.expect[i, k])}, {want} by construction"
    # the whole world keeps every valid cell; every class gets both verdicts somewhere
    valid = np.array([c != "invalid" for c in cs.cls])
    assert np.array_equal(cs.expect[FIXED_VIEWS.index(WORLD)].astype(bool), valid)
    assert not cs.expect[:, ~valid].any()
    for c in CLASSES:
        cols = cs.expect[:, [k for k in range(cells.size) if cs.cls[k] == c]]
        assert cols.size and cols.any() and not cols.all(), f"class {c}: one verdict only"
    return cs


def device_cells_in_view(cells, view, memory, device=0):
    """hm_cells_in_view on host or device pointers: uint8[n]"""
    import ctypes

    from mobheat import _lib
    lib = _lib.load()
    cells = np.ascontiguousarray(cells, np.uint64)
    n = cells.size
    keep = np.full(n, 7, np.uint8)
    v = _lib.view_struct(view)
    if memory == _lib.HM_MEM_HOST or n == 0:
        rc = lib.hm_cells_in_view(_lib.ptr(cells) if n else None, n, memory, device, ctypes.byref(v), _lib.ptr(keep) if n else None)
        _lib.check(rc, None, "hm_cells_in_view")
        return keep
    dc, dk = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.hm_device_alloc(device, n * 8, ctypes.byref(dc)), None, "hm_device_alloc")
    _lib.check(lib.hm_device_alloc(device, n, ctypes.byref(dk)), None, "hm_device_alloc")
    try:
        _lib.check(lib.hm_memcpy(dc, _lib.ptr(cells), n * 8, 0), None, "hm_memcpy")
        _lib.check(lib.hm_cells_in_view(dc, n, memory, device, ctypes.byref(v), dk), None, "hm_cells_in_view")
        _lib.check(lib.hm_memcpy(_lib.ptr(keep), dk, n, 1), None, "hm_memcpy")
    finally:
        lib.hm_device_free(device, dc)
        lib.hm_device_free(device, dk)
    return keep
