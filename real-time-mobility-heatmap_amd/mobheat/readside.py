"""The read side's hot loop: the reference's web API turns every tile of the latest window into
a GeoJSON polygon, one h3.cell_to_boundary call per tile (reference app.py:19-41 h3_boundary_geojson, :45-69
api_tiles_latest).  Here the boundaries of all the window's cells come from one GPU launch (hm_cells_to_boundary,
csrc/h3_boundary.h); the Flask app, MongoDB queries and the Leaflet page stay out of scope.

Mirrors the reference's helper names and output shapes:
  h3_boundary_geojson(cell_id) -> [[lng, lat], ..., [lng, lat]] closed ring (app.py:19-41)
  tiles_latest_collection(docs) -> the FeatureCollection dict api_tiles_latest returns for a window's tile docs
"""
import numpy as np

from . import _lib
from ._lib import HM_MEM_HOST, check, ptr


def cells_to_boundary(cells, device=0):
    """cellToBoundary of an array of cells on the GPU: (lat [n, 10], lng [n, 10], nverts [n]) in degrees,
    upstream's vertex order; nverts 0 for an invalid index."""
    lib = _lib.load()
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    lat = np.empty((cells.size, 10))
    lng = np.empty((cells.size, 10))
    nv = np.empty(cells.size, np.int32)
    if cells.size:
        check(lib.hm_cells_to_boundary(ptr(cells), cells.size, HM_MEM_HOST, int(device), ptr(lat), ptr(lng), ptr(nv)),
              None, "hm_cells_to_boundary")
    return lat, lng, nv


# ---- a map viewport: (west, south, east, north) in degrees (include/mobheat.h hm_view) ----
def view_valid(view):
    """All four finite, -90 <= south <= north <= 90, -180 <= west, east <= 180."""
    w, s, e, n = (float(x) for x in view)
    return -90.0 <= s <= n <= 90.0 and -180.0 <= w <= 180.0 and -180.0 <= e <= 180.0


def view_from_bbox(text):
    """The view of a query string's bbox=west,south,east,north (Leaflet's getBounds().toBBoxString()): a tuple of four
    floats.  ValueError for anything but four numbers that form a valid view (west > east is valid: the view crosses
    the antimeridian)."""
    parts = str(text).split(",")
    if len(parts) != 4:
        raise ValueError(f"bbox {text!r}: four comma-separated numbers expected (west,south,east,north)")
    try:
        view = tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError(f"bbox {text!r}: not a number") from None
    if not view_valid(view):
        raise ValueError(f"bbox {text!r}: finite, -90 <= south <= north <= 90 and -180 <= west, east <= 180 expected")
    return view


def _view_lngs(view):
    w, _, e, _ = view
    return [(w, e)] if w <= e else [(w, 180.0), (-180.0, e)]


def point_in_view(lat, lon, view):
    """south <= lat <= north and lon in the view's longitudes (closed; plain float comparisons)."""
    _, s, _, n = view
    return bool(s <= lat <= n and any(a <= lon <= b for a, b in _view_lngs(view)))


def ring_in_view(ring, view, pole=None):
    """Does the latitude-longitude box of a GeoJSON ring [[lng, lat], ...] meet the view?  The ring's longitudes are
    [min, max], or -- when they span more than 180 degrees, a ring across the antimeridian -- [min of the positive, 180]
    and [-180, max of the others].  pole "north" / "south": the ring is that of the cell containing the pole (every
    longitude, latitudes up to the pole).  An empty ring is never in view.  The comparison form of csrc/k_view.h."""
    if not ring:
        return False
    lngs, lats = [float(p[0]) for p in ring], [float(p[1]) for p in ring]
    la0, la1, lo0, lo1 = min(lats), max(lats), min(lngs), max(lngs)
    if pole == "north":
        la1 = 90.0
    elif pole == "south":
        la0 = -90.0
    elif pole is not None:
        raise ValueError("pole: None, 'north' or 'south'")
    _, s, _, n = view
    if not (la0 <= n and s <= la1):
        return False
    if pole is not None:
        mine = [(-180.0, 180.0)]
    elif lo1 - lo0 > 180.0:
        mine = [(min(x for x in lngs if x > 0.0), 180.0), (-180.0, max(x for x in lngs if not x > 0.0))]
    else:
        mine = [(lo0, lo1)]
    return any(a <= d and c <= b for a, b in mine for c, d in _view_lngs(view))


def pole_cells(res):
    """(north, south): the two cells of resolution res that contain a pole, latLngToCell(+-90, 0, res) (host execution)."""
    c = _lib.latlng_to_cell_host_selftest(np.array([90.0, -90.0]), np.array([0.0, 0.0]), int(res))
    return int(c[0]), int(c[1])


def cells_in_view(cells, view, device=0):
    """Which cells' boundary boxes meet the view, on the GPU (hm_cells_in_view): bool[n].  ValueError for an invalid view."""
    import ctypes
    if not view_valid(view):
        raise ValueError(f"invalid view {tuple(view)!r}")
    lib = _lib.load()
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    keep = np.zeros(cells.size, np.uint8)
    if cells.size:
        v = _lib.view_struct(view)
        check(lib.hm_cells_in_view(ptr(cells), cells.size, HM_MEM_HOST, int(device), ctypes.byref(v), ptr(keep)), None,
              "hm_cells_in_view")
    return keep.astype(bool)


def _tile_features_in_view(collection, view):
    """the collection's features whose ring meets the view (the pure-Python filter)"""
    if not view_valid(view):
        raise ValueError(f"invalid view {tuple(view)!r}")
    poles = {}
    kept = []
    for f in collection["features"]:
        cell = _cell_int(f["properties"]["cellId"])
        res = (cell >> 52) & 0xf
        if res not in poles:
            poles[res] = pole_cells(res)
        pole = "north" if cell == poles[res][0] else "south" if cell == poles[res][1] else None
        if ring_in_view(f["geometry"]["coordinates"][0], view, pole):
            kept.append(f)
    return {"type": "FeatureCollection", "features": kept}


def _cell_int(cell_id):
    return int(cell_id, 16) if isinstance(cell_id, str) else int(cell_id)


def rings(cells, device=0):
    """GeoJSON rings of many cells: [[lng, lat], ...] closed (first vertex repeated), as h3_boundary_geojson."""
    lat, lng, nv = cells_to_boundary(np.array([_cell_int(c) for c in cells], dtype=np.uint64), device)
    out = []
    for k in range(len(nv)):
        ring = [[float(lng[k, v]), float(lat[k, v])] for v in range(nv[k])]
        if ring and ring[0] != ring[-1]:
            ring.append(ring[0])
        out.append(ring)
    return out


def h3_boundary_geojson(cell_id, device=0):
    """Closed GeoJSON ring [[lng, lat], ...] of one cell (reference app.py:19-41); cell_id as h3-py's hex string."""
    return rings([cell_id], device)[0]


def tiles_latest_collection(docs, device=0):
    """The FeatureCollection of reference app.py:45-69 for the tile documents of the latest window (dicts with
    cellId, count, avgSpeedKmh, windowStart, windowEnd as the tiles collection stores them)."""
    docs = list(docs)
    geoms = rings([d["cellId"] for d in docs], device)
    features = []
    for d, ring in zip(docs, geoms):
        props = {"cellId": d["cellId"], "count": int(d.get("count", 0)), "avgSpeedKmh": float(d.get("avgSpeedKmh", 0.0)),
                 "windowStart": d["windowStart"].isoformat(), "windowEnd": d["windowEnd"].isoformat()}
        features.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [ring]},
                         "properties": props})
    return {"type": "FeatureCollection", "features": features}


def tile_docs_from_engine(engine, res=None, city="boston", tz=None, window_start_us=None):
    """The tile documents of one live window (None: the newest) as the sink stores them (cellId, windowStart,
    windowEnd, count, avgSpeedKmh, centroid, city, grid), read from the engine's state rolled up to resolution res
    (HeatmapEngine.window_tiles) -- no MongoDB in between.  windowStart / windowEnd are the naive local datetimes the
    sink writes (stream._spark_datetime: the process's zone), or zone tz's wall time when a tzinfo is given."""
    import datetime as _dt

    from .stream import _spark_datetime

    def when(us):
        us = int(us)
        if tz is None:
            return _spark_datetime(us)
        return _dt.datetime.fromtimestamp(us // 1000000, tz).replace(tzinfo=None, microsecond=us % 1000000)
    res = engine.h3_res if res is None else int(res)
    t = engine.window_tiles(window_start_us, res)
    docs = []
    for k in range(len(t)):
        docs.append({"city": city, "grid": f"h3r{res}", "cellId": format(int(t.cell[k]), "x"),
                     "windowStart": when(t.window_start_us[k]), "windowEnd": when(t.window_end_us[k]),
                     "count": int(t.count[k]), "avgSpeedKmh": 0.0 if t.speed_null[k] else float(t.avg_speed[k]),
                     "centroid": {"type": "Point", "coordinates": [float(t.avg_lon[k]), float(t.avg_lat[k])]}})
    return docs


def tiles_latest_from_engine(engine, res=None, city="boston", tz=None, view=None):
    """The FeatureCollection api_tiles_latest returns (reference app.py:45-69) for the newest window the engine's
    state still holds, at H3 resolution res <= the engine's (None: the engine's own): the window's tiles rolled up on
    the GPU (hm_window_rollup), their boundaries from one more launch (tiles_latest_collection).  "Latest" is the
    newest window the watermark has not evicted; the reference's Mongo keeps windows until their TTL.
    view=(west, south, east, north): only the tiles in view, filtered here in Python (ring_in_view)."""
    fc = tiles_latest_collection(tile_docs_from_engine(engine, res, city, tz), engine.device)
    return fc if view is None else _tile_features_in_view(fc, view)


def positions_latest_collection(docs):
    """The FeatureCollection of reference app.py:71-88 for documents shaped like the positions_latest collection
    (provider, vehicleId, ts, loc: {type: Point, coordinates: [lon, lat]})."""
    import datetime as _dt
    features = []
    for d in docs:
        lon, lat = d["loc"]["coordinates"]
        ts = d.get("ts")
        props = {"provider": d.get("provider"), "vehicleId": d.get("vehicleId"),
                 "ts": ts.isoformat() if isinstance(ts, _dt.datetime) else str(ts)}
        features.append({"type": "Feature", "geometry": {"type": "Point", "coordinates": [lon, lat]}, "properties": props})
    return {"type": "FeatureCollection", "features": features}


def position_docs_from_engine(engine, tz=None):
    """The engine's positions state (HeatmapEngine.positions) as positions_latest documents: _id "provider|vehicleId",
    provider, vehicleId, ts (the naive local datetime the sink writes, or zone tz's wall time: tile_docs_from_engine's
    convention), loc."""
    import datetime as _dt

    from .stream import _spark_datetime
    recs, providers, vehicles = engine.positions()
    docs = []
    for r in recs:
        us = int(r["ts_us"])
        ts = (_spark_datetime(us) if tz is None else
              _dt.datetime.fromtimestamp(us // 1000000, tz).replace(tzinfo=None, microsecond=us % 1000000))
        p, v = providers[int(r["provider"])], vehicles[int(r["vehicle"])]
        docs.append({"_id": f"{p}|{v}", "provider": p, "vehicleId": v, "ts": ts,
                     "loc": {"type": "Point", "coordinates": [float(r["lon"]), float(r["lat"])]}})
    return docs


def positions_latest_from_engine(engine, tz=None, view=None):
    """The FeatureCollection api_positions_latest returns (reference app.py:71-88), from the engine's positions state
    (HeatmapEngine.update_positions after each batch) -- no MongoDB in between.  view=(west, south, east, north): only
    the positions in view, filtered here in Python (point_in_view)."""
    fc = positions_latest_collection(position_docs_from_engine(engine, tz))
    if view is None:
        return fc
    if not view_valid(view):
        raise ValueError(f"invalid view {tuple(view)!r}")
    kept = [f for f in fc["features"] if point_in_view(f["geometry"]["coordinates"][1], f["geometry"]["coordinates"][0], view)]
    return {"type": "FeatureCollection", "features": kept}


def tiles_latest_body(engine, res=None, tz=None, view=None, top=None):
    """The response body of api_tiles_latest as bytes: json.dumps(tiles_latest_from_engine(engine, res, tz=tz),
    separators=(",", ":")), rolled up and encoded on the GPU in one call (HeatmapEngine.window_geojson).  The dict-building
    functions above stay as the comparison form, as stream.tile_ops is for the sink.  view: the tiles in view only,
    filtered on the GPU.  top=k: the body of a /api/tiles/top?n=k route -- the k busiest of those tiles in rank order,
    json.dumps(tiles_top_from_engine(engine, k, res, tz=tz, view=view), separators=(",", ":")), selected on the GPU."""
    return engine.window_geojson(None, res, tz, view=view, top=top)


def positions_latest_body(engine, tz=None, view=None):
    """The response body of api_positions_latest as bytes: json.dumps(positions_latest_from_engine(engine, tz),
    separators=(",", ":")), encoded on the GPU from the positions state (HeatmapEngine.positions_geojson).  view: the
    positions in view only, filtered on the GPU."""
    return engine.positions_geojson(tz, view=view)


# ---- the newest window as web-map raster tiles (HeatmapEngine.window_raster, csrc/k_raster.h) ----
# the reference page's colorByCount (app.py:135-142): class k = the number of thresholds a count exceeds; class 0 -- no
# tile -- is its '#FFEDA0' made fully transparent, the six others its colours in ascending order at its fillOpacity 0.6
COUNT_THRESHOLDS = (0, 2, 5, 10, 20, 50)
COUNT_PALETTE = ((0xFF, 0xED, 0xA0, 0), (0xFE, 0xB2, 0x4C, 153), (0xFD, 0x8D, 0x3C, 153), (0xFC, 0x4E, 0x2A, 153),
                 (0xE3, 0x1A, 0x1C, 153), (0xBD, 0x00, 0x26, 153), (0x80, 0x00, 0x26, 153))


def tile_grid(z, x, y, size=256):
    """(lat float64[size], lon float64[size]): the pixel centres of slippy-map tile z/x/y (spherical Mercator, the y axis
    pointing south), degrees -- row i's latitude and column j's longitude, the grid HeatmapEngine.window_raster takes.
    ValueError for z outside 0..30, x / y outside 0..2**z - 1, size outside 1..4096."""
    z, x, y, size = int(z), int(x), int(y), int(size)
    if not 0 <= z <= 30:
        raise ValueError(f"zoom {z}: 0..30 expected")
    if not (0 <= x < 2 ** z and 0 <= y < 2 ** z):
        raise ValueError(f"tile {z}/{x}/{y}: x and y in 0..{2 ** z - 1} expected")
    if not 1 <= size <= 4096:
        raise ValueError(f"size {size}: 1..4096 expected")
    k = (np.arange(size, dtype=np.float64) + 0.5) / size
    u = (x + k) / 2.0 ** z
    v = (y + k) / 2.0 ** z
    lon = u * 360.0 - 180.0
    lat = np.degrees(np.arctan(np.sinh(np.pi * (1.0 - 2.0 * v))))
    return lat, lon


def png_from_classes(classes, palette=COUNT_PALETTE):
    """An 8-bit indexed PNG of a uint8[rows, cols] class grid: PLTE + tRNS from palette ((r, g, b, a) per class), one
    IDAT, filter 0 on every row.  Runs on the host (zlib, struct): a 64 KB tile is not a hot path.  ValueError for an
    empty grid, a palette of more than 256 entries or a class outside the palette."""
    import struct
    import zlib
    a = np.ascontiguousarray(classes, dtype=np.uint8)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("classes: a non-empty 2-D grid expected")
    pal = [tuple(int(q) for q in p) for p in palette]
    if not 1 <= len(pal) <= 256 or any(len(p) != 4 or min(p) < 0 or max(p) > 255 for p in pal):
        raise ValueError("palette: 1..256 entries of (r, g, b, a), each 0..255, expected")
    if int(a.max()) >= len(pal):
        raise ValueError(f"class {int(a.max())} outside the palette's {len(pal)} entries")
    h, w = a.shape

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    rows = np.zeros((h, w + 1), np.uint8)   # (a filter byte 0 in front of every row)
    rows[:, 1:] = a
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)) +
            chunk(b"PLTE", bytes(c for p in pal for c in p[:3])) + chunk(b"tRNS", bytes(p[3] for p in pal)) +
            chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def tiles_latest_png(engine, z, x, y, res=None, size=256):
    """What a /api/tiles/latest/{z}/{x}/{y}.png route returns: the newest live window's tile z/x/y as an indexed PNG in
    the reference page's count classes (COUNT_THRESHOLDS, COUNT_PALETTE), every pixel snapped to its H3 cell at
    resolution res (None: the engine's) and looked up on the GPU.  Which res suits which zoom is the caller's choice."""
    lat, lon = tile_grid(z, x, y, size)
    _, classes = engine.window_raster(lat, lon, None, res, COUNT_THRESHOLDS, copy=False)
    return png_from_classes(classes, COUNT_PALETTE)


# ---- the positions state as density cells (HeatmapEngine.positions_density, csrc/k_density.h) ----
def positions_density_from_engine(engine, res=None, since_us=None, tz=None, as_of_us=None, view=None, top=None):
    """The FeatureCollection a /api/positions/density?res=&since=&bbox= route returns: one tile feature (the shape of
    tiles_latest_collection, so the reference page's tilesLayer colours it by properties.count as it is) per H3 cell of
    resolution res that holds a vehicle of the engine's positions state seen since since_us -- cellId, count,
    avgSpeedKmh 0.0 (positions carry no speed), windowStart = since_us and windowEnd = as_of_us (the caller's "now") as
    tile_docs_from_engine formats a window's bounds, "" for None, and the cell's ring.  view: only the cells whose ring
    meets it, filtered here in Python (ring_in_view).  top=k: the k features with the largest count in rank order, taken
    here in Python after the view (top_of's order).  The comparison form of positions_density_body."""
    recs = engine.positions_density(res, since_us)
    ws, we = _lib.wall_iso(since_us, tz), _lib.wall_iso(as_of_us, tz)
    geoms = rings([int(c) for c in recs["cell"]], engine.device)
    features = []
    for r, ring in zip(recs, geoms):
        props = {"cellId": format(int(r["cell"]), "x"), "count": int(r["count"]), "avgSpeedKmh": 0.0, "windowStart": ws,
                 "windowEnd": we}
        features.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [ring]}, "properties": props})
    fc = {"type": "FeatureCollection", "features": features}
    fc = fc if view is None else _tile_features_in_view(fc, view)
    return fc if top is None else _top_features(fc, top)


def positions_density_body(engine, res=None, since_us=None, tz=None, as_of_us=None, view=None, top=None):
    """The same response as bytes: json.dumps(positions_density_from_engine(...), separators=(",", ":")) up to the order of
    the features, grouped, filtered and encoded on the GPU (HeatmapEngine.positions_density_geojson).  top=k: the k cells
    with the most vehicles in rank order -- then the bytes are equal including the order of the features."""
    return engine.positions_density_geojson(res, since_us, tz, as_of_us, view=view, top=top)


def positions_density_png(engine, z, x, y, res=None, since_us=None, size=256):
    """What a /api/positions/density/{z}/{x}/{y}.png route returns: tile z/x/y of the positions density as an indexed PNG
    in the reference page's count classes (COUNT_THRESHOLDS, COUNT_PALETTE), every pixel snapped to its H3 cell at
    resolution res (None: the engine's) and looked up on the GPU."""
    lat, lon = tile_grid(z, x, y, size)
    _, classes = engine.positions_density_raster(lat, lon, res, since_us, COUNT_THRESHOLDS, copy=False)
    return png_from_classes(classes, COUNT_PALETTE)


# ---- top-k hotspots: the k records with the largest count in rank order (HeatmapEngine.top_records, csrc/k_top.h) ----
TOP_MAX = _lib.HM_TOP_MAX


def top_order(count, cell, k):
    """The input indices of the first min(k, n) records in the top's order: count descending as int64, then cell
    ascending as uint64, then input index ascending."""
    count, cell = np.asarray(count).astype(np.int64), np.asarray(cell).astype(np.uint64)
    k = int(k)
    if not 0 <= k <= TOP_MAX:
        raise ValueError(f"k = {k} outside 0..{TOP_MAX}")
    # (~count is -count - 1: descending count without the overflow of -INT64_MIN)
    return np.lexsort((np.arange(count.size), cell, ~count))[:k]


def top_of(records, k):
    """top(records, k) in numpy: the first min(k, n) STATE_REC_DTYPE records of the order, whole -- the comparison form of
    HeatmapEngine.top_records / window_top / positions_density(top=)."""
    records = np.asarray(records, dtype=_lib.STATE_REC_DTYPE)
    return records[top_order(records["count"], records["cell"], k)]


def _top_features(collection, k):
    """the k tile features with the largest properties.count, in rank order"""
    f = collection["features"]
    order = top_order([x["properties"]["count"] for x in f], [_cell_int(x["properties"]["cellId"]) for x in f], k)
    return {"type": "FeatureCollection", "features": [f[int(i)] for i in order]}


def tiles_top_from_engine(engine, k, res=None, city="boston", tz=None, view=None):
    """The FeatureCollection a /api/tiles/top?n=k&res=&bbox= route returns: the k busiest tiles of the newest live window
    at resolution res (in view, when a view is given -- the view comes first), in rank order; tiles_latest_from_engine's
    features, filtered, ranked and cut here in Python.  The comparison form of tiles_latest_body(top=k)."""
    return _top_features(tiles_latest_from_engine(engine, res, city, tz, view), k)


# ---- change between two live windows: rising and falling tiles (HeatmapEngine.window_change, csrc/k_change.h) ----
def change_of(cur_records, base_records, window_start_us, base_start_us):
    """change(A, B) in numpy from the two windows' STATE_REC_DTYPE records (cells distinct within each): one
    CHANGE_REC_DTYPE pair per cell of either, sorted by cell -- `cur` / `base` the window's record of the cell, whole, or
    the zero record {cell, that window's start, 0, ...} where it has none.  The comparison form of
    HeatmapEngine.window_change."""
    cur = np.asarray(cur_records, dtype=_lib.STATE_REC_DTYPE)
    base = np.asarray(base_records, dtype=_lib.STATE_REC_DTYPE)
    if int(window_start_us) == int(base_start_us):
        raise ValueError("the window and its base are the same window")
    cells = np.union1d(cur["cell"], base["cell"])
    out = np.zeros(cells.size, _lib.CHANGE_REC_DTYPE)
    for half, recs, ws in (("cur", cur, window_start_us), ("base", base, base_start_us)):
        h = out[half]   # (a view)
        h["cell"] = cells
        h["window_start_us"] = int(ws)
        h[np.searchsorted(cells, recs["cell"])] = recs
    return out


def change_order(change, cell, order, k):
    """The input indices of the first min(k, n) pairs in a change order: "rising" countChange descending, "falling"
    ascending, "abs" |countChange| descending; then cell ascending as uint64, then input index."""
    change, cell = np.asarray(change).astype(np.int64), np.asarray(cell).astype(np.uint64)
    k = int(k)
    if not 0 <= k <= TOP_MAX:
        raise ValueError(f"k = {k} outside 0..{TOP_MAX}")
    code = _lib.change_order_code(order)
    primary = -change if code == _lib.HM_CHANGE_RISING else change if code == _lib.HM_CHANGE_FALLING else -np.abs(change)
    return np.lexsort((np.arange(change.size), cell, primary))[:k]


def change_top_of(pairs, order, k=TOP_MAX):
    """the first min(k, n) CHANGE_REC_DTYPE pairs of the order, whole: the comparison form of window_change(order=, k=)"""
    pairs = np.asarray(pairs, dtype=_lib.CHANGE_REC_DTYPE)
    return pairs[change_order(pairs["cur"]["count"] - pairs["base"]["count"], pairs["cur"]["cell"], order, k)]


def tiles_change_collection(pairs, window_start, window_end, device=0):
    """The FeatureCollection of CHANGE_REC_DTYPE pairs, in their order: tiles_latest_collection's feature of every cur
    half (windowStart / windowEnd: the two datetimes given) with baseCount, baseAvgSpeedKmh and countChange after
    windowEnd."""
    pairs = np.asarray(pairs, dtype=_lib.CHANGE_REC_DTYPE)

    def avg(r):
        return float(r["sum_speed"] / r["n_speed"]) if r["n_speed"] else 0.0
    docs = [{"cellId": format(int(p["cur"]["cell"]), "x"), "count": int(p["cur"]["count"]), "avgSpeedKmh": avg(p["cur"]),
             "windowStart": window_start, "windowEnd": window_end} for p in pairs]
    fc = tiles_latest_collection(docs, device)
    for f, p in zip(fc["features"], pairs):
        f["properties"]["baseCount"] = int(p["base"]["count"])
        f["properties"]["baseAvgSpeedKmh"] = avg(p["base"])
        f["properties"]["countChange"] = int(p["cur"]["count"]) - int(p["base"]["count"])
    return fc


def tiles_change_from_engine(engine, window_start_us=None, base_start_us=None, res=None, view=None, order=None, k=None, tz=None):
    """The FeatureCollection a /api/tiles/change?res=&bbox=&order=&n= route returns, built here from two window_records
    calls: change_of, the view (cells_in_view), the order (change_top_of).  Without an order the features are sorted by
    cell.  The comparison form of tiles_change_body."""
    import datetime as _dt

    from .stream import _spark_datetime

    def when(us):
        if tz is None:
            return _spark_datetime(us)
        return _dt.datetime.fromtimestamp(us // 1000000, tz).replace(tzinfo=None, microsecond=us % 1000000)
    ws, bs = engine._change_windows(window_start_us, base_start_us)
    pairs = change_of(engine.window_records(ws, res), engine.window_records(bs, res), ws, bs)
    if view is not None:
        pairs = pairs[cells_in_view(pairs["cur"]["cell"], view, engine.device)]
    if order is not None:
        pairs = change_top_of(pairs, order, TOP_MAX if k is None else k)
    return tiles_change_collection(pairs, when(ws), when(ws + engine.tile_us), engine.device)


def tiles_change_body(engine, window_start_us=None, base_start_us=None, res=None, view=None, order=None, k=None, tz=None):
    """The response body of a /api/tiles/change route as bytes, rolled up, joined, ranked and encoded on the GPU in one call
    (HeatmapEngine.window_change_geojson); without an order the features come in the join's order, not sorted."""
    return engine.window_change_geojson(window_start_us, base_start_us, res, view, order, k, tz)


# ---- a trailing span of live windows: one heatmap with per-window counts (HeatmapEngine.window_span, csrc/k_span.h) ----
SPAN_MAX_WINDOWS = _lib.HM_SPAN_MAX_WINDOWS


def cell_to_parent(cells, res):
    """upstream cellToParent for res <= every cell's resolution, in numpy: the resolution field becomes res, the digits
    past res become 7"""
    cells = np.asarray(cells, dtype=np.uint64)
    res = int(res)
    unused = np.uint64((1 << (3 * (15 - res))) - 1)
    return (cells & ~np.uint64(0xF << 52)) | np.uint64(res << 52) | unused


def span_of(per_window_records, first_us, tile_us, res):
    """span(...) in numpy from one STATE_REC_DTYPE array per window of the span, in window order (window j starts at
    first_us + j * tile_us; an empty array: a window that is not live): (records sorted by cell, series int64[n, windows])
    -- the parent of every record at res, a group-by on it adding count, n_speed and the three sums, window_start_us =
    first_us, and per parent its count in each window.  The comparison form of HeatmapEngine.window_span."""
    per = [np.asarray(r, dtype=_lib.STATE_REC_DTYPE) for r in per_window_records]
    if not 1 <= len(per) <= SPAN_MAX_WINDOWS:
        raise ValueError(f"{len(per)} windows outside 1..{SPAN_MAX_WINDOWS}")
    recs = np.concatenate(per)
    col = np.repeat(np.arange(len(per)), [r.size for r in per])
    cells, inv = np.unique(cell_to_parent(recs["cell"], res), return_inverse=True)
    out = np.zeros(cells.size, _lib.STATE_REC_DTYPE)
    out["cell"], out["window_start_us"] = cells, int(first_us)
    for f in ("count", "n_speed"):
        np.add.at(out[f], inv, recs[f])
    for f in ("sum_speed", "sum_lat", "sum_lon"):
        out[f] = np.bincount(inv, weights=recs[f], minlength=cells.size)
    series = np.zeros((cells.size, len(per)), np.int64)
    np.add.at(series, (inv, col), recs["count"])
    return out, series


def span_windows(tile_us, minutes=None, windows=None):
    """the span's length in windows: `windows` itself, or ceil(minutes / the window's minutes); one of the two"""
    if (minutes is None) == (windows is None):
        raise ValueError("a span takes minutes or windows, one of them")
    if windows is None:
        us = int(round(float(minutes) * 60_000_000))
        windows = max(1, -(-us // int(tile_us)))
    windows = int(windows)
    if not 1 <= windows <= SPAN_MAX_WINDOWS:
        raise ValueError(f"{windows} windows outside 1..{SPAN_MAX_WINDOWS}")
    return windows


def tiles_span_collection(records, series, window_start, window_end, device=0):
    """The FeatureCollection of a span's records, in their order: tiles_latest_collection's feature of every record
    (windowStart / windowEnd: the two datetimes given) with windows and counts -- its series row -- after windowEnd."""
    records = np.asarray(records, dtype=_lib.STATE_REC_DTYPE)
    series = np.asarray(series, dtype=np.int64)
    assert series.ndim == 2 and series.shape[0] == records.size
    docs = [{"cellId": format(int(r["cell"]), "x"), "count": int(r["count"]),
             "avgSpeedKmh": float(r["sum_speed"] / r["n_speed"]) if r["n_speed"] else 0.0,
             "windowStart": window_start, "windowEnd": window_end} for r in records]
    fc = tiles_latest_collection(docs, device)
    for f, row in zip(fc["features"], series):
        f["properties"]["windows"] = int(row.size)
        f["properties"]["counts"] = [int(c) for c in row]
    return fc


def _span_end(engine, end_start_us):
    if end_start_us is not None:
        return int(end_start_us)
    ws, _ = engine.live_windows()
    return int(ws[-1]) if ws.size else 0


def tiles_span_from_engine(engine, minutes=None, windows=None, res=None, view=None, k=None, tz=None, end_start_us=None):
    """The FeatureCollection a /api/tiles/span?minutes=&res=&bbox=&n= route returns, built here from one window_records
    call per window: the trailing span -- the newest live window is its end (or end_start_us), windows = ceil(minutes /
    the window's minutes) -- through span_of, the view (cells_in_view) and the order (top_order).  Unranked, the features
    are sorted by cell.  The comparison form of tiles_span_body."""
    import datetime as _dt

    from .stream import _spark_datetime

    def when(us):
        if tz is None:
            return _spark_datetime(us)
        return _dt.datetime.fromtimestamp(us // 1000000, tz).replace(tzinfo=None, microsecond=us % 1000000)
    w = span_windows(engine.tile_us, minutes, windows)
    end = _span_end(engine, end_start_us)
    first = end - (w - 1) * engine.tile_us
    live = set(engine.live_windows()[0].tolist())
    per = [engine.window_records(first + j * engine.tile_us, engine.h3_res) if first + j * engine.tile_us in live
           else np.zeros(0, _lib.STATE_REC_DTYPE) for j in range(w)]
    recs, series = span_of(per, first, engine.tile_us, engine.h3_res if res is None else res)
    if view is not None:
        keep = cells_in_view(recs["cell"], view, engine.device)
        recs, series = recs[keep], series[keep]
    if k is not None:
        order = top_order(recs["count"], recs["cell"], k)
        recs, series = recs[order], series[order]
    return tiles_span_collection(recs, series, when(first), when(end + engine.tile_us), engine.device)


def tiles_span_body(engine, minutes=None, windows=None, res=None, view=None, k=None, tz=None, end_start_us=None):
    """The response body of a /api/tiles/span route as bytes, the span's windows aggregated, filtered, ranked and encoded
    on the GPU in one call (HeatmapEngine.window_span_geojson); unranked, the features come in the aggregation's order."""
    w = span_windows(engine.tile_us, minutes, windows)
    return engine.window_span_geojson(_span_end(engine, end_start_us), w, res, view, k, tz)


def tiles_span_png(engine, z, x, y, minutes=None, windows=None, res=None, size=256, end_start_us=None):
    """What a /api/tiles/span/{z}/{x}/{y}.png route returns: tile z/x/y of the trailing span's summed counts as an indexed
    PNG in the reference page's count classes, as tiles_latest_png."""
    w = span_windows(engine.tile_us, minutes, windows)
    lat, lon = tile_grid(z, x, y, size)
    _, classes = engine.window_span_raster(lat, lon, _span_end(engine, end_start_us), w, res, COUNT_THRESHOLDS, copy=False)
    return png_from_classes(classes, COUNT_PALETTE)


# ---- radius queries: what is around a point, nearest first (HeatmapEngine.positions_near / window_near, csrc/k_near.h) ----
EARTH_RADIUS_M = _lib.HM_EARTH_RADIUS_M   # MongoDB's sphere
_DEG = 0.017453292519943295               # the double math.radians multiplies by


def near_distance_m(lat0, lon0, lat, lon):
    """The distance in metres from (lat0, lon0) to (lat, lon), degrees: the comparison form of the device's distance
    (include/mobheat.h), the same binary64 operations in the same order, one rounding each -- sin / cos / asin through the
    running glibc (oracle.h3_oracle.libm), sqrt the correctly rounded one.  lat / lon: scalars (a float comes back) or
    arrays (each element on its own, the same operations: the vectorised form of one candidate at a time).  Needs the
    repository's oracle/ package on sys.path (the checker's libm binding); the engine's own calls do not."""
    from oracle.h3_oracle import libm
    scalar = np.ndim(lat) == 0 and np.ndim(lon) == 0
    lat = np.atleast_1d(np.asarray(lat, dtype=np.float64))
    lon = np.atleast_1d(np.asarray(lon, dtype=np.float64))
    lat, lon = np.broadcast_arrays(lat, lon)
    p0 = np.float64(lat0) * np.float64(_DEG)
    with np.errstate(invalid="ignore", over="ignore"):
        p1 = lat * np.float64(_DEG)
        s_h, _ = libm("sincos", (p1 - p0) * 0.5)
        s_l, _ = libm("sincos", ((lon - np.float64(lon0)) * np.float64(_DEG)) * 0.5)
        _, c0 = libm("sincos", np.full(1, p0))
        _, c1 = libm("sincos", p1)
        a = s_h * s_h + (c0[0] * c1) * (s_l * s_l)
        r = np.sqrt(a)
        r = np.where(r > 1.0, 1.0, r)
        d = (2.0 * EARTH_RADIUS_M) * libm("asin", r)
    return float(d[0]) if scalar else d


def near_valid(lat, lon, max_distance_m):
    """lat in [-90, 90], lon in [-180, 180], max_distance_m >= 0 or +inf, none NaN."""
    return -90.0 <= float(lat) <= 90.0 and -180.0 <= float(lon) <= 180.0 and float(max_distance_m) >= 0.0


def near_from_query(lat, lon, r=None):
    """The query of a route's lat=, lon= and r= (metres; None or "": no limit) strings: (lat, lon, max_distance_m) as
    floats.  ValueError for anything that is not a number or not a valid query."""
    try:
        q = (float(lat), float(lon), float("inf") if r is None or str(r) == "" else float(r))
    except (TypeError, ValueError):
        raise ValueError(f"near query ({lat!r}, {lon!r}, {r!r}): not a number") from None
    if not near_valid(*q):
        raise ValueError(f"near query {q!r}: -90 <= lat <= 90, -180 <= lon <= 180 and r >= 0 expected")
    return q


def near_order(dist, key, k):
    """The input indices of the first min(k, n) candidates in the near's order: distance ascending (non-negative doubles by
    their bits), then key ascending as uint64, then input index."""
    dist, key = np.asarray(dist, dtype=np.float64), np.asarray(key).astype(np.uint64)
    k = int(k)
    if not 0 <= k <= TOP_MAX:
        raise ValueError(f"k = {k} outside 0..{TOP_MAX}")
    return np.lexsort((np.arange(dist.size), key, dist.view(np.uint64)))[:k]


def near_of(lat0, lon0, lat, lon, key, max_distance_m=float("inf"), k=TOP_MAX, keep=None):
    """(input indices, distances) of the near query over candidate coordinates in numpy with near_distance_m: the
    candidates with keep (None: all), a distance that is not NaN and <= max_distance_m, the first k of near_order."""
    d = near_distance_m(lat0, lon0, np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    ok = (d == d) & (d <= float(max_distance_m))
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    idx = np.flatnonzero(ok)
    o = near_order(d[idx], np.asarray(key).astype(np.uint64)[idx], k)
    return idx[o], d[idx][o]


def positions_near_of(records, lat, lon, max_distance_m=float("inf"), k=TOP_MAX, since_us=None):
    """near(records, ...) in numpy on POSITION_REC_DTYPE records: (records, dist_m) -- the comparison form of
    HeatmapEngine.positions_near."""
    r = np.asarray(records, dtype=_lib.POSITION_REC_DTYPE)
    key = (r["provider"].astype(np.uint64) << np.uint64(32)) | r["vehicle"].astype(np.uint64)
    keep = None if since_us is None else r["ts_us"] >= int(since_us)
    idx, d = near_of(lat, lon, r["lat"], r["lon"], key, max_distance_m, k, keep)
    return r[idx], d


def tiles_near_of(records, lat, lon, max_distance_m=float("inf"), k=TOP_MAX):
    """The same on STATE_REC_DTYPE records by their centroid (sum_lat / count, sum_lon / count): the comparison form of
    HeatmapEngine.window_near."""
    r = np.asarray(records, dtype=_lib.STATE_REC_DTYPE)
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = r["count"].astype(np.uint64).astype(np.float64)
        idx, d = near_of(lat, lon, r["sum_lat"] / cnt, r["sum_lon"] / cnt, r["cell"], max_distance_m, k)
    return r[idx], d


def _near_features(features, lat0, lon0, point, key, max_distance_m, k, keep=None):
    """the features within the radius, nearest first, each with properties.distanceM as its last property"""
    if not near_valid(lat0, lon0, max_distance_m):
        raise ValueError(f"invalid near query {(lat0, lon0, max_distance_m)!r}")
    pts = [point(f) for f in features]
    idx, d = near_of(lat0, lon0, [p[0] for p in pts], [p[1] for p in pts], [key(f) for f in features], max_distance_m, k, keep)
    out = []
    for i, di in zip(idx, d):
        f = dict(features[int(i)])
        f["properties"] = dict(f["properties"], distanceM=float(di))
        out.append(f)
    return {"type": "FeatureCollection", "features": out}


def positions_near_from_engine(engine, lat, lon, max_distance_m=float("inf"), k=TOP_MAX, since_us=None, tz=None):
    """The FeatureCollection a /api/positions/near?lat=&lon=&r=&n= route returns: positions_latest_from_engine's features,
    filtered by since_us and the radius, ranked (distance, then provider code << 32 | vehicle code) and cut here in Python,
    with distanceM added.  The comparison form of positions_near_body."""
    recs, providers, vehicles = engine.positions()
    code = {(providers[int(r["provider"])], vehicles[int(r["vehicle"])]): (int(r["provider"]) << 32) | int(r["vehicle"]) for r in recs}
    ts = {(providers[int(r["provider"])], vehicles[int(r["vehicle"])]): int(r["ts_us"]) for r in recs}
    f = positions_latest_from_engine(engine, tz)["features"]
    name = [(x["properties"]["provider"], x["properties"]["vehicleId"]) for x in f]
    keep = None if since_us is None else [ts[m] >= int(since_us) for m in name]
    by_name = dict(zip(map(id, f), name))
    return _near_features(f, lat, lon, lambda x: (x["geometry"]["coordinates"][1], x["geometry"]["coordinates"][0]),
                          lambda x: code[by_name[id(x)]], max_distance_m, k, keep)


def tiles_near_from_engine(engine, lat, lon, max_distance_m=float("inf"), k=TOP_MAX, res=None, city="boston", tz=None):
    """The FeatureCollection a /api/tiles/near route returns: tiles_latest_from_engine's features of the newest live window
    at resolution res, ranked by the distance of the tile document's centroid (then cell) and cut here in Python, with
    distanceM added.  The comparison form of tiles_near_body."""
    docs = tile_docs_from_engine(engine, res, city, tz)
    centroid = {d["cellId"]: (d["centroid"]["coordinates"][1], d["centroid"]["coordinates"][0]) for d in docs}
    f = tiles_latest_collection(docs, engine.device)["features"]
    return _near_features(f, lat, lon, lambda x: centroid[x["properties"]["cellId"]], lambda x: _cell_int(x["properties"]["cellId"]),
                          max_distance_m, k)


def positions_near_body(engine, lat, lon, max_distance_m=float("inf"), k=TOP_MAX, since_us=None, tz=None):
    """The response body of a /api/positions/near route as bytes: json.dumps(positions_near_from_engine(...), separators=
    (",", ":")), selected, ranked and encoded on the GPU (HeatmapEngine.positions_near_geojson)."""
    return engine.positions_near_geojson(lat, lon, max_distance_m, k, since_us, tz)


def tiles_near_body(engine, lat, lon, max_distance_m=float("inf"), k=TOP_MAX, res=None, tz=None):
    """The response body of a /api/tiles/near route as bytes: json.dumps(tiles_near_from_engine(...), separators=(",", ":")),
    rolled up, ranked and encoded on the GPU (HeatmapEngine.window_near_geojson)."""
    return engine.window_near_geojson(lat, lon, max_distance_m, k, None, res, tz)


# ---- polygon geofences: what is inside zones (HeatmapEngine.positions_within / window_within, csrc/k_within.h) ----
def zones_from_geojson(obj):
    """The _lib.Zones of a GeoJSON Polygon, MultiPolygon, Feature or FeatureCollection (a dict, or its JSON text): one zone
    per Polygon, one zone of all its rings per MultiPolygon, in document order; positions are [lon, lat] (anything after
    them is ignored); a closed ring loses its last vertex.  ValueError for any other geometry.  The coordinates are the
    library's to validate (HM_E_INVALID)."""
    import json
    if isinstance(obj, (str, bytes)):
        obj = json.loads(obj)

    def ring(r):
        r = [(float(p[1]), float(p[0])) for p in r]
        return r[:-1] if len(r) > 1 and r[0] == r[-1] else r

    def zones(g):
        t = g.get("type")
        if t == "FeatureCollection":
            return [z for f in g["features"] for z in zones(f)]
        if t == "Feature":
            return zones(g["geometry"])
        if t == "Polygon":
            return [[ring(r) for r in g["coordinates"]]]
        if t == "MultiPolygon":
            return [[ring(r) for poly in g["coordinates"] for r in poly]]
        raise ValueError(f"zones_from_geojson: a {t!r} is no Polygon, MultiPolygon, Feature or FeatureCollection")
    return _lib.Zones.from_rings(zones(obj))


def zones_to_geojson(zones):
    """A FeatureCollection of one Polygon Feature per zone (its rings closed again, in the zone's order: a zone made from
    a MultiPolygon comes back as the Polygon of all its rings, which has the same members under the even-odd rule)."""
    feats = []
    for z in range(zones.n_zones):
        rings_ = []
        for la, lo in zones.rings(z):
            r = [[float(x), float(y)] for y, x in zip(la, lo)]
            rings_.append(r + [r[0]])
        feats.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": rings_}, "properties": {"zone": z}})
    return {"type": "FeatureCollection", "features": feats}


def points_in_zones(zones, lat, lon, block=1 << 21):
    """(first zone int32 or -1, hits uint32) of every point: the comparison form of the device's membership rule
    (include/mobheat.h), the same binary64 operations in the same order, one rounding each, in numpy -- per zone a points x
    edges matrix of the crossing predicate (in blocks of about `block` elements), a point is in the zone iff its row has
    an odd number of crossings."""
    lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
    first = np.full(lat.size, -1, np.int32)
    hits = np.zeros(lat.size, np.uint32)
    for z in range(zones.n_zones):
        a_lat, a_lon, b_lat, b_lon = [], [], [], []
        for la, lo in zones.rings(z):
            a_lat.append(la)
            a_lon.append(lo)
            b_lat.append(np.roll(la, -1))
            b_lon.append(np.roll(lo, -1))
        a_lat, a_lon, b_lat, b_lon = (np.concatenate(x) for x in (a_lat, a_lon, b_lat, b_lon))
        swap = a_lat > b_lat   # the canonical direction: a.lat < b.lat (a horizontal edge is never crossed: its range is empty)
        a_lat, b_lat = np.where(swap, b_lat, a_lat), np.where(swap, a_lat, b_lat)
        a_lon, b_lon = np.where(swap, b_lon, a_lon), np.where(swap, a_lon, b_lon)
        w, h = b_lon - a_lon, b_lat - a_lat
        step = max(int(block) // max(a_lat.size, 1), 1)
        inside = np.zeros(lat.size, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(0, lat.size, step):
                la, lo = lat[i:i + step, None], lon[i:i + step, None]
                straddles = (a_lat[None, :] <= la) & (la < b_lat[None, :])
                crossed = straddles & (w[None, :] * (la - a_lat[None, :]) > (lo - a_lon[None, :]) * h[None, :])
                inside[i:i + step] = (np.count_nonzero(crossed, axis=1) & 1) == 1
        first[inside & (first < 0)] = z
        hits += inside.astype(np.uint32)
    return first, hits


def zone_totals_of(zones, lat, lon, keep=None, count=None, n_speed=None, sum_speed=None, ts_us=None):
    """(inside: zones x points bool) and the ZONE_REC_DTYPE totals of candidate points by points_in_zones, one zone at a
    time: ts_us given -- positions (n = count = the members, newest_us their newest); else tiles (the members' sums)."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    keep = np.ones(lat.size, bool) if keep is None else np.asarray(keep, bool)
    tot = np.zeros(zones.n_zones, _lib.ZONE_REC_DTYPE)
    inside = np.zeros((zones.n_zones, lat.size), bool)
    for z in range(zones.n_zones):
        one = _lib.Zones.from_rings([[list(zip(la, lo)) for la, lo in zones.rings(z)]])
        inside[z] = (points_in_zones(one, lat, lon)[1] == 1) & keep
        m = inside[z]
        tot["n"][z] = int(m.sum())
        if ts_us is not None:
            tot["count"][z] = tot["n"][z]
            tot["newest_us"][z] = int(np.asarray(ts_us)[m].max()) if m.any() else _lib.INT64_MIN
        else:
            tot["count"][z] = int(np.asarray(count)[m].sum())
            tot["n_speed"][z] = int(np.asarray(n_speed)[m].sum())
            tot["sum_speed"][z] = float(np.asarray(sum_speed, np.float64)[m].sum())
    return inside, tot


def positions_within_from_engine(engine, zones, tz=None):
    """The FeatureCollection a /api/positions/within route returns: positions_latest_from_engine's features whose point is
    in at least one zone, filtered here in Python (points_in_zones).  The comparison form of positions_within_body."""
    f = positions_latest_from_engine(engine, tz)["features"]
    _, hits = points_in_zones(zones, [x["geometry"]["coordinates"][1] for x in f], [x["geometry"]["coordinates"][0] for x in f])
    return {"type": "FeatureCollection", "features": [x for x, k in zip(f, hits) if k]}


def tiles_within_from_engine(engine, zones, res=None, city="boston", tz=None):
    """The FeatureCollection a /api/tiles/within route returns: tiles_latest_from_engine's features of the newest live
    window at resolution res whose tile document's centroid is in at least one zone, filtered here in Python.  The
    comparison form of tiles_within_body."""
    docs = tile_docs_from_engine(engine, res, city, tz)
    f = tiles_latest_collection(docs, engine.device)["features"]
    _, hits = points_in_zones(zones, [d["centroid"]["coordinates"][1] for d in docs], [d["centroid"]["coordinates"][0] for d in docs])
    return {"type": "FeatureCollection", "features": [x for x, k in zip(f, hits) if k]}


def positions_within_body(engine, zones, tz=None):
    """The response body of a /api/positions/within route as bytes: json.dumps(positions_within_from_engine(...),
    separators=(",", ":")), feature order apart, filtered and encoded on the GPU (HeatmapEngine.positions_within_geojson)."""
    return engine.positions_within_geojson(zones, tz)


def tiles_within_body(engine, zones, res=None, tz=None):
    """The response body of a /api/tiles/within route as bytes: json.dumps(tiles_within_from_engine(...), separators=(",",
    ":")), feature order apart, rolled up, filtered and encoded on the GPU (HeatmapEngine.window_within_geojson)."""
    return engine.window_within_geojson(zones, None, res, tz)
