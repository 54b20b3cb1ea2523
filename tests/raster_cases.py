"""Shared by the raster tests (tests/test_raster_host.py, tests/test_gpu_raster.py): the rule of include/mobheat.h's
hm_window_raster restated with the CPU oracle and a Python dict -- on purpose none of the library's code -- and the grid of
edge coordinates the host execution and the device are held to.  No tolerance anywhere: every expectation is an integer.

The rule.  Pixel (r, c) of the grid lat[rows] x lon[cols] has the cell latLngToCell(lat[r], lon[c], res), or none when a
coordinate is NaN or outside [-90, 90] / [-180, 180] (the reference UDF's range guard, heatmap_stream.py:66-69).  Its count
is the sum of the counts of the records of that cell (0: no cell, no record); `counts` is that saturated at 2^32 - 1,
`classes` the number of thresholds the unsaturated count exceeds (strictly)."""
import numpy as np

PENTAGON_BASE_CELLS = [4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117]
# the counts on and around every threshold of readside.COUNT_THRESHOLDS and the uint32 saturation
EDGE_COUNTS = [1, 2, 3, 5, 6, 10, 11, 20, 21, 50, 51, 2 ** 32 - 1, 2 ** 32, 2 ** 40]


def pixel_cells(res, lat, lon):
    """the oracle's cell of every pixel, uint64[rows * cols], 0 where the range guard leaves none"""
    from oracle import h3_oracle
    la, lo = np.meshgrid(np.asarray(lat, np.float64), np.asarray(lon, np.float64), indexing="ij")
    la, lo = la.ravel(), lo.ravel()
    with np.errstate(invalid="ignore"):
        ok = (np.abs(la) <= 90.0) & (np.abs(lo) <= 180.0)   # (False on a NaN)
    cells = np.zeros(la.size, np.uint64)
    if ok.any():
        cells[ok] = h3_oracle.latlng_to_cell(la[ok], lo[ok], res)
    return cells


def expected(recs, res, lat, lon, thresholds):
    """(counts uint32[rows, cols], classes uint8[rows, cols]) by the rule; thresholds may be empty (classes all 0)"""
    by = {}
    for c, k in zip(recs["cell"].tolist(), recs["count"].tolist()):
        by[c] = by.get(c, 0) + k
    cells = pixel_cells(res, lat, lon)
    shape = (len(lat), len(lon))
    cnt = np.array([by.get(c, 0) if c else 0 for c in cells.tolist()], np.uint64)
    counts = np.minimum(cnt, np.uint64(0xFFFFFFFF)).astype(np.uint32)
    classes = (cnt[:, None] > np.asarray(thresholds, np.uint64).reshape(1, -1)).sum(1).astype(np.uint8)
    return counts.reshape(shape), classes.reshape(shape)


def records(cells, counts, window_start_us=0):
    """STATE_REC_DTYPE records of the given cells and counts (one non-null speed each, so that they import as state)"""
    from mobheat._lib import STATE_REC_DTYPE
    r = np.zeros(len(cells), STATE_REC_DTYPE)
    r["cell"], r["window_start_us"], r["count"], r["n_speed"] = cells, window_start_us, counts, 1
    return r


def face_centres():
    """(lat, lon) in degrees of the 20 icosahedron face centres: the centres of the res-0 cells whose home is a face's
    ijk origin (the oracle's derived baseCellData: face, i, j, k, ...)"""
    from oracle import h3_oracle
    bcd, _, _ = h3_oracle.tables()
    at_origin = [b for b in range(122) if not bcd[b, 1:4].any()]
    assert sorted(int(bcd[b, 0]) for b in at_origin) == list(range(20))
    cells = np.array([(1 << 59) | (b << 45) | ((1 << 45) - 1) for b in at_origin], np.uint64)
    return h3_oracle.cell_to_latlng(cells)


def pentagon_centres():
    from oracle import h3_oracle
    cells = np.array([(1 << 59) | (b << 45) | ((1 << 45) - 1) for b in PENTAGON_BASE_CELLS], np.uint64)
    return h3_oracle.cell_to_latlng(cells)


def edge_grid():
    """(lat, lon, n_faces): a grid whose pixel (k, k), k < 20, is face centre k -- the fast path hands a point that close
    to a face centre to the exact path (csrc/h3_device.h, the sqd test) -- followed by the poles, the antimeridian, both
    zeros, the 12 pentagon centres, synth.edge_points()'s coordinates (sub-normals, just-outside values, infinities), and
    last NaN and one finite out-of-range value per axis (lat 91, lon -181)."""
    from mobheat import synth
    fla, flo = face_centres()
    pla, plo = pentagon_centres()
    ela, elo = synth.edge_points()
    lat = np.r_[fla, 90.0, -90.0, 0.0, -0.0, pla, ela, np.nan, 91.0]
    lon = np.r_[flo, 180.0, -180.0, 0.0, -0.0, plo, elo, np.nan, -181.0]
    return lat, lon, 20


def tile_of(lat, lon, z):
    """the slippy-map tile (x, y) at zoom z that contains (lat, lon) -- the usual formula"""
    import math
    n = 2 ** z
    x = int((lon + 180.0) / 360.0 * n)
    y = int((1.0 - math.asinh(math.tan(math.radians(lat))) / math.pi) / 2.0 * n)
    return min(max(x, 0), n - 1), min(max(y, 0), n - 1)


def decode_png(png):
    """(classes uint8[h, w], palette [(r, g, b)], alpha bytes) of an 8-bit indexed, filter-0 PNG; every chunk's CRC checked"""
    import struct
    import zlib
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(png):
        n, tag = struct.unpack(">I4s", png[at: at + 8])
        data = png[at + 8: at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n: at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"] and chunks[-1][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 3, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[3][1]), np.uint8).reshape(h, w + 1)
    assert not rows[:, 0].any()   # filter 0 on every row
    plte = chunks[1][1]
    return rows[:, 1:].copy(), [tuple(plte[k: k + 3]) for k in range(0, len(plte), 3)], chunks[2][1]
