"""Shared by the span tests (tests/test_span_host.py, tests/test_gpu_span.py): span(end, windows, res) of
include/mobheat.h's hm_span_* restated with a plain dict loop on Python ints and floats -- on purpose none of the
library's code -- and the event batches the host execution and the device are held to.

The span.  The `windows` consecutive windows ending with the one that starts at `end`; one record per parent cell at
res that any of them holds, count / n_speed / the three sums added up, window_start_us = the first window's start, and
a series row: the parent's count in each window, 0 where the window or the cell is absent.

Everything is dyadic, as in tests/change_cases.py whose lattice and points these batches use: coordinates on a
1/1024-degree lattice, one point per res-8 cell, half-integer speeds, 1..3 events per cell and window -- every fp64 sum
is exact in any order of addition and "equal" means bit-equal.  Window j is [T0 + 5j min, T0 + 5(j + 1) min)."""
import functools
import json

import numpy as np

import change_cases as cc

T0, MINUTE, H3_RES, TOP_MAX = cc.T0, cc.MINUTE, cc.H3_RES, cc.TOP_MAX
TILE = 5 * MINUTE
MAX_WINDOWS = 16
DELAY_MS = 4 * 3600 * 1000        # the engines' watermark delay: every window of a batch stays live
EMPTY = cc.EMPTY
VIEW = cc.VIEW
REL, ABS_DEG = cc.REL, cc.ABS_DEG
ks_of = cc.ks_of


def wstart(j):
    return T0 + j * TILE


# ---- the reference ----
def parent(cell, res):
    """cellToParent on a Python int: resolution field = res, digits past res = 7"""
    cell = int(cell)
    return (cell & ~(0xF << 52)) | (res << 52) | ((1 << (3 * (15 - res))) - 1)


def ref_span(per_window, first_us, res):
    """(records sorted by cell, series) by a dict loop over the per-window record arrays"""
    from mobheat._lib import STATE_REC_DTYPE
    acc, w = {}, len(per_window)
    for j, recs in enumerate(per_window):
        for r in recs:
            a = acc.setdefault(parent(r["cell"], res), [0, 0, 0.0, 0.0, 0.0, [0] * w])
            a[0] += int(r["count"])
            a[1] += int(r["n_speed"])
            a[2] += float(r["sum_speed"])
            a[3] += float(r["sum_lat"])
            a[4] += float(r["sum_lon"])
            a[5][j] += int(r["count"])
    cells = sorted(acc)
    out = np.zeros(len(cells), STATE_REC_DTYPE)
    series = np.zeros((len(cells), w), np.int64)
    for i, c in enumerate(cells):
        a = acc[c]
        out[i] = (c, first_us, a[0], a[1], a[2], a[3], a[4], 0)
        series[i] = a[5]
    return out, series


def by_cell(recs, series):
    o = np.argsort(recs["cell"], kind="stable")
    return recs[o], series[o]


def same(got, want, what=""):
    """(records, series) against (records, series): whole, bit for bit, in order"""
    (gr, gs), (wr, ws) = got, want
    assert gr.size == wr.size and gs.shape == ws.shape, f"{what}: {gr.size} records {gs.shape}, {wr.size} {ws.shape} expected"
    if gr.tobytes() != wr.tobytes():
        bad = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(gr, wr)])
        raise AssertionError(f"{what}: {bad.size} of {gr.size} records differ, first at {bad[0]}: {gr[bad[0]]} != {wr[bad[0]]}")
    np.testing.assert_array_equal(gs, ws, err_msg=f"{what}: series")
    np.testing.assert_array_equal(gs.sum(axis=1), gr["count"], err_msg=f"{what}: a row does not add up to its count")


# ---- event batches ----
def batch_of(lat, lon, windows, seed, sizes=None, dyadic=True):
    """One batch of events over the points' distinct res-8 cells (one point per cell): every cell in a random non-empty
    subset of the window indices `windows`, 1..3 events per cell and window; sizes {j: n}: exactly n cells in window j,
    drawn on their own.  Returns (batch, {j: the sorted cells of window j})."""
    from mobheat import _lib
    rng = np.random.default_rng(seed)
    cell = _lib.latlng_to_cell_host_selftest(lat, lon, H3_RES)
    ucell, first = np.unique(cell, return_index=True)
    first = first[ucell != 0]
    p = rng.permutation(first.size)
    lat, lon, cell = lat[first][p], lon[first][p], cell[first][p]
    n, w = cell.size, len(windows)
    member = rng.integers(1, 1 << w, n)   # a non-empty subset as bits
    rows, ts, cells_of = [], [], {}
    for b, j in enumerate(windows):
        on = np.flatnonzero((member >> b) & 1)
        if sizes and j in sizes:
            assert n >= sizes[j], f"{n} cells, {sizes[j]} wanted"
            on = rng.permutation(n)[: sizes[j]]
        cells_of[j] = np.sort(cell[on])
        r = np.repeat(on, rng.integers(1, 4, on.size))
        rows.append(r)
        ts.append(np.full(r.size, wstart(j)) + rng.integers(0, 300, r.size) * 1_000_000)
    rows, ts = np.concatenate(rows), np.concatenate(ts)
    m = rows.size
    speed = rng.integers(0, 160, m) * 0.5 if dyadic else rng.uniform(0.0, 90.0, m)
    la, lo = lat[rows], lon[rows]
    if not dyadic:   # off the lattice: the test compares with the engine's own per-window records
        la, lo = la + rng.uniform(-1e-4, 1e-4, m), lo + rng.uniform(-1e-4, 1e-4, m)
    o = rng.permutation(m)
    b = dict(lat=la[o], lon=lo[o], ts_us=ts[o], speed=speed[o], speed_valid=(rng.random(m) >= 0.2)[o],
             vkey=rng.integers(0, 5000, m).astype(np.uint64), row_valid=np.ones(m, bool))
    return b, cells_of


@functools.lru_cache(maxsize=None)
def membership_batch():
    """about 4,500 cells in the box and over the sphere -- more parents at res 8 than an LDS table takes (1024) -- each in
    a random non-empty subset of windows 0, 1, 2"""
    la, lo = cc.box_points(5201, 4300)
    return batch_of(la, lo, (0, 1, 2), 5202)


@functools.lru_cache(maxsize=None)
def pentagon_batch():
    rng = np.random.default_rng(5301)
    la, lo = cc.pentagon_points(rng, 3000)
    return batch_of(la, lo, (0, 1, 2), 5302)


SPARSE = (3, 5, 18)   # the sparse batch's live windows: 4 is a gap; 3..18 are 16 windows with three live


@functools.lru_cache(maxsize=None)
def sparse_batch():
    rng = np.random.default_rng(5401)
    la, lo = cc.lattice(rng, 2500, cc.BOX)
    return batch_of(la, lo, SPARSE, 5402)


@functools.lru_cache(maxsize=None)
def unequal_batch():
    """window 0 with about 4,000 keys, window 1 with 3 (its table is smaller than one tile of the scan), window 2 with none"""
    rng = np.random.default_rng(5501)
    la, lo = cc.lattice(rng, 5200, cc.BOX)
    b, cells_of = batch_of(la, lo, (0, 1), 5502, sizes={0: 4000, 1: 3})
    assert cells_of[0].size == 4000 and cells_of[1].size == 3
    return b, cells_of


@functools.lru_cache(maxsize=None)
def random_batch():
    rng = np.random.default_rng(5601)
    la, lo = cc.lattice(rng, 4000, cc.BOX)
    return batch_of(la, lo, (0, 1, 2), 5602, dyadic=False)


# ---- record sets (host tests: no engine) ----
@functools.lru_cache(maxsize=None)
def record_cases():
    """(name, per-window record arrays at res 8, first window's start): dyadic records over shared and disjoint cells"""
    import top_cases as tc
    rng = np.random.default_rng(5701)
    cells = rng.permutation(tc.cells_of(900))

    def recs(sel, j, salt):
        return cc._records(cells[sel], rng.integers(1, 5, len(sel)), wstart(j), salt)
    i = np.arange(900)
    none = i[:0]
    return [("one window", [recs(i[:300], 0, 0)], wstart(0)),
            ("three overlapping", [recs(rng.permutation(i[:600]), 0, 0), recs(i[300:900], 1, 5), recs(i[100:400], 2, 9)], wstart(0)),
            ("a gap", [recs(i[:200], 4, 0), recs(none, 5, 0), recs(i[100:500], 6, 3)], wstart(4)),
            ("disjoint", [recs(i[:300], 0, 0), recs(i[300:700], 1, 5)], wstart(0)),
            ("all empty", [recs(none, 0, 0), recs(none, 1, 0)], wstart(0)),
            ("sixteen", [recs(rng.permutation(i)[: 50 * (j % 3)], j, j) for j in range(16)], wstart(0))]


# ---- GeoJSON ----
dumps = cc.dumps
Text = cc.Text
WS_TEXT, WE_TEXT = "2025-10-04T10:00:00", "2025-10-04T10:15:00"


def host_collection(recs, series, ws_text=WS_TEXT, we_text=WE_TEXT):
    """readside.tiles_span_collection of the records, its rings from the host execution of cellToBoundary (no GPU)"""
    from mobheat import _lib, readside
    saved = readside.cells_to_boundary
    readside.cells_to_boundary = lambda cells, device=0: _lib.cells_to_boundary_host_selftest(cells)
    try:
        return readside.tiles_span_collection(recs, series, Text(ws_text), Text(we_text))
    finally:
        readside.cells_to_boundary = saved


def check_body(body, offs, collection):
    cc.check_body(body, offs, collection)
    assert json.loads(bytes(body)) == collection
