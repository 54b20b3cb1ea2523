"""Shared by tests/test_gpu_read_grid.py: the sizes at which the read side's and the sink's streaming kernels take a second
grid-stride iteration under MOBHEAT_TEST_READ_GRID, the one state every call of that file reads, and which kernels a call
launches -- so that a launch site that ignores the knob fails its test instead of passing it on one iteration.

Everything is dyadic (coordinates on the 1/4096-degree lattice, speeds on 1/64): every fp64 sum is exact in any order, so
two engines with the same contents give the same records whatever their grids, and records and bodies compare byte for byte.
Nothing here has a tolerance."""
import functools

import numpy as np

import density_cases as dc

# csrc/dev_table.h's, csrc/k_rollup.h's, csrc/k_geojson.h's, csrc/bson_docs.h's and csrc/api_raster.h's constants, which the
# library does not export: a change there must be made here
DUMP_PER = 8
SCAN = 256 * DUMP_PER         # slots / records per workgroup iteration of the scans and compactions
GROUP = 1024 * DUMP_PER       # slots per iteration of k_rollup / k_density_group (RU_THREADS x DUMP_PER)
RU_FILL = 1024                # the keys a group-by workgroup's LDS table takes before it spills (RU_SLOTS / 2)
GJ_THREADS = 64               # k_gj_tile_write's features per iteration
TD_THREADS = 128              # k_tile_docs' statements per iteration
RASTER_UNITS = 4              # k_raster's units (a wave each) per iteration
GRIDS = (1, 3)                # 1: one workgroup runs every iteration; 3: the workgroups' iteration counts differ


def iterating(per_iteration):
    """the smallest size the issue asks for: every one of 3 workgroups iterates at least twice, the last tile is partial"""
    return 2 * 3 * per_iteration - 5


# per call of the engine: EVERY launch it makes through read_grid, as (kernel, items per workgroup iteration, size key) -- the
# tests assert that exactly those whose items are more than `grid` iterations ran on a lowered grid, so a site that ignores
# the knob fails its test, and so does a launch that is missing here.  A key "x+1" is size x plus one (a scan over the
# features and the prefix).
def _tiles_body(key):
    return [("k_gj_tile_sizes", 256, key), ("k_scan_add", 256, key + "+1"), ("k_gj_tile_write", GJ_THREADS, key)]


def _positions_body(key):
    return [("k_gj_pos_sizes", 256, key), ("k_scan_add", 256, key + "+1"), ("k_gj_pos_write", 256, key)]


ROLLUP = [("k_rollup", GROUP, "wslots"), ("k_rollup_emit", SCAN, "pslots")]
DENSITY = [("k_density_cells", 256, "cap"), ("k_density_group", GROUP, "cap"), ("k_density_emit", SCAN, "dslots")]
# engine.positions_buckets: hm_positions_buckets twice (the count, then the ids); the bodies of the positions call it first
BUCKETS = 2 * [("k_fill_i64", 256, "bslots"), ("k_gj_pos_buckets", 256, "cap")]
LAUNCHES = {
    "positions_within": [("k_pos_within", SCAN, "cap")],
    "window_within": ROLLUP + [("k_within_tiles", SCAN, "g")],
    "positions_within_geojson": BUCKETS + [("k_pos_within", SCAN, "cap")] + _positions_body("kept"),
    "window_within_geojson": ROLLUP + [("k_within_tiles", SCAN, "g")] + _tiles_body("kept"),
    "positions_density": DENSITY,
    "positions_density_view": DENSITY + [("k_view_tiles", SCAN, "groups")],
    "positions_density_raster": DENSITY + [("k_raster", RASTER_UNITS, "units")],
    "window_raster": ROLLUP + [("k_raster", RASTER_UNITS, "units")],
    "window_records": ROLLUP,
    "window_geojson": ROLLUP + _tiles_body("g"),
    "window_geojson_view": ROLLUP + [("k_view_tiles", SCAN, "g")] + _tiles_body("kept"),
    "encode_tile_features": _tiles_body("n"),
    "positions_buckets": BUCKETS,
    "positions_geojson": BUCKETS + [("k_pos_emit", SCAN, "cap")] + _positions_body("kept"),
    "positions_geojson_view": BUCKETS + [("k_pos_emit_view", SCAN, "cap")] + _positions_body("kept"),
    "positions": [("k_pos_emit", SCAN, "cap")],
    "export_state": [("k_dump_gen", SCAN, "wslots")],         # (one live window; the sizing call dumps nothing)
    "export_state_delta": [("k_dump_gen", SCAN, "wslots")],   # (the sizing call dumps, the fetching call reuses it)
    "tile_updates": [("k_tile_doc_sizes", 256, "n"), ("k_scan_add", 256, "n"), ("k_tile_docs", TD_THREADS, "n")],
    "tile_updates_direct": [("k_tile_doc_sizes", 256, "n"), ("k_scan_add", 256, "n"), ("k_tile_docs_direct", 256, "n")],
    "position_updates": [("k_pos_doc_sizes", 256, "n"), ("k_scan_add", 256, "n"), ("k_pos_docs", 256, "n")],
}


def _size(sizes, key):
    return int(sizes[key[:-2]]) + 1 if key.endswith("+1") else int(sizes[key])


def lowered(call, grid, **sizes):
    """the kernels of `call` whose grid MOBHEAT_TEST_READ_GRID=grid lowers (one entry per launch), given the items each
    runs over: those with more than `grid` workgroup iterations of items"""
    return [k for k, per, key in LAUNCHES[call] if _size(sizes, key) > 0 and -(-_size(sizes, key) // per) > grid]


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


T0 = dc.T0
WIDE_BOX = (25.0, 49.0, -125.0, -67.0)   # the contiguous United States, roughly: ~12,000 points in as many res-8 cells
N_BOSTON, N_WIDE = 4000, 12000
PROVIDERS = ("p", 'q"\\')


@functools.lru_cache(maxsize=None)
def world():
    """one micro-batch of N_BOSTON + N_WIDE rows, a vehicle each, in one window: N_BOSTON on the 1/4096-degree lattice of
    C1's box (where the zone sets lie: several rows per res-8 cell), N_WIDE over WIDE_BOX (a cell each, nearly), shuffled.
    Every third vehicle of provider 1 has a name that needs escaping.  Returns a positions_ref.Batch with speed /
    speed_valid columns."""
    from positions_ref import Batch
    rng = np.random.default_rng(20260)
    n = N_BOSTON + N_WIDE

    def lattice(lo, hi, m):
        return rng.integers(int(np.ceil(lo * 4096)), int(np.floor(hi * 4096)) + 1, m) / 4096.0
    B, W = dc.BOSTON_BOX, WIDE_BOX
    lat = np.r_[lattice(B[0], B[1], N_BOSTON), lattice(W[0], W[1], N_WIDE)]
    lon = np.r_[lattice(B[2], B[3], N_BOSTON), lattice(W[2], W[3], N_WIDE)]
    o = rng.permutation(n)
    lat, lon = lat[o], lon[o]
    ts = T0 + rng.integers(0, 200, n) * dc.SEC
    rows = [(PROVIDERS[k % 2], f"w\n{k}é\t" if k % 6 == 1 else f"v{k}", int(ts[k]), float(lat[k]), float(lon[k])) for k in range(n)]
    b = Batch(rows)
    b.speed = rng.integers(0, 4096, n) / 64.0
    b.speed_valid = rng.random(n) > 0.2
    return b


def load(eng):
    """the world as the engine's one window and its positions state"""
    b = world()
    res = eng.process_batch(0, b.lat, b.lon, b.ts, speed=b.speed, speed_valid=b.speed_valid, vkey=b.vkey,
                            row_valid=np.ones(len(b.rows), bool))
    eng.update_positions(b.providers, b.vehicles)
    return res


def batch_columns():
    b = world()
    return dict(lat=b.lat, lon=b.lon, ts_us=b.ts, speed=b.speed, speed_valid=b.speed_valid, vkey=b.vkey,
                row_valid=np.ones(len(b.rows), bool))


def spaced_batch(n, seed=1):
    """n rows 1/16 degree apart (a res-8 cell is ~1 km across: a tile each), a vehicle each, one window: a batch whose sink
    statements number exactly n of either kind"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return dict(lat=30.0 + (k // side) / 16.0, lon=-100.0 + (k % side) / 16.0, ts_us=T0 + rng.integers(0, 200, n) * dc.SEC,
                speed=rng.integers(0, 4096, n) / 64.0, speed_valid=rng.random(n) > 0.2, vkey=k.astype(np.uint64),
                row_valid=np.ones(n, bool))
