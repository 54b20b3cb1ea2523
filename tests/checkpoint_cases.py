"""Tile-state checkpoint cases: the states, batches and record sets that put hm_state_export / _export_touched /
_export_begin + _copy* / hm_state_import (csrc/api_state.h), k_dump_gen and the rehash merge under them ON their size,
order and restore edges (no GPU code is imported here; tests/test_checkpoint_cases_host.py checks the cases against the
oracle alone, tests/test_gpu_checkpoint_edges.py runs them on the device).

The constants the cases sit on (csrc/host_ctx.h gen_geometry / gens_prepare, csrc/dev_table.h, csrc/k_merge.h):

    MIN_SLOTS = 1024      the smallest window table
    DUMP_TILE = 2048      slots one k_dump_gen workgroup iteration scans (256 threads x DUMP_PER = 8)
    load 1/2              a window's table has next_pow2(2 * c) slots for a census of c records, and is regrown by a
                          batch bringing c records to its k keys when 2 * (k + c) > slots -- the census counts RECORDS,
                          so every batch here brings one row per key where a table size is claimed (`slots_for`,
                          `regrows`: the host-side restatement of those two lines)
    MAX_WINDOWS = 2048    GMAP_SLOTS / 2, the windows one context holds
    MERGE_CHUNK = 512     records of one k_merge_owned chunk (MO_THREADS): two records of one key inside a chunk meet in
                          its LDS claim set, two records 600 apart meet in the table

The reference is oracle/spark_oracle.py's SparkHeatmapOracle fed the same batches (`Reference`): the full state is
`ora.state`, the watermarks `ora.wm_cur` / `ora.wm_prev`, and the delta of a batch the keys of the tiles its result
emits whose window outlives the batch's eviction watermark (`ora.wm_prev` after the batch), each with its cumulative
values from `ora.state`.  Every comparison is bytes: points on multiples of 2^-20 degrees, speeds on multiples of 0.25
and a handful of rows per key make every fp64 sum exact in any order (`key_sums` adds them in two orders).
"""
import dataclasses

import numpy as np

T0 = 1_759_572_000_000_000   # 2025-10-04 10:00:00 UTC, a 5-minute window start
MINUTE = 60_000_000
TILE = 5 * MINUTE
DELAY_MS = 600_000
RES = 9
Q = 2.0 ** -20

MIN_SLOTS = 1024
DUMP_TILE = 2048
MAX_WINDOWS = 2048
MERGE_CHUNK = 512

# hm_state_rec (include/mobheat.h); the GPU tests assert that it is mobheat._lib.STATE_REC_DTYPE
REC_DTYPE = np.dtype([("cell", "<u8"), ("window_start_us", "<i8"), ("count", "<i8"), ("n_speed", "<i8"),
                      ("sum_speed", "<f8"), ("sum_lat", "<f8"), ("sum_lon", "<f8"), ("reserved", "<i8")])


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def slots_for(records):
    """gen_geometry's ordinary table for a census of `records` (fewer than 16k of them): load <= 1/2, >= MIN_SLOTS"""
    return max(MIN_SLOTS, next_pow2(2 * records))


def regrows(keys, records, slots):
    """gens_prepare's `full`: a table of `slots` holding `keys` keys is replaced by a batch bringing `records` records"""
    return 2 * (keys + records) > slots


def dyadic(x):
    return np.round(np.asarray(x, np.float64) / Q) * Q


def points(idx):
    """point `i` of the key grid: 0.01-degree steps (64 per row of the grid), rounded to multiples of 2^-20 degrees;
    ~0.9 km apart, so every point has a res-9 cell of its own (the host file counts them)"""
    idx = np.asarray(idx, np.int64)
    return dyadic(37.50 + (idx // 64) * 0.01), dyadic(23.00 + (idx % 64) * 0.01)


def rows(*groups, seed=1):
    """One batch.  A group is (point indices, window index, rows per point[, offset_us]): `rows per point` rows at each
    point (on it exactly: a tenth of a metre aside already leaves the cell at some points of the grid), with speeds and
    null speeds of their own, in window T0 + window index x TILE, within its first four minutes (or all at offset_us);
    a fixed permutation interleaves the groups."""
    lat, lon, ts, sp, sv, vk = [], [], [], [], [], []
    for g in groups:
        idx, w, reps = np.asarray(g[0], np.int64), int(g[1]), int(g[2])
        off = g[3] if len(g) > 3 else None
        la, lo = points(idx)
        for rep in range(reps):
            lat.append(la)
            lon.append(lo)
            o = (7 + 13 * idx + 101 * rep + 1009 * w) % (4 * MINUTE) if off is None else np.full(idx.size, off, np.int64)
            ts.append(T0 + w * TILE + o)
            sp.append(0.25 * ((3 * idx + 7 * rep + w) % 360))
            sv.append((idx + rep) % 5 != 0)
            vk.append(idx % 50)
    if not lat:
        z = np.zeros(0)
        return dict(lat=z, lon=z.copy(), ts_us=np.zeros(0, np.int64), speed=z.copy(), speed_valid=np.zeros(0, bool),
                    vkey=np.zeros(0, np.uint64), row_valid=np.zeros(0, bool))
    cat = [np.concatenate(a) for a in (lat, lon, ts, sp, sv, vk)]
    p = np.random.default_rng(seed).permutation(cat[0].size)
    return dict(lat=cat[0][p], lon=cat[1][p], ts_us=cat[2][p].astype(np.int64), speed=cat[3][p],
                speed_valid=cat[4][p].astype(bool), vkey=cat[5][p].astype(np.uint64), row_valid=np.ones(p.size, bool))


def permuted(batch, seed=99):
    """the same rows in another fixed order"""
    p = np.random.default_rng(seed).permutation(batch["lat"].size)
    return {k: v[p] for k, v in batch.items()}


def key_sums(batch, cells):
    """{(cell, window start): (count, n_speed, sum_speed, sum_lat, sum_lon)} of a batch's rows, added row after row in
    the order given (np.add.at: unbuffered, sequential)"""
    ws = batch["ts_us"] - np.mod(batch["ts_us"], TILE)
    keys = np.rec.fromarrays([cells, ws], names="c,w")
    uniq, inv = np.unique(keys, return_inverse=True)
    inv = inv.ravel()
    cnt, nsp = np.zeros(uniq.size, np.int64), np.zeros(uniq.size, np.int64)
    ssp, sla, slo = np.zeros(uniq.size), np.zeros(uniq.size), np.zeros(uniq.size)
    np.add.at(cnt, inv, 1)
    np.add.at(nsp, inv, batch["speed_valid"].astype(np.int64))
    np.add.at(ssp, inv, np.where(batch["speed_valid"], batch["speed"], 0.0))
    np.add.at(sla, inv, batch["lat"])
    np.add.at(slo, inv, batch["lon"])
    return {(int(uniq["c"][u]), int(uniq["w"][u])): (int(cnt[u]), int(nsp[u]), ssp[u].tobytes(), sla[u].tobytes(),
                                                      slo[u].tobytes()) for u in range(uniq.size)}


def keyed(recs):
    """records in key order: what two exports are compared as (`.tobytes()`)"""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    return recs[np.lexsort((recs["window_start_us"], recs["cell"]))]


class Reference:
    """SparkHeatmapOracle driven batch by batch, with the checkpoint's view of it"""

    def __init__(self):
        from oracle.spark_oracle import SparkHeatmapOracle
        self.ora = SparkHeatmapOracle(h3_res=RES)
        self.epoch = -1
        self.touched = []   # the last batch's emitted keys

    def batch(self, b, epoch=None):
        exp = self.ora.process_batch(**b)
        self.epoch = self.epoch + 1 if epoch is None else epoch
        self.touched = [(t["cell"], t["window_start_us"]) for t in exp["tiles"]]
        return exp

    def info(self):
        return dict(epoch_id=self.epoch, n_keys=len(self.ora.state), watermark_ms=self.ora.wm_cur,
                    prev_watermark_ms=self.ora.wm_prev, tile_us=TILE, watermark_delay_ms=DELAY_MS, h3_res=RES)

    def records(self, keys):
        r = np.zeros(len(keys), REC_DTYPE)
        for i, k in enumerate(keys):
            c, nsp, ssp, sla, slo = self.ora.state[k]
            r[i] = (k[0], k[1], c, nsp, ssp, sla, slo, 0)
        return keyed(r)

    def full(self):
        return self.records(list(self.ora.state))

    def delta_keys(self):
        """the last batch's emitted keys whose window outlives its eviction watermark (wm_prev, now)"""
        return [k for k in self.touched if k[1] + TILE > self.ora.wm_prev * 1000]

    def delta(self):
        return self.records(self.delta_keys())

    def windows(self):
        """{window start: live keys}"""
        out = {}
        for _, w in self.ora.state:
            out[w] = out.get(w, 0) + 1
        return out


# ---------------------------------------------------------------------------------------------------------
# 1. dump sizes: one window of n keys (one row each: the census is n), alone and beside a second window
# ---------------------------------------------------------------------------------------------------------
SIZES = (1, 511, 512, 513, 1024, 1025, 2049)
# below one dump tile (and the smallest table), the same at load 1/2 less one and at load 1/2 exactly, one dump tile,
# the same at load 1/2, two tiles, four
SIZE_SLOTS = {1: 1024, 511: 1024, 512: 1024, 513: 2048, 1024: 2048, 1025: 4096, 2049: 8192}


def second_window_keys(n):
    """the second window of the two-window sweep: never n keys, never an edge of its own"""
    return n // 3 + 2


@dataclasses.dataclass
class SizedCase:
    n: int
    two: bool
    batch: dict
    windows: dict   # window start -> intended keys


def sized_case(n, two):
    """window 1 holds the n keys of the edge; `two`: window 0 holds second_window_keys(n) keys of two rows each, so
    that the dump's records of the edge window start at an offset that is a multiple of nothing"""
    groups = [(np.arange(n), 1, 1)]
    windows = {T0 + TILE: n}
    if two:
        m = second_window_keys(n)
        groups.append((np.arange(m), 0, 2))
        windows[T0] = m
    return SizedCase(n, two, rows(*groups, seed=100 + n), windows)


# ---------------------------------------------------------------------------------------------------------
# 2. delta shapes
# ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class DeltaCase:
    name: str
    batches: list
    shape: str                   # of the LAST batch's delta: "empty", "every", "subset" (strict, non-empty), or
                                 # "subset_regrown" (a subset, with an untouched key in a window the batch regrew)
    n_delta: int                 # its records
    start: str = "fresh"         # "import": the first batch's state is imported into the engine under test instead
    regrown: tuple = ()          # window indices the last batch regrows
    evicted_touched: tuple = ()  # window indices the last batch touches and its watermark evicts


_BUILD = ((np.arange(40), 0, 2), (np.arange(30), 1, 1))

DELTA_CASES = [
    DeltaCase("fresh", [], "empty", 0),
    DeltaCase("after_import", [rows(*_BUILD)], "empty", 0, start="import"),
    DeltaCase("empty_batch", [rows(*_BUILD), rows()], "empty", 0),
    DeltaCase("every_key", [rows(*_BUILD), rows((np.arange(40), 0, 1), (np.arange(30), 1, 3), seed=2)], "every", 70),
    # 513 keys: a 2048-slot table, one dump tile; one key touched, 2 * (513 + 1) <= 2048: no regrow
    DeltaCase("one_of_513", [rows((np.arange(513), 1, 1)), rows(([200], 1, 1))], "subset", 1),
    # 512 keys fill a 1024-slot table to load 1/2; 10 new keys and 5 old ones regrow it: all 522 keys go through
    # k_dump_gen and the rehash merge, 15 are in the delta
    DeltaCase("regrow_15", [rows((np.arange(512), 1, 1)),
                            rows((np.r_[np.arange(512, 522), [3, 100, 255, 256, 511]], 1, 1), seed=3)],
              "subset_regrown", 15, regrown=(1,)),
    # batch 0's rows in window 4 put the watermark past window 0's end; batch 1 touches window 0 (not late: the late
    # rule uses the watermark before that) and window 4: window 0 is emitted, then evicted
    DeltaCase("evict_touched", [rows((np.arange(30), 0, 2), (np.arange(20), 4, 1)),
                                rows((np.arange(10, 40), 0, 1), (np.arange(5, 25), 4, 1), seed=4)],
              "subset", 20, evicted_touched=(0,)),
]
DELTA_IDS = [c.name for c in DELTA_CASES]

# the state the call orders and the slice edges run on: regrow_15's (522 keys, 15 in the delta)
ORDER_CASE = DELTA_CASES[DELTA_IDS.index("regrow_15")]


# ---------------------------------------------------------------------------------------------------------
# 3. import census: W windows of 3 keys, in three record orders
# ---------------------------------------------------------------------------------------------------------
CENSUS_WINDOWS = (1, 2, 7, MAX_WINDOWS)
CENSUS_ORDERS = ("grouped", "reversed", "interleaved")
CENSUS_KEYS = 3


def census_window_starts(W):
    """window 0 starts before 1970 (a negative multiple of TILE), the others follow T0"""
    return np.array([-3 * TILE] + [T0 + k * TILE for k in range(1, W)], np.int64)


def census_records(W, order="grouped"):
    """(info, records): W windows x CENSUS_KEYS cells, values dyadic; grouped = window after window, as an export's
    dump leaves them; reversed; interleaved = round-robin over the windows, the window changing on every record"""
    from oracle import h3_oracle
    la, lo = points(np.arange(CENSUS_KEYS))
    cells = h3_oracle.latlng_to_cell(la, lo, RES).astype(np.uint64)
    starts = census_window_starts(W)
    k, j = np.meshgrid(np.arange(W), np.arange(CENSUS_KEYS), indexing="ij")   # [window, key]: window-major
    if order == "interleaved":
        k, j = k.T, j.T
    k, j = k.ravel(), j.ravel()
    if order == "reversed":
        k, j = k[::-1], j[::-1]
    r = np.zeros(k.size, REC_DTYPE)
    r["cell"], r["window_start_us"] = cells[j], starts[k]
    r["count"] = 1 + (k + j) % 7
    r["n_speed"] = r["count"] - (j % 2)
    r["sum_speed"] = np.where(r["n_speed"] > 0, 0.25 * (k % 97 + j), 0.0)   # (no export has a sum over no speeds)
    r["sum_lat"], r["sum_lon"] = la[j] * r["count"], lo[j] * r["count"]
    info = dict(epoch_id=5, n_keys=int(r.size), watermark_ms=0, prev_watermark_ms=0, tile_us=TILE,
                watermark_delay_ms=DELAY_MS, h3_res=RES)
    return info, r


# ---------------------------------------------------------------------------------------------------------
# 4. restore, then continue
# ---------------------------------------------------------------------------------------------------------
# Engine A: batch 0 fills window 1 with 512 keys (1024 slots at load 1/2; an import sizes its table for 512 too) and
# window 0 with 40; batch 1 opens window 3, whose last row (T0 + 19 min) puts the watermark at T0 + 9 min -- past
# window 0's end, short of window 1's -- and re-touches window 0.
# Engine B's batch re-touches 30 keys of window 1 and adds 20 (regrow: 2 * (512 + 50) > 1024), re-touches window 0 (the
# restored watermark evicts it after the batch has emitted it) and window 3, and opens window 6, which moves the
# watermark on for the batch after.
RESTORE_BEFORE = [rows((np.arange(512), 1, 1), (np.arange(40), 0, 2), seed=5),
                  rows((np.arange(60), 3, 1), ([0], 3, 1, 4 * MINUTE), (np.arange(20), 0, 1), seed=6)]
RESTORE_AFTER = rows((np.arange(100, 130), 1, 1), (np.arange(512, 532), 1, 1), (np.arange(5, 15), 0, 1),
                     (np.arange(10, 25), 3, 1), (np.arange(25), 6, 1), seed=7)
RESTORE_GROWN, RESTORE_EVICTED, RESTORE_OPENED = 1, 0, 6   # window indices


# ---------------------------------------------------------------------------------------------------------
# 5. records an import refuses
# ---------------------------------------------------------------------------------------------------------
def refused_sets():
    """(good, {name: bad}): the good set is 1300 keys of one window (three merge chunks); each bad set is the good one
    with one record changed"""
    ref = Reference()
    ref.batch(rows((np.arange(1300), 1, 1), seed=8))
    info, good = ref.info(), ref.full()
    rng = np.random.default_rng(8)
    good = good[rng.permutation(good.size)]   # (no order the device could lean on)
    bad = {}
    b = good.copy()
    b[11] = b[10]                      # the two copies side by side: one chunk's claim set
    bad["repeat_adjacent"] = b
    b = good.copy()
    b[10 + 600] = b[10]                # 600 records apart: more than one MERGE_CHUNK
    bad["repeat_600_apart"] = b
    b = good.copy()
    b["cell"][20] = (b["cell"][20] & ~np.uint64(0xF << 52)) | np.uint64((RES - 1) << 52)   # the resolution bits of res 8
    bad["other_resolution"] = b
    b = good.copy()
    b["cell"][30] = (b["cell"][30] & ~np.uint64(0xF << 59)) | np.uint64(2 << 59)           # mode 2: a directed edge
    bad["other_mode"] = b
    return info, good, bad


REFUSED = ("repeat_adjacent", "repeat_600_apart", "other_resolution", "other_mode")


# ---------------------------------------------------------------------------------------------------------
# 6. queued export copies against the next batch
# ---------------------------------------------------------------------------------------------------------
# 512 keys in window 1 (1024 slots) and 1024 in window 2 (2048 slots), both at load 1/2: the export's dump is 1536
# records, copied in six slices of 256.  The batch adds 8 keys to either window: both regrow, and the regrow's
# k_dump_gen writes all 1536 keys over the dump the slices are queued from.  (It cannot outgrow the buffer: a regrow
# moves keys that were live when the dump was sized.)
QUEUED_BUILD = rows((np.arange(512), 1, 1), (np.arange(1024), 2, 1), seed=9)
QUEUED_BATCH = rows((np.arange(512, 520), 1, 1), (np.arange(1024, 1032), 2, 1), seed=10)
QUEUED_SLICE = 256
