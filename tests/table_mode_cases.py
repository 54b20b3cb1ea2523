"""Table-mode aggregation (csrc/k_table.h: k_agg + k_bin_reduce) at its flush, spill and bucket edges: the batches of
every case and the preconditions that make a case mean what it claims (no GPU code is imported here;
tests/test_table_mode_cases_host.py checks the cases against the oracle's cells alone, tests/test_gpu_table_mode.py runs
them on the device).

A case is a sequence of key ids per row (-1: an invalid row, skipped by k_agg like any row without a key).  Key id k is
the (cell, window) pair (k // W, k % W) of a pool of distinct H3 cells and W 5-minute windows from T0, so distinct ids
are distinct keys.  The pool's cells come from a grid of dyadic points (multiples of 2^-10 degrees) and the speeds are
multiples of 2^-10 km/h below 128, so every fp64 sum of a key is exact in any order and the averages can be compared bit
for bit.  A fifth of the speeds is null, and every row of key id 0 has a null speed.

With MOBHEAT_TEST_AGG_GRID=1 one k_agg workgroup streams all rows in order, 1024 (AG_THREADS) per round, so `simulate`
can follow its table from the key ids alone: the fresh keys per round, the flush when more than AG_FLUSH_AT keys were
inserted, the count classes the keep threshold reads and what it keeps -- as long as no insert fails its 64 probes,
which the device's hash decides and the tests observe (agg_spill_probe).
"""
import numpy as np

T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
TILE = 5 * MINUTE

# csrc/k_table.h
AG_THREADS = 1024
AG_SLOTS = 3833
AG_FLUSH_AT = AG_SLOTS - 640
AG_KEEP_MAX = AG_SLOTS // 8
AG_BINS = 256

CAP_SWEEP = (1, 2, 8, 16, 24, 32, 64, 4096)
_POOLS = {}
_CASES = {}


class Pool:
    """distinct cells of one resolution, each with the dyadic grid points that fall into it"""

    def __init__(self, res, side, lat0, lon0):
        from oracle import h3_oracle
        i, j = np.divmod(np.arange(side * side), side)
        lat, lon = lat0 + i / 1024.0, lon0 + j / 1024.0
        cells = h3_oracle.latlng_to_cell(lat, lon, res)
        order = np.argsort(cells, kind="stable")
        self.res = res
        self.lat, self.lon = lat[order], lon[order]
        self.cells, self.start, self.count = np.unique(cells[order], return_index=True, return_counts=True)
        # (cells in the order of a fixed shuffle, so that neighbouring ids are not neighbouring cells)
        p = np.random.default_rng(8800 + res).permutation(self.cells.size)
        self.cells, self.start, self.count = self.cells[p], self.start[p], self.count[p]

    def points(self, cell_idx, rng):
        at = self.start[cell_idx] + rng.integers(0, 1 << 30, cell_idx.size) % self.count[cell_idx]
        return self.lat[at], self.lon[at]


def pool(res):
    if res not in _POOLS:
        _POOLS[res] = Pool(9, 512, 37.5, 23.5) if res == 9 else Pool(res, 1280, 37.0, 23.0)
    return _POOLS[res]


def rows_of(ids, res, windows, seed, minute=0):
    """the batch whose row i has key id ids[i] (-1: row_valid false), its timestamps in minute `minute` .. `minute` + 3
    of the key's window"""
    ids = np.asarray(ids, np.int64)
    rng = np.random.default_rng(seed)
    P = pool(res)
    n = ids.size
    k = np.where(ids >= 0, ids, 0)
    assert k.max() // windows < P.cells.size, "more keys than the pool has cells"
    lat, lon = P.points(k // windows, rng)
    ts = T0 + (k % windows) * TILE + minute * MINUTE + rng.integers(0, 3 * MINUTE, n)
    speed = rng.integers(0, 1 << 17, n) / 1024.0
    sv = (rng.random(n) > 0.2) & (k != 0)
    return dict(lat=lat, lon=lon, ts_us=ts.astype(np.int64), speed=speed, speed_valid=sv,
                vkey=rng.integers(0, 40, n).astype(np.uint64), row_valid=ids >= 0)


def _shuffled(rng, *parts):
    a = np.concatenate([np.asarray(p, np.int64) for p in parts])
    return a[rng.permutation(a.size)]


# ---------------------------------------------------------------------------------------------------------
# k_agg's table policy, followed on the key ids (one workgroup: MOBHEAT_TEST_AGG_GRID=1)
# ---------------------------------------------------------------------------------------------------------
def keep_from(hist):
    """ag_flush's threshold: keep the entries of count >= 2^kf, the classes 15 .. 1 while at most AG_KEEP_MAX entries"""
    kf, acc = 16, 0
    for b in range(15, 0, -1):
        if acc + hist[b] > AG_KEEP_MAX:
            break
        acc += hist[b]
        kf = b
    return kf


def simulate(ids):
    """The span's flushes if no insert fails its probes: a list of dict(round, occ, hist, kf, kept, evicted, counts) for
    the non-final flushes (counts: key id -> rows in the table at the flush), then the aggregates evicted in all (the
    final flush included), the distinct keys, and the largest number of keys the table ever held."""
    ids = np.asarray(ids, np.int64)
    table, occ, flushes, evicted, max_occ = {}, 0, [], 0, 0
    for r0 in range(0, ids.size, AG_THREADS):
        for k in ids[r0:r0 + AG_THREADS].tolist():
            if k < 0:
                continue
            if k not in table:
                table[k] = 0
                occ += 1
            table[k] += 1
        assert occ == len(table)
        max_occ = max(max_occ, occ)
        if occ > AG_FLUSH_AT:
            hist = [0] * 16
            for c in table.values():
                hist[min(c.bit_length() - 1, 15)] += 1
            kf = keep_from(hist)
            kept = {k: c for k, c in table.items() if min(c.bit_length() - 1, 15) >= kf}
            flushes.append(dict(round=r0 // AG_THREADS + 1, occ=occ, hist=hist, kf=kf, kept=len(kept),
                                evicted=len(table) - len(kept), counts=dict(table)))
            evicted += len(table) - len(kept)
            table, occ = kept, len(kept)
    evicted += len(table)
    return dict(flushes=flushes, evicted=evicted, distinct=int(np.unique(ids[ids >= 0]).size), max_occ=max_occ)


# ---------------------------------------------------------------------------------------------------------
# the cases: name -> dict(res, windows, env, ids (one array per batch), batches)
# ---------------------------------------------------------------------------------------------------------
def _ids_resident(rng):
    return [_shuffled(rng, np.arange(3000), rng.integers(0, 3000, 8192 - 3000))]


HOT_KEYS, HOT_FRESH, HOT_ROUNDS = 32, 128, 51


def _ids_flush_keeps_hot(rng):
    out, nxt = [], HOT_KEYS
    for _ in range(HOT_ROUNDS):   # a round: 128 fresh singletons and 896 rows over the 32 hot keys
        out.append(_shuffled(rng, np.arange(nxt, nxt + HOT_FRESH), rng.integers(0, HOT_KEYS, AG_THREADS - HOT_FRESH)))
        nxt += HOT_FRESH
    return [np.concatenate(out)]


PAIR_KEYS, PAIR_SINGLES, PAIR_INTERVALS = 600, 2650, 3


def _ids_keep_class_over_cap(rng):
    # an interval = 4 rounds: the 600 recurring keys twice each, 2650 singletons (3250 keys > AG_FLUSH_AT at the end of
    # the 4th round, at most 3072 rows before) and 246 invalid rows that fill the 4 x 1024 rows
    out, nxt = [], PAIR_KEYS
    for _ in range(PAIR_INTERVALS):
        fill = 4 * AG_THREADS - 2 * PAIR_KEYS - PAIR_SINGLES
        out.append(_shuffled(rng, np.arange(PAIR_KEYS), np.arange(PAIR_KEYS), np.arange(nxt, nxt + PAIR_SINGLES),
                             np.full(fill, -1)))
        nxt += PAIR_SINGLES
    out.append(_shuffled(rng, np.arange(300), np.arange(nxt, nxt + 400)))   # the tail: half of the recurring keys again
    return [np.concatenate(out)]


TOP_HEAVY, TOP_LIGHT, TOP_SINGLES, TOP_INTERVALS = 300, 300, 2720, 3


def _ids_keep_top_class_only(rng):
    # an interval = 5 rounds: 300 heavy keys 4..7 times, 300 light keys 2..3 times, 2720 singletons (3320 keys at the
    # end of the 5th round; the heavy keys stay resident from the first flush on, the light ones recur as fresh keys)
    heavy = np.repeat(np.arange(TOP_HEAVY), 4 + np.arange(TOP_HEAVY) % 4)
    light = np.repeat(TOP_HEAVY + np.arange(TOP_LIGHT), 2 + np.arange(TOP_LIGHT) % 2)
    assert heavy.size + light.size + TOP_SINGLES == 5 * AG_THREADS
    out, nxt = [], TOP_HEAVY + TOP_LIGHT
    for _ in range(TOP_INTERVALS):
        out.append(_shuffled(rng, heavy, light, np.arange(nxt, nxt + TOP_SINGLES)))
        nxt += TOP_SINGLES
    out.append(_shuffled(rng, np.arange(TOP_HEAVY + TOP_LIGHT), np.arange(nxt, nxt + 400)))
    return [np.concatenate(out)]


def _ids_round_overflows_table(rng):
    return [rng.permutation(8192)]


SWEEP_A, SWEEP_B, SWEEP_INVALID = 3250, 2750, 3


def _ids_bucket_cap_sweep(rng):
    # 6000 distinct keys in 8192 rows, 3 of them invalid (8189 aggregated rows: the first batch's capacity is
    # max(floor, rows / 4096), which 8192 valid rows would make 2 under a floor of 1).  Rounds 1-4 hold 3250 keys
    # (a flush at the end of the 4th), rounds 5-8 2750 new ones and repeats of those alone, so that the table never
    # holds more than 3250 keys (85%) and no insert is expected to fail its probes.
    a = _shuffled(rng, np.arange(SWEEP_A), rng.integers(0, SWEEP_A, 4 * AG_THREADS - SWEEP_A - SWEEP_INVALID),
                  np.full(SWEEP_INVALID, -1))
    b = _shuffled(rng, SWEEP_A + np.arange(SWEEP_B), SWEEP_A + rng.integers(0, SWEEP_B, 4 * AG_THREADS - SWEEP_B))
    return [np.concatenate([a, b])]


def _ids_cap_adapts(rng):
    b = _ids_bucket_cap_sweep(np.random.default_rng(SEEDS["bucket_cap_sweep"]))[0]
    # batch A's 50 keys: id 0 and 49 drawn by the seed -- the capacity stays at its floor of 4 after A only if none of
    # the device's 256 buckets received more than 2 of them (2 x fullest <= 4), which the GPU test observes
    keys = np.r_[0, 1 + rng.choice(SWEEP_A + SWEEP_B - 1, 49, replace=False)]
    return [_shuffled(rng, keys, rng.choice(keys, 150)), b, b]


# bin_reduce_emits, on the production grid (256 CUs: spans of 8 rounds) and capacity.  A round is 520 keys never seen
# before, 120 keys of rounds at least 8 earlier (another workgroup's span: fresh here, a further bucket record of that
# key) and 384 repeats of the round's own 640 keys, so that a span inserts 640 keys a round, flushes at 3200 after its
# 5th (84% of the slots: hardly an insert fails) and leaves 640 bucket records per round.  1800 rounds leave 1 152 000
# records, about 4500 per bucket, on about 3650 keys per bucket: more than AG_FLUSH_AT keys AND more than four rounds
# of records, so a bucket's emission is followed by further inserts into the cleared table, and a key with records on
# either side of it leaves k_bin_reduce twice.  (With every record a key of its own the reducing table would pass
# its 3833 slots in the 4th round and spill about 70 records per bucket: the repeated keys keep it below.)
EMIT_ROUNDS, EMIT_NEW, EMIT_OLD, EMIT_REPEATS, EMIT_CUS = 1800, 520, 120, 384, 256
EMIT_KEYS = EMIT_ROUNDS * EMIT_NEW   # (+ 8 x 120 in the first span)
EMIT_DISTINCT = EMIT_KEYS + 8 * EMIT_OLD
EMIT_ROWS = EMIT_ROUNDS * AG_THREADS


def _ids_bin_reduce_emits(rng):
    assert EMIT_NEW + EMIT_OLD + EMIT_REPEATS == AG_THREADS
    out = np.empty((EMIT_ROUNDS, AG_THREADS), np.int64)
    for r in range(EMIT_ROUNDS):
        new = np.arange(r * EMIT_NEW, (r + 1) * EMIT_NEW)
        # (the first span has no earlier one: its rounds take 120 more new keys each, ids from EMIT_KEYS on)
        old = rng.integers(0, (r - 7) * EMIT_NEW, EMIT_OLD) if r >= 8 else EMIT_KEYS + r * EMIT_OLD + np.arange(EMIT_OLD)
        first = np.r_[new, np.unique(old)]
        rest = rng.choice(first, AG_THREADS - first.size)
        out[r] = np.r_[first, rest][rng.permutation(AG_THREADS)]
    a = out.ravel()
    return [a, a]


def emit_span():
    """rows per k_agg workgroup on a device of EMIT_CUS compute units (phase_table)"""
    per = -(-EMIT_ROWS // EMIT_CUS)
    return -(-per // AG_THREADS) * AG_THREADS


def _ids_many_windows_on_spill(rng):
    return [rng.permutation(8192)]


SEEDS = {"resident": 8101, "flush_keeps_hot": 8102, "keep_class_over_cap": 8103, "keep_top_class_only": 8104,
         "round_overflows_table": 8105, "bucket_cap_sweep": 8106, "cap_adapts": 8117, "bin_reduce_emits": 8108,
         "many_windows_on_spill": 8109}
# name -> (key ids, resolution, windows, MOBHEAT_TEST_AGG_GRID, MOBHEAT_TEST_AGG_CAP; None: unset, "sweep": CAP_SWEEP)
SPECS = {
    "resident": (_ids_resident, 9, 2, 1, None),
    "flush_keeps_hot": (_ids_flush_keeps_hot, 9, 2, 1, None),
    "keep_class_over_cap": (_ids_keep_class_over_cap, 9, 2, 1, None),
    "keep_top_class_only": (_ids_keep_top_class_only, 9, 2, 1, None),
    "round_overflows_table": (_ids_round_overflows_table, 9, 2, 1, None),
    "bucket_cap_sweep": (_ids_bucket_cap_sweep, 9, 2, 1, "sweep"),
    "cap_adapts": (_ids_cap_adapts, 9, 2, 1, 4),
    "bin_reduce_emits": (_ids_bin_reduce_emits, 12, 1, None, None),
    # (a floor of 1; with 8192 aggregated rows the first batch's capacity is max(1, 8192 / 4096) = 2)
    "many_windows_on_spill": (_ids_many_windows_on_spill, 9, 300, 1, 1),
}
# the stage case runs round_overflows_table's batch, one half per rank, under grid 1 and a capacity floor of 2
STAGE_WORLD2 = dict(of="round_overflows_table", grid=1, cap=2, world=2)


def case(name):
    """dict(name, res, windows, grid, cap, ids, batches); batch k's timestamps lie k minutes into its windows (the same
    keys a minute later, where a case repeats its ids)"""
    if name not in _CASES:
        make, res, windows, grid, cap = SPECS[name]
        ids = make(np.random.default_rng(SEEDS[name]))
        batches = [rows_of(a, res, windows, SEEDS[name] * 10 + k, minute=k) for k, a in enumerate(ids)]
        _CASES[name] = dict(name=name, res=res, windows=windows, grid=grid, cap=cap, ids=ids, batches=batches)
    return _CASES[name]


def env_of(c, cap=None):
    """the environment a case's engine is created under (cap: the sweep's value)"""
    env = {"MOBHEAT_INGEST_MODE": "table"}
    if c["grid"] is not None:
        env["MOBHEAT_TEST_AGG_GRID"] = str(c["grid"])
    f = cap if c["cap"] == "sweep" else c["cap"]
    if f is not None:
        env["MOBHEAT_TEST_AGG_CAP"] = str(f)
    return env


def _mix64(x):
    """csrc/kernels.h mix64 on a uint64 array"""
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def bucket_of(cells, wstarts):
    """each row's bucket, as the device places it: ag_bin (csrc/k_table.h) of the event key -- the cell's low 52 bits
    and the window's registry slot + 1 above them, the slot being the window number modulo WREG_SLOTS = 4095 when no
    two windows of the batch collide there (csrc/kernels.h ekey_make, csrc/dev_common.h wreg_find)"""
    w = np.asarray(wstarts, np.int64) // TILE
    slots = np.unique(w) % 4095
    assert np.unique(slots).size == slots.size
    k = (np.asarray(cells).astype(np.uint64) & np.uint64((1 << 52) - 1)) | ((w % 4095 + 1).astype(np.uint64) << np.uint64(52))
    return (_mix64(k ^ np.uint64(0x94d049bb133111eb)) & np.uint64(AG_BINS - 1)).astype(np.int64)


def bucket_counts(cells, wstarts):
    """distinct keys per bucket"""
    u = np.unique(np.rec.fromarrays([cells, wstarts], names="c,w"))
    return np.bincount(bucket_of(u["c"], u["w"]), minlength=AG_BINS)


def emit_bucket_records(c):
    """bin_reduce_emits: per bucket, the most records k_agg can leave there -- the distinct (key, span, before or after
    the span's flush) triples: a span flushes once, after its 5th round, and a key inserted twice between two flushes
    is one entry of the table"""
    b = c["batches"][0]
    cells, ws = keys_of(b, c["res"])
    row = np.arange(cells.size)
    span, late = row // emit_span(), row % emit_span() >= 5 * AG_THREADS
    u = np.unique(np.rec.fromarrays([cells, ws, span, late], names="c,w,s,l"))
    return np.bincount(bucket_of(u["c"], u["w"]), minlength=AG_BINS)


def keys_of(b, res):
    """(cell, window start) of a batch's valid rows, from the oracle's cells"""
    from oracle import h3_oracle
    v = b["row_valid"]
    return h3_oracle.latlng_to_cell(b["lat"][v], b["lon"][v], res), (b["ts_us"] - b["ts_us"] % TILE)[v]
