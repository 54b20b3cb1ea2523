"""Event-time boundary scenarios: scripted streams of small batches whose rows sit ON the window, lateness and eviction
edges (no GPU code is imported here; tests/test_event_time_cases_host.py checks the scenarios against the oracle alone,
tests/test_gpu_event_time.py runs them on the device).

For a configuration (tile_us, delay_ms, late_uses_prev_watermark) `scenario()` drives a SparkHeatmapOracle batch by
batch.  Before each batch it reads the oracle's wm_prev / wm_cur and places groups of rows relative to

    L = late watermark * 1000   (wm_prev under the previous-watermark rule, wm_cur otherwise)
    E = wm_cur * 1000           (the eviction bound of this batch)
    F = the eviction bound of the NEXT batch (known here: the batch's own maximum decides it)

with wl = floor(L / tile) * tile, the start of the window that contains L (wl == L when L is a window end):

    late_edge      window [wl - tile, wl): its end is the largest window end <= L          -> late (class 1)
    kept_edge      window [wl, wl + tile): ts = wl, L, wl + 1, the window's last us        -> kept (class 2)
    l_minus_1      ts = L - 1: late iff L is a window end                                  (class 2)
    evict_now      the last window whose end lies in (L, E]: kept, emitted, evicted by this batch (class 3; none when
                   the late rule uses wm_cur, for then L = E)
    replay_evicted the previous batch's evict_now rows again                               -> late (class 3)
    doomed_next    the last window whose end lies in (max(L, E), F]: kept and live after this batch, evicted by the next
                   one whatever that holds (an empty batch included)                        (classes 4, 5)
    head / head_prev  the window of the batch's maximum, and the previous batch's again (cumulative counts) (class 4)
    marker         the batch's maximum, ...999 us: it sets the next watermark (class 5)
    veh_*          vehicles with late rows only, a late and a kept row, tied late rows, tied kept rows (class 6; a late
                   and a kept row cannot tie: equal timestamps share a window)
    invalid        a null row with a far-future ts (it must not move the watermark), a NaN latitude, a longitude of 181

Every verdict is fixed by construction (the group's window relative to wl) and double-checked in Python integers
(`rule_late`); the expected n_late / n_valid of a batch are sums of group sizes, not oracle outputs.  The rows fall in
five res-9 cells on dyadic points with dyadic speeds, so every fp64 sum is exact in any order; a fixed permutation puts
late and kept rows side by side in every wave.
"""
import numpy as np

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
T0 = 1_759_572_000_000_000   # 2025-10-04 10:00:00 UTC, a 5-minute window start
RES = 9
GROUP_ROWS = 70

# (tile_us, delay_ms, purpose)
CONFIGS = [
    (300_000_000, 600_000, "the default"),
    (60_000_000, 0, "zero delay"),
    (3_600_000_000, 600_000, "delay shorter than the tile"),
    (86_400_000_000, 1, "one-day tile"),
    (420_000_000, 123_457, "window starts off the hour, delay not a multiple of anything"),
    (1_000_000, 1_500, "the smallest tile"),
    (1_000_001, 600_000, "window ends that are not whole milliseconds"),
]
CONFIG_IDS = [f"tile{t}-delay{d}" for t, d, _ in CONFIGS]


# Which boundary classes a (configuration, rule) can populate.  Class 3 (a window emitted and evicted by the same batch,
# its rows late in the next) needs L < E, which only the previous-watermark rule gives; an empty batch makes a kept row
# late under that rule only.  "end_equals_L": a window end can equal L only when window ends are whole milliseconds;
# the 1 000 001 us tile instead has ends within a millisecond of L on either side ("decided_at_us").
def expectations(tile_us, late_prev):
    whole_ms = tile_us % 1000 == 0
    return dict(evict_now=late_prev, replay_evicted=late_prev, late_by_empty_batch=late_prev, end_equals_L=whole_ms,
                decided_at_us=not whole_ms)


def rule_late(ts, tile_us, L):
    """the Spark rule in Python integers: window = [ts - floormod(ts, tile), + tile), late iff window.end <= L"""
    ts = int(ts)
    return ts - ts % tile_us + tile_us <= L


def valid_range(tile_us):
    """(lowest, highest) timestamp the engine and the oracle treat as valid"""
    return INT64_MIN + 2 * tile_us + 1, INT64_MAX - 2 * tile_us - 1


def _spread(lo, hi, n, rng):
    """n timestamps in [lo, hi], the two ends and lo + 1 among them"""
    hi = max(lo, hi)
    fixed = [lo, hi, min(lo + 1, hi)]
    span = hi - lo + 1
    rest = [lo + int(x) for x in rng.integers(0, min(span, 1 << 62), max(n - len(fixed), 0))]
    return (fixed + rest)[:n]


class _Batch:
    """rows of one batch, group by group; verdict: "late", "kept" or "invalid" """

    def __init__(self, tile_us, L):
        self.tile, self.L = tile_us, L
        self.ts, self.cellidx, self.vkey, self.kind, self.group = [], [], [], [], []
        self.invalid_how = []

    def add(self, group, ts_list, verdict, vkey=None, invalid_how=0, cell=None):
        lo, hi = valid_range(self.tile)
        for k, t in enumerate(ts_list):
            t = int(t)
            if verdict != "invalid":   # the construction must agree with the rule, in Python integers
                assert lo <= t <= hi, (group, t)
                assert rule_late(t, self.tile, self.L) == (verdict == "late"), (group, t, self.L, verdict)
            self.ts.append(t)
            self.cellidx.append(len(self.ts) % 5 if cell is None else cell)
            self.vkey.append(100 + len(self.ts) % 37 if vkey is None else vkey)
            self.kind.append(verdict)
            self.group.append(group)
            self.invalid_how.append(invalid_how if verdict == "invalid" else 0)


def _columns(b, rng):
    """the batch's columns in a fixed random order, and the meta data in the same order"""
    n = len(b.ts)
    p = rng.permutation(n) if n else np.zeros(0, np.int64)
    ts = np.array(b.ts, np.int64)[p] if n else np.zeros(0, np.int64)
    ci = np.array(b.cellidx, np.int64)[p] if n else np.zeros(0, np.int64)
    kind = np.array(b.kind, dtype=object)[p] if n else np.zeros(0, object)
    group = np.array(b.group, dtype=object)[p] if n else np.zeros(0, object)
    how = np.array(b.invalid_how, np.int64)[p] if n else np.zeros(0, np.int64)
    # five res-9 cells 1/64 degree apart, each row on one of 8 dyadic points 2^-20 degree apart inside its cell
    lat = 37.5 + ci / 64.0 + rng.integers(0, 8, n) / float(1 << 20)
    lon = 23.75 + ci / 64.0 + rng.integers(0, 8, n) / float(1 << 20)
    speed = rng.integers(0, 960, n) / 8.0
    sv = rng.random(n) > 0.2
    rv = np.ones(n, bool)
    rv[how == 1] = False
    lat = np.where(how == 2, np.nan, lat)
    lon = np.where(how == 3, 181.0, lon)
    cols = dict(lat=lat, lon=lon, ts_us=ts, speed=speed, speed_valid=sv,
                vkey=(np.array(b.vkey, np.uint64)[p] if n else np.zeros(0, np.uint64)), row_valid=rv)
    return cols, kind, group


def _generic(b, L, E, F, tile, rng, prev_evict_now, cap):
    """the groups every ordinary batch holds; returns its evict_now timestamps (for the next batch's replay) and tags"""
    hi = valid_range(tile)[1]
    hi = hi if cap is None else min(hi, cap)   # (no row above the batch's intended maximum)
    wl = L // tile * tile
    tags = dict(end_equals_L=wl == L, evict_now_window=None, doomed_window=None, late_edge_end=wl)
    b.add("late_edge", _spread(wl - tile, wl - 1, GROUP_ROWS, rng), "late")
    b.add("kept_edge", [L] + _spread(wl, min(wl + tile - 1, hi), GROUP_ROWS - 1, rng), "kept")
    b.add("l_minus_1", [L - 1], "late" if wl == L else "kept")
    # the window ends within a millisecond of L, on either side (what a comparison in milliseconds would get wrong)
    tags["kept_end_within_ms"] = 0 < wl + tile - L < 1000
    tags["late_end_within_ms"] = 0 < L - wl < 1000
    evict_now = []
    we = E // tile * tile
    if we > L:
        evict_now = _spread(we - tile, we - 1, GROUP_ROWS, rng)
        b.add("evict_now", evict_now, "kept")
        tags["evict_now_window"] = we - tile
    if prev_evict_now:
        b.add("replay_evicted", prev_evict_now, "late")
    if F is not None:
        wf = F // tile * tile
        if wf > E and wf > L and wf - 1 <= hi:
            b.add("doomed_next", _spread(wf - tile, wf - 1, GROUP_ROWS, rng), "kept")
            tags["doomed_window"] = wf - tile
    # class 6: dedup across lateness (latest rows are taken over the valid rows, late ones included)
    b.add("veh_late_newest", [wl - tile + 5, wl - tile + 9], "late", vkey=1)
    b.add("veh_late_only", [wl - 7], "late", vkey=2)
    b.add("veh_late_then_kept", [wl - 2], "late", vkey=3)
    b.add("veh_late_then_kept", [min(wl + 2, hi)], "kept", vkey=3)
    b.add("veh_tie_late", [wl - 3, wl - 3], "late", vkey=4)
    b.add("veh_tie_kept", [wl, wl], "kept", vkey=5)
    return evict_now, tags


def _invalid(b, future_ts):
    b.add("invalid", [future_ts], "invalid", invalid_how=1)   # a null row far in the future
    b.add("invalid", [b.L], "invalid", invalid_how=2)         # NaN latitude
    b.add("invalid", [b.L], "invalid", invalid_how=3)         # longitude 181


def _head(b, marker, tile, prev_head):
    """rows in the window of the batch's maximum (none above it), the previous batch's head window again, the marker"""
    x = marker // tile * tile
    width = min(marker - x + 1, 1000)
    b.add("head", [x + k % width for k in range(GROUP_ROWS // 2)], "kept")
    if prev_head is not None and prev_head != x:
        b.add("head_prev", [prev_head + k % 7 for k in range(GROUP_ROWS // 2)], "kept")
    b.add("marker", [marker], "kept")
    return x


def steps_per_batch(tile_us, delay_ms):
    """windows the watermark advances per stepping batch: one, unless the delay spans many windows (then half the
    delay, so that a head window is evicted two or three batches after it was created)"""
    d = delay_ms * 1000
    return 1 if d <= 3 * tile_us else -(-d // (2 * tile_us))


def scenario(tile_us, delay_ms, late_prev, oracle_factory):
    """[(name, columns, oracle result, meta)] of the scripted stream.  oracle_factory(**kw) -> SparkHeatmapOracle.
    meta: L, E, wm_prev / wm_cur before the batch, `groups` (name -> row indices), `kind` (per row), the hand counts
    n_valid / n_late, `tags`, `state_windows` (the oracle's live window starts after the batch)."""
    tile, D = int(tile_us), int(delay_ms) * 1000
    ora = oracle_factory(h3_res=RES, watermark_delay_ms=delay_ms, late_uses_prev_watermark=late_prev, tile_us=tile)
    rng = np.random.default_rng(8100 + tile % 9973 + delay_ms % 97 + (7 if late_prev else 0))
    lo, hi = valid_range(tile)
    A = -(-T0 // tile) * tile                 # the first window start at or after T0
    S = steps_per_batch(tile, delay_ms)
    whole_ms = tile % 1000 == 0

    def target(k):
        """the watermark (us) the k-th stepping batch aims at: a window end, or, where window ends are not whole
        milliseconds, the millisecond below (even k) or above (odd k) one"""
        we = A + (2 + k * S) * tile
        if whole_ms:
            return we
        return we // 1000 * 1000 + (1000 if k % 2 else 0)

    def marker_for(k):
        return target(k) + D + 999

    out = []
    state = dict(prev_evict_now=[], prev_head=None)

    def run(name, build, marker=None, ordinary=True):
        P, C = ora.wm_prev, ora.wm_cur
        L, E = (P if late_prev else C) * 1000, C * 1000
        F = None if marker is None else max(C, marker // 1000 - delay_ms) * 1000
        cap = None if marker is None else max(marker, L)   # (ts = L is always a row: the maximum where L > marker)
        b = _Batch(tile, L)
        tags = {}
        if ordinary:
            ev, tags = _generic(b, L, E, F, tile, rng, state["prev_evict_now"], cap)
            state["prev_evict_now"] = ev
            _invalid(b, hi)   # (the null row's ts is the largest valid one: it must not become the batch maximum)
        build(b, L, E)
        if marker is not None:
            state["prev_head"] = _head(b, marker, tile, state["prev_head"])
        cols, kind, group = _columns(b, rng)
        exp = ora.process_batch(**cols)
        groups = {g: np.flatnonzero(group == g) for g in sorted(set(group.tolist()))}
        meta = dict(L=L, E=E, F=F, wm_prev=P, wm_cur=C, kind=kind, groups=groups, tags=tags, marker=marker, batch_max=cap,
                    n_valid=int((kind != "invalid").sum()), n_late=int((kind == "late").sum()),
                    state_windows=sorted({k[1] for k in ora.state}),
                    n_state_keys=sum(1 for k in ora.state if k[1] + tile > E))   # keys of windows that outlive E
        out.append((name, cols, exp, meta))

    nothing = lambda b, L, E: None   # noqa: E731

    # 0: the only valid rows are late (L = 0: the window [-tile, 0) ends at 0), and the maximum is -1 us, which
    #    truncates to 0 ms (a floor would give -1)
    def negative_only(b, L, E):
        b.add("late_edge", _spread(-tile, -1, GROUP_ROWS, rng), "late")
        b.add("veh_late_newest", [-9, -5], "late", vkey=1)
        _invalid(b, hi)
    run("negative_only", negative_only, ordinary=False)

    # 1: the first ordinary batch, around L = 0, with window boundaries k * tile - 1, k * tile, k * tile + 1 for small k
    def first(b, L, E):
        b.add("small_k", [1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1], "kept")
        b.add("small_k", [-tile - 1, -tile, -tile + 1, -2 * tile], "late")
    run("first", first, marker=(A + tile // 3) // 1000 * 1000 + 999)
    # 2: a maximum below the first batch's: the watermark does not move back
    run("lower_max", nothing, marker=A + 999)
    # 3: L = E under both rules, not a window end
    run("steady", nothing, marker=marker_for(0))
    # 4 .. 10: the watermark advances by whole windows
    for k in range(1, 8):
        run(f"step{k}", nothing, marker=marker_for(k))
    # 11: rows, none valid: wm_prev <- wm_cur, and the windows up to the new eviction bound go
    def all_invalid(b, L, E):
        for _ in range(21):
            _invalid(b, hi)
    run("all_invalid", all_invalid, ordinary=False)
    run("after_invalid", nothing, marker=marker_for(8))
    # 13: no rows at all
    run("zero_rows", nothing, ordinary=False)
    # 14: a maximum a millisecond short of moving the watermark
    run("after_zero", nothing, marker=marker_for(8) - 999)
    # 15: ordinary late rows only
    def late_only(b, L, E):
        wl = L // tile * tile
        b.add("late_edge", _spread(wl - tile, wl - 1, GROUP_ROWS, rng), "late")
        b.add("late_old", _spread(wl - 3 * tile, wl - 2 * tile - 1, GROUP_ROWS, rng), "late")
        b.add("veh_tie_late", [wl - 3, wl - 3], "late", vkey=4)
        _invalid(b, hi)
    run("late_only", late_only, ordinary=False)

    # 16: the range edge: the largest and smallest valid timestamps, one past each (invalid), and the boundaries of
    #     the largest valid window
    def range_edge(b, L, E):
        kmax = hi // tile
        b.add("edge_valid", [hi], "kept", cell=0)
        b.add("edge_valid", [lo], "late")
        b.add("edge_invalid", [hi + 1, lo - 1, INT64_MAX, INT64_MIN], "invalid", invalid_how=0)
        b.add("edge_kmax", [t for t in (kmax * tile - 1, kmax * tile, kmax * tile + 1) if t <= hi], "kept")
    run("range_edge", range_edge)
    # 17, 18: after it the eviction bound, then (one batch later under the previous-watermark rule) the late bound too
    # lie at the range edge: every ordinary row is late
    ordinary_ts = [A, A + tile - 1, A + 2 * tile, target(8), target(8) + D]

    def aftermath(b, L, E):
        b.add("edge_valid", [hi], "kept", cell=0)
        for t in ordinary_ts:
            b.add("ordinary", [t], "late" if rule_late(t, tile, L) else "kept")
    run("aftermath1", aftermath)
    run("aftermath2", aftermath)
    assert all(rule_late(t, tile, out[-1][3]["L"]) for t in ordinary_ts)
    return out


# ---------------------------------------------------------------------------------------------------------
# A known-answer table for the default configuration (tile 300 s, delay 600 000 ms), worked out by hand from the Spark
# rule: late iff window.end <= late watermark * 1000, with the late watermark = the watermark before the previous batch
# (rule "prev") or before this batch ("cur"); watermark after a batch = max(before, trunc(max ts / 1000) - 600 000).
# Rows: (ts_us, verdict under "prev", verdict under "cur"); `after` = (wm_prev, wm_cur) after the batch, either rule.
#   T0 = 1 759 572 000 000 000 is a window start (1 759 572 000 s = 5 865 240 x 300 s).
# ---------------------------------------------------------------------------------------------------------
KNOWN_TILE_US, KNOWN_DELAY_MS = 300_000_000, 600_000
KNOWN_ANSWERS = [
    # before: (0, 0).  L = 0 under both rules: the window [-300 s, 0) ends at 0 <= 0.
    dict(rows=[(-1, "late", "late"), (0, "kept", "kept"),
               # the maximum: 10:15:00.123999 -> 1 759 572 900 123 ms - 600 000
               (1_759_572_900_123_999, "kept", "kept")],
         after=(0, 1_759_572_300_123)),
    # prev: L = 0.  cur: L = 1 759 572 300 123 000, past the end (10:05:00) of the windows of the first two rows.
    dict(rows=[(1_759_572_299_999_999, "kept", "late"), (1_759_571_999_999_999, "kept", "late"),
               (1_759_573_200_000_000, "kept", "kept")],   # 10:20:00 -> watermark 10:10:00.000
         after=(1_759_572_300_123, 1_759_572_600_000)),
    # prev: L = 1 759 572 300 123 000 (10:05:00.123).  cur: L = 1 759 572 600 000 000 (10:10:00), a window end.
    dict(rows=[(1_759_572_299_999_999, "late", "late"),    # window ends 10:05:00 <= L
               (1_759_572_300_000_000, "kept", "late"),    # window [10:05, 10:10): its end > 10:05:00.123, = 10:10:00
               (1_759_572_300_123_000, "kept", "late"),    # ts = L (prev)
               (1_759_572_600_000_000, "kept", "kept")],   # the maximum, 10:10:00 -> 10:00:00 < the watermark: no move
         after=(1_759_572_600_000, 1_759_572_600_000)),
    # L = 1 759 572 600 000 000 under both rules, a window end
    dict(rows=[(1_759_572_599_999_999, "late", "late"),    # ts = L - 1: its window ends AT L
               (1_759_572_600_000_000, "kept", "kept")],   # ts = L
         after=(1_759_572_600_000, 1_759_572_600_000)),
]


def known_answer_batches():
    """[(columns, rows)] of the table: every row in one cell, its own vehicle"""
    out = []
    for b in KNOWN_ANSWERS:
        n = len(b["rows"])
        out.append((dict(lat=np.full(n, 37.5), lon=np.full(n, 23.75), ts_us=np.array([r[0] for r in b["rows"]], np.int64),
                         speed=np.full(n, 8.0), speed_valid=np.ones(n, bool), vkey=np.arange(n, dtype=np.uint64),
                         row_valid=np.ones(n, bool)), b))
    return out
