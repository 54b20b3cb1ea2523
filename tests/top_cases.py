"""Shared by the top-k tests (tests/test_top_host.py, tests/test_gpu_top.py): the order of include/mobheat.h's hm_top_*
restated with Python's sorted on Python ints -- on purpose none of the library's code -- and the record sets the host
execution and the device are held to.  No tolerance anywhere: a selected record is returned whole, so the comparisons
are on the records' bytes.

The order.  Record a ranks before record b iff a.count > b.count as int64, then a.cell < b.cell as uint64, then a has the
lower input index; top(recs, k) is the first min(k, n) records of that order, k in 0..65536.

The sums of every record are dyadic (multiples of 1/1024 below 2^11), so that a roll-up that adds a few thousand of them
in any order is exact and whole records can be compared after it too."""
import functools

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TOP_MAX = 65536
# csrc/dev_table.h's constant, which the library does not export: a change there must be made here
DUMP_PER = 8
TILE = 256 * DUMP_PER            # the records one compaction workgroup takes per iteration
TEST_GRID = 2                    # MOBHEAT_TEST_TOP_GRID of the second-iteration case
WS = 1_759_572_000_000_000
MINUTE = 60_000_000


def ref_top(recs, k):
    """top(recs, k) by Python's sorted on (-count, cell, index)"""
    assert 0 <= k <= TOP_MAX
    cnt, cell = recs["count"].tolist(), recs["cell"].tolist()
    order = sorted(range(recs.size), key=lambda i: (-cnt[i], cell[i], i))[:k]
    return recs[np.array(order, np.int64)] if order else recs[:0]


def cells_of(n, res=8, start=0):
    """n distinct H3-shaped words of resolution res: mode 1, base cell i % 122, the digits of i // 122 in base 7 from the
    finest digit up, 7 below the resolution"""
    i = np.arange(start, start + n, dtype=np.uint64)
    word = np.full(n, (1 << 59) | (res << 52), np.uint64) | ((i % np.uint64(122)) << np.uint64(45))
    q = i // np.uint64(122)
    for d in range(15, 0, -1):
        if d > res:
            digit = np.full(n, 7, np.uint64)
        else:
            digit, q = q % np.uint64(7), q // np.uint64(7)
        word |= digit << np.uint64(3 * (15 - d))
    assert not q.any() and np.unique(word).size == n
    return word


def records(counts, cells, tag=False):
    """STATE_REC_DTYPE records of the given counts and cells with dyadic sums that differ from record to record; tag: the
    fields the order does not read hold a word of their own each (a caller record returned whole shows them)"""
    from mobheat._lib import STATE_REC_DTYPE
    counts = np.asarray(counts, np.int64)
    i = np.arange(counts.size)
    r = np.zeros(counts.size, STATE_REC_DTYPE)
    r["cell"], r["count"], r["window_start_us"] = cells, counts, WS
    r["n_speed"], r["sum_speed"] = 1 + i % 3, (i % 512) / 4.0
    r["sum_lat"], r["sum_lon"] = (i % 2048) / 1024.0, -((i * 7) % 2048) / 1024.0
    if tag:
        r["window_start_us"], r["reserved"] = WS + i, i ^ 0x5A5A5A5A
    return r


def _ks(n, *more):
    return sorted({k for k in (0, 1, n - 1, n, n + 1) + more if 0 <= k <= TOP_MAX})


def _case(name, recs, ks, distinct=True, **expect):
    """expect: per k, what hm_top_info must show (test_gpu_top.py reads it): count_passes / cell_passes / index_passes as
    "0" or ">0", tied = a number"""
    if distinct:
        assert np.unique(recs["cell"]).size == recs.size, name
    return {"name": name, "recs": recs, "ks": ks, "distinct": distinct, "expect": expect}


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]
# every workgroup of a TEST_GRID-workgroup compaction takes a second iteration, the last one a partial tile
SECOND_ITERATION = 2 * TEST_GRID * TILE - 5


@functools.lru_cache(maxsize=None)
def cases():
    """every record set with its k values, reference not included (ref_top is cheap); cached: the tests share them"""
    rng = np.random.default_rng(77)
    out = []
    for n in SIZES + [SECOND_ITERATION]:
        # counts 1..50: many ties, so the select goes on into the cell bytes
        out.append(_case(f"n {n}", records(rng.integers(1, 51, n), rng.permutation(cells_of(n)), tag=True), _ks(n, n // 2)))
    for n in (TOP_MAX + 1, 70000):
        out.append(_case(f"n {n}", records(rng.integers(1, 1001, n), rng.permutation(cells_of(n))), [TOP_MAX, 1]))
    n = 300
    cells = rng.permutation(cells_of(n))
    out.append(_case("counts all distinct", records(rng.permutation(n) + 1, cells), _ks(n, 100), cell_passes="0"))
    out.append(_case("counts all equal", records(np.full(n, 7), cells), [1, 100, n - 1], count_passes="0", cell_passes=">0"))
    groups = rng.permutation(np.repeat([9, 5, 2], 100))
    out.append(_case("tie group straddles k", records(groups, cells), [101, 150, 199], count_passes=">0", cell_passes=">0"))
    out.append(_case("tie group ends at k", records(groups, cells), [100, 200], count_passes=">0", cell_passes="0", tied=100))
    j = rng.permutation(200) + 1
    out.append(_case("counts differ in byte 4", records((j.astype(np.int64) << 32) + 5, cells[:200]), [1, 10, 199],
                     count_passes=">0", cell_passes="0", tied=1))
    j = rng.permutation(201) - 100
    out.append(_case("counts differ in byte 7", records(j.astype(np.int64) * (1 << 56) + 5, cells[:201]), [1, 100, 101, 200],
                     count_passes=">0", cell_passes="0", tied=1))
    a, b = rng.integers(0, 4, 500), rng.integers(0, 256, 500)
    out.append(_case("a constant byte between two varying", records((a << 16) | (0x11 << 8) | b, cells_of(500)), [1, 50, 250, 499]))
    ext = np.array([0, -1, INT64_MIN, INT64_MAX, 1, -5, 1 << 32, -(1 << 32), INT64_MAX - 1, INT64_MIN + 1] * 4, np.int64)
    out.append(_case("count extremes", records(ext, rng.permutation(cells_of(ext.size)), tag=True), _ks(ext.size, 3, 4, 5, 20)))
    mixed = np.concatenate([cells_of(100, 6), cells_of(100, 8, 100), cells_of(100, 9, 200)])
    out.append(_case("mixed resolutions", records(rng.integers(1, 4, n), rng.permutation(mixed)), _ks(n, 37, 150)))
    last = cells_of(1, 8)[0] & ~np.uint64(7 << 21)   # the res-8 digit cleared
    sibs = np.array([last | np.uint64(d << 21) for d in range(7)], np.uint64)
    out.append(_case("cells differ in the last digit", records(np.full(7, 3), sibs[rng.permutation(7)]), list(range(8)),
                     count_passes="0", cell_passes=">0"))
    # caller records only: 50 copies of one (count, cell) between 20 higher and 20 lower counts; k cuts the copies
    dup_cnt = np.r_[rng.integers(10, 20, 20), np.full(50, 4), rng.integers(1, 4, 20)]
    dup_cell = np.r_[cells_of(20), np.full(50, cells_of(1, 8, 999)[0]), cells_of(20, 8, 20)]
    p = rng.permutation(90)
    out.append(_case("repeated (count, cell) straddles k", records(dup_cnt[p], dup_cell[p], tag=True), [21, 40, 69], distinct=False,
                     index_passes=">0"))
    return out


def window_records_case(oracle_h3, n=6000, seed=5):
    """records of distinct res-8 cells (half of them in Boston, half anywhere on the sphere) for import_state: small counts
    with many ties, and every 97th at or above 2^32"""
    rng = np.random.default_rng(seed)
    la = np.r_[rng.uniform(42.20, 42.45, n // 2), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n // 2)))]
    lo = np.r_[rng.uniform(-71.20, -70.95, n // 2), rng.uniform(-180.0, 180.0, n // 2)]
    # points near the antimeridian, so that a view across it keeps something
    la[-200:], lo[-200:] = rng.uniform(-50.0, 50.0, 200), np.where(rng.random(200) < 0.5, 1.0, -1.0) * rng.uniform(175.0, 180.0, 200)
    cells = np.unique(oracle_h3.latlng_to_cell(la, lo, 8))
    counts = rng.integers(1, 30, cells.size).astype(np.int64)
    counts[::97] = (1 << 32) + rng.integers(0, 3, counts[::97].size)
    r = records(counts, rng.permutation(cells))
    r["n_speed"] = 1   # (a state record has n_speed <= count)
    return r


def state_info(n_keys):
    return dict(epoch_id=0, n_keys=int(n_keys), watermark_ms=0, prev_watermark_ms=0, tile_us=5 * MINUTE, watermark_delay_ms=600_000,
                h3_res=8)


def same(got, want, what=""):
    """whole records, bit for bit, in order"""
    assert got.size == want.size, f"{what}: {got.size} records, {want.size} expected"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])
        raise AssertionError(f"{what}: {bad.size} of {got.size} records differ, first at rank {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")
