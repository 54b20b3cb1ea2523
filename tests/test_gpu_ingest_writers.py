"""GPU: the binned ingest whose records reach their bins through writer waves (csrc/k_ingest.h, kWriters > 0).

Every environment setting below runs the same cases once, in a child process of its own (the library reads its
environment when a context is created; a child also keeps one setting's state out of the next), with the aggregation
path pinned by MOBHEAT_INGEST_MODE.  The tiles, latest rows and counts of every batch are compared
  - with oracle.heatmap_cpu.CpuHeatmap on the same batches (counts, keys and rows exact; averages within the project's
    1e-9 relative / 1e-12 degrees), and
  - bit for bit with the same batches under MOBHEAT_INGEST_MODE=direct, for the cases whose inputs are dyadic (multiples
    of 2^-10: every fp64 sum is exact in any order, so the order in which records reach a slab cannot show).

Cases: batch sizes around a wave (63, 64, 65), around the fused kernel's 256 rows per workgroup and the writer kernel's
512 (IGW_PROD = 8 producer waves), far below the grid (workgroups whose producer waves have no rows); batches that
produce no record (every row invalid, every row late); every row in one cell and window (one cursor, and a slab that
overflows -- under MOBHEAT_TEST_SLAB_CAP=16 after 16 records -- so that the batch re-partitions); rows alternating
between two cells; margin-exception rows on cell edges (test_device_numerics_host.hex_boundary_points) among ordinary
ones; a few thousand rows; and one batch through the stage API (whole bins, sub_bits 0).  Settings: the default;
sub-bins; small slabs; the fused kernel (MOBHEAT_INGEST_WRITERS=0); and the ring-full fallback, in which a producer
wave stores its round itself.  Batches this small are one round per producer wave on the full grid, and a ring holds
two rounds, so MOBHEAT_TEST_RING_POLLS=0 (no wait for room) alone never reaches it: MOBHEAT_TEST_RING_CAP=0 makes every
round find its ring full -- hm_last_counts [11], the records stored that way, is then every aggregated row that is no
margin exception -- and MOBHEAT_TEST_INGEST_GRID=1 runs the batch as up to 12 rounds of one workgroup, where the rings
wrap around, a writer takes several rounds from one ring and producers overlap their writer; there the fallback is
also taken as the race has it (no wait, whole and half-size rings), which the results must not show.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
REL, ABS_DEG = 1e-9, 1e-12
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)

ENVS = {
    "direct": {"MOBHEAT_INGEST_MODE": "direct"},
    "writers": {"MOBHEAT_INGEST_MODE": "binned"},
    "ring_full": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_RING_POLLS": "0", "MOBHEAT_TEST_RING_CAP": "0"},
    "one_workgroup": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_INGEST_GRID": "1"},
    "one_workgroup_ring_full": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_INGEST_GRID": "1",
                                "MOBHEAT_TEST_RING_POLLS": "0", "MOBHEAT_TEST_RING_CAP": "0"},
    "one_workgroup_no_wait": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_INGEST_GRID": "1", "MOBHEAT_TEST_RING_POLLS": "0"},
    "one_workgroup_half_ring": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_INGEST_GRID": "1",
                                "MOBHEAT_TEST_RING_POLLS": "0", "MOBHEAT_TEST_RING_CAP": "64"},
    "subbins": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_SUBBINS": "1"},
    "small_slabs": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_SLAB_CAP": "16"},
    "fused": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_INGEST_WRITERS": "0"},
}
BINNED_ENVS = [e for e in ENVS if e != "direct"]
KNOBS = ("MOBHEAT_INGEST_MODE", "MOBHEAT_TEST_RING_POLLS", "MOBHEAT_SUBBINS", "MOBHEAT_TEST_SLAB_CAP",
         "MOBHEAT_INGEST_WRITERS", "MOBHEAT_INGEST_WG_PER_CU", "MOBHEAT_PIPELINE", "MOBHEAT_TEST_RING_CAP",
         "MOBHEAT_TEST_INGEST_GRID")
ALL_DIRECT = ("ring_full", "one_workgroup_ring_full")   # every record takes the producers' own stores
NONE_DIRECT = ("writers", "subbins", "small_slabs", "fused")   # one round per wave (or no rings): never a full ring
FIELDS = ("cell", "window_start_us", "count", "avg_speed", "speed_null", "avg_lon", "avg_lat")


def _dyadic(rng, n, cells_lat=50, cells_lon=1):
    """n rows on a grid of multiples of 2^-10 degrees (about cells_lat x cells_lon res-9 cells), speeds multiples of
    2^-10, ts in the first 4 minutes of the window at T0, 40 vehicles"""
    lat = 37.5 + rng.integers(0, cells_lat, n) * (4 / 1024) + rng.integers(0, 2, n) / 1024
    lon = 23.5 + rng.integers(0, cells_lon, n) * (4 / 1024) + rng.integers(0, 2, n) / 1024
    return dict(lat=lat, lon=lon, ts_us=T0 + rng.integers(0, 4 * MINUTE, n).astype(np.int64),
                speed=rng.integers(0, 1 << 17, n) / 1024, speed_valid=rng.random(n) > 0.2,
                vkey=rng.integers(0, 40, n).astype(np.uint64), row_valid=np.ones(n, bool))


def _cases():
    """name -> (dyadic, overflows, [batches of one engine, in order])"""
    rng = np.random.default_rng(7700)
    out = {}
    out["sizes"] = (True, False, [_dyadic(rng, n) for n in SIZES])
    inv = _dyadic(rng, 2000)
    inv["row_valid"] = np.zeros(2000, bool)
    out["all_invalid"] = (True, False, [inv])
    # the watermark moves an hour ahead (two batches: a batch's late test may use the watermark before it), then a
    # batch whose rows are all late
    ahead = [_dyadic(rng, 100) for _ in range(2)]
    for b in ahead:
        b["ts_us"] = b["ts_us"] + 60 * MINUTE
    out["all_late"] = (True, False, ahead + [_dyadic(rng, 2000)])
    one = _dyadic(rng, 5000, 1, 1)
    one["lat"][:] = 37.5
    one["lon"][:] = 23.5
    out["one_cell"] = (True, True, [one])
    two = _dyadic(rng, 250, 1, 1)
    two["lat"] = 37.5 + (np.arange(250) % 2) * (64 / 1024)
    two["lon"][:] = 23.5
    out["two_cells"] = (True, False, [two])
    from test_device_numerics_host import hex_boundary_points
    mix = _dyadic(rng, 4000, 60, 60)
    elat, elon = hex_boundary_points(9, 3000, 7701)
    at = rng.permutation(4000)[:3000]
    mix["lat"][at], mix["lon"][at] = elat, elon
    out["edge_mix"] = (False, False, [mix])
    out["thousands"] = (True, False, [_dyadic(rng, 6000, 80, 80), _dyadic(rng, 6000, 80, 80)])
    return out


# ---------------------------------------------------------------------------------------------------------
# the child: every case under the environment it was started with -> one .npz
# ---------------------------------------------------------------------------------------------------------
def _child(path):
    for p in (ROOT, os.path.join(ROOT, "real-time-mobility-heatmap_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ctypes
    import mobheat
    out = {}
    lib = mobheat.load()

    def ring_direct(eng):   # hm_last_counts [11]
        c = (ctypes.c_int64 * 12)()
        assert lib.hm_last_counts(eng._ctx, c, 12) == 0
        return int(c[11])

    def put(name, k, tiles, latest, counts):
        order = np.lexsort((np.asarray(tiles.window_start_us), np.asarray(tiles.cell)))
        for f in FIELDS:
            out[f"{name}/{k}/{f}"] = np.asarray(getattr(tiles, f))[order]
        out[f"{name}/{k}/latest"] = np.sort(np.asarray(latest))
        out[f"{name}/{k}/counts"] = np.array(counts, np.int64)

    for name, (_, _, batches) in _cases().items():
        eng = mobheat.HeatmapEngine(h3_res=9)
        for k, b in enumerate(batches):
            res = eng.process_batch(k, **b)
            put(name, k, res.tiles, res.latest_rows, [res.n_valid, res.n_late, res.n_state, eng.last_counts()["binned"], ring_direct(eng)])
        eng.close()
    if os.environ.get("MOBHEAT_INGEST_MODE") == "binned":   # one batch through the stage API, two ranks
        from test_gpu_stages import _stage_batch
        b = _stage_input()
        n = b["lat"].size
        engines = [mobheat.HeatmapEngine(h3_res=9) for _ in range(2)]
        shards = [{kk: v[r * n // 2:(r + 1) * n // 2] for kk, v in b.items()} for r in range(2)]
        tiles, latest, _, _, table = _stage_batch(engines, lib, shards, 0)
        assert not table
        for r in range(2):
            put(f"stage{r}", 0, tiles[r], latest[r] + r * n // 2, [0, 0, 0, 0, 0])
        for e in engines:
            e.close()
    np.savez(path, **out)


def _stage_input():
    return _dyadic(np.random.default_rng(7702), 6000, 80, 80)


_RUNS, _CPU, _EXC = {}, {}, {}


def _exceptions(case, k):
    """margin exceptions among batch k's valid rows (the kernels' fast path executed on the host): k_ingest_exact's
    rows, which never pass through a ring"""
    if (case, k) not in _EXC:
        from mobheat import _lib
        b = _cases()[case][2][k]
        _, fb = _lib.latlng_to_cell_fast_host_selftest(b["lat"][b["row_valid"]], b["lon"][b["row_valid"]], 9)
        _EXC[(case, k)] = int(fb.sum())
    return _EXC[(case, k)]


def _run(env):
    if env not in _RUNS:
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(ENVS[env])
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "out.npz")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=e, capture_output=True, text=True)
            assert p.returncode == 0, f"child ({env}) exit {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
            with np.load(path) as z:
                _RUNS[env] = {k: z[k] for k in z.files}
    return _RUNS[env]


def _cpu(name):
    """CpuHeatmap's result after every batch of the case (computed once)"""
    if name not in _CPU:
        from oracle.heatmap_cpu import CpuHeatmap
        cpu = CpuHeatmap(h3_res=9, threads=4)
        batches = [_stage_input()] if name == "stage" else _cases()[name][2]
        _CPU[name] = [cpu.process_batch(**b) for b in batches]
        cpu.close()
    return _CPU[name]


def _close(a, b):
    return (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= np.maximum(REL * np.maximum(np.abs(a), np.abs(b)), ABS_DEG))


def _assert_tiles_match_cpu(got, exp, what):
    t = exp["tiles"]
    order = np.lexsort((t["window_start_us"], t["cell"]))
    assert np.array_equal(got["cell"], t["cell"][order]) and np.array_equal(got["window_start_us"], t["window_start_us"][order]), \
        f"{what}: key sets differ ({got['cell'].size} tiles, the CPU's {t['cell'].size})"
    assert np.array_equal(got["count"], t["count"][order]), f"{what}: counts differ"
    assert np.array_equal(got["speed_null"].astype(bool), t["speed_null"][order].astype(bool)), f"{what}: null speeds differ"
    live = ~got["speed_null"].astype(bool)
    assert _close(got["avg_speed"][live], t["avg_speed"][order][live]).all(), f"{what}: avg_speed"
    assert _close(got["avg_lat"], t["avg_lat"][order]).all() and _close(got["avg_lon"], t["avg_lon"][order]).all(), f"{what}: centroid"


CASES = ("sizes", "all_invalid", "all_late", "one_cell", "two_cells", "edge_mix", "thousands")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("env", BINNED_ENVS)
def test_against_cpu(env, case):
    run, exps = _run(env), _cpu(case)
    _, overflows, batches = _cases()[case]
    for k, (b, exp) in enumerate(zip(batches, exps)):
        what = f"{env}, {case}, batch {k} of {b['lat'].size} rows"
        got = {f: run[f"{case}/{k}/{f}"] for f in FIELDS}
        _assert_tiles_match_cpu(got, exp, what)
        assert np.array_equal(run[f"{case}/{k}/latest"], np.sort(exp["latest_rows"])), f"{what}: latest rows"
        n_valid, n_late, n_state, binned, direct = run[f"{case}/{k}/counts"]
        n_agg = exp["n_valid"] - exp["n_late"]
        print(f"{what}: {direct} of {n_agg} aggregated rows stored by their producer waves")
        if env in ALL_DIRECT and case == "edge_mix":
            # (knife-edge points: the host's count of margin exceptions need not be the device's to the last row)
            assert 0 < direct <= n_agg, f"{what}: {direct} records stored directly"
        elif env in ALL_DIRECT:   # (every valid row of these batches is aggregated, or none is)
            assert direct == (n_agg - _exceptions(case, k) if n_agg else 0), f"{what}: {direct} records stored directly"
        elif env in NONE_DIRECT:
            assert direct == 0, f"{what}: {direct} records stored directly"
        else:
            assert 0 <= direct <= n_agg, f"{what}: {direct} records stored directly"
        assert (n_valid, n_late, n_state) == (exp["n_valid"], exp["n_late"], exp["n_state"]), what
        # the batch was binned in k_ingest, unless a slab overflowed and it was partitioned from its keys again (slabs
        # of 16 records overflow in other cases too, wherever a bin gets a 17th row: only the overflow is pinned there)
        if overflows or env != "small_slabs":
            assert bool(binned) == (not overflows), f"{what}: binned {binned}"
    if case == "all_invalid":
        assert exps[0]["n_valid"] == 0 and exps[0]["tiles"]["cell"].size == 0
    if case == "all_late":
        assert exps[-1]["n_late"] == exps[-1]["n_valid"] == 2000


@pytest.mark.parametrize("case", [c for c in CASES if c != "edge_mix"])
@pytest.mark.parametrize("env", BINNED_ENVS)
def test_bitwise_against_direct(env, case):
    run, ref = _run(env), _run("direct")
    for k in range(len(_cases()[case][2])):
        for f in FIELDS + ("latest",):
            a, b = run[f"{case}/{k}/{f}"], ref[f"{case}/{k}/{f}"]
            if a.dtype == np.float64:
                a, b = a.view(np.uint64), b.view(np.uint64)
            assert np.array_equal(a, b), f"{env}, {case}, batch {k}: {f} differs from the direct path's"
        assert np.array_equal(run[f"{case}/{k}/counts"][:3], ref[f"{case}/{k}/counts"][:3])


@pytest.mark.parametrize("env", BINNED_ENVS)
def test_stage_batch(env):
    """one batch of two ranks through the stage API (its senders bin in whole bins): the owners' tiles together are the
    CPU's, the ranks' latest rows together the CPU's"""
    run, exp = _run(env), _cpu("stage")[0]
    got = {f: np.concatenate([run[f"stage{r}/0/{f}"] for r in range(2)]) for f in FIELDS}
    order = np.lexsort((got["window_start_us"], got["cell"]))
    _assert_tiles_match_cpu({f: v[order] for f, v in got.items()}, exp, f"{env}, stage")
    rows = np.sort(np.concatenate([run[f"stage{r}/0/latest"] for r in range(2)]))
    assert np.array_equal(rows, np.sort(exp["latest_rows"]))


if __name__ == "__main__":
    _child(sys.argv[1])
