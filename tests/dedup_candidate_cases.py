"""Cases of the latest-position dedup that runs from k_ingest's candidate list (csrc/k_dedup.h: k_dedup_list, k_bm_*).

cases() -> {name: {"envs": (...), "batches": [...], "cand": [...]}}: the micro-batches of one engine, the environment
settings (ENVS) the case runs under, and per batch what hm_last_counts [19] (last_counts()["dedup_candidates"]) must
say: "list" (the list path ran: a count >= 0), "fallback" (-1: the dedup ran from the flags), or an exact count where
the inputs fix it whatever the order the GPU sees the rows in (equal ts: every valid row; one wave of one vkey).

Inputs are dyadic (multiples of 2^-10), so every fp64 sum is exact and the tiles compare with the project's helpers.
`python tests/dedup_candidate_cases.py` checks the cases against the oracle alone (check_cases): every batch with rows
has latest rows, and the cases meant to overflow their list exceed its room in a sequential scan in row order.  That
scan is no lower bound of what the GPU's racing pass marks: in the ascending cases a wave that raised the max before
another wave read it would take that wave's rows off the list.  Every wave reads the max before the cell computation
and raises it after, behind one workgroup barrier, so these cases overflow in practice; all_equal_small_list overflows
in any order (equal ts: every row is a candidate whatever was seen before it).
"""
import functools

import numpy as np

T0 = 1_759_572_000_000_000   # a 5-minute window start
MINUTE = 60_000_000
CAP = 64                     # MOBHEAT_TEST_CAND_CAP of the small-list settings
DENSE_BOUND = 1 << 24        # vkeys above it never use the dense dedup table
SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 4097)
BIG_N = (1 << 23) + 5        # host inputs: two H2D chunks, two k_ingest launches on one cursor

ENVS = {
    "binned": {"MOBHEAT_INGEST_MODE": "binned"},   # the writer-wave kernel at any size
    "direct": {"MOBHEAT_INGEST_MODE": "direct"},   # k_ingest<false>
    "binned_cap": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_CAND_CAP": str(CAP)},
    "direct_cap": {"MOBHEAT_INGEST_MODE": "direct", "MOBHEAT_TEST_CAND_CAP": str(CAP)},
    "fused": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_INGEST_WRITERS": "0"},
    "one_workgroup": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_TEST_INGEST_GRID": "1"},
    "pipeline": {"MOBHEAT_INGEST_MODE": "binned", "MOBHEAT_PIPELINE": "2"},
    "default": {},
    "stage": {},   # the stage API at world 1 against one engine (the child compares them)
}
KNOBS = ("MOBHEAT_INGEST_MODE", "MOBHEAT_TEST_CAND_CAP", "MOBHEAT_TEST_INGEST_GRID", "MOBHEAT_PIPELINE",
         "MOBHEAT_INGEST_WRITERS", "MOBHEAT_DEDUP_STREAM", "MOBHEAT_DEDUP_EARLY", "MOBHEAT_DEDUP_DENSE",
         "MOBHEAT_TEST_SLAB_CAP", "MOBHEAT_TEST_RING_CAP", "MOBHEAT_TEST_RING_POLLS", "MOBHEAT_SUBBINS",
         "MOBHEAT_INGEST_WG_PER_CU")
BOTH = ("binned", "direct")
BOTH_CAP = ("binned_cap", "direct_cap")


def rows(rng, vkey, ts, cells=40):
    """a batch of vkey.size rows on a dyadic grid of about cells x cells res-9 cells"""
    n = int(np.asarray(vkey).size)
    lat = 37.5 + rng.integers(0, cells, n) * (4 / 1024) + rng.integers(0, 2, n) / 1024
    lon = 23.5 + rng.integers(0, cells, n) * (4 / 1024) + rng.integers(0, 2, n) / 1024
    return dict(lat=lat, lon=lon, ts_us=np.asarray(ts, np.int64).copy(), speed=rng.integers(0, 1 << 17, n) / 1024,
                speed_valid=rng.random(n) > 0.2, vkey=np.asarray(vkey, np.uint64).copy(), row_valid=np.ones(n, bool))


def _random(rng, n, n_vkeys, base=0, distinct_ts=50):
    """n rows of n_vkeys vehicles, ts among a few values (ties at the max are common)"""
    return rows(rng, base + rng.integers(0, n_vkeys, n), T0 + rng.integers(0, distinct_ts, n) * 1_000_000)


@functools.lru_cache(maxsize=None)
def _host_chunks():
    return [_random(np.random.default_rng(8801), BIG_N, 1000, distinct_ts=100_000)]


def batches(name):
    """the case's batches (the 2^23 + 5 rows of host_chunks only when asked for)"""
    b = cases()[name]["batches"]
    return b() if callable(b) else b


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(8800)
    out = {}

    def add(name, envs, batches, cand):
        assert callable(batches) or len(batches) == len(cand)
        out[name] = dict(envs=tuple(envs), batches=batches, cand=cand)

    # sizes around a bitmap word and a wave; the last row a winner of its own (the bit at n - 1), ties elsewhere
    for n in SIZES:
        b = _random(rng, n, 7)
        if n:
            b["vkey"][n - 1] = 99
            b["ts_us"][n - 1] = T0 + 200 * 1_000_000
        add(f"size_{n}", BOTH, [b], ["list"])
    one = np.zeros(4096, np.uint64) + 5
    asc = T0 + np.arange(4096, dtype=np.int64) * 1000
    add("ascending_small_list", BOTH_CAP, [rows(rng, one, asc)], ["fallback"])
    add("descending", BOTH, [rows(rng, one, asc[::-1])], ["list"])
    add("all_equal", BOTH, [rows(rng, rng.integers(0, 30, 4096), np.full(4096, T0 + 7_000_000))], [4096])
    # one wave of one vkey, ascending: its lanes read the max together, before any of them raises it -- every row a
    # candidate; a 65th row makes one more than the list of 64 holds
    add("all_equal_small_list", BOTH_CAP, [rows(rng, rng.integers(0, 30, 4096), np.full(4096, T0 + 9_000_000))], ["fallback"])
    add("at_cap", BOTH_CAP, [rows(rng, one[:CAP], asc[:CAP])], [CAP])
    add("cap_plus_1", BOTH_CAP, [rows(rng, one[:CAP + 1], asc[:CAP + 1])], ["fallback"])
    # vkeys above the dense bound: the hash table serves the list kernel; then dense and sparse ones in one batch (the
    # second batch: the context no longer keeps a dense table, every vkey in the hash table)
    add("sparse_vkeys", BOTH, [_random(rng, 3000, 200, base=DENSE_BOUND + 1)], ["list"])
    mix = [_random(rng, 3000, 150), _random(rng, 3000, 150)]
    for k, b in enumerate(mix):
        far = rng.random(3000) < 0.5
        b["vkey"][far] += np.uint64(DENSE_BOUND + (1 << 30))
        b["ts_us"] += k * MINUTE
    add("dense_and_sparse", BOTH, mix, ["list", "list"])
    # a second batch with late and invalid rows among the others (the watermark an hour ahead after two batches there)
    ahead = [_random(rng, 500, 20) for _ in range(2)]
    for b in ahead:
        b["ts_us"] += 60 * MINUTE
    late = _random(rng, 5000, 60)
    late["ts_us"][::3] += 60 * MINUTE              # (the others: late)
    late["row_valid"][1::7] = False
    late["lat"][5::11] = 95.0                      # (out of range: invalid)
    add("late_and_invalid", BOTH, ahead + [late], ["list", "list", "list"])
    # the list and the bitmap between batches: a batch that falls back, then one from the list, and the reverse
    small = _random(rng, 50, 9)
    add("fallback_then_list", BOTH_CAP, [rows(rng, one, asc), small], ["fallback", "list"])
    add("list_then_fallback", BOTH_CAP, [small, rows(rng, one, asc + MINUTE)], ["list", "fallback"])
    # the give-up rerun: after a small batch the fused table has 2^16 slots (host_ctx.h: dedup_fused_keys, 2^15 keys at
    # load 1/2); 70,000 distinct sparse vkeys cannot all find one, so the fused max gives up
    many = rows(rng, DENSE_BOUND + 1 + np.arange(80_000) % 70_000, T0 + rng.integers(0, 50, 80_000) * 1_000_000)
    add("give_up", BOTH, [_random(rng, 100, 10, base=DENSE_BOUND + 1), many], ["list", "fallback"])
    # one workgroup for 20,000 rows (many rounds of every wave), the same batch in two pipelined chunks, and through the
    # fused kernel
    add("many_rounds", ("one_workgroup", "pipeline", "fused"), [_random(rng, 20_000, 300, distinct_ts=4000)], ["list"])
    add("host_chunks", ("default",), _host_chunks, ["list"])
    add("stage_world_1", ("stage",), [_random(rng, 6000, 80), _random(rng, 6000, 80)], ["list", "list"])
    return out


def sequential_candidates(b):
    """rows a sequential scan in row order marks: ts >= the running max of the row's vkey (valid rows)"""
    ok = b["row_valid"].astype(bool) & (np.abs(b["lat"]) <= 90)
    best, cnt = {}, 0
    for v, t in zip(b["vkey"][ok].tolist(), b["ts_us"][ok].tolist()):
        if t >= best.get(v, -(1 << 63)):
            cnt += 1
            best[v] = t
    return cnt


def check_cases(oracle_factory):
    """the cases against the oracle alone; returns {name: [oracle result per batch]}"""
    res = {}
    for name, c in cases().items():
        if name == "host_chunks":   # (its oracle run is the GPU test's; here only its shape)
            assert batches(name)[0]["lat"].size == BIG_N and np.unique(batches(name)[0]["vkey"]).size == 1000
            continue
        cpu = oracle_factory()
        res[name] = [cpu.process_batch(**b) for b in c["batches"]]
        cpu.close()
        cap = CAP if c["envs"][0].endswith("_cap") else 65536
        for k, (b, exp, cand) in enumerate(zip(c["batches"], res[name], c["cand"])):
            what = f"{name}, batch {k}"
            assert (exp["latest_rows"].size > 0) == (b["lat"].size > 0), f"{what}: latest rows"
            seq = sequential_candidates(b)
            if cand == "fallback" and name != "give_up":
                assert seq > cap, f"{what}: {seq} sequential candidates do not overflow a list of {cap}"
            elif cand != "fallback":
                assert b["lat"].size <= cap or seq <= cap // 4, f"{what}: {seq} sequential candidates, list of {cap}"
            if isinstance(cand, int):
                assert cand == exp["n_valid"] <= cap, what
        if name == "late_and_invalid":
            assert 0 < res[name][-1]["n_late"] < res[name][-1]["n_valid"] < 5000, "late_and_invalid: no late or invalid rows"
        if name == "give_up":
            assert np.unique(c["batches"][1]["vkey"]).size == 70_000
    return res


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.heatmap_cpu import CpuHeatmap
    r = check_cases(lambda: CpuHeatmap(h3_res=9, threads=4))
    print(f"{len(r)} cases check against the oracle")
