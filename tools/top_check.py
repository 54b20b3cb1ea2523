#!/usr/bin/env python3
"""Times the top-k hotspots (hm_window_top, hm_positions_density_top) against what the library offered before them for
the same answer: the whole roll-up / density copied to the host (window_records / positions_density, the view by
readside.cells_in_view) and ranked in numpy (readside.top_of).

The window: bench.py's state -- --events (1e8) events uniform on the sphere at res 8 over 15 minutes, one step; the
largest window (~3.3e7 keys) at res 8 and --coarse (5), without a view and under --view.  The density: --vehicles (1e7)
vehicles uniform on the sphere at res 8 and 3, without a view and under --view.  Each at k = 1, 100 and 65536: one warm-up
call, then the median of --reps (3) calls, a host clock around a call that ends with the records in pinned host memory
(gpu_ms), hm_top_info's device time of the top's own kernels (top_device_us) and its passes; beside them the roll-up's /
density's own call without the top (base_ms: the floor the top sits on).  The host alternative once per (resolution,
view), one warm-up and the median of --reps: export + view + top_of (host_ms; it does not depend on k but for a slice).
Every case must equal the alternative's records in rank order (cell, count, n_speed and window_start_us; at a coarser
resolution two roll-ups may add the sums in different orders).  ordering_only_us: top_records of 65536 records with
k = 65536 -- no pass, so the key extraction, the compaction, the counting ranks and the scatter alone.

Prints one JSON line.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-mobility-heatmap_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

KS = (1, 100, 65536)
FIELDS = ("cell", "count", "n_speed", "window_start_us")


def timed(fn, reps):
    """(median ms of reps calls after one warm-up, the last result)"""
    ms, got = [], None
    for i in range(reps + 1):
        t = time.perf_counter()
        got = fn()
        if i:
            ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), got


def run_cases(eng, name, reps, base, top, rows):
    """base(view) -> every record (host); top(k, view) -> the ranked records (host).  Returns equality over the cases."""
    from mobheat import readside
    ok = True
    for view in rows["views"]:
        def host_path():
            recs = base(None)
            if view is not None:
                recs = recs[readside.cells_in_view(recs["cell"], view, eng.device)]
            return readside.top_of(recs, max(KS))
        host_ms, ranked = timed(host_path, reps)
        base_ms, _ = timed(lambda: base(view), reps)
        for k in KS:
            gpu_ms, got = timed(lambda: top(k, view), reps)
            info = eng.top_info()
            want = ranked[:k]
            same = bool(got.size == want.size and all(np.array_equal(got[f], want[f]) for f in FIELDS))
            ok &= same
            rows["cases"].append({"what": name, "view": view is not None, "k": k, "candidates": int(info["candidates"]),
                                  "returned": int(got.size), "gpu_ms": round(gpu_ms, 3), "base_ms": round(base_ms, 3),
                                  "top_device_us": int(info["device_us"]), "host_ms": round(host_ms, 1),
                                  "passes": [int(info["count_passes"]), int(info["cell_passes"]), int(info["index_passes"])],
                                  "tied": int(info["tied"]), "equal": same})
            print(f"{name} view {view is not None} k {k}: gpu {gpu_ms:.3f} ms (top {info['device_us']} us, base {base_ms:.3f} ms), "
                  f"host {host_ms:.1f} ms, equal {same}", file=sys.stderr, flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--vehicles", type=int, default=10_000_000)
    ap.add_argument("--coarse", type=int, default=5)
    ap.add_argument("--view", type=float, nargs=4, default=[-30.0, -30.0, 60.0, 60.0], metavar=("W", "S", "E", "N"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("top_check.py needs the GPU")
    import mobheat
    from mobheat._lib import POSITION_REC_DTYPE
    import density_check
    import rollup_check
    view = tuple(args.view)
    out = {"tool": "top_check", "events": args.events, "vehicles": args.vehicles, "reps": args.reps, "view": view, "views": [None, view],
           "cases": []}
    ok = True

    # ---- the window ----
    dev = torch.device("cuda:0")
    d = rollup_check.gen_batch(args.events, args.seed, dev)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, batch_capacity_hint=args.events)
    eng.process_batch_device(0, args.events, d["lat"].data_ptr(), d["lon"].data_ptr(), d["ts"].data_ptr(), d["speed"].data_ptr(),
                             d["sv"].data_ptr(), d["vkey"].data_ptr(), d["rv"].data_ptr())
    torch.cuda.synchronize()
    del d
    torch.cuda.empty_cache()
    wins, keys = eng.live_windows()
    ws = int(wins[int(np.argmax(keys))])
    out["window_keys"] = int(keys.max())
    for res in (8, args.coarse):
        # (the roll-up in view has no records-only entry point: its floor is timed without a view)
        good = run_cases(eng, f"window res {res}", args.reps, lambda v, res=res: eng.window_records(ws, res, copy=False),
                               lambda k, v, res=res: eng.window_top(k, ws, res, v, copy=False), out)
        ok &= good
    t_us = []
    some = eng.window_records(ws, 8)[:65536]
    for _ in range(args.reps + 1):
        eng.top_records(some, 65536)
        t_us.append(int(eng.top_info()["device_us"]))
    out["ordering_only_us"] = int(statistics.median(t_us[1:]))
    eng.close()

    # ---- the density ----
    n = args.vehicles
    rng = np.random.default_rng(args.seed)
    recs = np.zeros(n, POSITION_REC_DTYPE)
    recs["vehicle"] = np.arange(n)
    recs["lat"], recs["lon"] = density_check.shape_coords("sphere", n, rng)
    recs["ts_us"] = density_check.T0 + rng.integers(0, 3600 * 1_000_000, n)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    eng.import_positions(recs, *density_check.dictionaries(n))
    del recs
    for res in (8, 3):
        good = run_cases(eng, f"density res {res}", args.reps, lambda v, res=res: eng.positions_density(res, None, v, copy=False),
                            lambda k, v, res=res: eng.positions_density(res, None, v, copy=False, top=k), out)
        ok &= good
    eng.close()
    del out["views"]
    out["equal"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
