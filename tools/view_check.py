#!/usr/bin/env python3
"""Times the read side's GeoJSON bodies for a map viewport, filtered and encoded on the GPU (hm_window_geojson_view,
hm_positions_geojson_view), against the Python comparison path for the same bytes: readside.tiles_latest_from_engine /
positions_latest_from_engine with view=..., which build every feature and then filter, followed by json.dumps.

One window of --keys (1e6) events uniform on the sphere at res 8 (nearly as many tiles) and --vehicles (1e6) vehicles
uniform on the sphere, under four views: a city (0.25 x 0.25 degrees), about a tenth of the sphere, the whole world, and
a box across the antimeridian.  Per view and endpoint: the kept count, the body's bytes, the filter kernel's time (HIP
events, hm_geojson_info), the whole call's median of --reps, the Python path's time, and whether the two bodies hold the
same features (parsed, sorted by cellId / (provider, vehicleId), dumped again and compared).  unfiltered_*: the call
without a view, on the same engine.

Prints one JSON line.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-mobility-heatmap_amd")]

import numpy as np  # noqa: E402

T0 = 1759572000 * 1_000_000
VIEWS = {
    "city": (-71.25, 42.2, -71.0, 42.45),
    "tenth": (-36.0, -30.0, 36.0, 30.0),      # (sin 30 - sin -30) / 2 x 72 / 360 = 0.1 of the sphere
    "world": (-180.0, -90.0, 180.0, 90.0),
    "antimeridian": (170.0, -30.0, -170.0, 30.0),
}


def dumps(o):
    return json.dumps(o, separators=(",", ":"))


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), out


def same_features(gpu_body, py_collection, key):
    got = sorted(json.loads(gpu_body)["features"], key=key)
    exp = sorted(py_collection["features"], key=key)
    return len(got) == len(exp) and all(dumps(g) == dumps(e) for g, e in zip(got, exp))


def measure(eng, reps, gpu_body, py_collection, key, skip_python):
    out = {}
    for name, view in VIEWS.items():
        ms, body = timed(lambda: gpu_body(view), reps)
        info = eng.geojson_info()
        r = {"kept": None, "candidates": info["candidates"], "body_bytes": len(body), "view_kernel_ms": round(info["view_kernel_us"] / 1e3, 3),
             "gpu_call_ms": round(ms, 2)}
        if skip_python:
            r["kept"] = len(json.loads(body)["features"])
        else:
            t = time.perf_counter()
            fc = py_collection(view)
            py = dumps(fc)
            r["python_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            r["kept"] = len(fc["features"])
            r["equal"] = bool(same_features(body, fc, key) and len(py) == len(body))
            del fc, py
        out[name] = r
    ms, body = timed(lambda: gpu_body(None), reps)
    out["unfiltered_call_ms"], out["unfiltered_bytes"] = round(ms, 2), len(body)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--skip-python", action="store_true", help="GPU timings only (no comparison)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_check.py needs the GPU")
    import mobheat
    from mobheat import readside
    rng = np.random.default_rng(args.seed)
    out = {"tool": "view_check", "h3_res": args.res, "reps": args.reps, "views": {k: list(v) for k, v in VIEWS.items()}}

    n = args.keys
    eng = mobheat.HeatmapEngine(h3_res=args.res, device=0, batch_capacity_hint=max(n, args.vehicles))
    eng.process_batch(0, lat=np.degrees(np.arcsin(rng.uniform(-1, 1, n))), lon=rng.uniform(-180, 180, n),
                      ts_us=T0 + rng.integers(0, 300_000_000, n), speed=rng.uniform(0, 90, n), speed_valid=rng.random(n) > 0.1,
                      vkey=rng.integers(0, 50_000, n).astype(np.uint64), row_valid=np.ones(n, bool))
    assert eng.live_windows()[0].size == 1
    out["tiles"] = measure(eng, args.reps, lambda v: readside.tiles_latest_body(eng, args.res, view=v),
                           lambda v: readside.tiles_latest_from_engine(eng, args.res, view=v),
                           lambda f: f["properties"]["cellId"], args.skip_python)

    m = args.vehicles
    vehicles = [f"veh-{k:07d}" for k in range(m)]
    providers = ["mbta", "é-bus"]
    pc = rng.integers(0, 2, m)
    eng.process_batch(1, lat=np.degrees(np.arcsin(rng.uniform(-1, 1, m))), lon=rng.uniform(-180, 180, m),
                      ts_us=T0 + 600_000_000 + rng.integers(0, 3_000_000_000, m), speed=np.zeros(m), speed_valid=np.ones(m, bool),
                      vkey=(pc * m + np.arange(m)).astype(np.uint64), row_valid=np.ones(m, bool))
    eng.update_positions(providers, vehicles)
    out["positions"] = measure(eng, args.reps, lambda v: readside.positions_latest_body(eng, view=v),
                               lambda v: readside.positions_latest_from_engine(eng, view=v),
                               lambda f: (f["properties"]["provider"], f["properties"]["vehicleId"]), args.skip_python)
    eng.close()
    ok = args.skip_python or all(out[k][v]["equal"] for k in ("tiles", "positions") for v in VIEWS)
    out["equal"] = None if args.skip_python else bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
