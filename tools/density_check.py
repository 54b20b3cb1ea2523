#!/usr/bin/env python3
"""Times the positions density (hm_positions_density) against what the library offered before it for the same answer:
an export of the positions state (positions()), hm_latlng_to_cell on its coordinates and a numpy group-by.

The state: --vehicles (1e7) vehicles restored through import_positions in three shapes -- "city" (a 50 x 50 km box),
"sphere" (uniform on the sphere) and "point" (every vehicle at one point: one group at every resolution, the worst case
of a group-by's contention).  For res 15, 8, 3 and 0: one warm-up call, then the median of --reps (5) calls, each a host
clock around a call that ends in a stream synchronisation, records copied to pinned host memory; the host path once per
resolution on the same box in the same run (the export timed once: it does not depend on the resolution).  Cells, counts
and the newest ts must be equal.  positions_density_info() of each shape's last call is printed with the times.

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


def shape_coords(shape, n, rng):
    if shape == "city":
        return rng.uniform(37.75, 38.20, n), rng.uniform(23.45, 24.00, n)
    if shape == "sphere":
        return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)
    if shape == "point":
        return np.full(n, 42.3601), np.full(n, -71.0589)
    raise SystemExit(f"unknown shape {shape}")


def dictionaries(n):
    """one provider and n vehicles of 8 bytes each as (n, offsets, bytes)"""
    digits = np.zeros((n, 8), np.uint8)
    digits[:, 0] = ord("v")
    k = np.arange(n)
    for d in range(7):
        digits[:, 7 - d] = ord("0") + (k // 10 ** d) % 10
    return ((1, np.array([0, 1], np.int64), np.frombuffer(b"p", np.uint8).copy()),
            (n, np.arange(n + 1, dtype=np.int64) * 8, digits.reshape(-1)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vehicles", type=int, default=10_000_000)
    ap.add_argument("--shapes", nargs="+", default=["city", "sphere", "point"])
    ap.add_argument("--targets", type=int, nargs="+", default=[15, 8, 3, 0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import mobheat
    from mobheat._lib import POSITION_REC_DTYPE
    n = args.vehicles
    if n > 9_999_999 + 1:
        raise SystemExit("at most 1e7 vehicles (7-digit ids)")
    out = {"tool": "density_check", "vehicles": n, "reps": args.reps, "shapes": {}}
    ok = True
    prov, veh = dictionaries(n)
    for shape in args.shapes:
        rng = np.random.default_rng(args.seed)
        recs = np.zeros(n, POSITION_REC_DTYPE)
        recs["vehicle"] = np.arange(n)
        recs["lat"], recs["lon"] = shape_coords(shape, n, rng)
        recs["ts_us"] = T0 + rng.integers(0, 3600 * 1_000_000, n)
        eng = mobheat.HeatmapEngine(h3_res=8, device=0)
        eng.import_positions(recs, prov, veh)
        del recs
        t = time.perf_counter()
        pos = eng.positions(strings=False)[0]
        export_ms = (time.perf_counter() - t) * 1e3
        rows = {}
        for r in args.targets:
            ms = []
            for i in range(args.reps + 1):
                t = time.perf_counter()
                got = eng.positions_density(r, copy=False)
                if i:
                    ms.append((time.perf_counter() - t) * 1e3)
            got = got.copy()
            info = eng.positions_density_info()
            t = time.perf_counter()
            cells = mobheat.latlng_to_cell(pos["lat"], pos["lon"], r)
            snap_ms = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            u, inv = np.unique(cells, return_inverse=True)
            cnt = np.bincount(inv, minlength=u.size)
            newest = np.full(u.size, np.iinfo(np.int64).min, np.int64)
            np.maximum.at(newest, inv, pos["ts_us"])
            group_ms = (time.perf_counter() - t) * 1e3
            o = np.argsort(got["cell"])
            same = bool(got.size == u.size and np.array_equal(got["cell"][o], u) and np.array_equal(got["count"][o], cnt)
                        and np.array_equal(got["window_start_us"][o], newest))
            ok &= same
            g, host = statistics.median(ms), export_ms + snap_ms + group_ms
            rows[str(r)] = {"groups": int(got.size), "gpu_ms": round(g, 3), "gpu_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                            "device_us": int(info["device_us"]), "host_path_ms": round(host, 1), "export_ms": round(export_ms, 1),
                            "snap_ms": round(snap_ms, 1), "numpy_groupby_ms": round(group_ms, 1), "speedup": round(host / g, 1),
                            "equal_to_host_path": same, "info": {k: int(v) for k, v in info.items()}}
            print(f"{shape} res {r}: gpu {g:.3f} ms, host path {host:.1f} ms, equal {same}", file=sys.stderr, flush=True)
        out["shapes"][shape] = rows
        eng.close()
    out["equal_to_host_path"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
