#!/usr/bin/env python3
"""Times a live window's raster on the GPU (hm_window_raster: roll-up, k_raster, k_raster_exact, the copy back) against
the same job done by the entry points that existed before it, and compares the two grids for equality:

  composition   the grid's pixel centres materialised (numpy meshgrid), hm_latlng_to_cell over all of them (host arrays:
                two 8-byte columns up, one 8-byte column back), HeatmapEngine.window_records at the same resolution, and a
                numpy lookup of every pixel's cell in the sorted records (searchsorted), saturated to uint32

One window of --keys (1e6) events uniform on the sphere at res 8 (nearly as many tiles); the grid is the 16 x 16 block of
256-pixel tiles of zoom --zoom (4: the whole world, 4096 x 4096 pixels), rastered at each of --res (8: the window's own
keys, most pixels empty; 3: the roll-up, every pixel on a tile).  Per resolution: both medians of --reps after a warm-up,
their ratio, the raster's kernel time (HIP events, hm_raster_info), the pixels that took the exact path, and `equal`.

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


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--zoom", type=int, default=4)
    ap.add_argument("--block", type=int, default=16, help="tiles per side of the block (16: 4096 pixels per side)")
    ap.add_argument("--res", default="8,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raster_check.py needs the GPU")
    import mobheat
    from mobheat import readside
    rng = np.random.default_rng(args.seed)
    n = args.keys
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, batch_capacity_hint=n)
    eng.process_batch(0, lat=np.degrees(np.arcsin(rng.uniform(-1, 1, n))), lon=rng.uniform(-180, 180, n),
                      ts_us=T0 + rng.integers(0, 300_000_000, n), speed=rng.uniform(0, 90, n), speed_valid=rng.random(n) > 0.1,
                      vkey=rng.integers(0, 50_000, n).astype(np.uint64), row_valid=np.ones(n, bool))
    ws, keys = eng.live_windows()
    assert ws.size == 1
    x0 = y0 = (2 ** args.zoom - args.block) // 2   # the block in the middle of the map (zoom 4: all of it)
    lat = np.concatenate([readside.tile_grid(args.zoom, x0, y0 + k)[0] for k in range(args.block)])
    lon = np.concatenate([readside.tile_grid(args.zoom, x0 + k, y0)[1] for k in range(args.block)])
    out = {"tool": "raster_check", "tiles": int(keys[0]), "zoom": args.zoom, "rows": int(lat.size), "cols": int(lon.size),
           "reps": args.reps, "res": {}}

    def composition(res):
        la, lo = np.meshgrid(lat, lon, indexing="ij")
        cells = mobheat.latlng_to_cell(la.ravel(), lo.ravel(), res)
        recs = eng.window_records(int(ws[0]), res, copy=False)
        order = np.argsort(recs["cell"])
        have = recs["cell"][order]
        at = np.minimum(np.searchsorted(have, cells), have.size - 1)
        cnt = np.where(have[at] == cells, recs["count"][order][at], 0)
        return np.minimum(cnt, 0xFFFFFFFF).astype(np.uint32).reshape(lat.size, lon.size)

    ok = True
    for res in (int(r) for r in args.res.split(",")):
        fused_ms, fused = timed(lambda: eng.window_raster(lat, lon, int(ws[0]), res, copy=False), args.reps)
        info = eng.raster_info()
        fused = fused.copy()
        comp_ms, comp = timed(lambda: composition(res), args.reps)
        equal = bool(np.array_equal(fused, comp))
        ok &= equal
        out["res"][str(res)] = {"records": info["records"], "nonzero_pixels": int(np.count_nonzero(fused)),
                                "exact_pixels": info["exact_pixels"], "raster_kernels_ms": round(info["kernel_us"] / 1e3, 3),
                                "raster_call_ms": round(fused_ms, 2), "composition_ms": round(comp_ms, 1),
                                "ratio": round(comp_ms / fused_ms, 1), "equal": equal}
    eng.close()
    out["equal"] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
