#!/usr/bin/env python3
"""Times the change between two live windows (hm_window_change, hm_window_change_top) against what the library offered
before it for the same answer: two window_records calls and a numpy join (readside.change_of) with a lexsort
(readside.change_top_of).

The state: bench.py's -- --events (1e8) events uniform on the sphere at res 8 over 15 minutes, one step; the two largest
live windows (~3.3e7 keys each).  The grid: resolutions 8, 5 and 0; orders none, rising at k = 100 and abs at k = 65536.
Per point one warm-up call, then the median of --reps (5) calls by a host clock around a call that leaves the pairs in
device memory and ends in a stream synchronisation (gpu_ms_device); hm_change_info's device time of the change's own
kernels (change_device_us); per resolution the time of the two hm_window_rollup(HM_MEM_DEVICE) calls the change contains
(rollups_ms: the join's own share is the difference), the host alternative (export_numpy_ms: two window_records calls,
change_of, and for a ranked point change_top_of) and the traffic floor (mA 192 + base table slots 64 + (mA + mB) 128
bytes at 8 TB/s).  Every point must equal the host join: every pair's cell, window starts, counts and n_speed, sorted by
cell or in rank order (two roll-ups of one window may add the sums in different orders).

Prints one JSON line.  Needs the GPU; there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-mobility-heatmap_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

POINTS = ((None, None), ("rising", 100), ("abs", 65536))
FIELDS = ("cell", "window_start_us", "count", "n_speed")
HBM_BYTES_PER_S = 8e12


def timed(fn, reps):
    ms, got = [], None
    for i in range(reps + 1):
        t = time.perf_counter()
        got = fn()
        if i:
            ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), got


def change_device(eng, wa, wb, res, order, k):
    """one call that leaves the pairs on the device: (pointer, n)"""
    from mobheat import _lib
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    if order is None:
        rc = eng._lib.hm_window_change(eng._ctx, wa, wb, res, None, _lib.HM_MEM_DEVICE, ctypes.byref(p), ctypes.byref(n))
    else:
        rc = eng._lib.hm_window_change_top(eng._ctx, wa, wb, res, None, _lib.change_order_code(order), k, _lib.HM_MEM_DEVICE,
                                           ctypes.byref(p), ctypes.byref(n))
    _lib.check(rc, eng._ctx, "hm_window_change")
    return p, n.value


def pairs_to_host(eng, p, n):
    from mobheat import _lib
    out = np.zeros(n, _lib.CHANGE_REC_DTYPE)
    if n:
        _lib.check(eng._lib.hm_memcpy(out.ctypes.data, p, out.nbytes, 1), None, "hm_memcpy")
    return out


def same_pairs(got, want):
    return bool(got.size == want.size and all(np.array_equal(got[h][f], want[h][f]) for h in ("cur", "base") for f in FIELDS))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "change", "change_check.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("change_check.py needs the GPU")
    import mobheat
    from mobheat import readside
    import rollup_check
    dev = torch.device("cuda:0")
    d = rollup_check.gen_batch(args.events, args.seed, dev)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, batch_capacity_hint=args.events)
    eng.process_batch_device(0, args.events, d["lat"].data_ptr(), d["lon"].data_ptr(), d["ts"].data_ptr(), d["speed"].data_ptr(),
                             d["sv"].data_ptr(), d["vkey"].data_ptr(), d["rv"].data_ptr())
    torch.cuda.synchronize()
    del d
    torch.cuda.empty_cache()
    wins, keys = eng.live_windows()
    top2 = np.sort(wins[np.argsort(keys)[-2:]])
    wb, wa = int(top2[0]), int(top2[1])
    out = {"tool": "change_check", "events": args.events, "reps": args.reps, "window_keys": [int(keys[wins == wa][0]), int(keys[wins == wb][0])],
           "cases": []}
    ok = True
    for res in (8, 5, 0):
        def rollups():
            rollup_check.rollup(eng, wa, res, mobheat._lib.HM_MEM_DEVICE)
            rollup_check.rollup(eng, wb, res, mobheat._lib.HM_MEM_DEVICE)
        rollups_ms, _ = timed(rollups, args.reps)

        def host_join():
            return readside.change_of(eng.window_records(wa, res, copy=False).copy(), eng.window_records(wb, res, copy=False), wa, wb)
        export_ms, want = timed(host_join, 1)
        for order, k in POINTS:
            gpu_ms, (p, n) = timed(lambda: change_device(eng, wa, wb, res, order, k), args.reps)
            info = eng.change_info()
            got = pairs_to_host(eng, p, n)
            if order is None:
                got, ref, host_ms = got[np.argsort(got["cur"]["cell"], kind="stable")], want, export_ms
            else:
                t = time.perf_counter()
                ref = readside.change_top_of(want, order, k)
                host_ms = export_ms + (time.perf_counter() - t) * 1e3
            same = same_pairs(got, ref)
            ok &= same
            m_a, m_b = int(info["cur_cells"]), int(info["base_cells"])
            slots = 1 << max(10, (2 * m_b - 1).bit_length()) if m_b else 0
            floor_ms = (m_a * 192 + slots * 64 + (m_a + m_b) * 128) / HBM_BYTES_PER_S * 1e3
            out["cases"].append({"res": res, "order": order, "k": k, "cur_cells": m_a, "base_cells": m_b, "both": int(info["both"]),
                                 "returned": n, "gpu_ms_device": round(gpu_ms, 3), "rollups_ms": round(rollups_ms, 3),
                                 "join_ms": round(gpu_ms - rollups_ms, 3), "change_device_us": int(info["device_us"]),
                                 "export_numpy_ms": round(host_ms, 1), "floor_ms": round(floor_ms, 3), "equal": same})
            print(f"res {res} {order} k {k}: gpu {gpu_ms:.3f} ms (roll-ups {rollups_ms:.3f} ms, own kernels {info['device_us']} us), "
                  f"host {host_ms:.1f} ms, floor {floor_ms:.3f} ms, equal {same}", file=sys.stderr, flush=True)
            del got, ref
        del want
    eng.close()
    out["equal"] = ok
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
