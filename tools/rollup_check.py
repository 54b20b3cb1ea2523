#!/usr/bin/env python3
"""Times the window roll-up (hm_window_rollup) on the bench's state against what the library offered before it for the
same answer: a checkpoint export of the whole state (export_state) followed by a numpy group-by on parent cells.

The state is bench.py's: --events (1e8) events uniform on the sphere at res 8 over 15 minutes of event time, generated on
the device as bench.py's gen_batch does, one step (three windows of ~3.3e7 keys).  The largest window is rolled up to
res 8, 7, 5, 3 and 0: one warm-up call, then the median of --reps (5) calls, each a host clock around a call that
ends in a stream synchronisation -- with the records left on the device (gpu_ms_device) and copied to pinned host
memory (gpu_ms_host: what a caller that wants them in numpy pays).  The older path: export_state() (one warm-up, the
median of --export-reps) plus one numpy group-by per resolution; its parents and total count must equal the roll-up's.
scan_floor_ms = the window table's slots x 64 B over the peak HBM bandwidth: the least a pass over the table can take.

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
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-mobility-heatmap_amd")]

import numpy as np  # noqa: E402

T0 = 1759572000 * 1_000_000
SPAN_US = 15 * 60 * 1_000_000
HBM_PEAK_GBS = 8000.0   # as bench.py


def parent_rule(c, r):
    return (c & ~np.uint64(0xF << 52)) | np.uint64(r << 52) | np.uint64((1 << 3 * (15 - r)) - 1)


def gen_batch(n, seed, dev):
    """bench.py's gen_batch, one step"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lat = torch.rad2deg(torch.asin(torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1))
    lon = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 360.0 - 180.0
    ts = T0 + torch.randint(0, SPAN_US, (n,), generator=g, device=dev, dtype=torch.int64)
    speed = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 80.0
    sv = (torch.rand(n, generator=g, device=dev) >= 0.10).to(torch.uint8)
    vkey = torch.randint(0, 50_000, (n,), generator=g, device=dev, dtype=torch.int64)
    rv = torch.ones(n, dtype=torch.uint8, device=dev)
    return dict(lat=lat, lon=lon, ts=ts, speed=speed, sv=sv, vkey=vkey, rv=rv)


def rollup(eng, ws, res, memory):
    """one hm_window_rollup call: (ms, records pointer, n)"""
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    t = time.perf_counter()
    rc = eng._lib.hm_window_rollup(eng._ctx, int(ws), int(res), memory, ctypes.byref(p), ctypes.byref(n))
    ms = (time.perf_counter() - t) * 1e3
    from mobheat._lib import check
    check(rc, eng._ctx, "hm_window_rollup")
    return ms, p.value, int(n.value)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--targets", type=int, nargs="+", default=[8, 7, 5, 3, 0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--export-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollup_check.py needs the GPU")
    import mobheat
    from mobheat._lib import HM_MEM_DEVICE, HM_MEM_HOST, STATE_REC_DTYPE
    dev = torch.device("cuda:0")
    n = args.events
    d = gen_batch(n, args.seed, dev)
    eng = mobheat.HeatmapEngine(h3_res=args.res, device=0, batch_capacity_hint=n)
    eng.process_batch_device(0, n, d["lat"].data_ptr(), d["lon"].data_ptr(), d["ts"].data_ptr(), d["speed"].data_ptr(),
                             d["sv"].data_ptr(), d["vkey"].data_ptr(), d["rv"].data_ptr())
    torch.cuda.synchronize()
    del d
    torch.cuda.empty_cache()
    wins, keys = eng.live_windows()
    k = int(np.argmax(keys))
    ws, nkeys = int(wins[k]), int(keys[k])
    slots = 1 << max(int(2 * nkeys - 1).bit_length(), 10)   # the library's tables: a power of two at load <= 1/2
    out = {"tool": "rollup_check", "events": n, "h3_res": args.res, "live_windows": int(wins.size),
           "state_keys": int(keys.sum()), "window_start_us": ws, "keys_in": nkeys, "table_slots": slots,
           "scan_floor_ms": round(slots * 64 / (HBM_PEAK_GBS * 1e9) * 1e3, 3), "reps": args.reps, "rollup": {}}

    # the older path's first half: the whole state exported to the host
    exp_ms, recs = [], None
    for i in range(args.export_reps + 1):
        recs = None
        t = time.perf_counter()
        _, recs = eng.export_state()
        if i:
            exp_ms.append((time.perf_counter() - t) * 1e3)
    out["export_state_ms"] = round(statistics.median(exp_ms), 1)
    t = time.perf_counter()
    own = recs[recs["window_start_us"] == ws]
    select_ms = (time.perf_counter() - t) * 1e3
    del recs
    assert own.size == nkeys

    ok = True
    for r in args.targets:
        dev_ms, host_ms, m = [], [], 0
        for i in range(args.reps + 1):
            ms, _, m = rollup(eng, ws, r, HM_MEM_DEVICE)
            if i:
                dev_ms.append(ms)
        for i in range(args.reps + 1):
            ms, p, m = rollup(eng, ws, r, HM_MEM_HOST)
            if i:
                host_ms.append(ms)
        got = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)),
                                    shape=(m * STATE_REC_DTYPE.itemsize,)).view(STATE_REC_DTYPE)
        t = time.perf_counter()
        u, inv = np.unique(parent_rule(own["cell"], r), return_inverse=True)
        cnt = np.zeros(u.size, np.int64)
        np.add.at(cnt, inv, own["count"])
        nsp = np.zeros(u.size, np.int64)
        np.add.at(nsp, inv, own["n_speed"])
        sums = [np.bincount(inv, weights=own[f], minlength=u.size) for f in ("sum_speed", "sum_lat", "sum_lon")]
        group_ms = (time.perf_counter() - t) * 1e3
        o = np.argsort(got["cell"])
        same = bool(m == u.size and np.array_equal(got["cell"][o], u) and np.array_equal(got["count"][o], cnt)
                    and np.array_equal(got["n_speed"][o], nsp)
                    and np.allclose(got["sum_lat"][o], sums[1], rtol=1e-9, atol=1e-9 * float(cnt.max())))
        ok &= same
        older = out["export_state_ms"] + select_ms + group_ms
        g = statistics.median(host_ms)
        out["rollup"][str(r)] = {"parents_out": m, "gpu_ms_device": round(statistics.median(dev_ms), 3),
                                 "gpu_ms_host": round(g, 3), "gpu_ms_host_min_max": [round(min(host_ms), 3), round(max(host_ms), 3)],
                                 "export_numpy_ms": round(older, 1), "numpy_groupby_ms": round(select_ms + group_ms, 1),
                                 "speedup": round(older / g, 1), "equal_to_numpy": same}
    out["gpu_faster_at_every_resolution"] = all(v["gpu_ms_host"] < v["export_numpy_ms"] for v in out["rollup"].values())
    out["equal_to_numpy"] = ok
    eng.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
