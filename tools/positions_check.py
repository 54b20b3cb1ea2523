#!/usr/bin/env python3
"""Times the positions fold (hm_positions_update) at config C5's cardinality against what a user had before it for the
same answer: the batch's latest rows copied to the host and folded there in numpy.

Shape: --vehicles (1e7) vehicles under one provider, --updates (2) rows per vehicle and batch with distinct timestamps
(synth.c5_dedup's shape with fewer updates per vehicle: the fold sees one latest row per vehicle either way), generated on
the device; every batch hands in the 1e7 vehicleId strings in another order, so the same vehicle has another code -- and
another vkey -- in every batch.  --batches (5): batch 0 inserts every vehicle, the later ones update every vehicle.

Device time = the library's own HIP events around the call's stream work (hm_positions_info [8]: dictionaries' upload
included; [9]: from the first kernel on).  Batch 0 is reported alone; of the update batches the first is the warm-up
and the median of the rest is reported.  hm_positions_export: one warm-up, the median of --reps host-clocked calls that
end in a stream synchronisation.  Host fold: the latest rows' vkey / ts / lat / lon copied to the host (timed) and folded
in numpy by vehicle string (searchsorted on the sorted strings, first row per vehicle, strictly newer ts); its state
must equal the export.  bytes_per_row: what the two passes must move per latest row (rows 8 + vkey 8 + ts 8, the slot
32, candidate 4 + 4, slot_of 4 + 4, rows 8 + ts 8 + lat 8 + lon 8, the slot back 32, candidate 4 = 148 B) plus per
dictionary entry (offsets 8, ~W string bytes up and read, its slot 24, the code 4).

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
W = 12   # bytes per vehicleId: "v" + 11 digits


def vehicle_bytes(nv):
    """[nv, W] uint8: the vehicleId strings "v00000000000" ... by persistent id"""
    d = np.empty((nv, W), np.uint8)
    d[:, 0] = ord("v")
    x = np.arange(nv, dtype=np.int64)
    for k in range(W - 1, 0, -1):
        d[:, k] = 48 + x % 10
        x //= 10
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vehicles", type=int, default=10_000_000)
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("positions_check.py needs the GPU")
    import mobheat
    from mobheat import _lib
    dev = torch.device("cuda:0")
    nv, n = args.vehicles, args.vehicles * args.updates
    strings = vehicle_bytes(nv)
    offs = np.arange(nv + 1, dtype=np.int64) * W
    rng = np.random.default_rng(args.seed)
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, batch_capacity_hint=n)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    # the host fold's state, by persistent id (the strings are sorted by id: searchsorted finds it)
    sorted_strings = strings.view(f"S{W}").ravel()
    h_ts = np.full(nv, np.iinfo(np.int64).min)
    h_seen = np.zeros(nv, bool)
    h_lat, h_lon = np.zeros(nv), np.zeros(nv)
    dev_us, kern_us, host_fold_ms, d2h_ms = [], [], [], []
    for e in range(args.batches):
        code_of_id = rng.permutation(nv)                   # this batch's code of every vehicle
        id_of_code = np.argsort(code_of_id)
        vb = np.ascontiguousarray(strings[id_of_code]).ravel()
        ids = torch.arange(nv, device=dev, dtype=torch.int64).repeat(args.updates)[torch.randperm(n, generator=g, device=dev)]
        vkey = torch.from_numpy(code_of_id).to(dev)[ids].contiguous()
        ts = T0 + e * 60_000_000 + torch.randint(0, 50_000_000, (n,), generator=g, device=dev, dtype=torch.int64)
        lat = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 0.25 + 42.20
        lon = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 0.25 - 71.20
        speed = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 80.0
        sv = torch.ones(n, dtype=torch.uint8, device=dev)
        out = eng.process_batch_device(e, n, lat.data_ptr(), lon.data_ptr(), ts.data_ptr(), speed.data_ptr(), sv.data_ptr(),
                                       vkey.data_ptr(), sv.data_ptr())
        m = int(out.n_latest)
        eng.update_positions((1, np.array([0, 4], np.int64), np.frombuffer(b"mbta", np.uint8).copy()), (nv, offs, vb))
        info = eng.positions_info()
        dev_us.append(info["update_us"])
        kern_us.append(info["update_kernels_us"])
        # the alternative: the latest rows to the host, folded there
        t = time.perf_counter()
        rows_d = torch.empty(m, dtype=torch.int64, device=dev)
        _lib.check(eng._lib.hm_memcpy(rows_d.data_ptr(), out.latest_row, m * 8, 2), None, "hm_memcpy")
        h_vk, h_t = vkey[rows_d].cpu().numpy(), ts[rows_d].cpu().numpy()
        h_la, h_lo = lat[rows_d].cpu().numpy(), lon[rows_d].cpu().numpy()
        torch.cuda.synchronize()
        d2h_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        batch_strings = vb.view(f"S{W}")
        pid = np.searchsorted(sorted_strings, batch_strings)[h_vk % nv]      # persistent id of every latest row
        u, first = np.unique(pid, return_index=True)                          # (rows ascending: the lowest row of a key)
        win = ~h_seen[u] | (h_t[first] > h_ts[u])
        u, first = u[win], first[win]
        h_ts[u], h_lat[u], h_lon[u], h_seen[u] = h_t[first], h_la[first], h_lo[first], True
        host_fold_ms.append((time.perf_counter() - t) * 1e3)
        del rows_d, ids, vkey, ts, lat, lon, speed, sv
    exp_ms = []
    for i in range(args.reps + 1):
        p, cnt, cfg = ctypes.c_void_p(), ctypes.c_int64(), _lib.HmPositionDocCfg()
        t = time.perf_counter()
        _lib.check(eng._lib.hm_positions_export(eng._ctx, _lib.HM_MEM_DEVICE, ctypes.byref(p), ctypes.byref(cnt), ctypes.byref(cfg)),
                   eng._ctx, "hm_positions_export")
        if i:
            exp_ms.append((time.perf_counter() - t) * 1e3)
    recs, providers, vehicles = eng.positions(strings=False)
    pid = np.searchsorted(sorted_strings, vehicles[2][:nv * W].view(f"S{W}"))[recs["vehicle"]]
    o = np.argsort(pid)
    same = bool(recs.size == nv and np.array_equal(pid[o], np.arange(nv)) and np.array_equal(recs["ts_us"][o], h_ts)
                and np.array_equal(recs["lat"][o], h_lat) and np.array_equal(recs["lon"][o], h_lon))
    upd = dev_us[2:] if len(dev_us) > 2 else dev_us[1:]
    updk = kern_us[2:] if len(kern_us) > 2 else kern_us[1:]
    hostf = [a + b for a, b in zip(d2h_ms, host_fold_ms)]
    row_bytes, entry_bytes = 148, 8 + 2 * W + 24 + 4
    med_k = statistics.median(updk)
    res = {"tool": "positions_check", "vehicles": nv, "rows_per_batch": n, "latest_rows_per_batch": nv, "batches": args.batches,
           "insert_batch_device_ms": round(dev_us[0] / 1e3, 3), "insert_batch_kernels_ms": round(kern_us[0] / 1e3, 3),
           "update_batch_device_ms": round(statistics.median(upd) / 1e3, 3), "update_batch_kernels_ms": round(med_k / 1e3, 3),
           "update_batch_device_ms_all": [round(x / 1e3, 3) for x in dev_us],
           "export_device_ms": round(statistics.median(exp_ms), 3),
           "host_fold_ms_insert": round(hostf[0], 1), "host_fold_ms_update": round(statistics.median(hostf[2:] or hostf[1:]), 1),
           "host_fold_d2h_ms": round(statistics.median(d2h_ms), 1),
           "host_over_device_update": round(statistics.median(hostf[2:] or hostf[1:]) / (statistics.median(upd) / 1e3), 1),
           "bytes_per_row": row_bytes, "bytes_per_dictionary_entry": entry_bytes,
           "update_kernels_gb_s": round((nv * row_bytes + nv * entry_bytes) / (med_k * 1e-6) / 1e9, 1),
           "info": info, "equal_to_host_fold": same}
    eng.close()
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
