"""GPU: bench.py --dump-outputs writes what a caller of the timed path receives.  The C1 batch (4,000 rows, two
windows) goes through hm_process_batch twice: from host columns with host outputs (the reference result here, whose
own parity with the oracle tests/test_gpu_parity.py holds), and from device columns with the rows left on the device, as
the bench's steps run it; bench.dump_outputs of the latter must hold the former -- every row when it fits, else exactly
the rows whose key the seeded hash selects."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["cell_hi", "cell_lo", "window_start_us", "count", "avg_speed", "speed_null", "avg_lon", "avg_lat",
         "latest_rows", "counts"]
# an average here is a sum of at most n = 4000 same-signed binary64 terms (atomic adds in any order) divided by the
# count: its relative error is below n * 2^-53 = 4.5e-13
RTOL = 1e-12


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def run(bench):
    """(the host-path result, the engine holding the device-path outputs, its HmBatchOut, the device)"""
    import torch

    import mobheat
    from mobheat import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    b = synth.c1_boston(n=4000)
    ref_eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    ref = ref_eng.process_batch(0, **b)
    ref_eng.close()
    d = dict(lat=torch.from_numpy(b["lat"]).to(dev), lon=torch.from_numpy(b["lon"]).to(dev),
             ts_us=torch.from_numpy(b["ts_us"].astype(np.int64)).to(dev), speed=torch.from_numpy(b["speed"]).to(dev),
             speed_valid=torch.from_numpy(b["speed_valid"].astype(np.uint8)).to(dev),
             vkey=torch.from_numpy(b["vkey"].astype(np.int64)).to(dev),
             row_valid=torch.from_numpy(b["row_valid"].astype(np.uint8)).to(dev))
    torch.cuda.synchronize()
    eng = mobheat.HeatmapEngine(h3_res=8, device=0)
    out = eng.process_batch_device(0, n=b["lat"].size, **{k: v.data_ptr() for k, v in d.items()})
    torch.cuda.synchronize()
    yield ref, eng, out, dev
    eng.close()
    del d


def _load(path):
    got = {f: np.load(os.path.join(path, f + ".npy")) for f in FILES}
    assert sorted(os.listdir(path)) == sorted(f + ".npy" for f in FILES)
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in got.values())
    return got


def _check_rows(got, ref, sel):
    """got's tile rows are ref's rows `sel`, sorted by (window start, cell)."""
    t = ref.tiles
    order = sel[np.lexsort((t.cell[sel], t.window_start_us[sel]))]
    cell = (got["cell_hi"].astype(np.uint64) << np.uint64(32)) | got["cell_lo"].astype(np.uint64)
    assert np.array_equal(cell, t.cell[order])
    assert np.array_equal(got["window_start_us"], t.window_start_us[order].astype(np.float64))
    assert np.array_equal(got["count"], t.count[order].astype(np.float64))
    assert np.array_equal(got["speed_null"], t.speed_null[order].astype(np.float64))
    for f in ("avg_speed", "avg_lon", "avg_lat"):
        np.testing.assert_allclose(got[f], getattr(t, f)[order], rtol=RTOL, atol=0)


def test_dump_outputs_holds_every_row_of_a_small_batch(bench, run, tmp_path):
    ref, eng, out, dev = run
    assert len(ref.tiles) > 1 and np.unique(ref.tiles.window_start_us).size == 2
    bench.dump_outputs(str(tmp_path / "dump"), out, dev)
    got = _load(str(tmp_path / "dump"))
    _check_rows(got, ref, np.arange(len(ref.tiles)))
    assert np.array_equal(got["latest_rows"], np.sort(ref.latest_rows).astype(np.float64))
    assert got["counts"].tolist() == [len(ref.tiles), ref.latest_rows.size, ref.n_in, ref.n_valid, ref.n_late, ref.n_state,
                                      ref.batch_max_event_ms, ref.watermark_ms, ref.late_watermark_ms, ref.n_partials,
                                      0, 0]


def test_a_run_of_more_steps_than_timestamp_buffers_computes_the_same(bench, tmp_path, monkeypatch, capsys):
    """bench.py keeps at most TS_POOL steps' timestamps resident and advances a buffer to a later step once its step is
    over: the last of 6 steps returns the same rows from 2 buffers as from one buffer per step (20,000 events: a tile
    holds a few events at most, so its averages agree to a few ulps whatever the order of the atomic adds)."""
    import json
    got = {}
    for pool in (2, bench.TS_POOL):
        monkeypatch.setattr(bench, "TS_POOL", pool)
        monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--events", "20000",
                                         "--dump-outputs", str(tmp_path / str(pool))])
        bench.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["steps"] == 4 and line["ms_per_step"] > 0 and "state_read_leg" not in line and "cpu_baseline" not in line
        got[pool] = _load(str(tmp_path / str(pool)))
    a, b = got[2], got[bench.TS_POOL]
    assert a["counts"][0] > 0 and a["window_start_us"].min() >= bench.T0 + 5 * bench.SPAN_US   # the sixth step's windows
    for f in FILES:
        if f.startswith("avg_"):
            np.testing.assert_allclose(a[f], b[f], rtol=RTOL, atol=0)
        else:
            assert np.array_equal(a[f], b[f]), f


def test_dump_outputs_samples_by_key_over_the_size_limit(bench, run, tmp_path, monkeypatch):
    import torch
    ref, eng, out, dev = run
    t = ref.tiles
    monkeypatch.setattr(bench, "DUMP_TILE_BYTES", len(t) * 64 // 5)      # room for less than a fifth of the rows
    monkeypatch.setattr(bench, "DUMP_LATEST_BYTES", ref.latest_rows.size * 8 // 3)
    bench.dump_outputs(str(tmp_path / "dump"), out, dev)
    got = _load(str(tmp_path / "dump"))
    kt, kl = int(got["counts"][10]), int(got["counts"][11])
    assert kt == 3 and kl == 2
    h = bench._sample_hash(torch.from_numpy(t.cell.astype(np.int64)), torch.from_numpy(t.window_start_us)).numpy()
    sel = np.nonzero(h < (1 << (24 - kt)))[0]
    assert 0 < sel.size and got["cell_hi"].size * 64 <= len(t) * 64 // 5
    _check_rows(got, ref, sel)
    rows = np.sort(ref.latest_rows)
    keep = bench._sample_hash(torch.from_numpy(rows)).numpy() < (1 << (24 - kl))
    assert np.array_equal(got["latest_rows"], rows[keep].astype(np.float64))
    assert got["latest_rows"].size * 8 <= ref.latest_rows.size * 8 // 3
