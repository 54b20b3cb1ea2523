"""bench.py's host-side accounting (no GPU): the stage its roofline prices and the algorithmic bytes per stage
(DESIGN.md §5, §7)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dominant_stage_skips_the_concurrent_dedup():
    b = _bench()
    ms = {"ingest": 3.6, "aggregate": 0.08, "send": 0.0, "partition": 3.78, "merge": 3.84, "emit": 0.13, "dedup": 3.85}
    assert b.dominant_stage(ms) == "merge"           # the dedup's side-stream span is longer, but concurrent
    ms["partition"] = 3.9
    assert b.dominant_stage(ms) == "partition"
    assert "dedup" in b.CONCURRENT_STAGES


def test_stage_bytes_direct_path():
    b = _bench()
    n = 100_000_000
    c = {"partials": n, "tiles": 97_590_394, "state_new": 97_590_394, "table_mode": False, "sent": 0}
    s = b.stage_bytes(n, c)
    assert s["ingest"] == 42 * n
    # k_ev_hist reads the key (8); k_ev_scatter_rec reads key, speed, speed_valid, lat, lon (33) and writes 32
    assert s["partition"] == (8 + 33 + 32) * n
    assert s["merge"] == 32 * n + 113 * c["tiles"]   # no key existed before the batch
    assert s["emit"] == 98 * (n - c["tiles"])


def test_stage_bytes_multi_gpu_owner():
    b = _bench()
    n, R, S = 50_000_000, 49_000_000, 50_000_000
    c = {"partials": R, "tiles": R, "state_new": R, "table_mode": False, "sent": S}
    s = b.stage_bytes(n, c, world=2)
    # the sender's partition by region field (keys read twice; columns read, the 32-B record written), then each
    # record read from its bin and written into its destination's chunk; the owner merges without a partition
    assert s["partition"] == 16 * n + (25 + 32) * S
    assert s["send"] == (32 + 32) * S
    assert s["merge"] == 32 * R + 113 * R
    s = b.stage_bytes(n, dict(c, binned=1), world=2)
    assert s["partition"] == 0 and s["ingest"] == 43 * n + 32 * S and s["send"] == 64 * S


def test_full_and_dump_outputs_options(monkeypatch, capsys):
    """The command line has --full and --dump-outputs DIR."""
    import pytest
    monkeypatch.setattr("sys.argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        _bench().main()
    assert e.value.code == 0
    usage = capsys.readouterr().out
    assert "--full" in usage and "--dump-outputs DIR" in usage


def test_dump_sample_shift_keeps_the_sample_within_its_budget():
    b = _bench()
    assert b._sample_shift(4000, 64, b.DUMP_TILE_BYTES) == 0          # everything fits: every row
    assert b._sample_shift(0, 64, b.DUMP_TILE_BYTES) == 0
    n = 97_590_394                                                     # the bench's tiles per step
    k = b._sample_shift(n, 64, b.DUMP_TILE_BYTES)
    assert (n >> k) * 64 <= b.DUMP_TILE_BYTES * 7 // 8 < (n >> (k - 1)) * 64
    # all files together stay under 64 MB, with 1/8 of each budget left for the sample's own scatter
    assert b.DUMP_TILE_BYTES + b.DUMP_LATEST_BYTES + 12 * 8 + 10 * 128 < 64_000_000


def test_dump_sample_hash_depends_on_the_key_alone():
    """The sample of the tile rows is chosen by a hash of (cell, window start): the same keys whatever order the rows
    come in, and close to the fraction asked for on keys as regular as H3 indexes of one resolution are (their low 21
    bits all ones at res 8, three window starts)."""
    import numpy as np
    import torch
    b = _bench()
    n = 200_000
    rng = np.random.default_rng(5)
    cell = torch.from_numpy((0x0882A10000000000 + (rng.permutation(1 << 20)[:n].astype(np.int64) << 21)) | 0x1FFFFF)
    ws = torch.from_numpy(1759572000_000000 + 300_000_000 * rng.integers(0, 3, n))
    h = b._sample_hash(cell, ws)
    assert int(h.min()) >= 0 and int(h.max()) < 1 << 24
    p = torch.from_numpy(rng.permutation(n))
    assert torch.equal(b._sample_hash(cell[p], ws[p]), h[p])
    assert not torch.equal(b._sample_hash(cell, ws + 300_000_000), h)   # the window start is part of the key
    kept = int((h < (1 << 21)).sum())                                   # k = 3: one key in eight
    sd = (n * (1 / 8) * (7 / 8)) ** 0.5                                 # binomial; 5 sd: ~6e-7 two-sided
    assert abs(kept - n / 8) < 5 * sd, (kept, n / 8, sd)
    rows = torch.arange(n, dtype=torch.int64)                           # latest rows: hashed by the row index
    kept = int((b._sample_hash(rows) < (1 << 21)).sum())
    assert abs(kept - n / 8) < 5 * sd, (kept, n / 8, sd)


def test_stage_bytes_self_held_records():
    """The records of the bins a rank owns stay in its slabs (binned): only their keys are read (census), 8 B each;
    the bench's --sharded run prices the stage API at world 1 too."""
    b = _bench()
    n, S, H = 50_000_000, 50_000_000, 25_000_000
    c = {"partials": S, "tiles": S, "state_new": S, "table_mode": False, "sent": S, "binned": 1, "self_held": H}
    assert b.stage_bytes(n, c, world=2)["send"] == 64 * (S - H) + 8 * H
    c1 = dict(c, self_held=S)
    assert b.stage_bytes(n, c1, world=1, staged=True)["send"] == 8 * S
    assert b.stage_bytes(n, c1, world=1)["send"] == 0   # (hm_process_batch: no stage API)
