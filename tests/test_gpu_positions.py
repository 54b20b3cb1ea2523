"""GPU: every vehicle's latest position kept on the device across batches (hm_positions_*, k_positions.h).  Every case
compares the exported state, keyed by the (provider, vehicleId) string pair, with positions_ref.fold over each batch's
latest rows -- the plain-Python statement of the contract, which tests/test_positions_host.py ties to the reference's
own update statements.  ts equal, lat / lon bit-equal; no tolerance anywhere."""
import numpy as np
import pytest

from positions_ref import Batch, apply_ops, bits, exported, fold, run

pytestmark = pytest.mark.gpu
T0 = 1_759_572_000_000_000
SEC = 1_000_000


def _engine(hash_bits=None, **kw):
    import mobheat
    from mobheat import _lib
    eng = mobheat.HeatmapEngine(h3_res=8, device=0, **kw)
    if hash_bits is not None:
        _lib.check(eng._lib.hm_positions_debug_hash_bits(eng._ctx, hash_bits), eng._ctx, "hm_positions_debug_hash_bits")
    return eng


def _code(fn):
    from mobheat._lib import MobheatError
    with pytest.raises(MobheatError) as e:
        fn()
    return e.value.code


def _coords(rng, n):
    return rng.uniform(-80.0, 80.0, n), rng.uniform(-170.0, 170.0, n)


def case_one_batch(seed=5, n=1000, n_p=3, n_v=37):
    """1000 rows over 3 x 37 keys; ~10 % of the keys get a second and third row at their maximum with other lat / lon"""
    rng = np.random.default_rng(seed)
    lat, lon = _coords(rng, n)
    p, v = rng.integers(0, n_p, n), rng.integers(0, n_v, n)
    ts = T0 + rng.integers(0, 200, n) * SEC
    rows = [(f"prov{p[i]}", f"veh-{v[i]:03d}", int(ts[i]), lat[i], lon[i]) for i in range(n)]
    keys = sorted({(r[0], r[1]) for r in rows})
    for k in keys[::10]:
        top = max(r[2] for r in rows if (r[0], r[1]) == k)
        for _ in range(2):
            la, lo = _coords(rng, 1)
            rows.insert(int(rng.integers(0, len(rows))), (k[0], k[1], top, la[0], lo[0]))
    return [Batch(rows)]


def case_codes_move():
    """three batches over subsets of one set of strings in different orders: the same string gets another code each
    time and n_vehicles differs (12, 7, 9), so a vkey names another vehicle in every batch"""
    rng = np.random.default_rng(11)
    provs = ["p-east", "p-west", "p"]
    vehs = [f"bus{k}" for k in range(12)]
    out = []
    for b, (np_, nv) in enumerate(((3, 12), (2, 7), (3, 9))):
        po = list(rng.permutation(provs)[:np_])
        vo = list(rng.permutation(vehs)[:nv])
        n = 300
        lat, lon = _coords(rng, n)
        rows = [(po[int(rng.integers(0, np_))], vo[int(rng.integers(0, nv))], T0 + (b * 50 + int(rng.integers(0, 80))) * SEC,
                 lat[i], lon[i]) for i in range(n)]
        out.append(Batch(rows, p_order=po, v_order=vo))
    assert out[0].vehicles != out[1].vehicles[:len(out[0].vehicles)]
    return out


def case_strings():
    long_id = "L" * 299 + "x"
    keys = [("a", "bc"), ("ab", "c"), ("a", "b"), ("a", ""), ("", "a"), ("", ""), ("p1", "same"), ("p2", "same"),
            ("pre", "prefix"), ("pre", "pre"), ("pre", "p"), ("prefix", "pre"), ("é", "ü7"), ("日本", "バス12"),
            ("🚌", "🚍🚎"), ("agency", long_id), ("agency", long_id[:-1]), ("x", "y"), ("y", "x")]
    rng = np.random.default_rng(3)
    rows = []
    for rep in range(3):
        lat, lon = _coords(rng, len(keys))
        rows += [(p, v, T0 + int(rng.integers(0, 5)) * SEC, lat[i], lon[i]) for i, (p, v) in enumerate(keys)]
    return [Batch(rows)]


def _check_sequence(eng, batches, state=None, epoch0=0):
    state = {} if state is None else state
    for e, b in enumerate(batches):
        run(eng, epoch0 + e, b)
        fold(state, b.latest())
        assert exported(eng) == bits(state), f"batch {e}"
    return state


def test_one_batch_ties_resolve_to_the_lowest_row():
    eng = _engine()
    try:
        (b,) = case_one_batch()
        lat = b.latest()
        tied = len(lat) - len({(r[0], r[1]) for r in lat})
        assert tied >= 10   # (tied maxima with differing lat / lon are in the batch)
        state = _check_sequence(eng, [b])
        assert eng.positions_info()["keys"] == len(state) > 100
    finally:
        eng.close()


def test_identity_follows_the_strings_not_the_codes():
    eng = _engine()
    try:
        _check_sequence(eng, case_codes_move())
        assert eng.positions_info()["vehicles"] <= 12 and eng.positions_info()["providers"] == 3
    finally:
        eng.close()


def test_only_a_strictly_newer_ts_replaces():
    eng = _engine()
    try:
        first = Batch([("p", "v1", T0, 1.0, 2.0), ("p", "v2", -5, 3.0, 4.0), ("q", "v1", T0 + 9, 5.0, 6.0)])
        state = _check_sequence(eng, [first])
        stale = Batch([("q", "v1", T0 + 9, 50.0, 60.0), ("p", "v1", T0 - 1, 10.0, 20.0), ("p", "v2", -5, 30.0, 40.0),
                       ("p", "v2", -6, 31.0, 41.0)], v_order=["v2", "v1"])
        before = dict(state)
        _check_sequence(eng, [stale], state, 1)
        assert state == before
        newer = Batch([("p", "v2", -4, 7.0, 8.0), ("p", "v1", T0 + 1, 9.0, 10.0)])
        _check_sequence(eng, [newer], state, 2)
        assert state[("p", "v2")] == (-4, 7.0, 8.0) and state[("p", "v1")] == (T0 + 1, 9.0, 10.0)
        assert state[("q", "v1")] == (T0 + 9, 5.0, 6.0)
    finally:
        eng.close()


def test_string_edge_cases():
    eng = _engine()
    try:
        state = _check_sequence(eng, case_strings())
        assert ("a", "bc") in state and ("ab", "c") in state and ("", "") in state and len(state) == 19
    finally:
        eng.close()


def test_growth_over_four_batches():
    """2e5 vehicles arrive 5e4 at a time, the earlier ones re-reported with a newer ts: the pair table and the vehicle
    arena regrow at least twice, and the state is exact after every batch"""
    eng = _engine()
    try:
        rng = np.random.default_rng(9)
        state = {}
        for e in range(4):
            m = 50_000 * (e + 1)
            ids = rng.permutation(m)
            lat, lon = _coords(rng, m)
            rows = [("fleet", f"vehicle-{int(i):07d}", T0 + e * SEC + int(i) % 3, lat[j], lon[j]) for j, i in enumerate(ids)]
            _check_sequence(eng, [Batch(rows)], state, e)
        info = eng.positions_info()
        assert info["keys"] == 200_000 and info["vehicles"] == 200_000 and info["providers"] == 1
        assert info["pair_regrows"] >= 2 and info["vehicle_arena_regrows"] >= 2, info
        assert info["capacity"] >= 2 * info["keys"]
    finally:
        eng.close()


@pytest.mark.parametrize("keys", [1, 512, 513, 1025])
def test_export_at_the_compaction_edges(keys):
    """one row for each of `keys` distinct pairs: the pair table has next_pow2(max(2 * keys, 1024)) = 1024, 1024, 2048,
    4096 slots -- less than one 2048-slot tile of the export's compaction (the i < nslots guard), the same at load
    exactly 1/2, exactly one tile, two workgroups on one counter.  Then new pairs (600, or what it takes to pass load 1/2)
    take the state to the next table size: the old tables' slots are claimed again in the new ones (k_pos_pair_put,
    k_pos_str_rehash)."""
    eng = _engine()
    try:
        cap0 = max(1024, 1 << (2 * keys - 1).bit_length())
        more = max(600, cap0 // 2 - keys + 100)
        rng = np.random.default_rng(keys)
        lat, lon = _coords(rng, keys + more)
        rows = [(f"p{k % 3}", f"v{k}", T0 + k * SEC, lat[k], lon[k]) for k in range(keys + more)]
        state = _check_sequence(eng, [Batch(rows[:keys])])
        info = eng.positions_info()
        assert info["keys"] == len(state) == keys
        assert info["capacity"] == cap0
        _check_sequence(eng, [Batch(rows[keys:])], state, 1)
        info = eng.positions_info()
        assert info["keys"] == len(state) == keys + more
        assert info["capacity"] > cap0 and info["pair_regrows"] >= 1
    finally:
        eng.close()


@pytest.mark.parametrize("case", [case_one_batch, case_codes_move, case_strings])
def test_colliding_hashes_stay_exact(case):
    """string hashes cut to 4 bits: unequal strings with equal hashes everywhere; equal hash + unequal bytes probes on"""
    eng = _engine(hash_bits=4)
    try:
        _check_sequence(eng, case())
    finally:
        eng.close()


def test_every_hash_equal():
    eng = _engine(hash_bits=0)
    try:
        rng = np.random.default_rng(2)
        lat, lon = _coords(rng, 600)
        rows = [(f"p{(k // 50) % 4}", f"v{k % 50}", T0 + int(rng.integers(0, 9)) * SEC, lat[k], lon[k]) for k in range(600)]
        state = _check_sequence(eng, [Batch(rows[:300]), Batch(rows[300:], v_order=[f"v{k}" for k in range(49, -1, -1)])])
        assert len(state) == 200
        # the seam is refused once the state holds keys
        from mobheat import _lib
        assert eng._lib.hm_positions_debug_hash_bits(eng._ctx, 64) == _lib.HM_E_STATE
    finally:
        eng.close()


def test_probe_bound_surfaces_as_overflow():
    """more equal-hash strings than the probe bound: HM_E_OVERFLOW, never a wrong answer"""
    from mobheat import _lib
    eng = _engine(hash_bits=0)
    try:
        n = 4200
        rows = [("p", f"v{k}", T0, 1.0, 2.0) for k in range(n)]
        b = Batch(rows)
        eng.process_batch(0, b.lat, b.lon, b.ts, vkey=b.vkey, row_valid=np.ones(n, bool))
        assert _code(lambda: eng.update_positions(b.providers, b.vehicles)) == _lib.HM_E_OVERFLOW
    finally:
        eng.close()


def test_idempotence_and_call_order():
    from mobheat import _lib
    eng = _engine()
    try:
        (b,) = case_one_batch(seed=8, n=400)
        assert _code(lambda: eng.update_positions(b.providers, b.vehicles)) == _lib.HM_E_STATE   # no batch yet
        state = _check_sequence(eng, [b])
        eng.update_positions(b.providers, b.vehicles)   # the same batch again
        assert exported(eng) == bits(state)
        # a batch without a valid row: nothing to fold
        z = Batch([("zz", "nobody", T0, 1.0, 2.0)])
        res = eng.process_batch(1, z.lat, z.lon, z.ts, vkey=z.vkey, row_valid=np.zeros(1, bool))
        assert res.latest_rows.size == 0
        eng.update_positions(z.providers, z.vehicles)
        assert exported(eng) == bits(state) and eng.positions_info()["vehicles"] == len(b.vehicles)
        # codes outside the dictionaries handed in: HM_E_INVALID, the state as it was
        c = Batch([("pa", "v0", T0 + 500 * SEC, 1.0, 2.0), ("pb", "v1", T0 + 500 * SEC, 3.0, 4.0)])
        eng.process_batch(2, c.lat, c.lon, c.ts, vkey=c.vkey, row_valid=np.ones(2, bool))
        assert _code(lambda: eng.update_positions(c.providers[:1], c.vehicles)) == _lib.HM_E_INVALID
        assert _code(lambda: eng.update_positions(c.providers, [])) == _lib.HM_E_INVALID
        bad = (2, np.array([0, 2, 1], np.int64), np.frombuffer(b"v0v1", np.uint8).copy())   # offsets not ascending
        assert _code(lambda: eng.update_positions(c.providers, bad)) == _lib.HM_E_INVALID
        assert exported(eng) == bits(state)
        eng.update_positions(c.providers, c.vehicles)
        assert exported(eng) == bits(fold(state, c.latest()))
    finally:
        eng.close()


def test_export_import_round_trip():
    from mobheat import _lib
    batches = case_codes_move()
    a, b = _engine(), _engine()
    try:
        state = _check_sequence(a, batches[:2])
        recs, providers, vehicles = a.positions()
        b.import_positions(recs, providers, vehicles)
        assert exported(b) == bits(state)
        assert _code(lambda: b.import_positions(recs, providers, vehicles)) == _lib.HM_E_STATE   # not empty any more
        for eng, e in ((a, 2), (b, 0)):
            run(eng, e, batches[2])
        fold(state, batches[2].latest())
        assert exported(a) == bits(state) and exported(b) == bits(state)
        c = _engine()
        try:
            twice = np.concatenate([recs, recs[:1]])
            assert _code(lambda: c.import_positions(twice, providers, vehicles)) == _lib.HM_E_INVALID
            assert _code(lambda: c.import_positions(recs, providers, vehicles + vehicles[:1])) == _lib.HM_E_INVALID
            assert _code(lambda: c.import_positions(recs, providers[:1], vehicles)) == _lib.HM_E_INVALID
            assert c.positions_info()["keys"] == 0
            c.import_positions(recs[:0], [], [])
            assert exported(c) == {}
        finally:
            c.close()
    finally:
        a.close()
        b.close()


def test_steady_state_allocates_nothing():
    """batches over the same vehicles (every vehicle once more, at another of the same points, in another dictionary
    order): the positions calls allocate and free nothing from the second batch on (one warm batch), and hm_last_counts
    [6] / [7] stay as they are over the whole of the two batches after the warm one -- which is the engine's second:
    hm_process_batch itself still sizes its dedup table from the first batch's keys there (3 allocations, measured,
    none of them by a positions call)"""
    eng = _engine()
    try:
        rng = np.random.default_rng(4)
        vehs = [f"tram{k:04d}" for k in range(3000)]
        lat0, lon0 = _coords(rng, 3000)
        state = {}
        counts, own = [], []

        def now():
            c = eng.last_counts()
            return (c["allocs"], c["frees"])
        for e in range(4):
            order = list(rng.permutation(vehs))
            at = rng.permutation(3000)
            # (k and k + 3000 are the same vehicle with different ts: one latest row per vehicle in every batch)
            rows = [("city", order[k % 3000], T0 + (e * 10 + k % 7) * SEC, lat0[at[k % 3000]], lon0[at[k % 3000]])
                    for k in range(6000)]
            b = Batch(rows, v_order=order)
            run(eng, e, b, update=False)
            c0 = now()
            eng.update_positions(b.providers, b.vehicles)
            got = exported(eng)
            own.append(tuple(x - y for x, y in zip(now(), c0)))
            assert got == bits(fold(state, b.latest()))
            counts.append(now())
        print("allocs / frees after each batch:", counts, "by the positions calls alone:", own)
        assert own[1] == own[2] == own[3] == (0, 0), own
        assert counts[1] == counts[2] == counts[3], counts
    finally:
        eng.close()


def test_tile_state_and_read_side_untouched():
    eng = _engine()
    try:
        (b,) = case_one_batch(seed=21)
        run(eng, 0, b, update=False)
        v0 = eng.state_version()
        info0, recs0 = eng.export_state()
        tiles0 = eng.window_records(copy=True)
        eng.update_positions(b.providers, b.vehicles)
        pos0 = exported(eng)
        assert eng.state_version() == v0
        info1, recs1 = eng.export_state()
        assert info1 == info0 and np.array_equal(np.sort(recs0, order=["cell", "window_start_us"]),
                                                 np.sort(recs1, order=["cell", "window_start_us"]))
        view = eng.window_records(copy=False)   # the library's read-side buffer ...
        assert len(eng.window_tiles()) == tiles0.size > 0
        view = eng.window_records(copy=False)
        assert exported(eng) == pos0            # ... survives a positions export, and the other way round
        assert np.array_equal(np.sort(view, order="cell"), np.sort(tiles0, order="cell"))
        assert exported(eng) == bits(fold({}, b.latest()))
    finally:
        eng.close()


def test_foreach_batch_func_keeps_positions(monkeypatch):
    import pandas as pd
    from mobheat import readside, stream

    class Capture:
        ops = []

        def update_raw(self, coll, stmts):
            import types
            import bson
            if coll == "positions_latest":
                for st in stmts:
                    d = bson.decode(st.raw)
                    Capture.ops.append(types.SimpleNamespace(_filter=d["q"], _doc=d["u"]))

        def close(self):
            pass

    def frame(b):
        return pd.DataFrame({"provider": b.prov, "vehicleId": b.veh, "lat": b.lat, "lon": b.lon,
                             "speedKmh": np.full(len(b.rows), 30.0), "eventTs": pd.to_datetime(b.ts, unit="us")})
    batches = case_codes_move()[:2]
    monkeypatch.setattr(stream, "SINK_FACTORY", Capture)
    monkeypatch.setenv("MOBHEAT_POSITIONS", "1")
    stream.reset_engine()
    try:
        for e, b in enumerate(batches):
            stream.foreach_batch_func(frame(b), e)
        coll = apply_ops({}, Capture.ops)
        assert len(coll) > 20
        key = lambda f: (f["properties"]["provider"], f["properties"]["vehicleId"])   # noqa: E731
        got = readside.positions_latest_from_engine(stream.get_engine())
        exp = readside.positions_latest_collection(coll.values())
        assert sorted(got["features"], key=key) == sorted(exp["features"], key=key)
        assert got["type"] == "FeatureCollection" and len(got["features"]) == len(coll)
        # the variable unset: nothing is folded and nothing allocated
        monkeypatch.delenv("MOBHEAT_POSITIONS")
        stream.reset_engine()
        stream.foreach_batch_func(frame(batches[0]), 0)
        info = stream.get_engine().positions_info()
        assert info["keys"] == 0 and info["capacity"] == 0
    finally:
        stream.reset_engine()


def test_shard_context_is_unsupported():
    from mobheat import _lib
    eng = _engine(shard=(0, 2))
    try:
        assert _code(lambda: eng.update_positions(["p"], ["v"])) == _lib.HM_E_UNSUPPORTED
    finally:
        eng.close()
