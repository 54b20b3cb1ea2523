"""CPU: the positions read side (readside.positions_latest_collection against the dict reference app.py:71-88 builds),
the tests' reference fold against the reference's own statements (stream.position_ops, whose bytes the sink tests pin)
applied to a stand-in collection, and the ABI of the positions entry points."""
import datetime

import numpy as np

from positions_ref import apply_ops, fold, latest_rows


def test_positions_latest_collection_matches_app():
    from mobheat import readside
    ts = datetime.datetime(2025, 10, 4, 10, 0, 7, 123456)
    docs = [
        {"_id": "mbta|y1731", "provider": "mbta", "vehicleId": "y1731", "ts": ts,
         "loc": {"type": "Point", "coordinates": [-71.0589, 42.3601]}},
        {"_id": "x|", "provider": "x", "vehicleId": "", "ts": "2025-10-04T10:00:00Z",   # (not a datetime: str())
         "loc": {"type": "Point", "coordinates": [2.5, -1.25]}},
        {"_id": "n|1", "ts": None, "loc": {"type": "Point", "coordinates": [0.0, 0.0]}},   # (missing fields: .get)
    ]
    got = readside.positions_latest_collection(docs)
    assert got == {"type": "FeatureCollection", "features": [
        {"type": "Feature", "geometry": {"type": "Point", "coordinates": [-71.0589, 42.3601]},   # [lon, lat]
         "properties": {"provider": "mbta", "vehicleId": "y1731", "ts": "2025-10-04T10:00:07.123456"}},
        {"type": "Feature", "geometry": {"type": "Point", "coordinates": [2.5, -1.25]},
         "properties": {"provider": "x", "vehicleId": "", "ts": "2025-10-04T10:00:00Z"}},
        {"type": "Feature", "geometry": {"type": "Point", "coordinates": [0.0, 0.0]},
         "properties": {"provider": None, "vehicleId": None, "ts": "None"}},
    ]}
    assert readside.positions_latest_collection([]) == {"type": "FeatureCollection", "features": []}
    assert readside.positions_latest_collection(iter(docs[:1]))["features"][0]["properties"]["ts"] == ts.isoformat()


def _cols(rows):
    import pandas as pd
    return {"provider": pd.Series([r[0] for r in rows]), "vehicleId": pd.Series([r[1] for r in rows]),
            "ts_us": np.array([r[2] for r in rows], np.int64), "lat": np.array([r[3] for r in rows]),
            "lon": np.array([r[4] for r in rows])}


def test_fold_equals_the_reference_statements():
    """fold() over each batch's latest rows == the collection after stream.position_ops' statements, in order: a batch
    with tied maxima (the lowest row stays: the later tie's filter {ts: {$lt: ts}} matches nothing), a stale batch
    (older and equal ts change nothing), a batch one microsecond newer, negative ts."""
    from mobheat import stream
    t0 = 1_759_572_000_000_000
    batches = [
        [("a", "bc", t0, 1.0, 2.0), ("ab", "c", t0, 3.0, 4.0), ("a", "bc", t0, 5.0, 6.0), ("a", "bc", t0 - 1, 7.0, 8.0),
         ("m", "", -5, 9.0, 10.0), ("m", "", -5, 11.0, 12.0), ("m", "", -6, 13.0, 14.0)],
        [("a", "bc", t0, 15.0, 16.0), ("ab", "c", t0 - 7, 17.0, 18.0), ("m", "", -5, 19.0, 20.0)],          # stale
        [("a", "bc", t0 + 1, 21.0, 22.0), ("m", "", -4, 23.0, 24.0), ("new", "v", -(10 ** 9), 25.0, 26.0)],
    ]
    state, coll = {}, {}
    for rows in batches:
        idx = latest_rows([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        fold(state, [rows[i] for i in idx])
        apply_ops(coll, stream.position_ops(_cols(rows), idx))
        assert {k: (stream._spark_datetime(ts), lat, lon) for k, (ts, lat, lon) in state.items()} == \
            {(d["provider"], d["vehicleId"]): (d["ts"], d["loc"]["coordinates"][1], d["loc"]["coordinates"][0])
             for d in coll.values()}
    assert state[("a", "bc")] == (t0 + 1, 21.0, 22.0) and state[("ab", "c")] == (t0, 3.0, 4.0)
    assert state[("m", "")] == (-4, 23.0, 24.0) and len(state) == 4
    assert set(coll) == {"a|bc", "ab|c", "m|", "new|v"}


def test_abi_13_declares_the_positions_calls(mobheat_lib):
    from mobheat import _lib
    assert _lib.HM_ABI_VERSION == 13 and mobheat_lib.hm_abi_version() == 13
    for name in ("hm_positions_update", "hm_positions_export", "hm_positions_import", "hm_positions_info",
                 "hm_positions_debug_hash_bits"):
        assert name in _lib.SIGNATURES and hasattr(mobheat_lib, name)
    assert _lib.POSITION_REC_DTYPE.itemsize == 32
    # without a context: an error code, not a crash
    assert mobheat_lib.hm_positions_update(None, None) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_positions_debug_hash_bits(None, 4) == _lib.HM_E_INVALID
