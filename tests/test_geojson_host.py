"""CPU: the GeoJSON encoders of csrc/geojson_docs.h executed on the host (hm_selftest_tile_features,
hm_selftest_position_features) against json.dumps(..., separators=(",", ":")) of the features mobheat/readside.py builds
from the same records -- byte for byte, feature by feature and as a whole body."""
import json

import numpy as np
import pytest

import geojson_cases as gc
from mobheat import _lib


@pytest.fixture(scope="module")
def cells():
    return gc.tile_cells(_lib.cells_to_boundary_host_selftest)


@pytest.mark.parametrize("n", [0, 1, 300])
def test_tile_features_equal_json_dumps(cells, n):
    recs = gc.tile_records(cells)[:n] if n != 1 else gc.tile_records(cells)[40:41]
    body, offs = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    gc.check_body(body, offs, gc.tile_collection(recs, gc.WS_TEXT, gc.WE_TEXT, _lib.cells_to_boundary_host_selftest))
    if n == 0:
        assert bytes(body) == b'{"type":"FeatureCollection","features":[]}'


def test_tile_feature_edges(cells):
    recs = gc.tile_records(cells)
    body, offs = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    feat = [bytes(body[offs[i]: offs[i + 1] - 1]) for i in range(recs.size)]
    assert b'"coordinates":[[]]' in feat[0] and b'"cellId":"1234"' in feat[0]          # the invalid index
    assert b'"count":0,' in feat[1] and b'"count":-1,' in feat[2] and b'"count":9223372036854775807,' in feat[3]
    assert b'"avgSpeedKmh":0.0,' in feat[4] and b'"avgSpeedKmh":NaN,' in feat[5] and b'"avgSpeedKmh":-0.0,' in feat[6]
    assert b'"avgSpeedKmh":3.3333333333333334e-08,' in feat[7]
    for i in range(1, 25):   # pentagons: 5 and 10 vertices, closed
        ring = json.loads(feat[i].replace(b"NaN", b"null"))["geometry"]["coordinates"][0]
        assert len(ring) == (6 if i < 13 else 11) and ring[0] == ring[-1]
    assert max(len(f) for f in feat) < 872


def test_tile_body_parses(cells):
    recs = gc.finite(gc.tile_records(cells))
    assert 290 < recs.size < 300
    body, offs = _lib.tile_features_selftest(recs, gc.WS_TEXT, gc.WE_TEXT)
    parsed = json.loads(bytes(body), parse_constant=lambda s: pytest.fail(f"non-finite {s} in the finite subset"))
    assert parsed == gc.tile_collection(recs, gc.WS_TEXT, gc.WE_TEXT, _lib.cells_to_boundary_host_selftest)


@pytest.mark.parametrize("bad", ["x" * 41, 'a"b', "a\\b", "a\nb", "café", "\x7f"])
def test_bad_window_text_is_rejected(cells, bad):
    recs = gc.tile_records(cells)[:3]
    for args in ((bad, gc.WE_TEXT), (gc.WS_TEXT, bad)):
        with pytest.raises(_lib.MobheatError) as e:
            _lib.tile_features_selftest(recs, *args)
        assert e.value.code == _lib.HM_E_INVALID
    _lib.tile_features_selftest(recs, "x" * 40, "")   # the longest text, and the empty one


def _positions(rows, offset_of=None):
    ids, offs = gc.bucket_table([r[2] for r in rows], offset_of)
    recs = gc.position_records(rows, gc.POSITION_STRINGS, gc.POSITION_STRINGS)
    d = gc.dictionary(gc.POSITION_STRINGS)
    return recs, d, ids, offs


def test_position_features_equal_json_dumps():
    rows = gc.position_rows()
    recs, d, ids, offs = _positions(rows)
    body, o = _lib.position_features_selftest(recs, d, d, ids, offs)
    gc.check_body(body, o, gc.position_collection(rows, ids, offs))
    text = bytes(body)
    # (the 1970 buckets carry the table's -4 h)
    assert b'"ts":"1969-12-31T20:00:00"' in text and b'"ts":"1969-12-31T19:59:59.999999"' in text
    assert b'"ts":"1969-12-31T20:00:00.000001"' in text and b'"ts":"0001-01-01T00:00:00"' in text
    assert b'"ts":"9999-12-31T23:59:59.999999"' in text
    assert b'"ts":"2025-11-02T01:59:59.999999"' in text and b'"ts":"2025-11-02T01:00:00"' in text   # either side of the change
    assert b"\\u0000\\u0001" in text and b"\\u007f" in text and b"\\ud83d\\ude8c" in text and b"\\u00e9" in text
    assert b'"coordinates":[-0.0,NaN]' in text


@pytest.mark.parametrize("n", [0, 1])
def test_position_features_small(n):
    rows = gc.position_rows()[5:5 + n]
    recs, d, ids, offs = _positions(rows)
    body, o = _lib.position_features_selftest(recs, d, d, ids, offs)
    gc.check_body(body, o, gc.position_collection(rows, ids, offs))


@pytest.mark.parametrize("bad", [b"\xff", b"ab\xc3", b"\xed\xa0\x80", b"\xc0\x80", b"\xf4\x90\x80\x80", b"\x80"])
def test_invalid_utf8_is_rejected(bad):
    ids, offs = gc.bucket_table([0])
    recs = np.zeros(1, _lib.POSITION_REC_DTYPE)
    for prov, veh in (([bad], ["v"]), (["ok"], [bad])):
        with pytest.raises(_lib.MobheatError) as e:
            _lib.position_features_selftest(recs, gc.dictionary(prov), gc.dictionary(veh), ids, offs)
        assert e.value.code == _lib.HM_E_INVALID
    body, o = _lib.position_features_selftest(recs, gc.dictionary(["ok"]), gc.dictionary(["v"]), ids, offs)
    gc.check_body(body, o, gc.position_collection([("ok", "v", 0, 0.0, 0.0)], ids, offs))


def test_missing_bucket_and_year_range_are_rejected():
    rows = gc.position_rows()
    recs, d, ids, offs = _positions(rows)
    with pytest.raises(_lib.MobheatError) as e:
        _lib.position_features_selftest(recs, d, d, ids[1:], offs[1:])
    assert e.value.code == _lib.HM_E_INVALID
    # year 1 shifted west leaves year 1; year 9999 shifted east leaves year 9999
    for ts, off in ((gc.Y1_S * 1_000_000, -3600), (gc.Y9999_S * 1_000_000, 3600)):
        r = np.zeros(1, _lib.POSITION_REC_DTYPE)
        r["ts_us"] = ts
        b = np.array([ts // 1_000_000 // 900], np.int64)
        with pytest.raises(_lib.MobheatError) as e:
            _lib.position_features_selftest(r, gc.dictionary(["p"]), gc.dictionary(["v"]), b, np.array([off], np.int64))
        assert e.value.code == _lib.HM_E_INVALID
        _lib.position_features_selftest(r, gc.dictionary(["p"]), gc.dictionary(["v"]), b, np.array([0], np.int64))
