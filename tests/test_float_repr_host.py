"""CPU: csrc/float_repr.h executed on the host (hm_selftest_float_repr_host) equals json.dumps(x) -- CPython's
float.__repr__, NaN / Infinity / -Infinity for the non-finite -- byte for byte.  No tolerance, no exclusions."""
import numpy as np

from geojson_cases import check_float_texts, special_doubles
from mobheat import _lib


def _check(x):
    x = np.ascontiguousarray(x, np.float64)
    text, ln = _lib.float_repr_selftest(x)
    assert ln.min() >= 3 and ln.max() <= 24
    check_float_texts(x, text, ln)


def test_random_bit_patterns():
    rng = np.random.default_rng(20250607)
    _check(rng.integers(0, 1 << 64, size=2_000_000, dtype=np.uint64).view(np.float64))


def test_degrees_and_dyadic_fractions():
    rng = np.random.default_rng(20250608)
    _check(rng.uniform(-180.0, 180.0, 100_000))
    k = rng.integers(-(1 << 40), 1 << 40, 100_000).astype(np.float64)
    _check(k / np.exp2(rng.integers(0, 60, 100_000)))


def test_powers_ends_and_layout_thresholds():
    x = special_doubles()
    assert x.size > 8000
    _check(x)
    text, ln = _lib.float_repr_selftest(np.array([1e16, 1234567890123456.0, 0.0001, 0.00001, 1.5e-7, 5e-324, -0.0, 42.0]))
    assert [bytes(t[:n]) for t, n in zip(text, ln)] == [b"1e+16", b"1234567890123456.0", b"0.0001", b"1e-05", b"1.5e-07",
                                                      b"5e-324", b"-0.0", b"42.0"]


def test_abi_declares_the_geojson_calls(mobheat_lib):
    for name in ("hm_selftest_float_repr_host", "hm_selftest_float_repr_device", "hm_encode_tile_features", "hm_window_geojson",
                 "hm_selftest_tile_features", "hm_positions_buckets", "hm_positions_geojson", "hm_selftest_position_features",
                 "hm_geojson_info"):
        assert name in _lib.SIGNATURES and hasattr(mobheat_lib, name)
    assert mobheat_lib.hm_selftest_float_repr_host(None, 1, None, None) == _lib.HM_E_INVALID
    assert mobheat_lib.hm_positions_geojson(None, None, 0, None, None, None, None) == _lib.HM_E_INVALID
