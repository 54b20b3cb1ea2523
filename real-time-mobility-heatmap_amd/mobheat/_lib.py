"""ctypes binding of libmobheat.so (C ABI declared in include/mobheat.h).

The library is built in-tree (``real-time-mobility-heatmap_amd/csrc/libmobheat.so``); there is no CPU fallback:
if it cannot be loaded, every entry point raises.  Negative return codes raise ``RuntimeError`` with the
library's message, which keeps the reference's fail-the-batch behaviour (reference heatmap_stream.py:192-235
has no try/except around the writes; any exception kills the streaming query at :249).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MOBHEAT_LIB: load another build of the same ABI (kernel variants under csrc/variants/ for tuning runs)
LIB_PATH = os.environ.get("MOBHEAT_LIB") or os.path.normpath(os.path.join(_HERE, "..", "csrc", "libmobheat.so"))

HM_ABI_VERSION = 13
HM_MEM_HOST = 0
HM_MEM_DEVICE = 1
HM_MEM_HOST_STREAM = 2
HM_JSON_SPLICE = 1
HM_E_INVALID, HM_E_HIP, HM_E_NOMEM, HM_E_OVERFLOW, HM_E_STATE, HM_E_UNSUPPORTED = -1, -2, -3, -4, -5, -6
HM_STAGE_SUMMARY_WORDS = 8200
HM_TILE_REC_BYTES = 48       # table mode's tile partial
HM_EVENT_REC_BYTES = 32      # direct path: one record per aggregated row
HM_CAND_REC_BYTES = 32

c_i32, c_i64, c_u64, c_dbl, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p


class HmConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", c_i32), ("h3_res", c_i32), ("device", c_i32), ("late_uses_prev_watermark", c_i32),
        ("tile_us", c_i64), ("watermark_delay_ms", c_i64), ("state_capacity_hint", c_i64),
        ("batch_capacity_hint", c_i64), ("state_arena_bytes", c_i64), ("shard_rank", c_i32), ("shard_count", c_i32),
    ]


class HmBatchIn(ctypes.Structure):
    _fields_ = [
        ("n", c_i64), ("memory", c_i32), ("reserved", c_i32),
        ("lat", c_vp), ("lon", c_vp), ("ts_us", c_vp), ("speed", c_vp), ("speed_valid", c_vp),
        ("vkey", c_vp), ("row_valid", c_vp),
    ]


class HmBatchOut(ctypes.Structure):
    _fields_ = [
        ("n_tiles", c_i64), ("cell", c_vp), ("window_start_us", c_vp), ("count", c_vp), ("avg_speed", c_vp),
        ("speed_null", c_vp), ("avg_lon", c_vp), ("avg_lat", c_vp),
        ("n_latest", c_i64), ("latest_row", c_vp),
        ("n_in", c_i64), ("n_valid", c_i64), ("n_late", c_i64), ("n_state", c_i64),
        ("batch_max_event_ms", c_i64), ("watermark_ms", c_i64), ("late_watermark_ms", c_i64), ("n_partials", c_i64),
    ]


class HmJsonIn(ctypes.Structure):
    _fields_ = [("n", c_i64), ("memory", c_i32), ("flags", c_i32), ("bytes", c_vp), ("offsets", c_vp)]


class HmJsonOut(ctypes.Structure):
    _fields_ = [("batch", HmBatchIn), ("n_providers", c_i64), ("provider_offsets", c_vp), ("provider_bytes", c_vp),
                ("n_vehicles", c_i64), ("vehicle_offsets", c_vp), ("vehicle_bytes", c_vp), ("n_malformed", c_i64),
                ("n_unsupported", c_i64), ("unsupported_rows", c_vp)]


class HmArrowCol(ctypes.Structure):
    _fields_ = [("values", c_vp), ("data", c_vp), ("validity", c_vp), ("validity_offset", c_i64), ("offset_bytes", c_i32),
                ("unit", c_i32)]


class HmArrowIn(ctypes.Structure):
    _fields_ = [("n", c_i64), ("lat", HmArrowCol), ("lon", HmArrowCol), ("speed", HmArrowCol), ("ts_us", HmArrowCol),
                ("provider", HmArrowCol), ("vehicle", HmArrowCol)]


class HmStageSizes(ctypes.Structure):
    _fields_ = [("table_mode", c_i64), ("n_tile_records", c_i64), ("n_cands", c_i64), ("global_batch_max_event_ms", c_i64),
                ("n_valid", c_i64), ("n_late", c_i64), ("n_self_records", c_i64)]


class HmStateInfo(ctypes.Structure):
    _fields_ = [("epoch_id", c_i64), ("n_keys", c_i64), ("watermark_ms", c_i64), ("prev_watermark_ms", c_i64),
                ("tile_us", c_i64), ("watermark_delay_ms", c_i64), ("h3_res", c_i32), ("reserved", c_i32)]


class HmTileDocCfg(ctypes.Structure):
    _fields_ = [("city", ctypes.c_char_p), ("city_len", c_i32), ("reserved", c_i32), ("ttl_ms", c_i64),
                ("n_windows", c_i64), ("window_start_us", c_vp), ("start_offset_s", c_vp), ("end_offset_s", c_vp)]


class HmPositionDocCfg(ctypes.Structure):
    _fields_ = [("n_providers", c_i64), ("provider_offsets", c_vp), ("provider_bytes", c_vp),
                ("n_vehicles", c_i64), ("vehicle_offsets", c_vp), ("vehicle_bytes", c_vp),
                ("n_buckets", c_i64), ("bucket_ids", c_vp), ("bucket_offset_s", c_vp)]


class HmGeojsonCfg(ctypes.Structure):
    _fields_ = [("window_start_text", ctypes.c_char_p), ("start_len", c_i32), ("window_end_text", ctypes.c_char_p),
                ("end_len", c_i32)]


class HmView(ctypes.Structure):
    _fields_ = [("west", c_dbl), ("south", c_dbl), ("east", c_dbl), ("north", c_dbl)]


class HmNear(ctypes.Structure):
    _fields_ = [("lat", c_dbl), ("lon", c_dbl), ("max_distance_m", c_dbl)]


class HmZones(ctypes.Structure):
    _fields_ = [("n_zones", c_i32), ("zone_rings", c_vp), ("ring_verts", c_vp), ("lat", c_vp), ("lon", c_vp)]


# hm_zone_rec (48 B): one zone's totals of a within query
ZONE_REC_DTYPE = np.dtype([("n", "<i8"), ("count", "<i8"), ("n_speed", "<i8"), ("sum_speed", "<f8"), ("newest_us", "<i8"),
                           ("reserved", "<i8")])
assert ZONE_REC_DTYPE.itemsize == 48

# hm_state_rec (64 B): one live (cellId, windowStart) key of the tile state
STATE_REC_DTYPE = np.dtype([("cell", "<u8"), ("window_start_us", "<i8"), ("count", "<i8"), ("n_speed", "<i8"),
                            ("sum_speed", "<f8"), ("sum_lat", "<f8"), ("sum_lon", "<f8"), ("reserved", "<i8")])
assert STATE_REC_DTYPE.itemsize == 64

# hm_position_rec (32 B): one (provider, vehicleId) key of the positions state, by persistent dictionary codes
POSITION_REC_DTYPE = np.dtype([("provider", "<u4"), ("vehicle", "<u4"), ("ts_us", "<i8"), ("lat", "<f8"), ("lon", "<f8")])
assert POSITION_REC_DTYPE.itemsize == 32

_P = ctypes.POINTER
# name -> (restype, argtypes); must match include/mobheat.h (tests/test_abi.py checks the symbol set)
SIGNATURES = {
    "hm_create": (c_i32, [_P(HmConfig), _P(c_vp)]),
    "hm_destroy": (None, [c_vp]),
    "hm_last_error": (ctypes.c_char_p, [c_vp]),
    "hm_process_batch": (c_i32, [c_vp, c_i64, _P(HmBatchIn), c_i32, _P(HmBatchOut)]),
    "hm_latlng_to_cell": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp]),
    "hm_stage_ingest": (c_i32, [c_vp, c_i64, _P(HmBatchIn), c_i32, c_i32, c_vp]),
    "hm_stage_send_capacity": (c_i64, [c_i64, c_i32]),
    "hm_stage_send": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp, _P(HmStageSizes)]),
    "hm_stage_merge": (c_i32, [c_vp, c_vp, c_vp, c_i32, _P(HmBatchOut), c_vp, c_i64, c_vp]),
    "hm_stage_finish": (c_i32, [c_vp, c_vp, c_i64, c_i32, _P(HmBatchOut)]),
    "hm_stream_wait": (c_i32, [c_vp, c_vp]),
    "hm_device_memory": (c_i32, [c_i32, _P(c_i64), _P(c_i64)]),
    "hm_device_alloc": (c_i32, [c_i32, c_i64, _P(c_vp)]),
    "hm_device_free": (c_i32, [c_i32, c_vp]),
    "hm_host_alloc": (c_i32, [c_i64, _P(c_vp)]),
    "hm_host_free": (c_i32, [c_vp]),
    "hm_memcpy": (c_i32, [c_vp, c_vp, c_i64, c_i32]),
    "hm_selftest_ld_ops": (c_i32, [c_vp, c_i64, c_i32, c_vp]),
    "hm_selftest_floor_div": (c_i32, [c_vp, c_i64, c_i64, c_vp]),
    "hm_selftest_latlng_to_cell_host": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp]),
    "hm_selftest_latlng_to_cell_fast_host": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "hm_selftest_glibc_libm_host": (c_i32, [c_i32, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "hm_selftest_glibc_libm_device": (c_i32, [c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32]),
    "hm_state_export": (c_i32, [c_vp, _P(HmStateInfo), c_vp, c_i64]),
    "hm_state_export_touched": (c_i32, [c_vp, _P(HmStateInfo), c_vp, c_i64, c_vp]),
    "hm_state_export_begin": (c_i32, [c_vp, _P(HmStateInfo), c_i32, c_vp]),
    "hm_state_export_copy": (c_i32, [c_vp, c_vp, c_i64, c_i64]),
    "hm_state_export_copy_async": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_i32]),
    "hm_state_export_copy_wait": (c_i32, [c_vp, c_i32]),
    "hm_state_version": (c_i64, [c_vp]),
    "hm_state_import": (c_i32, [c_vp, _P(HmStateInfo), c_vp]),
    "hm_last_windows": (c_i32, [c_vp, c_vp, c_i64, _P(c_i64)]),
    "hm_encode_tile_updates": (c_i32, [c_vp, _P(HmTileDocCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_selftest_tile_statements": (c_i32, [_P(HmTileDocCfg), c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_i64, c_vp, c_i64, c_vp]),
    "hm_encode_position_updates": (c_i32, [c_vp, _P(HmPositionDocCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_statements_wait": (c_i32, [c_vp, c_i64]),
    "hm_selftest_position_statements": (c_i32, [_P(HmPositionDocCfg), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64,
                                                c_vp]),
    "hm_last_timings": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_last_counts": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_decode_json": (c_i32, [c_vp, _P(HmJsonIn), _P(HmJsonOut)]),
    "hm_arrow_columns": (c_i32, [c_vp, _P(HmArrowIn), _P(HmJsonOut)]),
    "hm_json_patch": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64]),
    "hm_latlng_to_cell_last_exact": (c_i64, [c_i32]),
    "hm_cells_to_boundary": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "hm_selftest_cells_to_boundary_host": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "hm_last_latest_buckets": (c_i32, [c_vp, c_vp, c_i64, _P(c_i64)]),
    "hm_selftest_json_records": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_vp]),
    "hm_selftest_decimal_to_double": (c_i32, [c_vp, c_vp, c_i64, c_vp]),
    "hm_live_windows": (c_i32, [c_vp, c_vp, c_vp, c_i64, _P(c_i64)]),
    "hm_window_rollup": (c_i32, [c_vp, c_i64, c_i32, c_i32, _P(c_vp), _P(c_i64)]),
    "hm_selftest_cell_to_parent": (c_i32, [c_vp, c_i64, c_i32, c_vp]),
    "hm_positions_update": (c_i32, [c_vp, _P(HmPositionDocCfg)]),
    "hm_positions_export": (c_i32, [c_vp, c_i32, _P(c_vp), _P(c_i64), _P(HmPositionDocCfg)]),
    "hm_positions_import": (c_i32, [c_vp, c_vp, c_i64, _P(HmPositionDocCfg)]),
    "hm_positions_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_positions_debug_hash_bits": (c_i32, [c_vp, c_i32]),
    "hm_encode_tile_features": (c_i32, [c_vp, _P(HmGeojsonCfg), c_i64, c_i32, c_vp, c_i32, _P(c_vp), _P(c_vp)]),
    "hm_window_geojson": (c_i32, [c_vp, c_i64, c_i32, _P(HmGeojsonCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp)]),
    "hm_selftest_tile_features": (c_i32, [_P(HmGeojsonCfg), c_vp, c_i64, c_vp, c_i64, c_vp]),
    "hm_positions_buckets": (c_i32, [c_vp, c_vp, c_i64, _P(c_i64)]),
    "hm_positions_geojson": (c_i32, [c_vp, _P(HmPositionDocCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp)]),
    "hm_selftest_position_features": (c_i32, [_P(HmPositionDocCfg), c_vp, c_i64, c_vp, c_i64, c_vp]),
    "hm_geojson_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_cells_in_view": (c_i32, [c_vp, c_i64, c_i32, c_i32, _P(HmView), c_vp]),
    "hm_selftest_cells_in_view": (c_i32, [c_vp, c_i64, _P(HmView), c_vp]),
    "hm_window_geojson_view": (c_i32, [c_vp, c_i64, c_i32, _P(HmGeojsonCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp),
                                       _P(HmView)]),
    "hm_positions_geojson_view": (c_i32, [c_vp, _P(HmPositionDocCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp),
                                          _P(HmView)]),
    "hm_window_raster": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, _P(c_vp), _P(c_vp)]),
    "hm_selftest_window_raster": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "hm_raster_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_positions_density": (c_i32, [c_vp, c_i32, c_i64, _P(HmView), c_i32, _P(c_vp), _P(c_i64)]),
    "hm_positions_density_raster": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, _P(c_vp),
                                            _P(c_vp)]),
    "hm_selftest_positions_density": (c_i32, [c_vp, c_i64, c_i32, c_i64, c_vp, c_i64, _P(c_i64), _P(c_i64)]),
    "hm_positions_density_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_top_records": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i64, c_i32, _P(c_vp), _P(c_i64)]),
    "hm_window_top": (c_i32, [c_vp, c_i64, c_i32, _P(HmView), c_i64, c_i32, _P(c_vp), _P(c_i64)]),
    "hm_window_geojson_top": (c_i32, [c_vp, c_i64, c_i32, _P(HmGeojsonCfg), _P(HmView), c_i64, c_i32, _P(c_vp), _P(c_vp),
                                      _P(c_i64), _P(c_vp)]),
    "hm_positions_density_top": (c_i32, [c_vp, c_i32, c_i64, _P(HmView), c_i64, c_i32, _P(c_vp), _P(c_i64)]),
    "hm_selftest_top_records": (c_i32, [c_vp, c_i64, c_i64, c_vp, _P(c_i64)]),
    "hm_top_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_near_distances": (c_i32, [_P(HmNear), c_vp, c_vp, c_i64, c_i32, c_i32, c_vp]),
    "hm_selftest_near_distances": (c_i32, [_P(HmNear), c_vp, c_vp, c_i64, c_vp]),
    "hm_positions_near": (c_i32, [c_vp, _P(HmNear), c_i64, c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_window_near": (c_i32, [c_vp, c_i64, c_i32, _P(HmNear), c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_selftest_positions_near": (c_i32, [_P(HmNear), c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, _P(c_i64)]),
    "hm_selftest_tiles_near": (c_i32, [_P(HmNear), c_vp, c_i64, c_i64, c_vp, c_vp, _P(c_i64)]),
    "hm_near_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_positions_geojson_near": (c_i32, [c_vp, _P(HmPositionDocCfg), _P(HmNear), c_i64, c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64),
                                          _P(c_vp), _P(c_vp)]),
    "hm_window_geojson_near": (c_i32, [c_vp, c_i64, c_i32, _P(HmGeojsonCfg), _P(HmNear), c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64),
                                       _P(c_vp), _P(c_vp)]),
    "hm_selftest_tile_features_near": (c_i32, [_P(HmGeojsonCfg), c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "hm_selftest_position_features_near": (c_i32, [_P(HmPositionDocCfg), c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "hm_points_in_zones": (c_i32, [_P(HmZones), c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "hm_selftest_points_in_zones": (c_i32, [_P(HmZones), c_vp, c_vp, c_i64, c_vp, c_vp]),
    "hm_positions_within": (c_i32, [c_vp, _P(HmZones), c_i64, c_i32, c_vp, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_window_within": (c_i32, [c_vp, c_i64, c_i32, _P(HmZones), c_i32, c_vp, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_positions_geojson_within": (c_i32, [c_vp, _P(HmPositionDocCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp), _P(HmZones)]),
    "hm_window_geojson_within": (c_i32, [c_vp, c_i64, c_i32, _P(HmGeojsonCfg), c_i32, _P(c_vp), _P(c_vp), _P(c_i64), _P(c_vp),
                                         _P(HmZones)]),
    "hm_selftest_positions_within": (c_i32, [_P(HmZones), c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, _P(c_i64)]),
    "hm_selftest_tiles_within": (c_i32, [_P(HmZones), c_vp, c_i64, c_vp, c_vp, c_vp, _P(c_i64)]),
    "hm_within_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_window_change": (c_i32, [c_vp, c_i64, c_i64, c_i32, _P(HmView), c_i32, _P(c_vp), _P(c_i64)]),
    "hm_window_change_top": (c_i32, [c_vp, c_i64, c_i64, c_i32, _P(HmView), c_i32, c_i64, c_i32, _P(c_vp), _P(c_i64)]),
    "hm_window_geojson_change": (c_i32, [c_vp, c_i64, c_i64, c_i32, _P(HmGeojsonCfg), _P(HmView), c_i32, c_i64, c_i32, _P(c_vp),
                                         _P(c_vp), _P(c_i64), _P(c_vp)]),
    "hm_selftest_window_change": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i64, c_i32, c_i64, c_vp, _P(c_i64)]),
    "hm_selftest_change_features": (c_i32, [_P(HmGeojsonCfg), c_vp, c_i64, c_vp, c_i64, c_vp]),
    "hm_change_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_span_rollup": (c_i32, [c_vp, c_i64, c_i32, c_i32, _P(HmView), c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_span_geojson": (c_i32, [c_vp, c_i64, c_i32, c_i32, _P(HmGeojsonCfg), _P(HmView), c_i64, c_i32, _P(c_vp), _P(c_vp), _P(c_i64)]),
    "hm_span_raster": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, _P(c_vp), _P(c_vp)]),
    "hm_span_info": (c_i32, [c_vp, c_vp, c_i32]),
    "hm_selftest_span": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_vp, c_vp, _P(c_i64)]),
    "hm_selftest_span_features": (c_i32, [_P(HmGeojsonCfg), c_vp, c_vp, c_i32, c_i64, c_vp, c_i64, c_vp]),
    "hm_test_read_grid_info": (c_i32, [c_vp, c_vp, c_vp, c_vp]),
    "hm_selftest_float_repr_host": (c_i32, [c_vp, c_i64, c_vp, c_vp]),
    "hm_selftest_float_repr_device": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i32]),
    "hm_abi_version": (c_i32, []),
}

_lib = None


def load():
    """Load libmobheat.so (raises if it is missing: the product path never falls back to the CPU)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libmobheat.so not built at {LIB_PATH}; run __graft_entry__.build() (or make -C csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.hm_abi_version() != HM_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} was built for ABI {lib.hm_abi_version()}, this binding is ABI {HM_ABI_VERSION}: "
                           "rebuild it (__graft_entry__.build())")
    _lib = lib
    return lib


class MobheatError(RuntimeError):
    """A failed library call: `code` is the C-ABI error code (HM_E_*)."""

    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


def check(rc, ctx=None, what="mobheat"):
    if rc < 0:
        lib = load()
        msg = lib.hm_last_error(ctx)
        raise MobheatError(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)
    return rc


def read_grid_info(ctx=None):
    """{"launches_lowered", "least_iterations", "most_iterations"} of MOBHEAT_TEST_READ_GRID on a context, or -- ctx None --
    of the process's context-free calls (hm_cells_in_view, hm_points_in_zones)."""
    v = [ctypes.c_int64() for _ in range(3)]
    check(load().hm_test_read_grid_info(ctx, *(ctypes.byref(x) for x in v)), ctx, "hm_test_read_grid_info")
    return {"launches_lowered": v[0].value, "least_iterations": v[1].value, "most_iterations": v[2].value}


def ptr(a):
    """Address of a contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays must be contiguous"
    return a.ctypes.data


def ld_ops_selftest(a, op):
    """Host execution of the kernels' x87 emulation (see hm_selftest_ld_ops)."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    check(lib.hm_selftest_ld_ops(ptr(a), a.size, op, ptr(out)))
    return out


def floor_div_selftest(t, d):
    """Host execution of k_ingest's window division floor(t / d) (kernels.h FloorDiv)."""
    lib = load()
    t = np.ascontiguousarray(t, dtype=np.int64)
    out = np.empty_like(t)
    check(lib.hm_selftest_floor_div(ptr(t), t.size, int(d), ptr(out)))
    return out


def latlng_to_cell_host_selftest(lat, lon, res):
    """Host execution of the device exact latLngToCell path (glibc's routines as restated in glibc_libm.h)."""
    lib = load()
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    out = np.empty(lat.size, dtype=np.uint64)
    check(lib.hm_selftest_latlng_to_cell_host(ptr(lat), ptr(lon), lat.size, res, ptr(out)))
    return out


GLIBC_FNS = {"sincos": 0, "acos": 1, "atan2": 2, "tan": 3, "asin": 4, "atan": 5}


def glibc_libm_selftest(fn, a, b=None, device=None):
    """glibc's sincos (-> (sin, cos)) / acos / atan2(a, b) / tan / asin / atan as csrc/glibc_libm.h restates them, executed on the
    host (device=None) or on GPU `device`."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty(a.size)
    out2 = np.empty(a.size) if fn == "sincos" else None
    args = (GLIBC_FNS[fn], ptr(a), None if b is None else ptr(b), a.size, ptr(out), None if out2 is None else ptr(out2))
    if device is None:
        check(lib.hm_selftest_glibc_libm_host(*args))
    else:
        check(lib.hm_selftest_glibc_libm_device(*args, int(device)))
    return (out, out2) if fn == "sincos" else out


def latlng_to_cell_fast_host_selftest(lat, lon, res):
    """Host execution of the kernels' fast path + exact fallback; returns (cells, fell_back mask)."""
    lib = load()
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    out = np.empty(lat.size, dtype=np.uint64)
    fb = np.empty(lat.size, dtype=np.uint8)
    check(lib.hm_selftest_latlng_to_cell_fast_host(ptr(lat), ptr(lon), lat.size, res, ptr(out), ptr(fb)))
    return out, fb.astype(bool)


def local_offsets_s(window_start_us, tile_us):
    """Local-time offsets (s) at each window's start and end, as the reference's datetimes carry them: pyspark's
    TimestampType.fromInternal gives naive local wall times (datetime.fromtimestamp), which bson then encodes as
    if they were UTC (reference heatmap_stream.py:166-177 via stream._spark_datetime)."""
    import calendar
    import datetime as _dt

    def off(us):
        s = int(us) // 1_000_000
        return calendar.timegm(_dt.datetime.fromtimestamp(s).timetuple()) - s
    ws = np.ascontiguousarray(window_start_us, dtype=np.int64)
    return (np.array([off(w) for w in ws], np.int64), np.array([off(w + tile_us) for w in ws], np.int64))


def tile_doc_cfg(city, ttl_minutes, window_start_us, tile_us):
    """hm_tile_doc_cfg for the given windows; the returned tuple keeps the arrays alive."""
    cb = city.encode("utf-8")
    ws = np.ascontiguousarray(window_start_us, dtype=np.int64)
    so, eo = local_offsets_s(ws, tile_us)
    cfg = HmTileDocCfg(city=cb, city_len=len(cb), ttl_ms=int(ttl_minutes) * 60_000, n_windows=ws.size,
                       window_start_us=ptr(ws), start_offset_s=ptr(so), end_offset_s=ptr(eo))
    return cfg, (cb, ws, so, eo)


def tile_statements_selftest(tiles, city, h3_res, ttl_minutes, tile_us):
    """Host execution of the GPU statement encoder on a TileRows (no GPU): (bytes uint8, offsets int64)."""
    lib = load()
    n = len(tiles)
    wins = np.unique(tiles.window_start_us) if n else np.zeros(1, np.int64)
    cfg, keep = tile_doc_cfg(city, ttl_minutes, wins, tile_us)
    cap = (600 + 3 * len(city.encode("utf-8"))) * max(n, 1)   # (the city is in q._id, $set._id and $set.city)
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(n + 1, np.int64)
    a = [np.ascontiguousarray(x) for x in (tiles.cell.astype(np.uint64), tiles.window_start_us.astype(np.int64),
                                           tiles.count.astype(np.int64), tiles.avg_speed.astype(np.float64),
                                           tiles.speed_null.astype(np.uint8), tiles.avg_lon.astype(np.float64),
                                           tiles.avg_lat.astype(np.float64))]
    check(lib.hm_selftest_tile_statements(ctypes.byref(cfg), int(h3_res), int(tile_us), *[ptr(x) for x in a], n,
                                          ptr(buf), cap, ptr(offs)), None, "hm_selftest_tile_statements")
    return buf[:offs[-1]].copy(), offs


def _dictionary(strings):
    """(n, offsets int64[n+1], bytes) of a list of str or an Arrow string array, UTF-8 (Arrow's string layout)."""
    import pyarrow as pa
    if isinstance(strings, pa.ChunkedArray):
        strings = strings.combine_chunks()
    arr = strings.cast(pa.large_string()) if isinstance(strings, pa.Array) else pa.array(list(strings), type=pa.large_string())
    n = len(arr)
    offs = np.frombuffer(arr.buffers()[1], dtype=np.int64, count=n + 1, offset=arr.offset * 8).copy() if n else np.zeros(1, np.int64)
    offs -= offs[0]
    data = arr.buffers()[2]
    raw = np.frombuffer(data, dtype=np.uint8).copy() if data is not None and offs[-1] else np.zeros(1, np.uint8)
    return n, offs, raw


def time_buckets(ts_us, bucket_ids=None):
    """The distinct 900-s buckets floor(ts_s / 900) of the rows' eventTs (ascending; or the given bucket_ids) and the
    local-time offset of each (pyspark's naive local datetimes, stream._spark_datetime).  Only the buckets the rows
    use are looked up, so a batch mixing a 1970 GPS time with current traffic costs two lookups, not 55 years of
    buckets."""
    import calendar
    import datetime as _dt
    if bucket_ids is not None:
        ids = np.unique(np.asarray(bucket_ids, dtype=np.int64))
    else:
        ts_us = np.asarray(ts_us, dtype=np.int64)
        ids = np.unique(np.floor_divide(np.floor_divide(ts_us, 1_000_000), 900)) if ts_us.size else np.zeros(0, np.int64)

    def off(s):
        return calendar.timegm(_dt.datetime.fromtimestamp(s).timetuple()) - s
    offs = np.array([off(int(b) * 900) for b in ids], np.int64)
    if any(off(int(b) * 900 + 899) != o for b, o in zip(ids, offs)):
        raise RuntimeError("a local-time offset change inside a 900-s bucket")
    return np.ascontiguousarray(ids, np.int64), offs


def position_doc_cfg(provider_uniques, vehicle_uniques, ts_us, bucket_ids=None):
    """hm_position_doc_cfg for a batch's string dictionaries (pandas.factorize uniques in the order the vkeys were
    built, or (n, offsets, bytes) as decode_json returns them) and the eventTs of its latest rows (or their 900-s
    buckets); the returned tuple keeps the arrays alive."""
    np_, po, pb = provider_uniques if isinstance(provider_uniques, tuple) else _dictionary(provider_uniques)
    nv, vo, vb = vehicle_uniques if isinstance(vehicle_uniques, tuple) else _dictionary(vehicle_uniques)
    bi, bo = time_buckets(ts_us, bucket_ids)
    cfg = HmPositionDocCfg(n_providers=np_, provider_offsets=ptr(po), provider_bytes=ptr(pb), n_vehicles=max(nv, 1),
                           vehicle_offsets=ptr(vo), vehicle_bytes=ptr(vb), n_buckets=bi.size,
                           bucket_ids=ptr(bi) if bi.size else None, bucket_offset_s=ptr(bo) if bo.size else None)
    if nv == 0:   # (no valid row: an empty dictionary of one empty string keeps the offsets well formed)
        vo2 = np.zeros(2, np.int64)
        cfg.vehicle_offsets = ptr(vo2)
        return cfg, (po, pb, vo, vb, bi, bo, vo2)
    return cfg, (po, pb, vo, vb, bi, bo)


def position_dicts_cfg(provider_uniques, vehicle_uniques):
    """hm_position_doc_cfg holding only the two dictionaries (hm_positions_update / hm_positions_import ignore the
    buckets): lists of str, Arrow string arrays or (n, offsets, bytes); the returned tuple keeps the arrays alive."""
    np_, po, pb = provider_uniques if isinstance(provider_uniques, tuple) else _dictionary(provider_uniques)
    nv, vo, vb = vehicle_uniques if isinstance(vehicle_uniques, tuple) else _dictionary(vehicle_uniques)
    po, vo = np.ascontiguousarray(po, np.int64), np.ascontiguousarray(vo, np.int64)
    pb, vb = np.ascontiguousarray(pb, np.uint8), np.ascontiguousarray(vb, np.uint8)
    cfg = HmPositionDocCfg(n_providers=np_, provider_offsets=ptr(po), provider_bytes=ptr(pb), n_vehicles=nv,
                           vehicle_offsets=ptr(vo), vehicle_bytes=ptr(vb), n_buckets=0, bucket_ids=None,
                           bucket_offset_s=None)
    return cfg, (po, pb, vo, vb)


def position_statements_selftest(provider_uniques, vehicle_uniques, vkey, ts_us, lat, lon):
    """Host execution of the GPU positions encoder on rows (no GPU): (bytes uint8, offsets int64)."""
    lib = load()
    vkey = np.ascontiguousarray(vkey, dtype=np.uint64)
    ts_us = np.ascontiguousarray(ts_us, dtype=np.int64)
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    n = vkey.size
    cfg, keep = position_doc_cfg(provider_uniques, vehicle_uniques, ts_us)
    cap = 1024 * max(n, 1) + 8 * int(keep[1].size + keep[3].size)
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(n + 1, np.int64)
    check(lib.hm_selftest_position_statements(ctypes.byref(cfg), ptr(vkey), ptr(ts_us), ptr(lat), ptr(lon), n, ptr(buf),
                                              cap, ptr(offs)), None, "hm_selftest_position_statements")
    return buf[:offs[-1]].copy(), offs


# ---- Kafka values (row f1) ----
JF = dict(LAT=1, LON=2, SPEED=4, TS=8, PROV=16, VEH=32, BEARING=64, ACC=128, PROV_ESC=256, VEH_ESC=512,
          MALFORMED=1 << 16, UNSUPPORTED=1 << 17)   # json_decode.h


def pack_values(values):
    """A list of bytes (Kafka values) -> (bytes uint8 with 16 spare bytes, offsets int64[n+1]) in Arrow's layout."""
    lens = np.fromiter((len(v) for v in values), dtype=np.int64, count=len(values))
    offs = np.zeros(len(values) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    buf = np.zeros(int(offs[-1]) + 16, np.uint8)
    if len(values):
        buf[:offs[-1]] = np.frombuffer(b"".join(values), np.uint8)
    return buf, offs


def json_records_selftest(values):
    """Host execution of the device record decoder (json_decode.h): per-record fields + decoded strings."""
    lib = load()
    buf, offs = pack_values(values)
    n = len(values)
    scratch = np.zeros_like(buf)
    o = {k: np.zeros(max(n, 1), dt) for k, dt in (("lat", np.float64), ("lon", np.float64), ("speed", np.float64),
                                                  ("ts_us", np.int64), ("bearing", np.int32), ("accuracy", np.int32),
                                                  ("p_off", np.int64), ("p_len", np.int32), ("v_off", np.int64),
                                                  ("v_len", np.int32), ("flags", np.uint32))}
    check(lib.hm_selftest_json_records(ptr(buf), ptr(offs), n, ptr(scratch), *[ptr(o[k]) for k in
                                       ("lat", "lon", "speed", "ts_us", "bearing", "accuracy", "p_off", "p_len", "v_off",
                                        "v_len", "flags")]), None, "hm_selftest_json_records")
    o = {k: v[:n] for k, v in o.items()}

    def strs(off, ln, esc_bit, present_bit):
        out = []
        for k in range(n):
            if not o["flags"][k] & present_bit:
                out.append(None)
                continue
            src = scratch if o["flags"][k] & esc_bit else buf
            out.append(bytes(src[o[off][k]:o[off][k] + o[ln][k]]))
        return out
    o["provider"] = strs("p_off", "p_len", JF["PROV_ESC"], JF["PROV"])
    o["vehicleId"] = strs("v_off", "v_len", JF["VEH_ESC"], JF["VEH"])
    return o


def decimal_to_double_selftest(w, q):
    lib = load()
    w = np.ascontiguousarray(w, dtype=np.uint64)
    q = np.ascontiguousarray(q, dtype=np.int64)
    out = np.empty(w.size, np.uint64)
    check(lib.hm_selftest_decimal_to_double(ptr(w), ptr(q), w.size, ptr(out)), None, "hm_selftest_decimal_to_double")
    return out


def cells_to_boundary_host_selftest(cells):
    """Host execution of the device cellToBoundary: (lat [n, 10], lng [n, 10], nverts [n])."""
    lib = load()
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    la = np.empty((cells.size, 10))
    lo = np.empty((cells.size, 10))
    nv = np.empty(cells.size, np.int32)
    check(lib.hm_selftest_cells_to_boundary_host(ptr(cells), cells.size, ptr(la), ptr(lo), ptr(nv)), None,
          "hm_selftest_cells_to_boundary_host")
    return la, lo, nv


# ---- the read side's GeoJSON bodies (csrc/geojson_docs.h, csrc/float_repr.h) ----
GEOJSON_PREFIX = b'{"type":"FeatureCollection","features":['


def geojson_body_len(offsets):
    """Length of the response body whose features' offsets are `offsets` (n + 1 entries): offsets[n] + 1, or the 42
    bytes of the empty collection when n == 0 (include/mobheat.h)."""
    n = len(offsets) - 1
    return int(offsets[n]) + (1 if n else 2)


def float_repr_selftest(x, device=None):
    """json.dumps of each double as csrc/float_repr.h writes it, executed on the host (device=None) or on GPU `device`:
    a list of bytes."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    text = np.zeros((x.size, 24), np.uint8)
    ln = np.zeros(x.size, np.int32)
    if device is None:
        check(lib.hm_selftest_float_repr_host(ptr(x), x.size, ptr(text), ptr(ln)), None, "hm_selftest_float_repr_host")
    else:
        check(lib.hm_selftest_float_repr_device(ptr(x), x.size, ptr(text), ptr(ln), int(device)), None,
              "hm_selftest_float_repr_device")
    return text, ln


def wall_iso(us, tz=None):
    """The text the read side writes for a time: isoformat of the naive local wall time of us microseconds (pyspark's
    naive datetimes, stream._spark_datetime), or of zone tz's wall time; "" for None."""
    if us is None:
        return ""
    import datetime as _dt

    from .stream import _spark_datetime
    us = int(us)
    if tz is None:
        return _spark_datetime(us).isoformat()
    return _dt.datetime.fromtimestamp(us // 1000000, tz).replace(tzinfo=None, microsecond=us % 1000000).isoformat()


def geojson_cfg(window_start_text, window_end_text):
    """hm_geojson_cfg for the two window texts (str or bytes); the returned tuple keeps the bytes alive."""
    a = window_start_text.encode("utf-8") if isinstance(window_start_text, str) else bytes(window_start_text)
    b = window_end_text.encode("utf-8") if isinstance(window_end_text, str) else bytes(window_end_text)
    return HmGeojsonCfg(window_start_text=a, start_len=len(a), window_end_text=b, end_len=len(b)), (a, b)


def tile_features_selftest(recs, window_start_text, window_end_text, dist_m=None):
    """Host execution of the GPU tile-feature encoder on STATE_REC_DTYPE records (no GPU): (body uint8, offsets int64).
    dist_m (float64 per record): hm_selftest_tile_features_near, the features with distanceM as their last property."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=STATE_REC_DTYPE)
    cfg, keep = geojson_cfg(window_start_text, window_end_text)
    cap = 64 + 920 * recs.size
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(recs.size + 1, np.int64)
    if dist_m is None:
        check(lib.hm_selftest_tile_features(ctypes.byref(cfg), ptr(recs) if recs.size else None, recs.size, ptr(buf), cap,
                                            ptr(offs)), None, "hm_selftest_tile_features")
    else:
        d = np.ascontiguousarray(dist_m, dtype=np.float64)
        assert d.size == recs.size
        check(lib.hm_selftest_tile_features_near(ctypes.byref(cfg), ptr(recs) if recs.size else None, recs.size,
                                                 ptr(d) if d.size else None, ptr(buf), cap, ptr(offs)), None,
              "hm_selftest_tile_features_near")
    return buf[:geojson_body_len(offs)].copy(), offs


def bucket_cfg(bucket_ids, tz=None):
    """hm_position_doc_cfg holding only the 900-s buckets and their local offsets: the process's zone (time_buckets), or
    zone tz's; the returned tuple keeps the arrays alive."""
    if tz is None:
        bi, bo = time_buckets(None, np.asarray(bucket_ids, np.int64))
    else:
        import datetime as _dt
        bi = np.unique(np.asarray(bucket_ids, dtype=np.int64))

        def off(s):
            return int(_dt.datetime.fromtimestamp(s, tz).utcoffset().total_seconds())
        bo = np.array([off(int(b) * 900) for b in bi], np.int64)
        if any(off(int(b) * 900 + 899) != o for b, o in zip(bi, bo)):
            raise RuntimeError("a local-time offset change inside a 900-s bucket")
    bi, bo = np.ascontiguousarray(bi, np.int64), np.ascontiguousarray(bo, np.int64)
    cfg = HmPositionDocCfg(n_buckets=bi.size, bucket_ids=ptr(bi) if bi.size else None,
                           bucket_offset_s=ptr(bo) if bo.size else None)
    return cfg, (bi, bo)


def position_features_selftest(recs, providers, vehicles, bucket_ids, bucket_offset_s, dist_m=None):
    """Host execution of the GPU position-feature encoder (no GPU) on POSITION_REC_DTYPE records, the two dictionaries
    ((n, offsets, bytes), so that any byte string can be given) and the bucket table: (body uint8, offsets int64)."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=POSITION_REC_DTYPE)
    cfg, keep = position_dicts_cfg(providers, vehicles)
    bi = np.ascontiguousarray(bucket_ids, np.int64)
    bo = np.ascontiguousarray(bucket_offset_s, np.int64)
    cfg.n_buckets, cfg.bucket_ids, cfg.bucket_offset_s = bi.size, ptr(bi) if bi.size else None, ptr(bo) if bo.size else None
    cap = 64 + recs.size * 300 + 12 * recs.size * int(max(keep[1].size, 1) + max(keep[3].size, 1))
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(recs.size + 1, np.int64)
    if dist_m is None:
        check(lib.hm_selftest_position_features(ctypes.byref(cfg), ptr(recs) if recs.size else None, recs.size, ptr(buf), cap,
                                                ptr(offs)), None, "hm_selftest_position_features")
    else:   # (the features with distanceM as their last property)
        d = np.ascontiguousarray(dist_m, dtype=np.float64)
        assert d.size == recs.size
        check(lib.hm_selftest_position_features_near(ctypes.byref(cfg), ptr(recs) if recs.size else None, recs.size,
                                                     ptr(d) if d.size else None, ptr(buf), cap, ptr(offs)), None,
              "hm_selftest_position_features_near")
    return buf[:geojson_body_len(offs)].copy(), offs


# ---- the read side for a map viewport (csrc/k_view.h) ----
def view_struct(view):
    """hm_view of (west, south, east, north) in degrees; validity is the library's to judge (HM_E_INVALID)."""
    w, s, e, n = (float(x) for x in view)
    return HmView(west=w, south=s, east=e, north=n)


def cells_in_view_selftest(cells, view):
    """Host execution of the device's view test (no GPU): uint8[n], 1 where the cell's boundary box meets the view."""
    lib = load()
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    keep = np.zeros(cells.size, np.uint8)
    v = view_struct(view)
    check(lib.hm_selftest_cells_in_view(ptr(cells) if cells.size else None, cells.size, ctypes.byref(v),
                                        ptr(keep) if cells.size else None), None, "hm_selftest_cells_in_view")
    return keep


# ---- a window as a raster (csrc/k_raster.h) ----
def raster_args(lat, lon, thresholds):
    """(lat float64[rows], lon float64[cols], thresholds int64[k] or None) as contiguous arrays; the limits are the
    library's to judge (HM_E_INVALID)."""
    lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
    thr = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.int64).reshape(-1)
    return lat, lon, thr


def raster_grids(pc, pk, lat, lon, thr, copy):
    """The outputs of a raster call (host pointers pc / pk) as counts uint32[rows, cols], or (counts, classes uint8[rows,
    cols]) when thresholds were given; zeros where the call wrote nothing; copy=False: views of the library's buffers."""
    shape, n = (lat.size, lon.size), lat.size * lon.size

    def grid(p, ct, dt):
        if n == 0 or not p:
            return np.zeros(shape, dt)
        a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(n,)).reshape(shape)
        return a.copy() if copy else a
    counts = grid(pc, ctypes.c_uint32, np.uint32)
    if thr is None:
        return counts
    return counts, (grid(pk, ctypes.c_uint8, np.uint8) if thr.size else np.zeros(shape, np.uint8))


def window_raster_selftest(recs, res, lat, lon, thresholds=None):
    """Host execution of the raster's per-pixel code (no GPU) on STATE_REC_DTYPE records: counts uint32[rows, cols], or
    (counts, classes uint8[rows, cols]) when thresholds are given."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=STATE_REC_DTYPE)
    lat, lon, thr = raster_args(lat, lon, thresholds)
    counts = np.zeros((lat.size, lon.size), np.uint32)
    classes = None if thr is None else np.zeros((lat.size, lon.size), np.uint8)
    check(lib.hm_selftest_window_raster(ptr(recs) if recs.size else None, recs.size, int(res), ptr(lat), lat.size, ptr(lon),
                                        lon.size, None if thr is None else ptr(thr), 0 if thr is None else thr.size,
                                        ptr(counts), None if classes is None else ptr(classes)), None,
          "hm_selftest_window_raster")
    return counts if thr is None else (counts, classes)


# ---- the positions state as H3 density cells (csrc/k_density.h) ----
INT64_MIN = -(1 << 63)


def positions_density_selftest(recs, res, since_us=None, cap=None):
    """Host execution of the density's per-key code (no GPU) on POSITION_REC_DTYPE records: (STATE_REC_DTYPE records, one
    per distinct cell among the keys with ts_us >= since_us (None: every key), window_start_us = the group's newest ts_us;
    the kept keys without a cell).  cap: room for that many groups (None: one per record); too few raise HM_E_INVALID."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=POSITION_REC_DTYPE)
    cap = recs.size if cap is None else int(cap)
    out = np.zeros(max(cap, 1), STATE_REC_DTYPE)
    n, bad = c_i64(), c_i64()
    check(lib.hm_selftest_positions_density(ptr(recs) if recs.size else None, recs.size, int(res),
                                            INT64_MIN if since_us is None else int(since_us), ptr(out), cap,
                                            ctypes.byref(n), ctypes.byref(bad)), None, "hm_selftest_positions_density")
    return out[:n.value].copy(), int(bad.value)


# ---- top-k hotspots (csrc/k_top.h) ----
HM_TOP_MAX = 65536


def top_records_selftest(recs, k):
    """Host execution of the top's select and ordering (no GPU) on STATE_REC_DTYPE records: the first min(k, n) records of
    the order (count descending as int64, then cell ascending, then input index), whole."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=STATE_REC_DTYPE)
    out = np.zeros(max(min(int(k), recs.size), 1), STATE_REC_DTYPE)
    n = c_i64()
    check(lib.hm_selftest_top_records(ptr(recs) if recs.size else None, recs.size, int(k), ptr(out), ctypes.byref(n)), None,
          "hm_selftest_top_records")
    return out[:n.value].copy()


def state_recs_at(p, n, copy=True):
    """n hm_state_rec at host pointer p as a STATE_REC_DTYPE array (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros(0, STATE_REC_DTYPE)
    recs = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_uint8)), shape=(n * STATE_REC_DTYPE.itemsize,)).view(STATE_REC_DTYPE)
    return recs.copy() if copy else recs


# ---- change between two live windows (csrc/k_change.h) ----
HM_CHANGE_RISING, HM_CHANGE_FALLING, HM_CHANGE_ABS = 0, 1, 2
CHANGE_ORDERS = {"rising": HM_CHANGE_RISING, "falling": HM_CHANGE_FALLING, "abs": HM_CHANGE_ABS}
# hm_change_rec (128 B): a cell's record in the current window and in the base window
CHANGE_REC_DTYPE = np.dtype([("cur", STATE_REC_DTYPE), ("base", STATE_REC_DTYPE)])
assert CHANGE_REC_DTYPE.itemsize == 128


def change_order_code(order):
    """HM_CHANGE_* of "rising" / "falling" / "abs" (or of the code itself); ValueError otherwise."""
    if isinstance(order, str) and order in CHANGE_ORDERS:
        return CHANGE_ORDERS[order]
    if not isinstance(order, str) and int(order) in CHANGE_ORDERS.values():
        return int(order)
    raise ValueError(f"order {order!r} is none of {sorted(CHANGE_ORDERS)}")


def change_recs_at(p, n, copy=True):
    """n hm_change_rec at host pointer p as a CHANGE_REC_DTYPE array (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros(0, CHANGE_REC_DTYPE)
    recs = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_uint8)), shape=(n * CHANGE_REC_DTYPE.itemsize,)).view(CHANGE_REC_DTYPE)
    return recs.copy() if copy else recs


def window_change_selftest(cur, base, window_start_us, base_start_us, order=None, k=None):
    """Host execution of the change's join, key and ordering (no GPU) on two STATE_REC_DTYPE arrays: every pair sorted by
    cell (order None), or the first min(k, n) pairs of the order (k None: HM_TOP_MAX)."""
    lib = load()
    cur = np.ascontiguousarray(cur, dtype=STATE_REC_DTYPE)
    base = np.ascontiguousarray(base, dtype=STATE_REC_DTYPE)
    kk = -1 if order is None else HM_TOP_MAX if k is None else int(k)
    out = np.zeros(max(cur.size + base.size, 1), CHANGE_REC_DTYPE)
    n = c_i64()
    check(lib.hm_selftest_window_change(ptr(cur) if cur.size else None, cur.size, ptr(base) if base.size else None, base.size,
                                        int(window_start_us), int(base_start_us), 0 if order is None else change_order_code(order), kk,
                                        ptr(out), ctypes.byref(n)), None, "hm_selftest_window_change")
    return out[:n.value].copy()


def change_features_selftest(pairs, window_start_text, window_end_text):
    """Host execution of the GPU encoder on CHANGE_REC_DTYPE pairs (no GPU): (body uint8, offsets int64)."""
    lib = load()
    pairs = np.ascontiguousarray(pairs, dtype=CHANGE_REC_DTYPE)
    cfg, keep = geojson_cfg(window_start_text, window_end_text)
    cap = 64 + 1040 * pairs.size
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(pairs.size + 1, np.int64)
    check(lib.hm_selftest_change_features(ctypes.byref(cfg), ptr(pairs) if pairs.size else None, pairs.size, ptr(buf), cap, ptr(offs)),
          None, "hm_selftest_change_features")
    return buf[:geojson_body_len(offs)].copy(), offs


# ---- a trailing span of live windows (csrc/k_span.h) ----
HM_SPAN_MAX_WINDOWS = 16


def span_rows_at(p, n, windows, copy=True):
    """n series rows at host pointer p as int64[n, windows] (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros((0, int(windows)), np.int64)
    rows = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_int64)), shape=(n * int(windows),)).reshape(n, int(windows))
    return rows.copy() if copy else rows


def span_selftest(per_window_records, first_us, tile_us, res):
    """Host execution of the span (no GPU) on one STATE_REC_DTYPE array per window of the span, in window order:
    (records sorted by cell, series int64[n, windows])."""
    lib = load()
    per = [np.ascontiguousarray(r, dtype=STATE_REC_DTYPE) for r in per_window_records]
    counts = np.array([r.size for r in per], np.int64)
    recs = np.concatenate(per) if per else np.zeros(0, STATE_REC_DTYPE)
    out = np.zeros(max(recs.size, 1), STATE_REC_DTYPE)
    series = np.zeros((max(recs.size, 1), max(len(per), 1)), np.int64)
    n = c_i64()
    check(lib.hm_selftest_span(ptr(recs) if recs.size else None, ptr(counts) if counts.size else None, len(per), int(first_us),
                               int(tile_us), int(res), ptr(out), ptr(series), ctypes.byref(n)), None, "hm_selftest_span")
    return out[:n.value].copy(), series[:n.value].copy()


def span_features_selftest(recs, series, window_start_text, window_end_text):
    """Host execution of the GPU encoder on a span's STATE_REC_DTYPE records and their series rows (no GPU): (body uint8,
    offsets int64)."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=STATE_REC_DTYPE)
    series = np.ascontiguousarray(series, dtype=np.int64)
    assert series.ndim == 2 and series.shape[0] == recs.size
    cfg, keep = geojson_cfg(window_start_text, window_end_text)
    cap = 64 + (920 + 24 + 21 * series.shape[1]) * recs.size
    buf = np.zeros(cap, np.uint8)
    offs = np.zeros(recs.size + 1, np.int64)
    check(lib.hm_selftest_span_features(ctypes.byref(cfg), ptr(recs) if recs.size else None, ptr(series) if recs.size else None,
                                        series.shape[1], recs.size, ptr(buf), cap, ptr(offs)), None, "hm_selftest_span_features")
    return buf[:geojson_body_len(offs)].copy(), offs


# ---- radius queries (csrc/k_near.h) ----
HM_EARTH_RADIUS_M = 6378100.0


def near_struct(lat, lon, max_distance_m=float("inf")):
    """hm_near of a query point in degrees and a radius in metres; validity is the library's to judge (HM_E_INVALID)."""
    return HmNear(lat=float(lat), lon=float(lon), max_distance_m=float(max_distance_m))


def near_distances_selftest(lat0, lon0, lat, lon, device=None):
    """The distance in metres from (lat0, lon0) to every (lat[i], lon[i]): host execution of the kernels' code (no GPU), or
    on GPU `device` (hm_near_distances)."""
    lib = load()
    lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
    assert lat.size == lon.size
    q = near_struct(lat0, lon0)
    out = np.zeros(lat.size, np.float64)
    p = (lambda a: ptr(a) if a.size else None)
    if device is None:
        check(lib.hm_selftest_near_distances(ctypes.byref(q), p(lat), p(lon), lat.size, p(out)), None, "hm_selftest_near_distances")
    else:
        check(lib.hm_near_distances(ctypes.byref(q), p(lat), p(lon), lat.size, HM_MEM_HOST, int(device), p(out)), None,
              "hm_near_distances")
    return out


def _near_selftest(fn, name, dtype, q, recs, k, *lead):
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=dtype)
    room = max(min(int(k), recs.size), 1)
    out, dist, n = np.zeros(room, dtype), np.zeros(room, np.float64), c_i64()
    check(getattr(lib, fn)(ctypes.byref(q), *lead, ptr(recs) if recs.size else None, recs.size, int(k), ptr(out), ptr(dist),
                           ctypes.byref(n)), None, name)
    return out[:n.value].copy(), dist[:n.value].copy()


def positions_near_selftest(recs, lat, lon, max_distance_m=float("inf"), k=HM_TOP_MAX, since_us=None):
    """Host execution of the near query (no GPU) on POSITION_REC_DTYPE records: (the first min(k, kept) records nearest
    first, then provider << 32 | vehicle ascending, then input index; their distances in metres)."""
    return _near_selftest("hm_selftest_positions_near", "hm_selftest_positions_near", POSITION_REC_DTYPE,
                          near_struct(lat, lon, max_distance_m), recs, k, INT64_MIN if since_us is None else int(since_us))


def tiles_near_selftest(recs, lat, lon, max_distance_m=float("inf"), k=HM_TOP_MAX):
    """The same on STATE_REC_DTYPE records by their centroid (sum_lat / count, sum_lon / count); ties by cell ascending."""
    return _near_selftest("hm_selftest_tiles_near", "hm_selftest_tiles_near", STATE_REC_DTYPE, near_struct(lat, lon, max_distance_m),
                          recs, k)


def doubles_at(p, n, copy=True):
    """n doubles at host pointer p (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros(0, np.float64)
    a = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_double)), shape=(n,))
    return a.copy() if copy else a


def position_recs_at(p, n, copy=True):
    """n hm_position_rec at host pointer p as a POSITION_REC_DTYPE array (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros(0, POSITION_REC_DTYPE)
    recs = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_uint8)), shape=(n * POSITION_REC_DTYPE.itemsize,)).view(POSITION_REC_DTYPE)
    return recs.copy() if copy else recs


# ---- polygon geofences (csrc/k_within.h) ----
HM_ZONES_MAX = 4096
HM_ZONE_VERTS_MAX = 65536


class Zones:
    """A zone set as the library takes it: zone z is the rings zone_rings[z] .. zone_rings[z + 1] - 1, ring r the vertices
    ring_verts[r] .. ring_verts[r + 1] - 1 of (lat, lon) in degrees, without the repeated closing vertex.  Validity is
    the library's to judge (HM_E_INVALID)."""

    def __init__(self, zone_rings, ring_verts, lat, lon):
        self.zone_rings = np.ascontiguousarray(zone_rings, dtype=np.int32).reshape(-1)
        self.ring_verts = np.ascontiguousarray(ring_verts, dtype=np.int32).reshape(-1)
        self.lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
        self.lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)

    @property
    def n_zones(self):
        return max(self.zone_rings.size - 1, 0)

    @classmethod
    def from_rings(cls, zones):
        """zones: a list of zones, each a list of rings, each a list of (lat, lon) vertices"""
        zr, rv, la, lo = [0], [0], [], []
        for rings in zones:
            for ring in rings:
                la += [float(v[0]) for v in ring]
                lo += [float(v[1]) for v in ring]
                rv.append(len(la))
            zr.append(len(rv) - 1)
        return cls(zr, rv, la, lo)

    def rings(self, z):
        """zone z as a list of (lat, lon) arrays, one pair per ring"""
        return [(self.lat[self.ring_verts[r]:self.ring_verts[r + 1]], self.lon[self.ring_verts[r]:self.ring_verts[r + 1]])
                for r in range(int(self.zone_rings[z]), int(self.zone_rings[z + 1]))]


def zones_struct(zones):
    """(hm_zones, what must stay alive) of a Zones"""
    p = (lambda a: ptr(a) if a.size else None)
    return HmZones(n_zones=zones.n_zones, zone_rings=p(zones.zone_rings), ring_verts=p(zones.ring_verts), lat=p(zones.lat),
                   lon=p(zones.lon)), zones


def points_in_zones_selftest(zones, lat, lon, device=None):
    """(first zone int32 or -1, hits uint32) of every (lat[i], lon[i]): host execution of the kernels' predicate (no GPU),
    or on GPU `device` (hm_points_in_zones)."""
    lib = load()
    lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
    assert lat.size == lon.size
    z, keep = zones_struct(zones)
    first, hits = np.zeros(lat.size, np.int32), np.zeros(lat.size, np.uint32)
    p = (lambda a: ptr(a) if a.size else None)
    if device is None:
        check(lib.hm_selftest_points_in_zones(ctypes.byref(z), p(lat), p(lon), lat.size, p(first), p(hits)), None,
              "hm_selftest_points_in_zones")
    else:
        check(lib.hm_points_in_zones(ctypes.byref(z), p(lat), p(lon), lat.size, HM_MEM_HOST, int(device), p(first), p(hits)), None,
              "hm_points_in_zones")
    return first, hits


def _within_selftest(fn, dtype, zones, recs, *lead):
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=dtype)
    z, keep = zones_struct(zones)
    room = max(recs.size, 1)
    out, zone, tot, n = np.zeros(room, dtype), np.zeros(room, np.int32), np.zeros(max(zones.n_zones, 1), ZONE_REC_DTYPE), c_i64()
    check(getattr(lib, fn)(ctypes.byref(z), *lead, ptr(recs) if recs.size else None, recs.size, ptr(tot), ptr(out), ptr(zone),
                           ctypes.byref(n)), None, fn)
    return out[:n.value].copy(), zone[:n.value].copy(), tot[:zones.n_zones].copy()


def positions_within_selftest(zones, recs, since_us=None):
    """Host execution of the within query (no GPU) on POSITION_REC_DTYPE records: (the records with ts_us >= since_us in at
    least one zone, in input order; their labels int32; the zones' totals ZONE_REC_DTYPE)."""
    return _within_selftest("hm_selftest_positions_within", POSITION_REC_DTYPE, zones, recs, INT64_MIN if since_us is None else int(since_us))


def tiles_within_selftest(zones, recs):
    """The same on STATE_REC_DTYPE records by their centroid (sum_lat / count, sum_lon / count)."""
    return _within_selftest("hm_selftest_tiles_within", STATE_REC_DTYPE, zones, recs)


def int32s_at(p, n, copy=True):
    """n int32 at host pointer p (a copy, or a view of the library's buffer)."""
    if n == 0:
        return np.zeros(0, np.int32)
    a = np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_int32)), shape=(n,))
    return a.copy() if copy else a
