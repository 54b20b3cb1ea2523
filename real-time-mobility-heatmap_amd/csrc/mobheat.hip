// mobheat: MI355X-native per-micro-batch hot path of the reference's streaming job (heatmap_stream.py).
//
// One translation unit (the device code shares __constant__ tables and inlines across stages); its parts, in
// dependency order:
//   dev_common.h    wave primitives, per-window state-table lookups, census sinks, the batch's window registry
//   dev_table.h     the off-hot-path global hash tables' probe loop (tab_probe), the live-slot compaction (block256_compact)
//   k_partition.h   radix partition into (window, region) bins / owner ranks (k_ev_hist, k_ev_scatter_rec, k_rp_*)
//   k_table.h       table mode for low-cardinality batches (k_agg, k_bin_reduce)
//   k_merge.h       census, growth dump, the region-owned merge into the update-mode state (k_merge_owned), rows
//   k_dedup.h       latest position per (provider, vehicleId) (k_dedup_*), ordered compaction
//   k_ingest.h      the per-event pass (k_ingest: filter + latLngToCell + window + late test + dedup max + event key)
//   k_json.h        Kafka values -> columns, string dictionaries
//   k_stage.h       multi-GPU exchange helpers
//   k_rollup.h      read side: one window's tiles rolled up to a coarser resolution (k_rollup, k_rollup_emit)
//   k_positions.h   the latest position per (provider, vehicleId) across batches (k_pos_*)
//   k_geojson.h     read side: the response bodies as GeoJSON (geojson_docs.h, float_repr.h: k_gj_*)
//   k_view.h        read side: a map viewport applied to cells, roll-up records and positions (k_cells_in_view, k_view_tiles)
//   k_raster.h      read side: a window's counts over a pixel grid, each pixel snapped to its cell (k_raster, k_raster_exact)
//   k_density.h     read side: the positions state grouped into H3 density cells (k_density_cells, k_density_group)
//   k_top.h         read side: the k records with the largest count in rank order (k_top_keys, k_top_hist, k_top_rank)
//   k_near.h        read side: the records nearest a point within a radius (k_near_distances, k_pos_emit_near, k_near_tiles)
//   k_change.h      read side: two windows' roll-ups joined on the cell, ranked by their count change (k_change_match, k_change_rest, k_change_keys)
//   k_span.h        read side: a trailing span of windows rolled up in one launch, with each parent's count per window (k_span, k_span_emit, k_span_rows)
//   k_within.h      read side: polygon geofences -- points, positions and tile centroids inside zones (k_points_in_zones, k_pos_within, k_within_tiles)
//   host_ctx.h      the context, allocation, per-window tables, launchers;  host_batch.h: the batch phases
//   api_*.h         the C ABI of include/mobheat.h (batch, UDF/read side, stage API, checkpoint, sink, JSON, window reads, positions, GeoJSON, viewport, self-tests)
//
// Pipeline per batch (one HIP stream per context; every arithmetic step runs on the GPU):
//   k_ingest      filter (heatmap_stream.py:96-104) + H3 latLngToCell UDF (:65-75,105) + tumbling window (:115) +
//                 late-row test against the watermark (:107) + batch max event time + per-vkey max ts for the dedup
//                 (:200-203) + one 8-B event key per row (cell, window slot) + the census of rows per window
//   direct path   k_ev_hist / k_ev_scatter_rec: 32-B event records into (window, region) bins; k_merge_owned: one
//                 workgroup per bin merges them into the persistent per-window state tables (update mode, :243;
//                 Spark's StateStoreRestore/Save) and writes each touched key's cumulative row (:124-132)
//   table mode    k_agg + k_bin_reduce aggregate in LDS first (one partial per key), then partition + merge
//   k_fill_gaps   the per-bin row segments -> dense update-mode rows (in place)
//   eviction      (watermark, :107) releases a window's whole table; k_dump_gen + a rehash merge grow one
//   k_dedup_list  latest position per (provider, vehicleId): rows whose ts equals the max (:204-207), looked for among
//                 the candidates k_ingest listed; their bits compacted in order (k_bm_count / k_bm_write).  k_dedup_flag
//                 over every row's flag when the list overflowed or the fused max gave up
//   [multi-GPU: records grouped by owner rank, exchanged by the caller with RCCL all-to-all (api_stage.h)]
//
// Semantics follow SURVEY.md App. A (Spark 3.5.1): see DESIGN.md for the rules and their provenance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <ctime>
#include <string>
#include <string_view>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "../../include/mobheat.h"
#include "kernels.h"
#include "bson_docs.h"
#include "json_decode.h"
#include "h3_boundary.h"
#include "geojson_docs.h"
#include <chrono>
#include <mutex>

#define H3T_CONST static const
#include "h3_tables.inc"

using namespace hm;

__constant__ H3Tables c_tab;
// glibc's sincos/acos/atan2/tan tables for the exact path (glibc_libm.h); c_tab.glm points here
__device__ glm::Tables g_glm = {GLM_TABLE_INIT};   // (not const: a const namespace-scope symbol has internal linkage, which hipGetSymbolAddress cannot resolve)

#include "h3_tables_host.h"
static H3Tables make_tables() { return hm_make_tables(); }
// c_tab of the current device, its glibc table pointer aimed at the device copy
static hipError_t upload_tables() {
    H3Tables T = make_tables();
    void *g = nullptr;
    hipError_t e = hipGetSymbolAddress(&g, HIP_SYMBOL(g_glm));
    if (e != hipSuccess) return e;
    T.glm = (const glm::Tables *)g;
    return hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &T, sizeof(T));
}

#include "dev_common.h"
#include "dev_table.h"
#include "k_partition.h"
#include "k_table.h"
#include "k_merge.h"
#include "k_dedup.h"
#include "k_ingest.h"
#include "k_json.h"
#include "k_stage.h"
#include "k_rollup.h"
#include "k_positions.h"
#include "k_geojson.h"
#include "k_view.h"
#include "k_raster.h"
#include "k_density.h"
#include "k_top.h"
#include "k_near.h"
#include "k_change.h"
#include "k_span.h"
#include "k_within.h"
#include "host_ctx.h"
#include "host_batch.h"
#include "host_pipe.h"

extern "C" {

#include "api_batch.h"
#include "api_udf.h"
#include "api_stage.h"
#include "api_state.h"
#include "api_sink.h"
#include "api_json.h"
#include "api_read.h"
#include "api_positions.h"
#include "api_geojson.h"
#include "api_view.h"
#include "api_raster.h"
#include "api_density.h"
#include "api_top.h"
#include "api_near.h"
#include "api_change.h"
#include "api_span.h"
#include "api_within.h"
#include "api_selftest.h"

}  // extern "C"
