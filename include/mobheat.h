/*
 * mobheat -- MI355X-native drop-in for the per-micro-batch hot path of
 * panosporf99/real-time-mobility-heatmap (reference heatmap_stream.py).
 *
 * C ABI only: plain pointers and sizes, no C++ or torch types. Every function returns 0 on success or a
 * negative HM_E_* code; hm_last_error() returns the message. The ctypes host binding raises RuntimeError
 * on a negative code, which keeps the reference's "exception fails the micro-batch" behaviour
 * (reference heatmap_stream.py:192,196,231,235 have no try/except; the query dies in awaitTermination, :249).
 *
 * What each entry point replaces (reference file:line):
 *   hm_create / hm_destroy       -- the Spark session + stateful query plan (heatmap_stream.py:41-47,241-249):
 *                                   config H3_RES (:26), TILE_MINUTES (:29), withWatermark 10 min (:107).
 *   hm_process_batch             -- everything between from_json (:88-93) and the Mongo writes for one
 *                                   micro-batch: the sanity filter (:96-104), the to_h3 UDF (:65-75,105-106),
 *                                   the watermark (:107), window(eventTs, TILE) x cellId count/avg aggregation
 *                                   in update mode (:111-133,243), and the in-batch latest-position dedup
 *                                   groupBy(provider,vehicleId).max(eventTs) + join back (:198-207).
 *   hm_latlng_to_cell            -- the per-row UDF alone: h3.latlng_to_cell(lat, lon, H3_RES) (:73).
 *   hm_stage_* (multi-GPU)       -- the same batch split into local pre-aggregation, an owner-partitioned
 *                                   exchange (the caller moves the records with RCCL all-to-all), and the
 *                                   owner-side merge; replaces Spark's shuffle (spark.sql.shuffle.partitions, :44).
 *   hm_state_export / _import    -- the state store behind .option("checkpointLocation", CHECKPOINT_DIR)
 *                                   (:37,244): the tile state + watermark after a committed epoch, and its
 *                                   restore into a fresh context after a restart (the epoch is then replayed).
 *   hm_encode_tile_updates       -- the tiles half of the batch writer (:164-196): one MongoDB `update`
 *                                   statement {q, u: {$set: doc}, multi, upsert} per emitted tile, BSON-encoded
 *                                   on the GPU exactly as pymongo encodes the reference's UpdateOne.
 *   hm_encode_position_updates   -- the positions half (:198-235): one positions_latest statement per latest row.
 *   hm_live_windows / hm_window_rollup -- the web API's read of the latest window's tiles (app.py:45-69), from the
 *                                   engine's state instead of MongoDB, at any H3 resolution <= H3_RES.
 *   hm_positions_*               -- the positions_latest collection itself (:217-228 and app.py:71-88): every vehicle's
 *                                   newest position so far, folded across batches on the device.
 *   hm_window_geojson / hm_positions_geojson -- the two endpoints' response bodies (app.py:45-88) as GeoJSON encoded on
 *                                   the GPU, byte for byte json.dumps of the collections the reference builds in Python.
 *   hm_window_geojson_view / hm_positions_geojson_view / hm_cells_in_view -- the same for a client's map viewport.
 *   hm_window_raster             -- a live window's counts per pixel of a grid, for z/x/y raster tiles of the heatmap.
 *   hm_positions_density*        -- the positions state grouped into H3 cells: vehicles per cell at any resolution.
 *   hm_*_near / hm_*_within      -- what is around a point (radius queries) and what is inside polygon zones (geofences).
 *   hm_window_change* / hm_span_* -- two live windows against each other, and a trailing span of them as one heatmap
 *                                   with every cell's count per window ("the last 15 minutes").
 */
#ifndef MOBHEAT_H
#define MOBHEAT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_ABI_VERSION 13

/* error codes */
#define HM_OK 0
#define HM_E_INVALID (-1)   /* bad argument */
#define HM_E_HIP (-2)       /* HIP runtime error */
#define HM_E_NOMEM (-3)     /* device or host allocation failed */
#define HM_E_OVERFLOW (-4)  /* a device hash table overflowed its probe bound */
#define HM_E_STATE (-5)     /* call out of order (stage API) */
#define HM_E_UNSUPPORTED (-6) /* input outside what the device decoder handles (hm_decode_json) */

/* memory kinds for batch pointers */
#define HM_MEM_HOST 0
#define HM_MEM_DEVICE 1
#define HM_MEM_HOST_STREAM 2   /* hm_encode_* outputs only: pinned host memory; the offsets have landed when the call
                                  returns, the bytes land in pieces after it (hm_statements_wait) */

typedef struct hm_config {
    int32_t abi_version;            /* must be HM_ABI_VERSION */
    int32_t h3_res;                 /* H3_RES, 0..15 (reference default 8, heatmap_stream.py:26) */
    int32_t device;                 /* HIP device ordinal */
    int32_t late_uses_prev_watermark; /* 1 = Spark 3.5 default: late rows filtered by the previous batch's
                                         watermark, state evicted by the current one; 0 = both current */
    int64_t tile_us;                /* window length in microseconds: TILE_MINUTES*60e6 (default 5 min) */
    int64_t watermark_delay_ms;     /* withWatermark delay (reference: 10 minutes = 600000) */
    int64_t state_capacity_hint;    /* expected keys of the largest window: its table is reserved at create
                                       (0 = allocate on demand) */
    int64_t batch_capacity_hint;    /* expected max events per batch (0 = grow on demand) */
    int64_t state_arena_bytes;      /* device memory reserved (and zeroed) at create for the window tables; tables
                                       are carved from it before any allocation in a batch (0 = none) */
    int32_t shard_rank;             /* multi-GPU: this context is rank shard_rank of shard_count (the stage API); its
                                       state holds only the keys that rank owns.  shard_count 0 = not fixed at create
                                       (the first hm_stage_ingest fixes it), 1 = a single GPU */
    int32_t shard_count;
} hm_config;

/* One micro-batch of raw events, structure of arrays. All arrays have n entries.
 * row_valid: 1 iff provider, vehicleId and eventTs are all non-null (NULL pointer = all 1).
 * lat/lon: degrees; a null lat/lon is passed as NaN (it then fails the range filter, like Spark's between).
 * ts_us: eventTs as Spark TimestampType, microseconds since the epoch, UTC.
 * speed/speed_valid: speedKmh and its non-null flag (speed_valid NULL = all non-null; speed NULL = all null).
 * vkey: identity of (provider, vehicleId); equal pairs must give equal keys, distinct pairs distinct keys.
 *       UINT64_MAX is reserved. */
typedef struct hm_batch_in {
    int64_t n;
    int32_t memory;        /* HM_MEM_HOST or HM_MEM_DEVICE */
    int32_t reserved;
    const double *lat;
    const double *lon;
    const int64_t *ts_us;
    const double *speed;
    const uint8_t *speed_valid;
    const uint64_t *vkey;
    const uint8_t *row_valid;
} hm_batch_in;

/* Per-batch results. Arrays are library-owned and stay valid until the next call on this context
 * (or hm_destroy). With out_memory == HM_MEM_DEVICE they are device pointers.
 * Tiles (update mode: every (cell, window) changed by this batch, with cumulative aggregates):
 *   cell, window_start_us, count, avg_speed (0.0 when speed_null), speed_null, avg_lon, avg_lat.
 *   window end = window_start_us + tile_us.
 * Latest positions: row indices (into this batch's input) of every row whose eventTs equals the max
 *   eventTs of its (provider, vehicleId) among this batch's valid rows; ties give several rows. Sorted. */
typedef struct hm_batch_out {
    int64_t n_tiles;
    const uint64_t *cell;
    const int64_t *window_start_us;
    const int64_t *count;
    const double *avg_speed;
    const uint8_t *speed_null;
    const double *avg_lon;
    const double *avg_lat;
    int64_t n_latest;
    const int64_t *latest_row;
    /* batch statistics */
    int64_t n_in;                 /* input rows */
    int64_t n_valid;              /* rows passing the filter (heatmap_stream.py:98-106) */
    int64_t n_late;               /* valid rows dropped by the watermark */
    int64_t n_state;              /* live keys in the persistent tile state after the batch */
    int64_t batch_max_event_ms;   /* max(eventTs/1000) over valid rows, INT64_MIN if none */
    int64_t watermark_ms;         /* watermark used for eviction in this batch */
    int64_t late_watermark_ms;    /* watermark used to drop late rows in this batch */
    int64_t n_partials;           /* partial records merged (after the in-batch LDS pre-aggregation) */
} hm_batch_out;

typedef struct hm_ctx hm_ctx;

int hm_create(const hm_config *cfg, hm_ctx **out);
void hm_destroy(hm_ctx *ctx);
const char *hm_last_error(const hm_ctx *ctx);   /* ctx may be NULL: last error of hm_create */

/* Single-GPU hot path for one micro-batch. epoch_id is recorded (Spark's batch id); batches must be
 * passed in order, including empty (no-data) batches. out_memory selects host or device result arrays. */
int hm_process_batch(hm_ctx *ctx, int64_t epoch_id, const hm_batch_in *in, int32_t out_memory,
                     hm_batch_out *out);

/* Per-row UDF: cells for n points (degrees) at resolution res; 0 for rows the UDF maps to None.
 * Pointers are in `memory` space (host pointers are copied). Runs on device `device`. */
int hm_latlng_to_cell(const double *lat, const double *lon, int64_t n, int32_t res, int32_t memory,
                      int32_t device, uint64_t *out);
/* Inputs of the last hm_latlng_to_cell call on `device` that the fast path handed to the exact path (its near-tie
 * exceptions; tests check that constructed near-ties exercise it). */
int64_t hm_latlng_to_cell_last_exact(int32_t device);

/* ---- multi-GPU stage API (one context per GPU/rank; the caller performs the exchanges) ----
 * Replaces Spark's shuffle of the groupBy and of the latest-position join (heatmap_stream.py:44,112-133,198-207).
 * Per micro-batch:
 * 1. hm_stage_ingest: snap + filter + window + late test + this rank's latest-position max; writes this rank's
 *    summary (HM_STAGE_SUMMARY_WORDS int64 words, host memory) for the caller to all-gather.
 * 2. hm_stage_send(all ranks' summaries, [nranks][HM_STAGE_SUMMARY_WORDS], rank-major): every rank derives the
 *    same batch-wide decisions from them -- the global max event time (the watermark's input, :107), the
 *    aggregation path and the batch's global window registry -- and writes ONE chunk per destination rank into the
 *    caller's device send buffer (send_cap bytes; hm_stage_send_capacity(n, nranks) bytes are always enough), its
 *    size in bytes into send_bytes[r].  A tile key's destination owns a contiguous range of the key hash's 13-bit
 *    region field (rank r: [ceil(r 8192 / nranks), ceil((r + 1) 8192 / nranks))); a candidate's is a hash of its
 *    vkey.  Chunk (little-endian, every part 32-B aligned):
 *      header, 8 int64: magic 0x314b4e5548434d48, records, candidates, record bytes, bins, records offset,
 *        candidates offset, chunk bytes
 *      direct path (sizes.table_mode == 0): u32 counts[bins] (the records of each region field the destination
 *        owns, in order), u32 census[4096] (records per global window slot), then one 32-B record per aggregated
 *        row, grouped by region field: u64 cell's low 52 bits | (1 + the window's global registry slot) << 52,
 *        speed bits (null = 0x7ff0000000000001, NaN canonical), f64 lat, f64 lon;
 *      table mode (sizes.table_mode == 1, low-cardinality batches): bins = 0, one 48-B tile partial per key of the
 *        rank's shard: u64 cell, i64 window_start_us, u32 count, u32 n_speed, f64 sum_speed, f64 sum_lat, f64 sum_lon;
 *      then the latest candidates, 32 B: u64 vkey, i64 ts_us, i64 row, i64 origin_rank.
 * 3. caller: one all_to_all of the chunks (sizes first); recv_buf holds the chunks of ranks 0..nranks-1 in order.
 * 4. hm_stage_merge: the owner merges the received tile records into the persistent state it owns (each of its
 *    (window, region) bins from its senders' segments: no second partition), emits the tiles it owns, reduces the
 *    received candidates to winners, and writes the winners' row indices grouped by origin rank into
 *    winner_send_buf (capacity >= the candidates received) with per-origin counts.
 * 5. caller: exchange winners back; hm_stage_finish takes the received winners (rows of this rank).
 * After hm_stage_merge the owner's tiles can be encoded (hm_last_windows, hm_encode_tile_updates); after hm_stage_finish
 * the rank's latest rows can (hm_last_latest_buckets, hm_encode_position_updates, with the batch's dictionaries): every
 * rank writes the statements of what it owns, so no statement crosses the exchange.  A device caller keeps its input
 * buffers until then.  A context serves one rank of one world size (hm_config.shard_rank / shard_count, or fixed by
 * its first hm_stage_ingest): its tables hold that rank's keys only. */
#define HM_STAGE_SUMMARY_WORDS 8200
#define HM_TILE_REC_BYTES 48
#define HM_EVENT_REC_BYTES 32
#define HM_CAND_REC_BYTES 32
typedef struct hm_stage_sizes {
    int64_t table_mode;                  /* the batch's aggregation path (the same on every rank) */
    int64_t n_tile_records;              /* tile records this rank sent */
    int64_t n_cands;                     /* latest candidates this rank sent */
    int64_t global_batch_max_event_ms;   /* max over all ranks */
    int64_t n_valid, n_late;             /* this rank's rows */
    int64_t n_self_records;              /* of n_tile_records: the ones of bins this rank owns, kept in its own slabs
                                            (the chunk it addresses to itself carries their counts and census, and
                                            records = 0 in its header; hm_stage_merge merges them from the slabs) */
} hm_stage_sizes;

int hm_stage_ingest(hm_ctx *ctx, int64_t epoch_id, const hm_batch_in *in, int32_t nranks, int32_t rank,
                    int64_t *summary);
int64_t hm_stage_send_capacity(int64_t n_rows, int32_t nranks);
int hm_stage_send(hm_ctx *ctx, const int64_t *summaries, void *send_buf, int64_t send_cap, int64_t *send_bytes,
                  hm_stage_sizes *sizes);
int hm_stage_merge(hm_ctx *ctx, const void *recv_buf, const int64_t *recv_bytes, int32_t out_memory, hm_batch_out *out,
                   void *winner_send_buf, int64_t winner_send_cap, int64_t *winner_send_counts);
int hm_stage_finish(hm_ctx *ctx, const void *winner_recv_dev, int64_t n_winner_recv, int32_t out_memory,
                    hm_batch_out *out);
/* Orders the context's stream after the work queued so far on `stream` (a hipStream_t of the caller: the stream its
 * collective ran on, e.g. torch's current stream after RCCL's all_to_all): an event recorded there and waited for on
 * the library's stream, so that the next stage reads the received buffer without a host synchronization.  NULL = the
 * legacy default stream. */
int hm_stream_wait(hm_ctx *ctx, void *stream);

/* device helpers for the caller's exchange buffers */
int hm_device_memory(int32_t device, int64_t *free_bytes, int64_t *total_bytes);   /* (sizes a state arena) */
int hm_device_alloc(int32_t device, int64_t bytes, void **ptr);
int hm_device_free(int32_t device, void *ptr);
int hm_memcpy(void *dst, const void *src, int64_t bytes, int32_t kind); /* 0 H2D 1 D2H 2 D2D */
/* page-locked host memory (the checkpoint's export buffer: a device-to-host copy into it runs at the link's rate) */
int hm_host_alloc(int64_t bytes, void **ptr);
int hm_host_free(void *ptr);

/* Self-test entry (host-side execution of the device numerics; no GPU needed): evaluates the
 * extended-precision emulation used by the kernels, op codes as oracle_ld_ops(). */
int hm_selftest_ld_ops(const double *a, int64_t n, int32_t op, double *out);
/* floor(t[i] / d) by k_ingest's invariant-divisor multiply (kernels.h FloorDiv), executed on the host */
int hm_selftest_floor_div(const int64_t *t, int64_t n, int64_t d, int64_t *out);
/* Host-side execution of the device latLngToCell exact path (upstream's sequence with glibc's transcendentals as
 * restated in csrc/glibc_libm.h: the same numerics as k_ingest_exact / k_cells_exact). */
int hm_selftest_latlng_to_cell_host(const double *lat, const double *lon, int64_t n, int32_t res,
                                    uint64_t *out);
/* Host-side execution of the kernels' fast path (latLngToCellFast: direct gnomonic projection with a margin
 * test) with the exact path as fallback, as k_ingest + k_ingest_exact run it; fell_back[i] = 1 where the
 * exact path was taken (may be NULL). */
int hm_selftest_latlng_to_cell_fast_host(const double *lat, const double *lon, int64_t n, int32_t res,
                                         uint64_t *out, uint8_t *fell_back);
/* glibc 2.35's sincos / acos / atan2 / tan as the exact path restates them (csrc/glibc_libm.h; what the
 * reference's h3 calls through the host libm, heatmap_stream.py:65-75): fn 0 sincos(a) -> out = sin, out2 = cos;
 * 1 acos(a); 2 atan2(a, b); 3 tan(a).  _host runs the code on the CPU, _device on GPU `device` (host arrays). */
int hm_selftest_glibc_libm_host(int32_t fn, const double *a, const double *b, int64_t n, double *out, double *out2);
int hm_selftest_glibc_libm_device(int32_t fn, const double *a, const double *b, int64_t n, double *out, double *out2,
                                  int32_t device);

/* Tile-state checkpoint (Spark's state store version after an epoch, heatmap_stream.py:37,244).
 * One record per live (cellId, windowStart) key: the cumulative aggregates the next batches build on.
 * reserved must be 0 on import. Records are in no particular order. */
typedef struct hm_state_rec {
    uint64_t cell;
    int64_t window_start_us;
    int64_t count;        /* count(1) so far */
    int64_t n_speed;      /* non-null speedKmh rows so far */
    double sum_speed;
    double sum_lat;
    double sum_lon;
    int64_t reserved;
} hm_state_rec;   /* 64 B */

typedef struct hm_state_info {
    int64_t epoch_id;            /* last epoch processed by the context (-1: none) */
    int64_t n_keys;              /* records */
    int64_t watermark_ms;        /* the watermark the next batch evicts with */
    int64_t prev_watermark_ms;   /* the one it drops late rows with (late_uses_prev_watermark) */
    int64_t tile_us;             /* must match the importing context's config */
    int64_t watermark_delay_ms;  /* idem */
    int32_t h3_res;              /* idem */
    int32_t reserved;
} hm_state_info;

/* Fills *info; with recs != NULL also writes info->n_keys records to recs (host memory, cap records:
 * HM_E_INVALID if cap < n_keys). Call once with recs = NULL for the size. Not between stage calls. */
int hm_state_export(hm_ctx *ctx, hm_state_info *info, hm_state_rec *recs, int64_t cap);
/* Incremental checkpoint (Spark's state store delta files): the records of the keys the last batch touched (their
 * cumulative values), *n_out of them (recs = NULL: count only); info as hm_state_export (n_keys = all live keys).  The
 * state after that batch = the last-written record of every key of an older full export followed by the deltas of the
 * batches since, keeping keys whose window end > info->prev_watermark_ms * 1000. */
int hm_state_export_touched(hm_ctx *ctx, hm_state_info *info, hm_state_rec *recs, int64_t cap, int64_t *n_out);
/* The same exports in two halves, for a checkpoint file writer that overlaps the device-to-host copy with the
 * statements' encode and the file write (the reference's state store write, heatmap_stream.py:37,244): _begin dumps the
 * state -- every live key, or (touched_only) the last batch's touched keys -- into device memory and returns
 * *n_out; _copy writes records [first, first + count) of that dump to host memory `recs` (page-locked memory: the
 * copy runs at the link's rate).  _copy may run on another thread while hm_encode_tile_updates /
 * hm_encode_position_updates run on this context (it uses a stream of its own), never beside hm_process_batch, a
 * stage call or another export.  A _copy / _copy_async CALLED after a batch, or after another export that rewrote the
 * dump, fails (HM_E_STATE): the dump it names is gone. */
int hm_state_export_begin(hm_ctx *ctx, hm_state_info *info, int32_t touched_only, int64_t *n_out);
int hm_state_export_copy(hm_ctx *ctx, hm_state_rec *recs, int64_t first, int64_t count);
/* _copy split in two: _async enqueues the copy and marks its completion in slot (0..63) -- call it on the engine's
 * thread BEFORE the statements' encode, so that the encode's copies queue behind it, not the other way round -- and
 * _wait (any thread) blocks until the copy marked in slot has landed.
 * A copy that _async has queued is safe against what the context does next: hm_process_batch, a stage call,
 * hm_state_export, hm_state_export_touched, hm_state_export_begin and hm_state_import make their stream wait for the
 * last queued copy before they rewrite or reallocate the dump, so a slice waited for only afterwards still holds the
 * records of the dump it was queued from (and _wait still returns HM_OK).  What the caller owes is `recs`: it must stay
 * valid until _wait has returned for the slot, and a slot is reused only after its _wait. */
int hm_state_export_copy_async(hm_ctx *ctx, hm_state_rec *recs, int64_t first, int64_t count, int32_t slot);
int hm_state_export_copy_wait(hm_ctx *ctx, int32_t slot);
/* Restores an exported state into a context that has processed no batch (HM_E_STATE otherwise); the
 * config fields of info must equal the context's (HM_E_INVALID). recs: info->n_keys distinct keys, host memory, in any
 * order.  Refused with HM_E_INVALID: a record with a zero cell, reserved != 0, count < 1, n_speed outside [0, count] or
 * a window_start_us that is no window start; a cell that is not an H3 cell (mode 1) of the context's h3_res; on a shard
 * context a key another rank owns; a (cell, window_start_us) key given twice.  Refused with HM_E_OVERFLOW: more than
 * 2048 windows.  A refused import leaves the context as it was: fresh, and free to import again. */
int hm_state_import(hm_ctx *ctx, const hm_state_info *info, const hm_state_rec *recs);

/* Tiles of the last batch as MongoDB update statements (reference heatmap_stream.py:164-196): statement i is
 * bytes[offsets[i], offsets[i+1]), the BSON document {q: {_id}, u: {$set: doc}, multi: false, upsert: true}
 * that pymongo sends for the reference's UpdateOne({"_id": _id}, {"$set": doc}, upsert=True), doc as :164-188.
 * Datetimes are pyspark's naive local wall times: the caller gives, for each window of hm_last_windows (same
 * order), the local UTC offset in seconds at the window's start and at its end. Outputs are library-owned
 * until the next call (device or pinned host memory per out_memory). */
typedef struct hm_tile_doc_cfg {
    const char *city;               /* CITY, UTF-8, at most 64 bytes */
    int32_t city_len;
    int32_t reserved;
    int64_t ttl_ms;                 /* TTL_MINUTES * 60000 (staleAt = windowEnd + TTL) */
    int64_t n_windows;
    const int64_t *window_start_us; /* = hm_last_windows */
    const int64_t *start_offset_s;
    const int64_t *end_offset_s;
} hm_tile_doc_cfg;

/* The distinct window starts of the last batch's emitted tiles, ascending (*n = count; up to cap written). */
int hm_last_windows(hm_ctx *ctx, int64_t *window_start_us, int64_t cap, int64_t *n);
int hm_encode_tile_updates(hm_ctx *ctx, const hm_tile_doc_cfg *cfg, int32_t out_memory, const uint8_t **bytes,
                           const int64_t **offsets, int64_t *n_docs);

/* Latest positions of the last hm_process_batch as positions_latest update statements (reference
 * heatmap_stream.py:211-235): {q: {_id: "provider|vehicleId", $or: [{ts: {$exists: false}}, {ts: {$lt: ts}}]},
 * u: {$set: {provider, vehicleId, ts, loc}}, multi: false, upsert: true}, in latest_row order. The strings come
 * from the batch's dictionaries (the vkey the caller passed = provider_code * n_vehicles + vehicle_code; string k
 * of a dictionary = bytes[offsets[k], offsets[k+1]), UTF-8); ts is the naive local datetime of eventTs, with the
 * local UTC offset of the row's 900-s bucket floor(ts_s / 900): bucket_offset_s[k] for bucket_ids[k] (the distinct
 * buckets of the latest rows, strictly ascending; a row whose bucket is absent fails the call). After the stage API:
 * this rank's latest rows (hm_stage_finish). Outputs as hm_encode_tile_updates. */
typedef struct hm_position_doc_cfg {
    int64_t n_providers;
    const int64_t *provider_offsets;   /* n_providers + 1 */
    const char *provider_bytes;
    int64_t n_vehicles;
    const int64_t *vehicle_offsets;    /* n_vehicles + 1 */
    const char *vehicle_bytes;
    int64_t n_buckets;
    const int64_t *bucket_ids;         /* n_buckets, strictly ascending */
    const int64_t *bucket_offset_s;    /* n_buckets */
} hm_position_doc_cfg;
int hm_encode_position_updates(hm_ctx *ctx, const hm_position_doc_cfg *cfg, int32_t out_memory, const uint8_t **bytes,
                               const int64_t **offsets, int64_t *n_docs);
/* After an hm_encode_* call with HM_MEM_HOST_STREAM: blocks until bytes [0, upto) of its statements have landed in
 * the host buffer (any thread), so that a sink sends each command as soon as its statements are there -- the
 * statements' device-to-host copy overlaps the sink's writes instead of preceding them (reference :191-196,230-235). */
int hm_statements_wait(hm_ctx *ctx, int64_t upto);

/* Host execution of hm_encode_tile_updates' statement encoder on caller arrays (no GPU needed): statement i
 * is bytes[offsets[i], offsets[i+1]) (offsets: n+1 entries; HM_E_INVALID if cap bytes do not suffice). */
int hm_selftest_tile_statements(const hm_tile_doc_cfg *cfg, int32_t h3_res, int64_t tile_us, const uint64_t *cell,
                                const int64_t *ws, const int64_t *cnt, const double *sp, const uint8_t *spn,
                                const double *lon, const double *lat, int64_t n, uint8_t *bytes, int64_t cap,
                                int64_t *offsets);

/* Host execution of hm_encode_position_updates' encoder on caller rows (row i: vkey[i], ts[i], lat[i], lon[i]). */
int hm_selftest_position_statements(const hm_position_doc_cfg *cfg, const uint64_t *vkey, const int64_t *ts,
                                    const double *lat, const double *lon, int64_t n, uint8_t *bytes, int64_t cap,
                                    int64_t *offsets);

/* Timing of the last hm_process_batch / stage batch on the library's stream (HIP events), milliseconds
 * per phase: index 0 ingest (k_ingest: filter + cells + windows + event keys + latest max), 1 table-mode
 * aggregation (k_agg + k_bin_reduce), 2 merge, 3 emit, 4 dedup (flag + compaction), 5 total, 6 (window, region)
 * partition, 7 stage API: the sender's partition by owner rank.  Host side of the last hm_process_batch (wall
 * clock): 8 the call, 9 blocked in stream synchronizations, 10 in device/pinned allocations and frees, 11 the
 * longest single synchronization, 12 its source line in the library, 13 allocations + frees made. */
int hm_last_timings(const hm_ctx *ctx, double *ms, int32_t n);

/* ---- Kafka message values -> batch columns (reference heatmap_stream.py:51-61, 88-93) ----
 * The micro-batch's Kafka values (the producer's JSON records, mbta_to_kafka.py:66-74), back to back with
 * n + 1 offsets (Arrow binary/string layout; offsets[0] may be > 0), parsed on the device like
 * from_json(value, schema) in PERMISSIVE mode + to_timestamp(ts) (rules: csrc/json_decode.h): the columns of
 * hm_batch_in (device memory, valid until the next hm_decode_json on this context) with row_valid = provider,
 * vehicleId and eventTs non-null, and vkey = provider_code * n_vehicles + vehicle_code from the batch's exact
 * string dictionaries (code order unspecified; strings as Arrow offsets + UTF-8 bytes in pinned host memory, the
 * layout hm_encode_position_updates takes).  Records the device decoder does not handle (see json_decode.h) fail
 * the call with HM_E_UNSUPPORTED, unless flags holds HM_JSON_SPLICE: then they decode to all-null rows listed in
 * unsupported_rows, the dictionaries hold the other rows' strings only, and the caller decodes those records on the
 * host and writes them in with hm_json_patch before hm_process_batch (mobheat/engine.py decode_json).  Malformed
 * records decode to all-null rows (counted). */
#define HM_JSON_SPLICE 1
typedef struct hm_json_in {
    int64_t n;
    int32_t memory;            /* HM_MEM_HOST or HM_MEM_DEVICE: where bytes and offsets live */
    int32_t flags;             /* HM_JSON_SPLICE or 0 */
    const uint8_t *bytes;
    const int64_t *offsets;    /* n + 1 */
} hm_json_in;
typedef struct hm_json_out {
    hm_batch_in batch;         /* device columns, ready for hm_process_batch */
    int64_t n_providers;
    const int64_t *provider_offsets;   /* n_providers + 1 */
    const uint8_t *provider_bytes;
    int64_t n_vehicles;
    const int64_t *vehicle_offsets;    /* n_vehicles + 1 */
    const uint8_t *vehicle_bytes;
    int64_t n_malformed;       /* records that decoded to all-null rows (from_json's malformed records) */
    int64_t n_unsupported;     /* records outside the device decoder (HM_E_UNSUPPORTED, or spliced) */
    const int64_t *unsupported_rows;   /* HM_JSON_SPLICE: their row indices, ascending (host memory, valid until the
                                          next hm_decode_json) */
} hm_json_out;
int hm_decode_json(hm_ctx *ctx, const hm_json_in *in, hm_json_out *out);
/* The splice step: rows[k] (from unsupported_rows) of the last hm_decode_json get lat / lon / ts_us / speed /
 * speed_valid / row_valid and the dictionary codes pcode[k] / vcode[k] (host arrays, m entries; codes index the
 * extended dictionaries of n_providers / n_vehicles strings: the decoder's strings with the caller's appended);
 * every other valid row's vkey is re-encoded for the new n_vehicles.  The batch from hm_decode_json then holds the
 * whole micro-batch. */
int hm_json_patch(hm_ctx *ctx, int64_t m, const int64_t *rows, const double *lat, const double *lon,
                  const int64_t *ts_us, const double *speed, const uint8_t *speed_valid, const uint8_t *row_valid,
                  const int64_t *pcode, const int64_t *vcode, int64_t n_providers, int64_t n_vehicles);

/* ---- Arrow columns -> batch columns on the device (the boundary's Spark / Arrow / pandas frames; reference
 * heatmap_stream.py:51-61,150) ----
 * The micro-batch's columns in Arrow's memory layout, in host memory (zero-copy views of a pyarrow Table, of pyspark's
 * collected Arrow batches or of a pandas frame converted to Arrow): the library copies them to the device and builds
 * hm_batch_in there -- lat / lon null -> NaN (fails between(), :101-102), speedKmh null -> speed_valid 0, row_valid =
 * provider, vehicleId and eventTs non-null (:99-103) -- and factorises provider and vehicleId with the exact device
 * string dictionaries of hm_decode_json (vkey = provider_code * n_vehicles + vehicle_code; the dictionaries come back
 * as Arrow offsets + UTF-8 bytes for hm_encode_position_updates).  Outputs as hm_decode_json (n_malformed and
 * n_unsupported 0), valid until the next hm_decode_json / hm_arrow_columns on this context. */
typedef struct hm_arrow_col {
    const void *values;        /* float64 (lat, lon, speed) / int64 (ts_us, microseconds UTC) values, or a string column's
                                  n + 1 offsets into data; NULL = the column is absent (every row null) */
    const uint8_t *data;       /* string columns: the UTF-8 bytes the offsets point into */
    const uint8_t *validity;   /* Arrow validity bitmap (bit validity_offset + i, least significant bit first); NULL =
                                  no nulls */
    int64_t validity_offset;
    int32_t offset_bytes;      /* string columns: 4 (Arrow string) or 8 (large_string) */
    int32_t unit;              /* ts_us only: 0 = microseconds, 1 = nanoseconds (pandas' datetime64[ns], handed over as it
                                  is: the device truncates toward zero to microseconds, as Arrow's unsafe cast does);
                                  0 for every other column */
} hm_arrow_col;
typedef struct hm_arrow_in {
    int64_t n;
    hm_arrow_col lat, lon, speed, ts_us, provider, vehicle;
} hm_arrow_in;
int hm_arrow_columns(hm_ctx *ctx, const hm_arrow_in *in, hm_json_out *out);

/* The distinct 900-s buckets floor(ts_s / 900) of the last hm_process_batch's latest rows, ascending (computed on
 * the device; *n = count, up to cap written): the buckets whose local offsets hm_encode_position_updates needs. */
int hm_last_latest_buckets(hm_ctx *ctx, int64_t *bucket_ids, int64_t cap, int64_t *n);

/* Host execution of the record decoder (json_decode.h) on n records (bytes readable up to 16 bytes past the last
 * record: the decoder reads 16-B windows); scratch (same size as bytes) receives escaped strings' decoded bytes.
 * Per record: lat, lon, speed (NaN when null), ts_us, bearing, accuracy, the provider / vehicleId spans (absolute
 * offsets into bytes, or into scratch when the JF_*_ESC flag is set) and the field flags. */
int hm_selftest_json_records(const uint8_t *bytes, const int64_t *offsets, int64_t n, uint8_t *scratch, double *lat,
                             double *lon, double *speed, int64_t *ts_us, int32_t *bearing, int32_t *accuracy,
                             int64_t *p_off, int32_t *p_len, int64_t *v_off, int32_t *v_len, uint32_t *flags);
/* Host execution of the decoder's decimal -> binary64 conversion: bits[i] = w[i] * 10^q[i] correctly rounded. */
int hm_selftest_decimal_to_double(const uint64_t *w, const int64_t *q, int64_t n, uint64_t *bits);

/* ---- read side (reference app.py:19-41 h3_boundary_geojson -> h3.cell_to_boundary) ----
 * cellToBoundary of n cells: vertex k of cell i at lat[10 i + k], lng[10 i + k] (degrees, upstream's vertex order;
 * unused slots NaN), nverts[i] vertices (5-10; 0 for an invalid index).  memory as hm_latlng_to_cell. */
int hm_cells_to_boundary(const uint64_t *cells, int64_t n, int32_t memory, int32_t device, double *lat, double *lng,
                         int32_t *nverts);
/* Host execution of the same device code (no GPU; the CPU tests compare it with the oracle). */
int hm_selftest_cells_to_boundary_host(const uint64_t *cells, int64_t n, double *lat, double *lng, int32_t *nverts);

/* ---- read side without MongoDB: the tile state's windows at any zoom level (reference app.py:45-69 reads the latest
 * window's tiles from the tiles collection; here they come straight from the state the engine holds) ----
 * live windows of the tile state, ascending by start: *n = count, up to cap written; keys[i] = live keys of window i
 * (either array may be NULL).  "Live" = not yet evicted by the watermark. */
int hm_live_windows(hm_ctx *ctx, int64_t *window_start_us, int64_t *keys, int64_t cap, int64_t *n);
/* the tiles of live window window_start_us at resolution res (0..h3_res): one record per distinct parent cell with
 * the cumulative count / n_speed / sums of its children (avg = sum / count on the caller's side; reserved = 0);
 * res == h3_res: the window's own keys.  One GPU pass over the window's table.  Records are in no particular order.
 * Library-owned (device or pinned host per out_memory: HM_MEM_DEVICE / HM_MEM_HOST), valid until the next call on the
 * context.  A window that is not live: *n = 0.  res outside 0..h3_res: HM_E_INVALID; between stage calls: HM_E_STATE.
 * Reads the state only (hm_state_version, the next batch and a checkpoint export in progress are unaffected); a
 * repeated call with the same window and resolution allocates nothing.
 * On a shard context (hm_config.shard_count > 1) the records cover the keys that rank owns: a parent whose children
 * are spread over several ranks appears once per such rank, and the caller adds the records of equal cell (they carry
 * sums, not averages, for that reason).  The library does not combine across ranks. */
int hm_window_rollup(hm_ctx *ctx, int64_t window_start_us, int32_t res, int32_t out_memory,
                     const hm_state_rec **recs, int64_t *n);
/* host execution of the kernels' h3_cell_to_parent (no GPU): out[i] = upstream cellToParent(cells[i], res) for
 * res <= the cells' resolution (resolution field := res, digits res+1..15 := 7) */
int hm_selftest_cell_to_parent(const uint64_t *cells, int64_t n, int32_t res, uint64_t *out);

/* ---- latest position per vehicle across batches (reference heatmap_stream.py:217-228: the positions_latest collection;
 * app.py:71-88 reads it) ----
 * An opt-in, device-resident state S: (provider bytes, vehicleId bytes) -> (ts_us, lat, lon).  The two strings are a
 * pair, not a concatenation; an empty string is a valid part; comparison is byte-exact.  Folding a batch walks its
 * latest_row in ascending row order: row i of key k replaces S[k] iff k is absent or ts_us[i] > S[k].ts_us (strictly) --
 * what the collection holds after the reference's statements are applied in order.  lat / lon are the input doubles
 * bit for bit; folding a batch twice changes nothing; nothing is evicted (the collection has no TTL).
 * The state is keyed by the strings because a batch's vkey is built from that batch's own dictionaries: the same
 * vehicle has another vkey in the next batch.  None of these calls touches the tile state or hm_state_version. */
typedef struct hm_position_rec {
    uint32_t provider;   /* persistent codes: indices into the dictionaries hm_positions_export returns */
    uint32_t vehicle;
    int64_t ts_us;
    double lat;
    double lon;
} hm_position_rec;   /* 32 B */
/* Folds the last hm_process_batch's latest rows into S.  dicts: the batch's dictionaries, as
 * hm_encode_position_updates takes them (host memory; the bucket fields are ignored), with that call's preconditions:
 * the batch's device inputs are still valid; without a processed batch HM_E_STATE.  A latest row whose codes fall
 * outside the dictionaries, or malformed offsets: HM_E_INVALID, S untouched.  A shard context (shard_count > 1):
 * HM_E_UNSUPPORTED (the stage API leaves latest rows on the rank that received them).  A batch without latest rows is
 * a no-op.  A batch that brings no new vehicle allocates nothing. */
int hm_positions_update(hm_ctx *ctx, const hm_position_doc_cfg *dicts);
/* S as *n records in no particular order, and the two persistent dictionaries in dicts (Arrow offsets + UTF-8 bytes;
 * the bucket fields 0).  Library-owned, in device or pinned host memory per out_memory (HM_MEM_DEVICE / HM_MEM_HOST),
 * valid until the next hm_positions_* call on the context. */
int hm_positions_export(hm_ctx *ctx, int32_t out_memory, const hm_position_rec **recs, int64_t *n,
                        hm_position_doc_cfg *dicts);
/* Restores an export (host memory) into a context whose positions state is empty (HM_E_STATE otherwise).  Duplicate
 * keys, duplicate dictionary strings, codes outside the dictionaries: HM_E_INVALID. */
int hm_positions_import(hm_ctx *ctx, const hm_position_rec *recs, int64_t n, const hm_position_doc_cfg *dicts);
/* up to n of: [0] keys, [1] pair-table capacity (slots), [2] provider strings, [3] vehicle strings, [4] arena bytes in
 * use (both dictionaries), [5] regrows since create (tables, arenas, code lists), [6] of those: the pair table's,
 * [7] the vehicle arena's, [8] the last hm_positions_update on the device, microseconds, upload of the dictionaries
 * included, [9] the same from the first kernel on.  All 0 on a context that never made a positions call. */
int hm_positions_info(const hm_ctx *ctx, int64_t *v, int32_t n);
/* Test seam: every string hash is cut to its low `bits` bits (0..64; 64 = off), so that unequal strings with equal
 * hashes are the common case.  Results stay exact.  Only while the state is empty (HM_E_STATE otherwise). */
int hm_positions_debug_hash_bits(hm_ctx *ctx, int32_t bits);

/* ---- the read side's response bodies as GeoJSON, encoded on the GPU (reference app.py:45-88: api_tiles_latest /
 * api_positions_latest build one dict per tile / vehicle and json.dumps walks them) ----
 * Every call returns one contiguous response body and the features' offsets in it:
 *   bytes[0, 40)                      {"type":"FeatureCollection","features":[
 *   bytes[offsets[i], offsets[i+1]-1) feature i, exactly json.dumps(feature, separators=(",", ":")) of the feature
 *                                     mobheat/readside.py builds (ensure_ascii, NaN / Infinity / -Infinity as json.dumps)
 *   bytes[offsets[i+1]-1]             ',' after every feature but the last, ']' after the last
 *   bytes[offsets[n]]                 '}'
 * offsets has n + 1 entries, offsets[0] = 40.  The body is bytes[0, offsets[n] + 1) for n >= 1.  For n == 0 there is no
 * separator slot: offsets[0] = 40 and the body is the 42 bytes {"type":"FeatureCollection","features":[]}, so the body
 * length is offsets[n] + (n ? 1 : 2) and a caller never reads past "]}".  Doubles are written as Python's float.__repr__
 * writes them (shortest round-trip digits, csrc/float_repr.h).  Outputs are library-owned, in device or pinned host
 * memory per out_memory (HM_MEM_DEVICE / HM_MEM_HOST), valid until the next call on the context; the encoders use
 * buffers of their own (a streamed statement encode and a checkpoint export in progress are unaffected), and a repeated
 * call of the same size allocates nothing.  Not between stage calls (HM_E_STATE).
 *
 * Tile feature (one call = one window, so the two window texts are per call):
 *   {"type":"Feature","geometry":{"type":"Polygon","coordinates":[[[lng,lat],...]]},"properties":{"cellId":"<hex>",
 *    "count":<int>,"avgSpeedKmh":<repr>,"windowStart":"<text>","windowEnd":"<text>"}}
 * ring: the cell's boundary (hm_cells_to_boundary: upstream order, degrees), the first vertex repeated at the end iff
 * there is one and it differs from the last by value; an invalid cell index gives "coordinates":[[]].  cellId =
 * format(cell, "x"); count in decimal; avgSpeedKmh = 0.0 when n_speed == 0, else sum_speed / n_speed (IEEE binary64
 * division; a NaN sum prints NaN).  window_start_text / window_end_text: the caller's pre-formatted ASCII, e.g.
 * datetime.isoformat() of the wall time, at most 40 bytes each of 0x20-0x7e without '"' and '\' (HM_E_INVALID otherwise). */
typedef struct hm_geojson_cfg {
    const char *window_start_text;
    int32_t start_len;
    const char *window_end_text;
    int32_t end_len;
} hm_geojson_cfg;
/* the features of n caller records (recs in host or device memory per `memory`; window_start_us, sums of lat / lon and
 * reserved are not read) */
int hm_encode_tile_features(hm_ctx *ctx, const hm_geojson_cfg *cfg, int64_t n, int32_t memory, const hm_state_rec *recs,
                            int32_t out_memory, const uint8_t **bytes, const int64_t **offsets);
/* hm_window_rollup of live window window_start_us at res (same validity rules, same errors; a window that is not live:
 * *n = 0 and the empty body) and its records' features, the records never leaving the device.  recs (optional): the
 * records in feature order, pinned host memory.  Reads the tile state only: hm_state_version, the next batch and a
 * checkpoint export in progress are unaffected. */
int hm_window_geojson(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                      const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs);
/* Host execution of the same encoder (no GPU): the whole body into bytes (cap bytes: HM_E_INVALID if they do not
 * suffice, at least 42), offsets n + 1 entries. */
int hm_selftest_tile_features(const hm_geojson_cfg *cfg, const hm_state_rec *recs, int64_t n, uint8_t *bytes, int64_t cap,
                              int64_t *offsets);

/* Position feature, from the positions state S (hm_positions_update):
 *   {"type":"Feature","geometry":{"type":"Point","coordinates":[lon,lat]},"properties":{"provider":"..","vehicleId":"..",
 *    "ts":"YYYY-MM-DDTHH:MM:SS[.ffffff]"}}
 * The strings come from S's persistent dictionaries, escaped as json.dumps(ensure_ascii=True) escapes them (\" \\ \n \r
 * \t \b \f, every other byte below 0x20, 0x7f and every non-ASCII code point as \uxxxx in lowercase hex, a code point
 * above U+FFFF as a surrogate pair); a string that is not valid UTF-8 fails the call (HM_E_INVALID).  ts =
 * datetime.isoformat() of the naive wall time of ts_us shifted by the local offset of its 900-s bucket floor(ts_s / 900)
 * (bucket_ids / bucket_offset_s of hm_position_doc_cfg, strictly ascending; the other fields are not read); the fraction
 * only when the microseconds are non-zero.  A record whose bucket is absent, or a local year outside 1..9999: HM_E_INVALID.
 * Neither call touches the tile state or S.  A shard context (shard_count > 1): HM_E_UNSUPPORTED, as hm_positions_update. */
/* the distinct 900-s buckets of S's ts, ascending (*n = count; up to cap written) */
int hm_positions_buckets(hm_ctx *ctx, int64_t *bucket_ids, int64_t cap, int64_t *n);
/* recs (optional): S's records in feature order, pinned host memory (codes index hm_positions_export's dictionaries) */
int hm_positions_geojson(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                         const int64_t **offsets, int64_t *n, const hm_position_rec **recs);
/* Host execution of the same encoder on caller records, dictionaries (Arrow offsets + bytes) and buckets (no GPU); a
 * record outside the dictionaries or buckets, a bad string or year, or cap too small: HM_E_INVALID. */
int hm_selftest_position_features(const hm_position_doc_cfg *cfg, const hm_position_rec *recs, int64_t n, uint8_t *bytes,
                                  int64_t cap, int64_t *offsets);
/* up to n of, for the last GeoJSON call on the context (HIP events): [0] its sizes kernel (for tiles: the boundaries
 * included), microseconds, [1] its write kernel, [2] from the first kernel to the last, the offsets' scan and its
 * read-back included, [3] the body's length in bytes, [4] the candidates of the last hm_*_geojson_view call (the roll-up's
 * records, or the positions state's keys), [5] that call's filter kernel, microseconds. */
int hm_geojson_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- the same bodies for a map viewport (a Leaflet client's bbox), filtered on the GPU ----
 * A view is (west, south, east, north) in degrees, valid when all four are finite, -90 <= south <= north <= 90 and
 * -180 <= west, east <= 180; its longitudes are [west, east], or [west, 180] U [-180, east] when west > east (the view
 * crosses the antimeridian).  Every interval is closed and every test a plain binary64 comparison: no tolerance.
 *   position  in view iff south <= lat <= north and lon is one of the view's longitudes (the stored doubles).
 *   tile      in view iff the latitude-longitude box of its boundary ring (hm_cells_to_boundary's vertices) meets the
 *             view: latitudes [min lat, max lat]; longitudes [min lng, max lng], unless max lng - min lng > 180 -- the
 *             ring wraps: [min of the lng > 0, 180] U [-180, max of the lng <= 0].  The two cells of a resolution that
 *             contain a pole (latLngToCell(+-90, 0, res)) cover every longitude and latitudes up to their pole.  An
 *             invalid index (0 vertices) is never in view.  "Meets": the latitude ranges intersect and an interval of
 *             one longitude set intersects an interval of the other.
 * An invalid view: HM_E_INVALID, nothing touched. */
typedef struct { double west, south, east, north; } hm_view;
/* keep_u8[i] = 1 iff cells[i] is in view (cells of any mix of resolutions; memory / device as hm_cells_to_boundary:
 * with HM_MEM_DEVICE cells and keep_u8 are device pointers) */
int hm_cells_in_view(const uint64_t *cells, int64_t n, int32_t memory, int32_t device, const hm_view *view, uint8_t *keep_u8);
/* Host execution of the same code (no GPU). */
int hm_selftest_cells_in_view(const uint64_t *cells, int64_t n, const hm_view *view, uint8_t *keep_u8);
/* hm_window_geojson of the tiles in view: roll up, filter, encode the kept records; *n = the kept count, recs (optional)
 * the kept records in feature order; none kept: the 42-byte empty body.  hm_window_geojson's errors, and HM_E_INVALID
 * for an invalid view.  On a shard context: the rank's own keys, as hm_window_rollup.  Reads only, as hm_window_geojson;
 * a repeated call allocates nothing. */
int hm_window_geojson_view(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                           const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs,
                           const hm_view *view);
/* hm_positions_geojson of the positions in view (*n = the kept count); its errors, and HM_E_INVALID for an invalid view */
int hm_positions_geojson_view(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                              const int64_t **offsets, int64_t *n, const hm_position_rec **recs, const hm_view *view);

/* ---- a live window as a raster, for web-map z/x/y tiles (the reference's UI loads its base layer as such tiles,
 * app.py:122, and colours hexagons in seven count classes, colorByCount, app.py:135-142) ----
 * The grid is separable: rows latitudes lat[rows] and cols longitudes lon[cols], degrees, host memory; pixel (r, c) has
 * the centre (lat[r], lon[c]) and the index r * cols + c.  The caller projects (mobheat/readside.py tile_grid: the pixel
 * centres of slippy-map tile z/x/y); the library never does.  A pixel's value is the count of the record hm_window_rollup
 * gives for the cell latLngToCell(lat[r], lon[c], res) -- the hexagon that contains the pixel's centre, the one
 * hm_window_geojson draws there; exact, no tolerance.  A NaN or out-of-range coordinate has no cell: count 0.
 *   counts   uint32 per pixel: the record's count saturated at 0xFFFFFFFF; 0 where the window has no tile at that cell
 *   classes  uint8 per pixel (only with n_thresholds > 0 and classes non-NULL; classes may be NULL otherwise): the number
 *            of thresholds t with count > t -- strict, on the unsaturated 64-bit count.  thresholds: host memory, 0..15 of
 *            them, each >= 0, strictly ascending.  (0, 2, 5, 10, 20, 50) gives colorByCount's classes, 0 = no tile.
 * Outputs as hm_window_rollup's: library-owned, device or pinned host memory per out_memory, valid until the next call on
 * the context; buffers of the raster's own.  Reads the state only (hm_state_version, the next batch and a checkpoint
 * export in progress are unaffected); a repeated call of the same shape allocates nothing.  A window that is not live:
 * an all-zero grid.  rows * cols == 0: HM_OK, nothing written (*counts NULL).  HM_E_INVALID, the message naming the limit:
 * rows or cols < 0 or > 16384, rows * cols > 2^26, bad thresholds, res outside 0..h3_res.  Between stage calls: HM_E_STATE.
 * On a shard context the counts cover the keys that rank owns: the caller adds the ranks' grids (counts add exactly up to
 * the saturation) and classifies the sum; n_thresholds > 0 there is HM_E_INVALID. */
int hm_window_raster(hm_ctx *ctx, int64_t window_start_us, int32_t res, const double *lat, int32_t rows, const double *lon,
                     int32_t cols, const int64_t *thresholds, int32_t n_thresholds, int32_t out_memory,
                     const uint32_t **counts, const uint8_t **classes);
/* Host execution of the same per-pixel code on caller records (no GPU; records of equal cell add up; window_start_us and
 * the sums are not read).  res 0..15; the grid's and the thresholds' limits as above. */
int hm_selftest_window_raster(const hm_state_rec *recs, int64_t n, int32_t res, const double *lat, int32_t rows,
                              const double *lon, int32_t cols, const int64_t *thresholds, int32_t n_thresholds,
                              uint32_t *counts, uint8_t *classes);
/* up to n of, for the last hm_window_raster call on the context: [0] its pixels, [1] of those, the pixels the fast
 * latLngToCell handed to the exact path, [2] the records in the roll-up's table (0: the window was not live), [3] its two
 * kernels, microseconds (HIP events). */
int hm_raster_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- the positions state S as H3 density cells: how many vehicles are in each cell right now ----
 * density(S, res, since_us), res 0..15 -- independent of the context's h3_res: positions are raw coordinates.
 *   kept keys  a key of S is kept iff ts_us >= since_us (a plain int64 compare; INT64_MIN keeps every key).  S is never
 *              evicted, so since_us is how a reader leaves out vehicles that stopped reporting.
 *   snapping   each kept key by latLngToCell(lat, lon, res), exactly the cell hm_latlng_to_cell gives.  A key without a
 *              cell (hm_positions_import does not check coordinates: NaN, |lat| > 90, |lon| > 180) belongs to no group
 *              and is counted as unsnapped.
 *   groups     one hm_state_rec per distinct cell, in no particular order: cell; count = the vehicles in it; sum_lat /
 *              sum_lon = the sums of their stored doubles (fp64 adds in arrival order, as hm_window_rollup's: avg = sum /
 *              count on the caller's side); n_speed 0, sum_speed +0.0, reserved 0; and window_start_us REUSED for the
 *              NEWEST ts_us in the group (S has no window; the field tells how fresh a cell's count is).
 *   view       (optional) a group is kept iff its CELL is in view by hm_cells_in_view's tile rule (the ring's box, pole
 *              cells, antimeridian) -- not a point test on the vehicles: a hexagon on the view's edge shows its whole
 *              count, so panning does not change numbers.
 * An empty S, a since_us newer than every key or a view that meets nothing: *n = 0.  Records are library-owned, in device
 * or pinned host memory per out_memory (HM_MEM_DEVICE / HM_MEM_HOST), valid until the next hm_positions_* call on the
 * context; hm_encode_tile_features(..., HM_MEM_DEVICE, recs, ...) on the same context may read the device records (the
 * encoder has buffers of its own) -- the tile feature is the density's feature.  The calls read S only: S, the tile state,
 * hm_state_version and a roll-up's table (hm_window_raster) are unaffected, and a repeated call of the same size allocates
 * nothing.  res outside 0..15, a bad out_memory, an invalid view: HM_E_INVALID, nothing touched.  A shard context
 * (shard_count > 1): HM_E_UNSUPPORTED, as hm_positions_update.  Between stage calls: HM_E_STATE. */
int hm_positions_density(hm_ctx *ctx, int32_t res, int64_t since_us, const hm_view *view /* NULL: no filter */,
                         int32_t out_memory, const hm_state_rec **recs, int64_t *n);
/* hm_window_raster's grid, thresholds, limits, saturation, classes and outputs (its buffers too); a pixel's value is the
 * density count of latLngToCell(lat[r], lon[c], res), 0 where no kept vehicle is in that cell.  hm_raster_info afterwards
 * reports this call ([2]: the density's groups).  Errors as hm_positions_density's and hm_window_raster's grid errors. */
int hm_positions_density_raster(hm_ctx *ctx, int32_t res, int64_t since_us, const double *lat, int32_t rows,
                                const double *lon, int32_t cols, const int64_t *thresholds, int32_t n_thresholds,
                                int32_t out_memory, const uint32_t **counts, const uint8_t **classes);
/* Host execution of the same per-key code on caller records, no view (no GPU): the groups into out (cap records; *n_out =
 * their number, HM_E_INVALID if cap does not suffice), *unsnapped (optional) = the kept keys without a cell.  Sums are added
 * in record order. */
int hm_selftest_positions_density(const hm_position_rec *recs, int64_t n, int32_t res, int64_t since_us,
                                  hm_state_rec *out, int64_t cap, int64_t *n_out, int64_t *unsnapped);
/* up to n of, for the last density call on the context (either entry point): [0] keys scanned, [1] keys kept by since_us,
 * [2] unsnapped keys, [3] groups before the view, [4] groups returned, [5] keys that took the exact latLngToCell path,
 * [6] adds into the group-by's global table (spills of the per-workgroup tables plus their final flushes), [7] workgroups
 * the group-by launched, [8] device time from the first kernel to the last, microseconds (HIP events; with a view the filter kernel's time is
 * added, the host's read of the group count in between is not), [9] the global
 * table's slots.  All 0 before the first call. */
int hm_positions_density_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- top-k hotspots: the k records with the largest count, in rank order, selected and ordered on the GPU ----
 * The order: record a ranks before record b iff, lexicographically,
 *   1. a.count > b.count, counts compared as int64 (the library's own records have count >= 1; caller records may hold 0
 *      or negative counts);
 *   2. a.cell < b.cell as uint64;
 *   3. a has the lower input index (decides only among caller records with repeated (count, cell); roll-up and density
 *      records have distinct cells).
 * Only count and cell are read; top(recs, k) = the first min(k, n) records of that order, in that order, each returned
 * whole and unchanged, bit for bit.  k is 0..HM_TOP_MAX (a contract limit: no page draws more); k < 0 or k > HM_TOP_MAX:
 * HM_E_INVALID, nothing touched.  k == 0 or no candidate: HM_OK with *n = 0.
 * Outputs are library-owned, in device or pinned host memory per out_memory (HM_MEM_DEVICE / HM_MEM_HOST), valid until
 * the next call on the context; the top has buffers of its own (a checkpoint export in progress, a streamed statement
 * encode and the GeoJSON encoder's buffers are unaffected).  The calls read state only: hm_state_version, the tile
 * state and the positions state are untouched, and a repeated call of the same size allocates nothing.  Between stage
 * calls: HM_E_STATE. */
#define HM_TOP_MAX 65536
/* top(recs[0, n), k) of caller records in host or device memory per `memory` (as hm_encode_tile_features takes them; n at
 * most 2^31; device records 16-byte aligned).  Allowed on a shard context: a sharded caller adds the ranks' records of
 * equal cell and ranks the sums here. */
int hm_top_records(hm_ctx *ctx, const hm_state_rec *recs, int64_t n, int32_t memory, int64_t k, int32_t out_memory,
                   const hm_state_rec **top, int64_t *n_top);
/* top(hm_window_rollup(window_start_us, res) [cut to view, hm_window_geojson_view's rule], k): the view is applied
 * before the selection, so the result is the busiest tiles in view.  hm_window_rollup's validity rules and errors,
 * HM_E_INVALID for an invalid view; a window that is not live: *n = 0.  A shard context (shard_count > 1):
 * HM_E_UNSUPPORTED -- a rank's own top-k is not the global one when a parent's children are spread over ranks. */
int hm_window_top(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_view *view /* NULL: no filter */, int64_t k,
                  int32_t out_memory, const hm_state_rec **recs, int64_t *n);
/* The same, then the selected records' features in rank order by hm_window_geojson's encoder, the records never leaving
 * the device: body, offsets and *n as hm_window_geojson's (none selected: the 42-byte empty body); recs (optional): the
 * records in feature order, pinned host memory.  Errors as hm_window_top's and hm_window_geojson's. */
int hm_window_geojson_top(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg,
                          const hm_view *view /* NULL: no filter */, int64_t k, int32_t out_memory, const uint8_t **bytes,
                          const int64_t **offsets, int64_t *n, const hm_state_rec **recs);
/* top(hm_positions_density(res, since_us, view), k): the density's groups, selected and ranked (window_start_us keeps
 * its reused meaning, the cell's newest ts_us).  hm_positions_density's errors (a shard context: HM_E_UNSUPPORTED).  The
 * GeoJSON form is hm_encode_tile_features(..., HM_MEM_DEVICE, recs, ...) on the ranked device records: the features come
 * out in rank order. */
int hm_positions_density_top(hm_ctx *ctx, int32_t res, int64_t since_us, const hm_view *view /* NULL: no filter */,
                             int64_t k, int32_t out_memory, const hm_state_rec **recs, int64_t *n);
/* Host execution of the select and the ordering with the kernels' own key, digit and comparator code (no GPU):
 * top(recs, k) into out (room for min(k, n) records), *n_out = min(k, n). */
int hm_selftest_top_records(const hm_state_rec *recs, int64_t n, int64_t k, hm_state_rec *out, int64_t *n_out);
/* up to n of, for the last top call on the context: [0] candidates (after the view), [1] records returned, [2] select
 * passes that examined a byte of the count, [3] of the cell, [4] of the input index, [5] the candidates still tied with
 * the threshold when the select stopped -- all of them are taken, so this is also what was still needed then, [6] device
 * time of the top's own kernels from the key extraction to the ordered records, microseconds (HIP events; the host's
 * read-backs between the passes are not counted, nor are the roll-up, the density or the view filter).  All 0 before
 * the first call. */
int hm_top_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- radius queries: the vehicles / tiles nearest a point, nearest first (what the reference's 2dsphere indexes on
 * positions_latest.loc and tiles.centroid serve: $nearSphere, $geoWithin $centerSphere) ----
 * Distance of the query point (lat0, lon0) to a candidate (lat, lon), degrees, in binary64, every operation one
 * rounding in this order, no FMA contraction:
 *   D   = 0.017453292519943295                      (the double Python's math.radians multiplies by)
 *   p0  = lat0 * D;  p1 = lat * D
 *   s_h = sin((p1 - p0) * 0.5);  s_l = sin(((lon - lon0) * D) * 0.5);  c0 = cos(p0);  c1 = cos(p1)
 *   a   = s_h * s_h + (c0 * c1) * (s_l * s_l)
 *   r   = sqrt(a);  if (r > 1.0) r = 1.0
 *   d   = (2.0 * HM_EARTH_RADIUS_M) * asin(r)
 * sin / cos / asin are glibc's (csrc/glibc_libm.h, the ones latLngToCell and cellToBoundary use), sqrt the correctly
 * rounded one.  The longitude difference is not normalised: sin^2 of its half is periodic, the antimeridian needs no
 * case.  +0.0 <= d <= pi R, or NaN when a stored coordinate is not finite (hm_positions_import does not check them): a
 * NaN candidate is dropped and counted (hm_near_info).  mobheat/readside.py near_distance_m is the same lines in Python;
 * equality is bit equality of d -- there is no tolerance anywhere.
 *   filter  a candidate is kept iff d <= max_distance_m, a closed comparison; max_distance_m finite and >= 0, or +inf
 *           for no limit.  Positions calls also take since_us with hm_positions_density's meaning (kept iff ts_us >=
 *           since_us; INT64_MIN keeps all).
 *   order   nearest first; ties by the second key word ascending -- provider code << 32 | vehicle code for positions,
 *           the cell for tiles --, then by the candidate's input index (decides only among caller records that repeat
 *           both).  As the top's key: word 0 = the bits of d (non-negative doubles order as unsigned integers).
 *   k       0..HM_TOP_MAX with the top's rules: outside gives HM_E_INVALID, k == 0 gives HM_OK with *n = 0.
 *   a tile's point is its centroid as the sink writes it: (sum_lat / count, sum_lon / count) of the rolled-up record,
 *           one division each, computed before the distance.
 * Query validation: lat in [-90, 90], lon in [-180, 180], max_distance_m >= 0 or +inf, none NaN; anything else:
 * HM_E_INVALID, nothing touched.  Outputs are library-owned with buffers of their own, in device or pinned host memory
 * per out_memory, valid until the next call on the context; the calls read state only (hm_state_version untouched) and
 * a repeated call of the same size allocates nothing. */
#define HM_EARTH_RADIUS_M 6378100.0   /* MongoDB's sphere */
typedef struct { double lat, lon, max_distance_m; } hm_near;
/* dist_m[i] = d(q, (lat[i], lon[i])) on GPU `device`; memory / device as hm_cells_to_boundary (with HM_MEM_DEVICE lat,
 * lon and dist_m are device pointers).  max_distance_m is validated, not applied. */
int hm_near_distances(const hm_near *q, const double *lat, const double *lon, int64_t n, int32_t memory, int32_t device,
                      double *dist_m);
/* Host execution of the same code (no GPU). */
int hm_selftest_near_distances(const hm_near *q, const double *lat, const double *lon, int64_t n, double *dist_m);
/* The k nearest of the positions state S within the radius: *n records in rank order and their distances.  State
 * errors as hm_positions_density's (a shard context: HM_E_UNSUPPORTED; between stage calls: HM_E_STATE); an empty S:
 * *n = 0. */
int hm_positions_near(hm_ctx *ctx, const hm_near *q, int64_t since_us, int64_t k, int32_t out_memory,
                      const hm_position_rec **recs, const double **dist_m, int64_t *n);
/* The k tiles of hm_window_rollup(window_start_us, res) whose centroid is nearest within the radius.  hm_window_top's
 * rules: a window that is not live: *n = 0; a shard context: HM_E_UNSUPPORTED (a parent split over ranks has no
 * rank-local centroid); between stage calls: HM_E_STATE. */
int hm_window_near(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_near *q, int64_t k, int32_t out_memory,
                   const hm_state_rec **recs, const double **dist_m, int64_t *n);
/* hm_positions_near, then the ranked records' features in rank order by hm_positions_geojson's encoder with
 * ,"distanceM":<repr of d> appended as the last property, the records never leaving the device: body, offsets and *n as
 * hm_positions_geojson's (none returned: the 42-byte empty body); recs / dist_m (optional): the records in feature order
 * and their distances, pinned host memory.  Errors as hm_positions_near's and hm_positions_geojson's. */
int hm_positions_geojson_near(hm_ctx *ctx, const hm_position_doc_cfg *buckets, const hm_near *q, int64_t since_us, int64_t k,
                              int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n,
                              const hm_position_rec **recs, const double **dist_m);
/* hm_window_near, then the tile features in rank order with distanceM as their last property; as hm_window_geojson_top. */
int hm_window_geojson_near(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, const hm_near *q,
                           int64_t k, int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n,
                           const hm_state_rec **recs, const double **dist_m);
/* hm_selftest_tile_features / hm_selftest_position_features with an optional distance per record (dist_m NULL: the
 * bytes of those calls): host execution of the encoders the near bodies use. */
int hm_selftest_tile_features_near(const hm_geojson_cfg *cfg, const hm_state_rec *recs, int64_t n, const double *dist_m,
                                   uint8_t *bytes, int64_t cap, int64_t *offsets);
int hm_selftest_position_features_near(const hm_position_doc_cfg *cfg, const hm_position_rec *recs, int64_t n,
                                       const double *dist_m, uint8_t *bytes, int64_t cap, int64_t *offsets);
/* Host execution of the filter, the keys, the select and the ordering with the kernels' own code on caller records (no
 * GPU): out / dist_m have room for min(k, n), *n_out = the records returned. */
int hm_selftest_positions_near(const hm_near *q, int64_t since_us, const hm_position_rec *recs, int64_t n, int64_t k,
                               hm_position_rec *out, double *dist_m, int64_t *n_out);
int hm_selftest_tiles_near(const hm_near *q, const hm_state_rec *recs, int64_t n, int64_t k, hm_state_rec *out,
                           double *dist_m, int64_t *n_out);
/* up to n of, for the last near call on the context: [0] pair-table slots / roll-up records scanned, [1] kept by since_us,
 * [2] dropped as NaN, [3] within the radius (the select's candidates), [4] returned, [5] select passes, [6] device
 * microseconds of the emit kernel, [7] of the select and the scatter (HIP events, as the top's).  All 0 before the first
 * call. */
int hm_near_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- polygon geofences: the vehicles / tiles inside zones (the other half of what the reference's 2dsphere indexes
 * serve: $geoWithin: {$geometry: Polygon}) ----
 * A zone set is n_zones zones; zone z is the rings zone_rings[z] .. zone_rings[z + 1] - 1 (a GeoJSON Polygon's exterior
 * and holes; a MultiPolygon is one zone of all its rings); ring r is the vertices ring_verts[r] .. ring_verts[r + 1] - 1
 * of (lat, lon) in degrees, at least 3, WITHOUT the repeated closing vertex; edge k of a ring runs from its vertex k to
 * its vertex (k + 1) mod n.  Edges are straight in the (lon, lat) plane, as RFC 7946 and the reference page's map draw
 * them (MongoDB's geodesic edges are not reproduced); a zone across the antimeridian is the caller's to split, longitudes
 * are never normalised; ring orientation is free.
 *   membership  a point (lat, lon) is in a zone iff it crosses an odd number of the zone's edges, all rings together
 *               (holes need no case).  Edge (a, b), in binary64, one rounding per operation in this order, no FMA:
 *                 a.lat == b.lat: never crossed;  else the endpoints ordered so that a.lat < b.lat
 *                 straddles = (a.lat <= lat) && (lat < b.lat)
 *                 crossed   = straddles && ((b.lon - a.lon) * (lat - a.lat) > (lon - a.lon) * (b.lat - a.lat))
 *               The ordering makes two zones that share an edge evaluate one predicate for it: zones that tile a region
 *               hold each of its points an odd number of times.  A NaN coordinate is in no zone.
 *               mobheat/readside.py points_in_zones is the same lines in numpy; there is no tolerance anywhere.
 *   overlap     per-zone totals count a point in EVERY zone that contains it; a kept record's label is the LOWEST-index
 *               zone that contains it.
 *   a tile's point is its centroid as the near queries take it (sum_lat / count, sum_lon / count, one division each).
 * Validation: n_zones <= HM_ZONES_MAX, at most HM_ZONE_VERTS_MAX vertices in total, zone_rings[0] = ring_verts[0] = 0,
 * every zone at least one ring, every ring at least 3 vertices, every vertex finite with -90 <= lat <= 90 and
 * -180 <= lon <= 180; anything else: HM_E_INVALID, nothing touched, the message names the limit.  The zone arrays are
 * host memory and are read during the call only. */
#define HM_ZONES_MAX 4096
#define HM_ZONE_VERTS_MAX 65536
typedef struct { int32_t n_zones; const int32_t *zone_rings;  /* n_zones + 1: a zone's rings */
                 const int32_t *ring_verts;                    /* n_rings + 1: a ring's vertices */
                 const double *lat, *lon; } hm_zones;          /* host memory */
typedef struct { int64_t n;          /* vehicles / tiles in the zone */
                 int64_t count;      /* vehicles again / the tiles' summed count */
                 int64_t n_speed; double sum_speed;            /* tiles: summed; positions: 0, +0.0 */
                 int64_t newest_us;  /* positions: the zone's newest ts_us (INT64_MIN when empty); tiles: 0 */
                 int64_t reserved; } hm_zone_rec;              /* 48 B */
/* first_zone_i32[i] = the lowest zone that contains (lat[i], lon[i]) or -1, hits_u32[i] = how many zones contain it, on
 * GPU `device`; memory / device as hm_near_distances (with HM_MEM_DEVICE lat, lon and the two outputs are device
 * pointers; the zone set is host memory always). */
int hm_points_in_zones(const hm_zones *zones, const double *lat, const double *lon, int64_t n, int32_t memory, int32_t device,
                       int32_t *first_zone_i32, uint32_t *hits_u32);
/* Host execution of the same predicate (no GPU, no reject ahead of the edges). */
int hm_selftest_points_in_zones(const hm_zones *zones, const double *lat, const double *lon, int64_t n, int32_t *first_zone_i32,
                                uint32_t *hits_u32);
/* The vehicles of the positions state S with ts_us >= since_us (hm_positions_density's meaning; INT64_MIN keeps all)
 * that are in at least one zone, in one scan of the pair table: *n of them; with recs != NULL the records and their
 * labels (a set: in no particular order; library-owned, device or pinned host memory per out_memory, valid until the
 * next call on the context); recs == NULL: totals only (zone may be NULL then).  totals (host memory, n_zones records,
 * may be NULL): every zone's n = count = its vehicles, newest_us their newest ts_us.  State errors as
 * hm_positions_near's (a shard context: HM_E_UNSUPPORTED; between stage calls: HM_E_STATE); an empty S: *n = 0. */
int hm_positions_within(hm_ctx *ctx, const hm_zones *zones, int64_t since_us, int32_t out_memory, hm_zone_rec *totals,
                        const hm_position_rec **recs, const int32_t **zone, int64_t *n);
/* The same over the tiles of hm_window_rollup(window_start_us, res) by their centroid: totals n = the zone's tiles,
 * count / n_speed / sum_speed their sums (sum_speed an fp64 sum in no particular order).  hm_window_near's rules: a
 * window that is not live: *n = 0 and zero totals; a shard context: HM_E_UNSUPPORTED; between stage calls: HM_E_STATE;
 * res outside 0..h3_res: HM_E_INVALID. */
int hm_window_within(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_zones *zones, int32_t out_memory,
                     hm_zone_rec *totals, const hm_state_rec **recs, const int32_t **zone, int64_t *n);
/* hm_positions_geojson_view / hm_window_geojson_view with a zone set in place of the view: the features of the records
 * in at least one zone (every vehicle of S / every tile of the window), the feature bytes unchanged (no new property),
 * the records never leaving the device between the scan and the encoder; none kept: the 42-byte empty body. */
int hm_positions_geojson_within(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                                const int64_t **offsets, int64_t *n, const hm_position_rec **recs, const hm_zones *zones);
int hm_window_geojson_within(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                             const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs,
                             const hm_zones *zones);
/* Host execution of the two queries on caller records (no GPU): the kept records in input order with their labels
 * (out / zone: room for n, or both NULL), the totals (n_zones records, may be NULL), *n_out = the records kept. */
int hm_selftest_positions_within(const hm_zones *zones, int64_t since_us, const hm_position_rec *recs, int64_t n,
                                 hm_zone_rec *totals, hm_position_rec *out, int32_t *zone, int64_t *n_out);
int hm_selftest_tiles_within(const hm_zones *zones, const hm_state_rec *recs, int64_t n, hm_zone_rec *totals, hm_state_rec *out,
                             int32_t *zone, int64_t *n_out);
/* up to n of, for the last within call on the context: [0] pair-table slots / roll-up records scanned, [1] kept by
 * since_us, [2] in at least one zone, [3] the set's zones, [4] its vertices, [5] device microseconds of the scan (HIP
 * events around it).  All 0 before the first call. */
int hm_within_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- change between two live windows: where traffic rises or falls against the window before ----
 * change(A, B, r): A = live window window_start_us (the current one), B = live window base_start_us (the base),
 * 0 <= r <= h3_res.  With RA = hm_window_rollup(A, r) and RB = hm_window_rollup(B, r), the result holds one pair per cell
 * of cells(RA) U cells(RB), in no particular order: cur is, bit for bit, RA's record of the cell and base RB's; a window
 * without the cell (or a window that is not live) contributes the zero record {cell, that window's start, 0, 0, 0.0,
 * 0.0, 0.0, 0}.  Nothing is added across windows; countChange = cur.count - base.count as int64 (counts are >= 0: no
 * overflow).  Neither window live: *n = 0.  window_start_us == base_start_us: HM_E_INVALID.  A resolution out of range, a
 * call between stage calls and a parent-table overflow are reported as hm_window_rollup reports them.
 * view (NULL: none) keeps a pair iff hm_window_geojson_view's rule keeps its cell, before any ranking.
 * Outputs are library-owned with buffers of their own, in device or pinned host memory per out_memory, valid until the
 * next call on the context; the calls read the state only (hm_state_version, the tile and positions states, a checkpoint
 * export in progress and a streamed statement encode are unaffected); a repeated call of the same size allocates
 * nothing.  A change call counts as a roll-up for hm_window_rollup's buffers: its records handed out on the device, and
 * the parent table hm_window_raster answers from, are valid until the next roll-up OR change call. */
typedef struct hm_change_rec {   /* 128 B */
    hm_state_rec cur;    /* RA's record of the cell; absent: {cell, window_start_us, 0, 0, 0.0, 0.0, 0.0, 0} */
    hm_state_rec base;   /* RB's record of the cell; absent: {cell, base_start_us,   0, 0, 0.0, 0.0, 0.0, 0} */
} hm_change_rec;
#define HM_CHANGE_RISING 0    /* countChange descending */
#define HM_CHANGE_FALLING 1   /* countChange ascending */
#define HM_CHANGE_ABS 2       /* |countChange| descending (+c and -c tie) */
/* every pair.  On a shard context: the rank's own cells (a caller adds the halves of equal cell across ranks). */
int hm_window_change(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view /* NULL: no filter */,
                     int32_t out_memory, const hm_change_rec **recs, int64_t *n);
/* the first min(k, n) pairs of `order`, in that order, each whole and unchanged; ties break on the cell ascending as
 * uint64, then on the pair's index (the top's key, hm_top_records).  k outside 0..HM_TOP_MAX or an unknown order:
 * HM_E_INVALID, nothing touched.  A shard context: HM_E_UNSUPPORTED, as hm_window_top. */
int hm_window_change_top(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view /* NULL: no filter */,
                         int32_t order, int64_t k, int32_t out_memory, const hm_change_rec **recs, int64_t *n);
/* the same pairs as a FeatureCollection encoded where they lie: feature i is hm_window_geojson's feature of pair i's cur
 * half with ,"baseCount":<int>,"baseAvgSpeedKmh":<repr>,"countChange":<int> after windowEnd (baseAvgSpeedKmh by
 * avgSpeedKmh's rule: 0.0 without a speed).  k < 0: every pair in the join's order (order is ignored); else the ranked
 * ones (k <= HM_TOP_MAX; a shard context: HM_E_UNSUPPORTED).  Body, offsets and *n as hm_window_geojson's; nothing
 * selected: the 42-byte empty body.  recs (optional): the pairs in feature order, pinned host memory. */
int hm_window_geojson_change(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_geojson_cfg *cfg,
                             const hm_view *view /* NULL: no filter */, int32_t order, int64_t k, int32_t out_memory,
                             const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_change_rec **recs);
/* Host execution (no GPU) from two record arrays (cells distinct within each), with the kernels' pair-building, key and
 * comparator code: the zero halves carry window_start_us / base_start_us.  k < 0: every pair, sorted by cell; else the
 * first min(k, n) of `order`.  out: room for n_cur + n_base pairs (or min(k, that)). */
int hm_selftest_window_change(const hm_state_rec *cur, int64_t n_cur, const hm_state_rec *base, int64_t n_base,
                              int64_t window_start_us, int64_t base_start_us, int32_t order, int64_t k, hm_change_rec *out,
                              int64_t *n_out);
/* host execution of the encoder on n pairs, as hm_selftest_tile_features */
int hm_selftest_change_features(const hm_geojson_cfg *cfg, const hm_change_rec *pairs, int64_t n, uint8_t *bytes, int64_t cap,
                                int64_t *offsets);
/* up to n of, for the last change call on the context: [0] cells in RA, [1] cells in RB, [2] cells in both, [3] pairs
 * after the view, [4] pairs returned, [5] device microseconds of the change's own kernels (HIP events around the join,
 * the view and the ranking; the two roll-ups excluded).  All 0 before the first call. */
int hm_change_info(const hm_ctx *ctx, int64_t *v, int32_t n);

/* ---- a trailing span of live windows as one heatmap, with every cell's count per window ("the last 15 minutes") ----
 * span(end_start_us, windows, r): the `windows` consecutive tumbling windows whose starts are first = end_start_us -
 * (windows - 1) * tile_us, ..., end_start_us; 1 <= windows <= HM_SPAN_MAX_WINDOWS, end_start_us a multiple of tile_us
 * (HM_E_INVALID otherwise), 0 <= r <= h3_res.  A window of the span that is not live contributes nothing and is no error;
 * no live window: *n = 0.  The records are hm_state_recs, one per parent cell at r that any of the windows holds, in no
 * particular order: count, n_speed and the three sums added up over the windows and the children (counts and n_speed
 * exact; the sums fp64 additions in no fixed order, as hm_window_rollup's), window_start_us = first, reserved = 0.
 * series: int64[*n][windows], row i record i's, column j the cell's count in window first + j * tile_us (0 where the
 * window or the cell is absent); the row adds up to the record's count.  All selected windows' tables are aggregated
 * in one launch (csrc/k_span.h).
 * view (NULL: none) keeps a record iff hm_window_geojson_view's rule keeps its cell; k >= 0: the first min(k, n) records
 * of hm_top_records' order (k <= HM_TOP_MAX), after the view; k < 0: unranked.  The rows follow their records.
 * Outputs are library-owned, in device or pinned host memory per out_memory, valid until the next call on the context.
 * A span call counts as a roll-up for hm_window_rollup's buffers (as a change call does): its parent table is what
 * hm_span_raster looks the pixels up in.  The calls read the tile state only (hm_state_version, an export in progress
 * are unaffected); a repeated identical call allocates nothing.  Checks in hm_window_top's order: the arguments, the
 * resolution, the shard, the stage.  On a shard context the unranked records are the rank's partial (add the records
 * and rows of equal cell across ranks); ranked calls and hm_span_raster: HM_E_UNSUPPORTED -- for the raster that is
 * stricter than hm_window_raster, which allows counts on a shard and refuses only classes (HM_E_INVALID): a rank's
 * per-window grids still add up to the span's.  A parent-table overflow: HM_E_OVERFLOW. */
#define HM_SPAN_MAX_WINDOWS 16
int hm_span_rollup(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_view *view /* NULL: no filter */,
                   int64_t k /* < 0: unranked */, int32_t out_memory, const hm_state_rec **recs, const int64_t **series, int64_t *n);
/* the same records as a FeatureCollection: hm_window_geojson's feature of record i (cfg's texts: windowStart = first,
 * windowEnd = end_start_us + tile_us) with ,"windows":<windows>,"counts":[c0,...] -- row i -- after windowEnd.  Body,
 * offsets and *n as hm_window_geojson's; nothing selected: the 42-byte empty body.  A feature may be up to 1232 bytes
 * with its series; the encoder's workgroup holds features of at most 1008, so a call whose longest feature is longer
 * (counts of 13 and more digits in most of 16 windows: no real count) fails with HM_E_UNSUPPORTED, nothing returned. */
int hm_span_geojson(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_geojson_cfg *cfg,
                    const hm_view *view /* NULL: no filter */, int64_t k /* < 0: unranked */, int32_t out_memory,
                    const uint8_t **bytes, const int64_t **offsets, int64_t *n);
/* hm_window_raster of the span's summed counts: its grid, thresholds, limits, classes, outputs and buffers */
int hm_span_raster(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const double *lat, int32_t rows,
                   const double *lon, int32_t cols, const int64_t *thresholds, int32_t n_thresholds, int32_t out_memory,
                   const uint32_t **counts, const uint8_t **classes);
/* up to n of, for the last span call on the context: [0] live windows used, [1] their keys (scanned), [2] parents,
 * [3] records kept by the view, [4] records returned, [5] parent-table slots, [6] device microseconds of the span's
 * kernels (HIP events around the aggregation, the view, the ranking and the rows).  All 0 before the first call. */
int hm_span_info(const hm_ctx *ctx, int64_t *v, int32_t n);
/* Host execution (no GPU) over per-window record arrays at any resolutions >= res: recs holds window j's n_per_window[j]
 * records after those of the windows before it (window j = first_us + j * tile_us).  out: room for all of them; series:
 * int64[that many][windows]; the records come sorted by cell, the sums added in input order. */
int hm_selftest_span(const hm_state_rec *recs, const int64_t *n_per_window, int32_t windows, int64_t first_us, int64_t tile_us,
                     int32_t res, hm_state_rec *out, int64_t *series, int64_t *n_out);
/* host execution of the encoder on n records and their rows, as hm_selftest_tile_features */
int hm_selftest_span_features(const hm_geojson_cfg *cfg, const hm_state_rec *recs, const int64_t *series, int32_t windows,
                              int64_t n, uint8_t *bytes, int64_t cap, int64_t *offsets);

/* Tests: MOBHEAT_TEST_READ_GRID=<G>, read at hm_create (and by every hm_cells_in_view / hm_points_in_zones on a device),
 * runs the streaming kernels of the read side (view, roll-up, density, within, raster, GeoJSON, positions export), of the
 * state dump and of the sink on at most G workgroups, so that a few thousand items are several grid-stride iterations
 * of every workgroup; 0 or unset: every grid as without it.  *launches_lowered: the launches whose grid it lowered since
 * the context was created; *least_iterations / *most_iterations: the fewest / most iterations ceil(items / (items per
 * workgroup iteration * G)) among them (0, 0 when none).  ctx NULL: the same of the process's context-free calls. */
int hm_test_read_grid_info(const hm_ctx *ctx, int64_t *launches_lowered, int64_t *least_iterations, int64_t *most_iterations);

/* json.dumps(x) of n doubles -- CPython's float.__repr__, NaN / Infinity / -Infinity for the non-finite -- as the GeoJSON
 * encoders write them (csrc/float_repr.h), executed on the host and on GPU `device` (test entry points): value i's
 * len[i] <= 24 bytes at text[24 i]. */
int hm_selftest_float_repr_host(const double *x, int64_t n, uint8_t *text, int32_t *len);
int hm_selftest_float_repr_device(const double *x, int64_t n, uint8_t *text, int32_t *len, int32_t device);

/* Counts of the last hm_process_batch / stage batch (up to n of them): [0] keys created in the tile state, [1] partial
 * records merged (direct path: aggregated rows; table mode: ~ distinct keys; stage API: the records this rank
 * received as owner), [2] tiles emitted, [3] 1 if table mode ran, [4] table mode: aggregates evicted from k_agg's
 * LDS tables into its buckets, [5] stage API: tile records this rank sent, [6] device + pinned-host allocations and
 * [7] frees the context made since hm_create (steady-state batches make none: tests/test_gpu_parity.py), [8] 1 if the
 * direct path's rows were binned by the ingest itself (no separate partition pass), [9] stage API: of [5], the records
 * of bins this rank owns, kept in its slabs (hm_stage_sizes.n_self_records), [10] hm_process_batch: the chunks the
 * batch was pipelined in (each chunk's ingest overlapping the previous chunk's merge; 0: not pipelined), [11]
 * hm_process_batch: records of a binned batch that the ingest's producer waves stored themselves because their ring to
 * the writer waves stayed full (0 on the other paths), [12] the variant of the owner merge kernel at the batch's last
 * launch of it, a bit set: 1 resident-only (every window's region tags in LDS, no HBM-probing fallback), 2 the
 * wave-cooperative probe, 4 the bins' records read as segments, 8 at least one record of the batch probed its slot
 * through HBM (0: the batch merged nothing; a growth's rehash merge is not recorded).  Tests choose the variant with
 * MOBHEAT_TEST_MERGE_TAGS=<bytes> (at most that much LDS for resident tags; 0: none) and MOBHEAT_TEST_MERGE_COOP=0|1
 * (the probe of a resident-only merge), read at hm_create.  [13]..[18] the regimes of a table-mode batch (0 on the
 * other paths): [13] flushes of a full aggregation table before a workgroup's last one, summed over workgroups, [14]
 * rows sent as partial records of their own because the table's probe bound was reached, [15] evicted aggregates sent
 * so because their bucket was full, [16] bucket records sent so because the reducing table's probe bound was reached,
 * [17] emissions of a full reducing table before a bucket's last one, summed over buckets, [18] the bucket capacity
 * (records per sub-bucket) the batch ran with.  Tests reach them on small batches with MOBHEAT_TEST_AGG_GRID=<g> (the
 * aggregation's row spans as if the device had g compute units) and MOBHEAT_TEST_AGG_CAP=<f> (the floor of the bucket
 * capacity instead of 4096), read at hm_create.  [19] the rows the per-event pass listed as candidates of the
 * latest-position dedup (a superset of the latest rows), or -1 when the batch's dedup ran from the per-row flags
 * instead: the list held fewer rows than that (max(n / 16, 65536); tests: MOBHEAT_TEST_CAND_CAP=<rows>, read at
 * hm_create), or the fused per-vkey max gave up. */
int hm_last_counts(const hm_ctx *ctx, int64_t *c, int32_t n);
/* Version of the persistent tile state: incremented when a batch starts merging into it (hm_process_batch,
 * hm_stage_merge, growth).  A call that failed without changing it left the state as it was (-1: ctx NULL). */
int64_t hm_state_version(const hm_ctx *ctx);

/* HM_ABI_VERSION the library was built with (callers check it before hm_create). */
int32_t hm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
