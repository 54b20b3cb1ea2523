// C ABI: polygon geofences -- the vehicles of the positions state / the tiles of a live window by centroid inside the
// zones of a zone set, with their labels and per-zone totals, as records and as GeoJSON bodies (k_within.h; the roll-up
// is rollup_on_device, the bodies are gj_positions / gj_tiles on what the scan kept).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// ---- validation and packing (host) ----
// *n_edges = the set's vertices = its edges.  Anything invalid: HM_E_INVALID with the reason in err.
static int zones_check(const hm_zones *z, int *n_edges, std::string &err) {
    char buf[256];
    const auto bad = [&](const char *fmt, long long a, long long b, long long c) {
        snprintf(buf, sizeof buf, fmt, a, b, c);
        err = buf;
        return HM_E_INVALID;
    };
    *n_edges = 0;
    if (!z) return bad("zones: NULL", 0, 0, 0);
    if (z->n_zones < 0 || z->n_zones > HM_ZONES_MAX) return bad("zones: %lld zones, at most HM_ZONES_MAX = %lld", z->n_zones, HM_ZONES_MAX, 0);
    if (z->n_zones == 0) return HM_OK;
    if (!z->zone_rings || !z->ring_verts || !z->lat || !z->lon) return bad("zones: a NULL array", 0, 0, 0);
    if (z->zone_rings[0] != 0) return bad("zones: zone_rings[0] = %lld, 0 expected", z->zone_rings[0], 0, 0);
    for (int k = 0; k < z->n_zones; k++) {
        if (z->zone_rings[k + 1] <= z->zone_rings[k]) return bad("zones: zone %lld has no ring (zone_rings must ascend)", k, 0, 0);
        if (z->zone_rings[k + 1] > HM_ZONE_VERTS_MAX / 3)
            return bad("zones: more than %lld rings cannot stay within HM_ZONE_VERTS_MAX = %lld vertices", HM_ZONE_VERTS_MAX / 3, HM_ZONE_VERTS_MAX, 0);
    }
    const int n_rings = z->zone_rings[z->n_zones];
    if (z->ring_verts[0] != 0) return bad("zones: ring_verts[0] = %lld, 0 expected", z->ring_verts[0], 0, 0);
    for (int r = 0; r < n_rings; r++) {
        const long long nv = (long long)z->ring_verts[r + 1] - z->ring_verts[r];
        if (nv < 3) return bad("zones: ring %lld has %lld vertices, at least 3 expected (without the closing one)", r, nv, 0);
        if (z->ring_verts[r + 1] > HM_ZONE_VERTS_MAX)
            return bad("zones: more than HM_ZONE_VERTS_MAX = %lld vertices in total", HM_ZONE_VERTS_MAX, 0, 0);
    }
    const int nv = z->ring_verts[n_rings];
    for (int v = 0; v < nv; v++)
        if (!(z->lat[v] >= -90.0 && z->lat[v] <= 90.0 && z->lon[v] >= -180.0 && z->lon[v] <= 180.0))
            return bad("zones: vertex %lld: finite, -90 <= lat <= 90, -180 <= lon <= 180 expected", v, 0, 0);
    *n_edges = nv;
    return HM_OK;
}
static size_t zones_blob_bytes(int n_zones, int n_edges) { return ((size_t)5 * n_edges + (size_t)3 * n_zones) * 8 + ((size_t)n_zones + 1) * 4; }
// the packed set's arrays inside a blob at `base` (host or device memory)
static ZoneSet zones_view(const void *base, int n_zones, int n_edges) {
    ZoneSet s;
    const double *d = (const double *)base;
    s.n_zones = n_zones;
    s.n_edges = n_edges;
    s.alat = d;
    s.blat = d + n_edges;
    s.alon = d + 2 * (size_t)n_edges;
    s.w = d + 3 * (size_t)n_edges;
    s.h = d + 4 * (size_t)n_edges;
    s.zmin = d + 5 * (size_t)n_edges;
    s.zmax = s.zmin + n_zones;
    s.zlon = s.zmax + n_zones;
    s.eoff = (const int *)(s.zlon + n_zones);
    return s;
}
// a checked set into a blob of zones_blob_bytes: every edge in its canonical direction with w and h, every zone's box
// (min / max of its vertices: exact)
static void zones_pack(const hm_zones *z, int n_edges, void *blob) {
    const ZoneSet s = zones_view(blob, z->n_zones, n_edges);
    double *alat = (double *)s.alat, *blat = (double *)s.blat, *alon = (double *)s.alon, *w = (double *)s.w, *h = (double *)s.h;
    double *zmin = (double *)s.zmin, *zmax = (double *)s.zmax, *zlon = (double *)s.zlon;
    int *eoff = (int *)s.eoff;
    eoff[0] = 0;
    for (int k = 0; k < z->n_zones; k++) {
        const int v0 = z->ring_verts[z->zone_rings[k]], v1 = z->ring_verts[z->zone_rings[k + 1]];
        double lo = z->lat[v0], hi = z->lat[v0], east = z->lon[v0];
        for (int v = v0; v < v1; v++) {
            lo = z->lat[v] < lo ? z->lat[v] : lo;
            hi = z->lat[v] > hi ? z->lat[v] : hi;
            east = z->lon[v] > east ? z->lon[v] : east;
        }
        zmin[k] = lo;
        zmax[k] = hi;
        zlon[k] = east;
        eoff[k + 1] = v1;
        for (int r = z->zone_rings[k]; r < z->zone_rings[k + 1]; r++) {
            const int r0 = z->ring_verts[r], nv = z->ring_verts[r + 1] - r0;
            for (int j = 0; j < nv; j++) {
                int a = r0 + j, b = r0 + (j + 1) % nv;
                if (z->lat[a] > z->lat[b]) std::swap(a, b);
                const int e = r0 + j;
                alat[e] = z->lat[a];
                blat[e] = z->lat[b];
                alon[e] = z->lon[a];
                w[e] = z->lon[b] - z->lon[a];
                h[e] = z->lat[b] - z->lat[a];
            }
        }
    }
}
// device totals -> hm_zone_rec: the newest ts_us decoded (positions; INT64_MIN when the zone is empty) or 0 (tiles)
static void zones_totals_out(const unsigned long long *t, int n_zones, bool positions, hm_zone_rec *out) {
    for (int z = 0; z < n_zones; z++, t += WT_WORDS) {
        hm_zone_rec &r = out[z];
        r.n = (int64_t)t[WT_N];
        r.count = positions ? r.n : (int64_t)t[WT_COUNT];
        r.n_speed = (int64_t)t[WT_NSPEED];
        memcpy(&r.sum_speed, &t[WT_SSPEED], 8);
        r.newest_us = positions ? wdec(t[WT_NEWEST]) : 0;
        r.reserved = 0;
    }
}

int hm_points_in_zones(const hm_zones *zones, const double *lat, const double *lon, int64_t n, int32_t memory, int32_t device,
                       int32_t *first_zone_i32, uint32_t *hits_u32) {
    int ne = 0;
    std::string err;
    if (zones_check(zones, &ne, err) || n < 0 || n > (int64_t)UINT32_MAX || (n > 0 && (!lat || !lon || !first_zone_i32 || !hits_u32)) ||
        (memory != HM_MEM_HOST && memory != HM_MEM_DEVICE))
        return HM_E_INVALID;
    if (n == 0) return HM_OK;
    std::vector<char> blob(zones_blob_bytes(zones->n_zones, ne));
    if (zones->n_zones) zones_pack(zones, ne, blob.data());
    std::lock_guard<std::mutex> lock(g_udf_mu);
    UdfState *S = nullptr;
    int rc;
    if ((rc = udf_begin(device, S))) return rc;
    if (udf_buf(S->zones, blob.size())) return HM_E_NOMEM;
    const double *dlat = lat, *dlon = lon;
    int *dfirst = first_zone_i32;
    unsigned *dhits = hits_u32;
    hipError_t e = hipMemcpyAsync(S->zones.p, blob.data(), blob.size(), hipMemcpyHostToDevice, S->stream);
    if (memory == HM_MEM_HOST) {
        if (udf_buf(S->in0, n * 8) || udf_buf(S->in1, n * 8) || udf_buf(S->out0, n * 4) || udf_buf(S->out1, n * 4)) return HM_E_NOMEM;
        if (e == hipSuccess) e = hipMemcpyAsync(S->in0.p, lat, n * 8, hipMemcpyHostToDevice, S->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S->in1.p, lon, n * 8, hipMemcpyHostToDevice, S->stream);
        dlat = (const double *)S->in0.p;
        dlon = (const double *)S->in1.p;
        dfirst = (int *)S->out0.p;
        dhits = (unsigned *)S->out1.p;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_points_in_zones, dim3(read_grid(udf_read_grid(), n, 256 * DUMP_PER)), dim3(256), 0, S->stream,
                           zones_view(S->zones.p, zones->n_zones, ne), dlat, dlon, n, dfirst, dhits);
        e = hipGetLastError();
    }
    if (e == hipSuccess && memory == HM_MEM_HOST) {
        e = hipMemcpyAsync(first_zone_i32, dfirst, n * 4, hipMemcpyDeviceToHost, S->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hits_u32, dhits, n * 4, hipMemcpyDeviceToHost, S->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(S->stream);   // (always: the blob is this call's own)
    return e == hipSuccess && e2 == hipSuccess ? HM_OK : HM_E_HIP;
}

int hm_selftest_points_in_zones(const hm_zones *zones, const double *lat, const double *lon, int64_t n, int32_t *first_zone_i32,
                                uint32_t *hits_u32) {
    int ne = 0;
    std::string err;
    if (zones_check(zones, &ne, err) || n < 0 || (n > 0 && (!lat || !lon || !first_zone_i32 || !hits_u32))) return HM_E_INVALID;
    std::vector<char> blob(zones_blob_bytes(zones->n_zones, ne));
    if (zones->n_zones) zones_pack(zones, ne, blob.data());
    const ZoneSet s = zones_view(blob.data(), zones->n_zones, ne);
    for (int64_t i = 0; i < n; i++) {
        int first;
        unsigned hits;
        zones_of_point_host(s, lat[i], lon[i], first, hits);
        first_zone_i32[i] = first;
        hits_u32[i] = hits;
    }
    return HM_OK;
}

// ---- the two scans on a context ----
static int within_init(hm_ctx *ctx) {
    hm_ctx::Within &W = ctx->within;
    if (W.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, W.words, WW_WORDS * 8))) return rc;
    for (auto &e : W.ev) HIPCHK(ctx, hipEventCreate(&e));
    W.ready = true;
    return HM_OK;
}
// the checks every within entry point shares after its own argument checks: the zone set, then the state
static int within_args_ok(hm_ctx *ctx, const hm_zones *zones, const char *who, bool window, int *n_edges) {
    std::string err;
    if (zones_check(zones, n_edges, err)) return set_err(ctx, HM_E_INVALID, "%s: %s", who, err.c_str());
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, window ? "%s on shard %d of %d: a parent split over ranks has no rank-local centroid"
                                                     : "%s on shard %d of %d: a rank holds only the latest rows it received",
                       who, ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    return HM_OK;
}
// the packed set on the device (W.zones) and the zeroed totals and control words, all on the context's stream
static int within_begin(hm_ctx *ctx, const hm_zones *zones, int n_edges, ZoneSet &zs) {
    hm_ctx::Within &W = ctx->within;
    const size_t bytes = zones_blob_bytes(zones->n_zones, n_edges);
    int rc;
    if ((rc = within_init(ctx)) || (rc = ensure(ctx, W.zones, bytes)) || (rc = ensure(ctx, W.tot, (size_t)zones->n_zones * WT_WORDS * 8)) ||
        (rc = host_pinned(ctx, &W.h_zones, W.h_zones_cap, bytes)) ||
        (rc = host_pinned(ctx, &W.h_tot, W.h_tot_cap, (size_t)zones->n_zones * WT_WORDS * 8)))
        return rc;
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));   // (an earlier call's copy out of the pinned blob has landed)
    zones_pack(zones, n_edges, W.h_zones);
    HIPCHK(ctx, hipMemcpyAsync(W.zones.p, W.h_zones, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(W.tot.p, 0, (size_t)zones->n_zones * WT_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(W.words.p, 0, WW_WORDS * 8, ctx->stream));
    zs = zones_view(W.zones.p, zones->n_zones, n_edges);
    return HM_OK;
}
// after the scan's launch: the counters into W.info, the totals into W.h_tot; *n = the records in at least one zone
static int within_scan_done(hm_ctx *ctx, const ZoneSet &zs, int64_t cap, bool emitted, int64_t *n) {
    hm_ctx::Within &W = ctx->within;
    HIPCHK(ctx, hipGetLastError());
    unsigned long long w[WW_WORDS] = {};
    HIPCHK(ctx, hipMemcpyAsync(w, W.words.p, WW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W.h_tot, W.tot.p, (size_t)zs.n_zones * WT_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    float ms = 0;
    if (hipEventElapsedTime(&ms, W.ev[0], W.ev[1]) != hipSuccess) ms = 0;
    if ((int64_t)w[WW_IN] > cap || (emitted && w[WW_OUT] != w[WW_IN]))
        return set_err(ctx, HM_E_STATE, "within kept %llu records (%llu emitted) of at most %lld", w[WW_IN], w[WW_OUT], (long long)cap);
    W.info[0] = (int64_t)w[WW_SCANNED];
    W.info[1] = (int64_t)w[WW_SINCE];
    W.info[2] = (int64_t)w[WW_IN];
    W.info[5] = (int64_t)(1e3 * ms);
    *n = (int64_t)w[WW_IN];
    return HM_OK;
}
static void within_info_reset(hm_ctx *ctx, const hm_zones *zones, int n_edges) {
    hm_ctx::Within &W = ctx->within;
    for (int64_t &x : W.info) x = 0;
    W.info[3] = zones->n_zones;
    W.info[4] = n_edges;
    W.tot_zones = 0;
}

// within(S, zones, since_us) on the device: with emit the kept records in W.out and their labels in W.zone; the totals
// in W.h_tot (W.tot_zones of them); *n = the records in at least one zone.  The arguments are checked by the caller.
static int within_positions(hm_ctx *ctx, const hm_zones *zones, int n_edges, int64_t since_us, bool emit, int64_t *n) {
    hm_ctx::Positions &P = ctx->pos;
    hm_ctx::Within &W = ctx->within;
    *n = 0;
    within_info_reset(ctx, zones, n_edges);
    if (zones->n_zones == 0 || P.keys == 0 || !P.tab) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t cap = (int64_t)P.cap, keys = P.keys;
    ZoneSet zs;
    int rc;
    if ((emit && ((rc = ensure(ctx, W.out, (size_t)keys * sizeof(hm_position_rec))) || (rc = ensure(ctx, W.zone, (size_t)keys * 4)))) ||
        (rc = within_begin(ctx, zones, n_edges, zs)))
        return rc;
    HIPCHK(ctx, hipEventRecord(W.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_pos_within, dim3(read_grid(ctx->read_grid, cap, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab, cap, zs,
                       (long long)since_us, emit ? (hm_position_rec *)W.out.p : nullptr, (int *)W.zone.p, keys,
                       (unsigned long long *)W.tot.p, (unsigned long long *)W.words.p);
    HIPCHK(ctx, hipEventRecord(W.ev[1], ctx->stream));
    if ((rc = within_scan_done(ctx, zs, keys, emit, n))) return rc;
    W.tot_zones = zones->n_zones;
    return HM_OK;
}
// within(hm_window_rollup(window_start_us, res), zones) on the device, as within_positions; hm_window_near's state rules
static int within_window(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_zones *zones, int n_edges, bool emit, const char *who,
                         int64_t *n) {
    hm_ctx::Within &W = ctx->within;
    *n = 0;
    within_info_reset(ctx, zones, n_edges);
    int64_t g = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, who, &g))) return rc;
    if (zones->n_zones == 0 || g == 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ZoneSet zs;
    if ((emit && ((rc = ensure(ctx, W.out, (size_t)g * sizeof(GrowRec))) || (rc = ensure(ctx, W.zone, (size_t)g * 4)))) ||
        (rc = within_begin(ctx, zones, n_edges, zs)))
        return rc;
    HIPCHK(ctx, hipEventRecord(W.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_within_tiles, dim3(read_grid(ctx->read_grid, g, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const GrowRec *)ctx->ru_out.p, g, zs,
                       emit ? (GrowRec *)W.out.p : nullptr, (int *)W.zone.p, (unsigned long long *)W.tot.p, (unsigned long long *)W.words.p);
    HIPCHK(ctx, hipEventRecord(W.ev[1], ctx->stream));
    if ((rc = within_scan_done(ctx, zs, g, emit, n))) return rc;
    W.tot_zones = zones->n_zones;
    return HM_OK;
}
// the caller's totals from W.h_tot (zeros for what the scan did not reach: an empty state, a window that is not live)
static void within_totals(hm_ctx *ctx, const hm_zones *zones, bool positions, hm_zone_rec *totals) {
    hm_ctx::Within &W = ctx->within;
    if (!totals) return;
    if (W.tot_zones == zones->n_zones && W.tot_zones > 0) {
        zones_totals_out((const unsigned long long *)W.h_tot, zones->n_zones, positions, totals);
        return;
    }
    for (int z = 0; z < zones->n_zones; z++) {
        memset(&totals[z], 0, sizeof(hm_zone_rec));
        if (positions) totals[z].newest_us = INT64_MIN;
    }
}
// the kept records and labels handed out where they are, or copied to the within's pinned buffers
static int within_out(hm_ctx *ctx, int64_t m, size_t rec_bytes, int32_t out_memory, const void **recs, const int32_t **zone) {
    hm_ctx::Within &W = ctx->within;
    *recs = nullptr;
    if (zone) *zone = nullptr;
    if (m == 0) return HM_OK;
    *recs = W.out.p;
    if (zone) *zone = (const int32_t *)W.zone.p;
    if (out_memory == HM_MEM_DEVICE) return HM_OK;
    int rc;
    if ((rc = host_pinned(ctx, &W.h_out, W.h_out_cap, (size_t)m * rec_bytes)) || (rc = host_pinned(ctx, &W.h_zone, W.h_zone_cap, (size_t)m * 4)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(W.h_out, W.out.p, (size_t)m * rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W.h_zone, W.zone.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    *recs = W.h_out;
    if (zone) *zone = (const int32_t *)W.h_zone;
    return HM_OK;
}

int hm_positions_within(hm_ctx *ctx, const hm_zones *zones, int64_t since_us, int32_t out_memory, hm_zone_rec *totals,
                        const hm_position_rec **recs, const int32_t **zone, int64_t *n) {
    if (!ctx || !n || (recs && !zone) || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    int ne = 0, rc;
    if ((rc = within_args_ok(ctx, zones, "hm_positions_within", false, &ne))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    if (zone) *zone = nullptr;
    int64_t m = 0;
    if ((rc = within_positions(ctx, zones, ne, since_us, recs != nullptr, &m))) return rc;
    within_totals(ctx, zones, true, totals);
    if (recs && (rc = within_out(ctx, m, sizeof(hm_position_rec), out_memory, (const void **)recs, zone))) return rc;
    *n = m;
    return HM_OK;
}

int hm_window_within(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_zones *zones, int32_t out_memory, hm_zone_rec *totals,
                     const hm_state_rec **recs, const int32_t **zone, int64_t *n) {
    if (!ctx || !n || (recs && !zone) || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (res < 0 || res > ctx->cfg.h3_res) return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    int ne = 0, rc;
    if ((rc = within_args_ok(ctx, zones, "hm_window_within", true, &ne))) return rc;
    int64_t m = 0;
    if ((rc = within_window(ctx, window_start_us, res, zones, ne, recs != nullptr, "hm_window_within", &m))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    if (zone) *zone = nullptr;
    within_totals(ctx, zones, false, totals);
    if (recs && (rc = within_out(ctx, m, sizeof(GrowRec), out_memory, (const void **)recs, zone))) return rc;
    *n = m;
    return HM_OK;
}

int hm_positions_geojson_within(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                                const int64_t **offsets, int64_t *n, const hm_position_rec **recs, const hm_zones *zones) {
    if (!ctx || !buckets || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    int ne = 0, rc;
    if ((rc = within_args_ok(ctx, zones, "hm_positions_geojson_within", false, &ne)) || (rc = gj_buckets_ok(ctx, buckets))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    int64_t m = 0;
    if ((rc = within_positions(ctx, zones, ne, INT64_MIN, true, &m))) return rc;
    const GjGiven given = {(const hm_position_rec *)ctx->within.out.p, nullptr, m};
    return gj_positions(ctx, buckets, out_memory, bytes, offsets, n, recs, nullptr, "hm_positions_geojson_within", &given);
}

int hm_window_geojson_within(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                             const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs,
                             const hm_zones *zones) {
    if (!ctx || !cfg || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (res < 0 || res > ctx->cfg.h3_res) return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    int ne = 0, rc;
    if ((rc = within_args_ok(ctx, zones, "hm_window_geojson_within", true, &ne))) return rc;
    GjTexts X;
    if (gj_texts(cfg, X)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    int64_t m = 0;
    if ((rc = within_window(ctx, window_start_us, res, zones, ne, true, "hm_window_geojson_within", &m))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (recs && m > 0) {   // the kept records in feature order (the within's pinned copy)
        const void *r = nullptr;
        if ((rc = within_out(ctx, m, sizeof(GrowRec), HM_MEM_HOST, &r, nullptr))) return rc;
        *recs = (const hm_state_rec *)r;
    }
    if ((rc = gj_tiles(ctx, X, (const GrowRec *)ctx->within.out.p, m, out_memory, bytes, offsets))) return rc;
    *n = m;
    return HM_OK;
}

// Host execution with the kernels' HM_HD code on caller records: the kept records in input order, labels, totals
extern "C++" {
template <class Rec, class Point, class Add>
static int within_selftest(const hm_zones *zones, const Rec *recs, int64_t n, hm_zone_rec *totals, Rec *out, int32_t *zone, int64_t *n_out,
                           bool positions, Point point, Add add) {
    int ne = 0;
    std::string err;
    if (zones_check(zones, &ne, err) || n < 0 || n > (int64_t(1) << 31) || (n > 0 && !recs) || !n_out || (out && !zone)) return HM_E_INVALID;
    std::vector<char> blob(zones_blob_bytes(zones->n_zones, ne));
    if (zones->n_zones) zones_pack(zones, ne, blob.data());
    const ZoneSet s = zones_view(blob.data(), zones->n_zones, ne);
    std::vector<hm_zone_rec> tot((size_t)zones->n_zones);
    for (auto &t : tot) {
        memset(&t, 0, sizeof t);
        if (positions) t.newest_us = INT64_MIN;
    }
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++) {
        double lat, lon;
        if (!point(recs[i], lat, lon)) continue;
        int first = -1;
        for (int z = 0; z < s.n_zones; z++) {
            unsigned par = 0;
            for (int e = s.eoff[z]; e < s.eoff[z + 1]; e++) par ^= edge_crossed(s.alat[e], s.blat[e], s.alon[e], s.w[e], s.h[e], lat, lon) ? 1u : 0u;
            if (!par) continue;
            if (first < 0) first = z;
            add(tot[z], recs[i]);
        }
        if (first < 0) continue;
        if (out) {
            out[m] = recs[i];
            zone[m] = first;
        }
        m++;
    }
    if (totals)
        for (int z = 0; z < zones->n_zones; z++) totals[z] = tot[z];
    *n_out = m;
    return HM_OK;
}
}  // extern "C++"

int hm_selftest_positions_within(const hm_zones *zones, int64_t since_us, const hm_position_rec *recs, int64_t n, hm_zone_rec *totals,
                                 hm_position_rec *out, int32_t *zone, int64_t *n_out) {
    return within_selftest(
        zones, recs, n, totals, out, zone, n_out, true,
        [=](const hm_position_rec &r, double &lat, double &lon) {
            lat = r.lat;
            lon = r.lon;
            return r.ts_us >= since_us;
        },
        [](hm_zone_rec &t, const hm_position_rec &r) {
            t.n++;
            t.count++;
            if (r.ts_us > t.newest_us) t.newest_us = r.ts_us;
        });
}

int hm_selftest_tiles_within(const hm_zones *zones, const hm_state_rec *recs, int64_t n, hm_zone_rec *totals, hm_state_rec *out,
                             int32_t *zone, int64_t *n_out) {
    return within_selftest(
        zones, recs, n, totals, out, zone, n_out, false,
        [](const hm_state_rec &r, double &lat, double &lon) {
            lat = near_centroid(r.sum_lat, (unsigned long long)r.count);
            lon = near_centroid(r.sum_lon, (unsigned long long)r.count);
            return true;
        },
        [](hm_zone_rec &t, const hm_state_rec &r) {
            t.n++;
            t.count += r.count;
            if (r.n_speed) {
                t.n_speed += r.n_speed;
                t.sum_speed += r.sum_speed;
            }
        });
}

int hm_within_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 6; i++) v[i] = ctx->within.info[i];
    return HM_OK;
}
