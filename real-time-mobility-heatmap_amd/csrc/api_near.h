// C ABI: radius queries -- the k positions / tiles of a live window nearest a point within a radius, nearest first
// (k_near.h; the select, the compaction of the selected and their ranks are the top's, api_top.h; the roll-up is
// rollup_on_device).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

static int near_init(hm_ctx *ctx) {
    hm_ctx::Near &N = ctx->near;
    if (N.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, N.words, NW_WORDS * 8))) return rc;
    for (auto &e : N.ev) HIPCHK(ctx, hipEventCreate(&e));
    N.ready = true;
    return HM_OK;
}
static int near_bad_query(hm_ctx *ctx, const char *who, const hm_near *q) {
    return set_err(ctx, HM_E_INVALID, "%s: query (%g, %g, %g): -90 <= lat <= 90, -180 <= lon <= 180, max_distance_m >= 0 or +inf", who,
                   q->lat, q->lon, q->max_distance_m);
}

int hm_near_distances(const hm_near *q, const double *lat, const double *lon, int64_t n, int32_t memory, int32_t device,
                      double *dist_m) {
    if (!q || !near_valid(*q) || n < 0 || n > (int64_t)UINT32_MAX || (n > 0 && (!lat || !lon || !dist_m)) ||
        (memory != HM_MEM_HOST && memory != HM_MEM_DEVICE))
        return HM_E_INVALID;
    if (n == 0) return HM_OK;
    std::lock_guard<std::mutex> lock(g_udf_mu);
    UdfState *S = nullptr;
    int rc;
    if ((rc = udf_begin(device, S))) return rc;
    const double *dlat = lat, *dlon = lon;
    double *dd = dist_m;
    hipError_t e = hipSuccess;
    if (memory == HM_MEM_HOST) {
        if (udf_buf(S->in0, n * 8) || udf_buf(S->in1, n * 8) || udf_buf(S->out0, n * 8)) return HM_E_NOMEM;
        e = hipMemcpyAsync(S->in0.p, lat, n * 8, hipMemcpyHostToDevice, S->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S->in1.p, lon, n * 8, hipMemcpyHostToDevice, S->stream);
        dlat = (const double *)S->in0.p;
        dlon = (const double *)S->in1.p;
        dd = (double *)S->out0.p;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_near_distances, dim3(grid_for(n, 256, 256 * 32)), dim3(256), 0, S->stream, *q, dlat, dlon, n, dd);
        e = hipGetLastError();
    }
    if (e == hipSuccess && memory == HM_MEM_HOST) e = hipMemcpyAsync(dist_m, dd, n * 8, hipMemcpyDeviceToHost, S->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(S->stream);
    return e == hipSuccess ? HM_OK : HM_E_HIP;
}

int hm_selftest_near_distances(const hm_near *q, const double *lat, const double *lon, int64_t n, double *dist_m) {
    if (!q || !near_valid(*q) || n < 0 || (n > 0 && (!lat || !lon || !dist_m))) return HM_E_INVALID;
    const NearPoint pt = near_point(q->lat, q->lon, hm_glm_host);
    for (int64_t i = 0; i < n; i++) dist_m[i] = near_distance_m(pt, lat[i], lon[i], hm_glm_host);
    return HM_OK;
}

// The n candidates in N.cand (records of Q 16-byte quarters) with their key words in the top's kc / cell: the first
// m = min(k, n) of the order into N.out, their distances into N.dist, both in rank order.  Fills N.info[4], [5], [7].
extern "C++" {
template <int Q>
static int near_rank(hm_ctx *ctx, int64_t n, int64_t m) {
    hm_ctx::Top &T = ctx->top;
    hm_ctx::Near &N = ctx->near;
    int rc;
    if ((rc = top_select_buffers(ctx, m)) || (rc = ensure(ctx, N.out, (size_t)m * 16 * Q)) || (rc = ensure(ctx, N.dist, (size_t)m * 8))) return rc;
    const unsigned long long *k0 = (const unsigned long long *)T.kc.p, *k1 = (const unsigned long long *)T.cell.p;
    const int max_grid = T.test_grid ? T.test_grid : 8 * std::max(ctx->n_cus, 1);
    double us = 0;
    int64_t passes[3] = {0, 0, 0}, tied = 0;
    rc = top_run(
        ctx, k0, k1, n, m, us, passes, &tied,
        [&] {
            hipLaunchKernelGGL(k_near_vary, dim3(grid_for(n, 256, max_grid)), dim3(256), 0, ctx->stream, k0, k1, n,
                               (unsigned long long *)T.words.p);
        },
        [&] {
            hipLaunchKernelGGL(k_near_scatter<Q>, dim3(grid_for(Q * m, 256)), dim3(256), 0, ctx->stream, (const uint4 *)N.cand.p, n, k0,
                               (const unsigned *)T.sidx.p, (const unsigned *)T.rank.p, (int)m, (uint4 *)N.out.p,
                               (unsigned long long *)N.dist.p);
        });
    if (rc) return rc;
    N.info[4] = m;
    N.info[5] = passes[0] + passes[1] + passes[2];
    N.info[7] = (int64_t)us;
    return HM_OK;
}
}  // extern "C++"
// the scan's counters into N.info[0..3] and [6]; *n = the candidates within the radius (at most cap)
static int near_scan_done(hm_ctx *ctx, int64_t cap, int64_t *n) {
    hm_ctx::Near &N = ctx->near;
    HIPCHK(ctx, hipGetLastError());
    unsigned long long w[NW_WORDS] = {};
    HIPCHK(ctx, hipMemcpyAsync(w, N.words.p, NW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    float ms = 0;
    if (hipEventElapsedTime(&ms, N.ev[0], N.ev[1]) != hipSuccess) ms = 0;
    if ((int64_t)w[NW_OUT] > cap) return set_err(ctx, HM_E_STATE, "near kept %llu candidates of at most %lld", w[NW_OUT], (long long)cap);
    N.info[0] = (int64_t)w[NW_SCANNED];
    N.info[1] = (int64_t)w[NW_SINCE];
    N.info[2] = (int64_t)w[NW_NAN];
    N.info[3] = (int64_t)w[NW_OUT];
    N.info[6] = (int64_t)(1e3 * ms);
    *n = (int64_t)w[NW_OUT];
    return HM_OK;
}

// near(S, q, since_us, k) on the device: the ranked records in N.out, their distances in N.dist; *m_out their number.
// The arguments are checked by the caller.  Reads S only.
static int near_positions(hm_ctx *ctx, const hm_near *q, int64_t since_us, int64_t k, int64_t *m_out) {
    hm_ctx::Positions &P = ctx->pos;
    hm_ctx::Top &T = ctx->top;
    hm_ctx::Near &N = ctx->near;
    *m_out = 0;
    for (int64_t &x : N.info) x = 0;
    if (k == 0 || P.keys == 0 || !P.tab) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t cap = (int64_t)P.cap, keys = P.keys;
    int rc;
    if ((rc = near_init(ctx)) || (rc = top_init(ctx)) || (rc = ensure(ctx, N.cand, (size_t)keys * sizeof(hm_position_rec))) ||
        (rc = ensure(ctx, T.kc, (size_t)keys * 8)) || (rc = ensure(ctx, T.cell, (size_t)keys * 8)))
        return rc;
    const int max_grid = T.test_grid ? T.test_grid : 256 * 16;
    HIPCHK(ctx, hipMemsetAsync(N.words.p, 0, NW_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipEventRecord(N.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_pos_emit_near, dim3(grid_for(cap, 256 * DUMP_PER, max_grid)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab, cap,
                       *q, (long long)since_us, (hm_position_rec *)N.cand.p, (unsigned long long *)T.kc.p, (unsigned long long *)T.cell.p,
                       keys, (unsigned long long *)N.words.p);
    HIPCHK(ctx, hipEventRecord(N.ev[1], ctx->stream));
    int64_t n = 0;
    if ((rc = near_scan_done(ctx, keys, &n))) return rc;
    const int64_t m = std::min(k, n);
    if (m == 0) return HM_OK;
    if ((rc = near_rank<2>(ctx, n, m))) return rc;
    *m_out = m;
    return HM_OK;
}

// near(hm_window_rollup(window_start_us, res), q, k) on the device, as near_positions; hm_window_top's state rules
static int near_window(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_near *q, int64_t k, const char *who, int64_t *m_out) {
    hm_ctx::Top &T = ctx->top;
    hm_ctx::Near &N = ctx->near;
    *m_out = 0;
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a parent split over ranks has no rank-local centroid", who,
                       ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    for (int64_t &x : N.info) x = 0;
    if (k == 0) return HM_OK;
    int64_t g = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, who, &g))) return rc;
    if (g == 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = near_init(ctx)) || (rc = top_init(ctx)) || (rc = ensure(ctx, N.cand, (size_t)g * sizeof(GrowRec))) ||
        (rc = ensure(ctx, T.kc, (size_t)g * 8)) || (rc = ensure(ctx, T.cell, (size_t)g * 8)))
        return rc;
    const int max_grid = T.test_grid ? T.test_grid : 256 * 16;
    HIPCHK(ctx, hipMemsetAsync(N.words.p, 0, NW_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipEventRecord(N.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_near_tiles, dim3(grid_for(g, 256 * DUMP_PER, max_grid)), dim3(256), 0, ctx->stream, (const GrowRec *)ctx->ru_out.p, g,
                       *q, (GrowRec *)N.cand.p, (unsigned long long *)T.kc.p, (unsigned long long *)T.cell.p, (unsigned long long *)N.words.p);
    HIPCHK(ctx, hipEventRecord(N.ev[1], ctx->stream));
    int64_t n = 0;
    if ((rc = near_scan_done(ctx, g, &n))) return rc;
    const int64_t m = std::min(k, n);
    if (m == 0) return HM_OK;
    if ((rc = near_rank<4>(ctx, n, m))) return rc;
    *m_out = m;
    return HM_OK;
}

// the ranked records and distances handed out where they are, or copied to the near's pinned buffers
static int near_out(hm_ctx *ctx, int64_t m, size_t rec_bytes, int32_t out_memory, const void **recs, const double **dist_m) {
    hm_ctx::Near &N = ctx->near;
    *recs = nullptr;
    *dist_m = nullptr;
    if (m == 0) return HM_OK;
    *recs = N.out.p;
    *dist_m = (const double *)N.dist.p;
    if (out_memory == HM_MEM_DEVICE) return HM_OK;
    int rc;
    if ((rc = host_pinned(ctx, &N.h_out, N.h_out_cap, (size_t)m * rec_bytes)) || (rc = host_pinned(ctx, &N.h_dist, N.h_dist_cap, (size_t)m * 8)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(N.h_out, N.out.p, (size_t)m * rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(N.h_dist, N.dist.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    *recs = N.h_out;
    *dist_m = (const double *)N.h_dist;
    return HM_OK;
}

int hm_positions_near(hm_ctx *ctx, const hm_near *q, int64_t since_us, int64_t k, int32_t out_memory, const hm_position_rec **recs,
                      const double **dist_m, int64_t *n) {
    if (!ctx || !q || !recs || !dist_m || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_positions_near", k);
    if (!near_valid(*q)) return near_bad_query(ctx, "hm_positions_near", q);
    int rc;
    if ((rc = density_state_ok(ctx, "hm_positions_near"))) return rc;
    *recs = nullptr;
    *dist_m = nullptr;
    *n = 0;
    int64_t m = 0;
    if ((rc = near_positions(ctx, q, since_us, k, &m)) ||
        (rc = near_out(ctx, m, sizeof(hm_position_rec), out_memory, (const void **)recs, dist_m)))
        return rc;
    *n = m;
    return HM_OK;
}

int hm_window_near(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_near *q, int64_t k, int32_t out_memory,
                   const hm_state_rec **recs, const double **dist_m, int64_t *n) {
    if (!ctx || !q || !recs || !dist_m || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_window_near", k);
    if (!near_valid(*q)) return near_bad_query(ctx, "hm_window_near", q);
    int64_t m = 0;
    int rc;
    if ((rc = near_window(ctx, window_start_us, res, q, k, "hm_window_near", &m))) return rc;
    *recs = nullptr;
    *dist_m = nullptr;
    *n = 0;
    if ((rc = near_out(ctx, m, sizeof(GrowRec), out_memory, (const void **)recs, dist_m))) return rc;
    *n = m;
    return HM_OK;
}

int hm_positions_geojson_near(hm_ctx *ctx, const hm_position_doc_cfg *buckets, const hm_near *q, int64_t since_us, int64_t k,
                              int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n,
                              const hm_position_rec **recs, const double **dist_m) {
    if (!ctx || !buckets || !q || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_positions_geojson_near", k);
    if (!near_valid(*q)) return near_bad_query(ctx, "hm_positions_geojson_near", q);
    int rc;
    if ((rc = density_state_ok(ctx, "hm_positions_geojson_near")) || (rc = gj_buckets_ok(ctx, buckets))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    if (dist_m) *dist_m = nullptr;
    int64_t m = 0;
    if ((rc = near_positions(ctx, q, since_us, k, &m))) return rc;
    if (recs || dist_m) {   // the records in feature order = rank order, and their distances (the near's pinned copies)
        const void *r = nullptr;
        const double *d = nullptr;
        if ((rc = near_out(ctx, m, sizeof(hm_position_rec), HM_MEM_HOST, &r, &d))) return rc;
        if (recs) *recs = (const hm_position_rec *)r;
        if (dist_m) *dist_m = d;
    }
    const GjGiven given = {(const hm_position_rec *)ctx->near.out.p, (const double *)ctx->near.dist.p, m};
    int64_t got = 0;
    if ((rc = gj_positions(ctx, buckets, out_memory, bytes, offsets, &got, nullptr, nullptr, "hm_positions_geojson_near", &given))) return rc;
    *n = m;
    return HM_OK;
}

int hm_window_geojson_near(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, const hm_near *q, int64_t k,
                           int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n,
                           const hm_state_rec **recs, const double **dist_m) {
    if (!ctx || !cfg || !q || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_window_geojson_near", k);
    if (!near_valid(*q)) return near_bad_query(ctx, "hm_window_geojson_near", q);
    GjTexts X;
    if (gj_texts(cfg, X)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    int64_t m = 0;
    int rc;
    if ((rc = near_window(ctx, window_start_us, res, q, k, "hm_window_geojson_near", &m))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    if (dist_m) *dist_m = nullptr;
    if (recs || dist_m) {
        const void *r = nullptr;
        const double *d = nullptr;
        if ((rc = near_out(ctx, m, sizeof(GrowRec), HM_MEM_HOST, &r, &d))) return rc;
        if (recs) *recs = (const hm_state_rec *)r;
        if (dist_m) *dist_m = d;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = gj_tiles(ctx, X, (const GrowRec *)ctx->near.out.p, m, out_memory, bytes, offsets, m ? (const double *)ctx->near.dist.p : nullptr)))
        return rc;
    *n = m;
    return HM_OK;
}

// Host execution with the kernels' HM_HD code: the distances, the filter, the key words, then the top's host select
extern "C++" {
template <class Rec, class Point, class Word1>
static int near_selftest(const hm_near *q, const Rec *recs, int64_t n, int64_t k, Rec *out, double *dist_m, int64_t *n_out, Point point,
                         Word1 word1) {
    if (!q || !near_valid(*q) || n < 0 || n > (int64_t(1) << 31) || (n > 0 && !recs) || !top_k_ok(k) || !n_out) return HM_E_INVALID;
    *n_out = 0;
    if (k == 0) return HM_OK;
    const NearPoint pt = near_point(q->lat, q->lon, hm_glm_host);
    std::vector<unsigned long long> k0, k1;
    std::vector<int64_t> src;
    for (int64_t i = 0; i < n; i++) {
        double lat, lon;
        if (!point(recs[i], lat, lon)) continue;
        const double d = near_distance_m(pt, lat, lon, hm_glm_host);
        if (!(d == d && d <= q->max_distance_m)) continue;
        k0.push_back(near_bits(d));
        k1.push_back(word1(recs[i]));
        src.push_back(i);
    }
    const int64_t c = (int64_t)src.size(), m = std::min(k, c);
    if (m == 0) return HM_OK;
    if (!out || !dist_m) return HM_E_INVALID;
    std::vector<unsigned> sel;
    if (int rc = top_select_host(k0.data(), k1.data(), c, m, sel)) return rc;
    for (int64_t j = 0; j < m; j++) {
        out[j] = recs[src[sel[j]]];
        memcpy(&dist_m[j], &k0[sel[j]], 8);
    }
    *n_out = m;
    return HM_OK;
}
}  // extern "C++"

int hm_selftest_positions_near(const hm_near *q, int64_t since_us, const hm_position_rec *recs, int64_t n, int64_t k,
                               hm_position_rec *out, double *dist_m, int64_t *n_out) {
    return near_selftest(
        q, recs, n, k, out, dist_m, n_out,
        [=](const hm_position_rec &r, double &lat, double &lon) {
            lat = r.lat;
            lon = r.lon;
            return r.ts_us >= since_us;
        },
        [](const hm_position_rec &r) { return ((unsigned long long)r.provider << 32) | r.vehicle; });
}

int hm_selftest_tiles_near(const hm_near *q, const hm_state_rec *recs, int64_t n, int64_t k, hm_state_rec *out, double *dist_m,
                           int64_t *n_out) {
    return near_selftest(
        q, recs, n, k, out, dist_m, n_out,
        [](const hm_state_rec &r, double &lat, double &lon) {
            lat = near_centroid(r.sum_lat, (unsigned long long)r.count);
            lon = near_centroid(r.sum_lon, (unsigned long long)r.count);
            return true;
        },
        [](const hm_state_rec &r) { return (unsigned long long)r.cell; });
}

int hm_near_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 8; i++) v[i] = ctx->near.info[i];
    return HM_OK;
}
