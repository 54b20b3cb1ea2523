// C ABI: a trailing span of live windows as one heatmap with every parent's count per window -- as records and their
// series rows, as the GeoJSON body, as a raster (k_span.h; the view is k_view_tiles, the ranking top_on_device, the
// encoder gj_tiles, the pixel lookup raster_from_table).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

enum { SW_VIEW = 0, SW_MISSING, SW_WORDS };   // the span's device words: the records in view, rows k_span_rows did not find

static int span_init(hm_ctx *ctx) {
    hm_ctx::Span &S = ctx->span;
    if (S.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, S.words, SW_WORDS * 8))) return rc;
    for (auto &e : S.ev) HIPCHK(ctx, hipEventCreate(&e));
    S.ready = true;
    return HM_OK;
}

// span(end, windows, res) [cut to view] [the first k] on the device: *out = the records, *rows_out their series rows
// (int64[n][windows]), *n_out their number; *m_out / *nslots_out (optional): the parents before the view and the slots
// of the parent table in ctx->ru_tab (what raster_from_table takes).  The arguments and the stage are checked by the
// caller.  Fills S.info.  The parent table and the emitted records are ctx->ru_tab / ctx->ru_out, as any roll-up's.
static int span_on_device(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_view *view, int64_t k,
                          const GrowRec **out, const int64_t **rows_out, int64_t *n_out, int64_t *m_out = nullptr,
                          int64_t *nslots_out = nullptr) {
    hm_ctx::Span &S = ctx->span;
    *out = nullptr;
    *rows_out = nullptr;
    *n_out = 0;
    if (m_out) *m_out = 0;
    if (nslots_out) *nslots_out = 0;
    for (int64_t &x : S.info) x = 0;
    const int64_t first = end_start_us - (int64_t)(windows - 1) * ctx->cfg.tile_us;
    const int64_t tile = (int64_t)RU_THREADS * DUMP_PER;
    SpanDescs D{};
    int64_t keys = 0;
    for (int j = 0; j < windows; j++) {
        const hm_ctx::Gen *g = live_gen(ctx, first + (int64_t)j * ctx->cfg.tile_us);   // (the roll-up's rule)
        if (!g) continue;
        D.g[D.n] = gen_desc(*g);
        D.col[D.n] = j;
        D.tile0[D.n + 1] = D.tile0[D.n] + ((int64_t(1) << g->log2cap) + tile - 1) / tile;
        D.n++;
        keys += g->keys;
    }
    S.info[0] = D.n;
    S.info[1] = keys;
    if (D.n == 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // distinct parents possible: the windows' keys (a cell in two windows counted twice), and the cells of the resolution
    const int64_t bound = std::min(keys, h3_cells_at(res));
    const int64_t nslots = (int64_t)next_pow2((uint64_t)std::max<int64_t>(2 * bound, 1024));
    const size_t row = (size_t)windows * 8;
    int rc;
    if ((rc = span_init(ctx)) || (rc = ensure(ctx, ctx->ru_tab, (size_t)nslots * sizeof(GrowRec))) ||
        (rc = ensure(ctx, ctx->ru_out, (size_t)bound * sizeof(GrowRec))) || (rc = ensure(ctx, S.series, (size_t)nslots * row)) ||
        (rc = ensure(ctx, S.rows, (size_t)bound * row)))
        return rc;
    GrowRec *tab = (GrowRec *)ctx->ru_tab.p;
    unsigned long long *series = (unsigned long long *)S.series.p;
    unsigned long long *words = ctx->d_scratch + ROLLUP_WORD;   // parents emitted, overflow
    unsigned long long *sw = (unsigned long long *)S.words.p;
    const unsigned long long mask = (unsigned long long)(nslots - 1);
    double us = 0;
    float ms = 0;
    HIPCHK(ctx, hipMemsetAsync(tab, 0, (size_t)nslots * sizeof(GrowRec), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(series, 0, (size_t)nslots * row, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(words, 0, 16, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(sw, 0, SW_WORDS * 8, ctx->stream));
    // one workgroup per CU (its LDS table takes most of a CU's LDS), each a contiguous block of the tables' tiles
    const int grid = read_grid(ctx->read_grid, D.tile0[D.n] * tile, RU_THREADS * DUMP_PER, std::max(ctx->n_cus, 1));
    HIPCHK(ctx, hipEventRecord(S.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_span, dim3(grid), dim3(RU_THREADS), 0, ctx->stream, D, (int)res, (int)windows, tab, mask, series, words + 1);
    hipLaunchKernelGGL(k_span_emit, dim3(read_grid(ctx->read_grid, nslots, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, tab, nslots,
                       (const unsigned long long *)series, (int)windows, first, (GrowRec *)ctx->ru_out.p, (unsigned long long *)S.rows.p,
                       bound, words);
    HIPCHK(ctx, hipEventRecord(S.ev[1], ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    unsigned long long got[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(got, words, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if (hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess) us += 1e3 * ms;
    if (got[1]) return set_err(ctx, HM_E_OVERFLOW, "span parent table of %lld slots overflowed", (long long)nslots);
    if ((int64_t)got[0] > bound)
        return set_err(ctx, HM_E_STATE, "the span found %llu parents, at most %lld expected", got[0], (long long)bound);
    int64_t n = (int64_t)got[0];
    S.info[2] = n;
    S.info[5] = nslots;
    if (m_out) *m_out = n;
    if (nslots_out) *nslots_out = nslots;
    const GrowRec *recs = (const GrowRec *)ctx->ru_out.p;
    bool moved = false;   // the records are no longer where k_span_emit wrote them and their rows
    if (view && n > 0) {
        if ((rc = ensure(ctx, S.vout, (size_t)n * sizeof(GrowRec)))) return rc;
        const ViewPoles &poles = view_poles();
        unsigned long long kept = 0;
        HIPCHK(ctx, hipEventRecord(S.ev[2], ctx->stream));
        hipLaunchKernelGGL(k_view_tiles, dim3(read_grid(ctx->read_grid, n, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, recs, n,
                           poles.north[res], poles.south[res], *view, (GrowRec *)S.vout.p, sw + SW_VIEW);
        HIPCHK(ctx, hipEventRecord(S.ev[3], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&kept, sw + SW_VIEW, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if (hipEventElapsedTime(&ms, S.ev[2], S.ev[3]) == hipSuccess) us += 1e3 * ms;
        if ((int64_t)kept > n) return set_err(ctx, HM_E_STATE, "the view kept %llu of %lld records", kept, (long long)n);
        n = (int64_t)kept;
        recs = (const GrowRec *)S.vout.p;
        moved = true;
    }
    S.info[3] = n;
    if (k >= 0) {
        const GrowRec *o = nullptr;
        int64_t m = 0;
        if ((rc = top_on_device(ctx, recs, n, k, &o, &m))) return rc;
        us += (double)ctx->top.info[6];
        n = m;
        recs = o;
        moved = true;
    }
    const int64_t *rows = (const int64_t *)S.rows.p;
    if (moved && n > 0) {
        if ((rc = ensure(ctx, S.frows, (size_t)n * row))) return rc;
        unsigned long long missing = 0;
        HIPCHK(ctx, hipEventRecord(S.ev[4], ctx->stream));
        hipLaunchKernelGGL(k_span_rows, dim3(read_grid(ctx->read_grid, n, 256)), dim3(256), 0, ctx->stream, recs, n, (const GrowRec *)tab, mask,
                           (const unsigned long long *)series, (int)windows, (unsigned long long *)S.frows.p, sw + SW_MISSING);
        HIPCHK(ctx, hipEventRecord(S.ev[5], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&missing, sw + SW_MISSING, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if (hipEventElapsedTime(&ms, S.ev[4], S.ev[5]) == hipSuccess) us += 1e3 * ms;
        if (missing) return set_err(ctx, HM_E_STATE, "%llu of the span's %lld records are not in its parent table", missing, (long long)n);
        rows = (const int64_t *)S.frows.p;
    }
    S.info[4] = n;
    S.info[6] = (int64_t)us;
    *out = n ? recs : nullptr;
    *rows_out = n ? rows : nullptr;
    *n_out = n;
    return HM_OK;
}

// the checks every span call shares, in hm_window_top's order: the arguments, the resolution, the shard, the state
static int span_args(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_view *view, int64_t k, bool whole,
                     const char *who) {
    if (k >= 0 && !top_k_ok(k)) return top_bad_k(ctx, who, k);
    if (view && !view_valid(*view)) return top_bad_view(ctx, view);
    if (windows < 1 || windows > HM_SPAN_MAX_WINDOWS)
        return set_err(ctx, HM_E_INVALID, "%s: %d windows outside 1..%d", who, windows, HM_SPAN_MAX_WINDOWS);
    int64_t first;
    if (end_start_us % ctx->cfg.tile_us != 0 ||
        __builtin_sub_overflow(end_start_us, (int64_t)(windows - 1) * ctx->cfg.tile_us, &first))
        return set_err(ctx, HM_E_INVALID, "%s: the span's end %lld is not the start of a window of %lld us", who, (long long)end_start_us,
                       (long long)ctx->cfg.tile_us);
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (k >= 0 && ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank's top is not the global one (hm_top_records on the added records is)",
                       who, ctx->shard_rank, ctx->shard_count);
    if (whole && ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank's grid is its own keys' (add the ranks' hm_window_raster counts)", who,
                       ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    return HM_OK;
}

int hm_span_rollup(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_view *view, int64_t k, int32_t out_memory,
                   const hm_state_rec **recs, const int64_t **series, int64_t *n) {
    if (!ctx || !recs || !series || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    int rc;
    if ((rc = span_args(ctx, end_start_us, windows, res, view, k < 0 ? -1 : k, false, "hm_span_rollup"))) return rc;
    *recs = nullptr;
    *series = nullptr;
    *n = 0;
    hm_ctx::Span &S = ctx->span;
    const GrowRec *o = nullptr;
    const int64_t *rows = nullptr;
    int64_t m = 0;
    if ((rc = span_on_device(ctx, end_start_us, windows, res, view, k < 0 ? -1 : k, &o, &rows, &m))) return rc;
    if (m == 0) return HM_OK;
    if (out_memory == HM_MEM_HOST) {
        const size_t rbytes = (size_t)m * windows * 8;
        if ((rc = host_pinned(ctx, &S.h_recs, S.h_recs_cap, (size_t)m * sizeof(GrowRec))) ||
            (rc = host_pinned(ctx, &S.h_rows, S.h_rows_cap, rbytes)))
            return rc;
        HIPCHK(ctx, hipMemcpyAsync(S.h_recs, o, (size_t)m * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(S.h_rows, rows, rbytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *recs = (const hm_state_rec *)S.h_recs;
        *series = (const int64_t *)S.h_rows;
    } else {
        *recs = (const hm_state_rec *)o;
        *series = rows;
    }
    *n = m;
    return HM_OK;
}

int hm_span_geojson(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const hm_geojson_cfg *cfg, const hm_view *view,
                    int64_t k, int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n) {
    if (!ctx || !cfg || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    GjTexts X;
    if (gj_texts(cfg, X)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    int rc;
    if ((rc = span_args(ctx, end_start_us, windows, res, view, k < 0 ? -1 : k, false, "hm_span_geojson"))) return rc;
    *n = 0;
    const GrowRec *o = nullptr;
    const int64_t *rows = nullptr;
    int64_t m = 0;
    if ((rc = span_on_device(ctx, end_start_us, windows, res, view, k < 0 ? -1 : k, &o, &rows, &m))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = gj_tiles(ctx, X, o, m, out_memory, bytes, offsets, nullptr, false, rows, windows))) return rc;
    *n = m;
    return HM_OK;
}

int hm_span_raster(hm_ctx *ctx, int64_t end_start_us, int32_t windows, int32_t res, const double *lat, int32_t rows, const double *lon,
                   int32_t cols, const int64_t *thresholds, int32_t n_thresholds, int32_t out_memory, const uint32_t **counts,
                   const uint8_t **classes) {
    if (!ctx || !counts || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (const char *why = raster_grid_error(rows, cols)) return set_err(ctx, HM_E_INVALID, "hm_span_raster: %s", why);
    RasterThr thr;
    if (!raster_thresholds(thresholds, n_thresholds, thr))
        return set_err(ctx, HM_E_INVALID, "hm_span_raster: 0..%d thresholds, each >= 0, strictly ascending", RASTER_MAX_THRESHOLDS);
    int rc;
    if ((rc = span_args(ctx, end_start_us, windows, res, nullptr, -1, true, "hm_span_raster"))) return rc;
    const int64_t n = (int64_t)rows * cols;
    if (n > 0 && (!lat || !lon)) return set_err(ctx, HM_E_INVALID, "bad argument");
    *counts = nullptr;
    if (classes) *classes = nullptr;
    hm_ctx::Raster &R = ctx->raster;
    R.info[0] = n;
    R.info[1] = R.info[2] = R.info[3] = 0;
    if (n == 0) return HM_OK;
    const bool want_classes = n_thresholds > 0 && classes;
    const GrowRec *o = nullptr;
    const int64_t *srows = nullptr;
    int64_t kept = 0, m = 0, nslots = 0;
    if ((rc = span_on_device(ctx, end_start_us, windows, res, nullptr, -1, &o, &srows, &kept, &m, &nslots))) return rc;
    return raster_from_table(ctx, (const GrowRec *)ctx->ru_tab.p, nslots, m, res, lat, rows, lon, cols, thr, want_classes, out_memory, counts,
                             classes);
}

int hm_span_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 7; i++) v[i] = ctx->span.info[i];
    return HM_OK;
}

// Host execution of the span over per-window record arrays with the kernels' HM_HD parent code: a group-by on
// h3_cell_to_parent(cell, res), the sums in input order, the rows' column = the record's window
int hm_selftest_span(const hm_state_rec *recs, const int64_t *n_per_window, int32_t windows, int64_t first_us, int64_t tile_us, int32_t res,
                     hm_state_rec *out, int64_t *series, int64_t *n_out) {
    if (windows < 1 || windows > HM_SPAN_MAX_WINDOWS || !n_per_window || !n_out || res < 0 || res > 15 || tile_us < 1) return HM_E_INVALID;
    int64_t total = 0;
    for (int j = 0; j < windows; j++) {
        if (n_per_window[j] < 0 || n_per_window[j] > (int64_t(1) << 31)) return HM_E_INVALID;
        total += n_per_window[j];
    }
    *n_out = 0;
    if (total == 0) return HM_OK;
    if (!recs || !out || !series) return HM_E_INVALID;
    std::vector<std::pair<uint64_t, int64_t>> order((size_t)total);   // (parent, input index)
    std::vector<int> col((size_t)total);
    int64_t i = 0;
    for (int j = 0; j < windows; j++)
        for (int64_t q = 0; q < n_per_window[j]; q++, i++) {
            const int r = (int)((recs[i].cell >> 52) & 0xf);
            if (recs[i].cell == 0 || r < res) return HM_E_INVALID;
            order[i] = {h3_cell_to_parent(recs[i].cell, res), i};
            col[i] = j;
        }
    std::sort(order.begin(), order.end());
    int64_t m = 0;
    for (int64_t a = 0; a < total; a++) {
        const hm_state_rec &r = recs[order[a].second];
        if (a == 0 || order[a].first != order[a - 1].first) {
            hm_state_rec z = {};
            z.cell = order[a].first;
            z.window_start_us = first_us;
            out[m] = z;
            for (int j = 0; j < windows; j++) series[m * windows + j] = 0;
            m++;
        }
        hm_state_rec &o = out[m - 1];
        o.count += r.count;
        o.n_speed += r.n_speed;
        if (r.n_speed) o.sum_speed += r.sum_speed;
        o.sum_lat += r.sum_lat;
        o.sum_lon += r.sum_lon;
        series[(m - 1) * windows + col[order[a].second]] += r.count;
    }
    *n_out = m;
    return HM_OK;
}

int hm_selftest_span_features(const hm_geojson_cfg *cfg, const hm_state_rec *recs, const int64_t *series, int32_t windows, int64_t n,
                              uint8_t *bytes, int64_t cap, int64_t *offsets) {
    GjTexts T;
    if (n < 0 || windows < 1 || windows > HM_SPAN_MAX_WINDOWS || !bytes || !offsets || (n > 0 && (!recs || !series)) ||
        cap < (int64_t)sizeof(GJ_EMPTY_BODY) - 1)
        return HM_E_INVALID;
    if (gj_texts(cfg, T)) return HM_E_INVALID;
    static const H3Tables H = make_tables();
    memcpy(bytes, GJ_EMPTY_BODY, GJ_PREFIX_LEN);
    int64_t o = GJ_PREFIX_LEN;
    for (int64_t i = 0; i < n; i++) {
        offsets[i] = o;
        const hm_state_rec &r = recs[i];
        const GjSpan gs = {windows, series + i * windows};
        double la[10], lo[10];
        const int nv = cellToBoundaryDeg(r.cell, H, la, lo);
        const int len = tile_feature(nullptr, T, r.cell, r.count, r.n_speed, r.sum_speed, nv, la, lo, 1, nullptr, nullptr, &gs);
        if (o + len + 2 > cap) return HM_E_INVALID;
        tile_feature(bytes + o, T, r.cell, r.count, r.n_speed, r.sum_speed, nv, la, lo, 1, nullptr, nullptr, &gs);
        o += len;
        bytes[o++] = i == n - 1 ? ']' : ',';
    }
    offsets[n] = o;
    if (n == 0) bytes[o++] = ']';
    bytes[o] = '}';
    return HM_OK;
}
