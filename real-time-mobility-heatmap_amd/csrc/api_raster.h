// C ABI: the read side as a raster -- one live window's counts over a separable pixel grid (k_raster.h), what a
// /api/tiles/latest/{z}/{x}/{y}.png route colours (mobheat/readside.py tiles_latest_png; the reference's UI loads its base
// layer as such tiles, app.py:122, and colours hexagons in seven count classes, app.py:135-142).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// the grid's limits; the message names the one that failed
static const char *raster_grid_error(int32_t rows, int32_t cols) {
    if (rows < 0 || rows > RASTER_MAX_DIM) return "rows outside 0..16384";
    if (cols < 0 || cols > RASTER_MAX_DIM) return "cols outside 0..16384";
    if ((int64_t)rows * cols > RASTER_MAX_PIXELS) return "rows * cols above 2^26";
    return nullptr;
}

static int raster_init(hm_ctx *ctx) {
    hm_ctx::Raster &R = ctx->raster;
    if (R.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, R.words, 256))) return rc;
    for (auto &e : R.ev) HIPCHK(ctx, hipEventCreate(&e));
    R.ready = true;
    return HM_OK;
}

// The grid looked up in a group table of nslots GrowRec slots holding m records (m == 0: no table, an all-zero grid):
// upload lat / lon, k_raster + k_raster_exact, the outputs handed out per out_memory.  R.info[0] is the caller's;
// [1]-[3] are set here.  Shared by hm_window_raster (the roll-up's table) and hm_positions_density_raster (the density's).
static int raster_from_table(hm_ctx *ctx, const GrowRec *tab, int64_t nslots, int64_t m, int32_t res, const double *lat, int32_t rows,
                             const double *lon, int32_t cols, const RasterThr &thr, bool want_classes, int32_t out_memory,
                             const uint32_t **counts, const uint8_t **classes) {
    hm_ctx::Raster &R = ctx->raster;
    const int64_t n = (int64_t)rows * cols;
    int rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = raster_init(ctx)) || (rc = ensure(ctx, R.counts, (size_t)n * 4)) ||
        (want_classes && (rc = ensure(ctx, R.classes, (size_t)n))))
        return rc;
    uint32_t *d_counts = (uint32_t *)R.counts.p;
    uint8_t *d_classes = want_classes ? (uint8_t *)R.classes.p : nullptr;
    R.info[2] = m;
    if (m == 0) {   // nothing to look anything up in
        HIPCHK(ctx, hipMemsetAsync(d_counts, 0, (size_t)n * 4, ctx->stream));
        if (d_classes) HIPCHK(ctx, hipMemsetAsync(d_classes, 0, (size_t)n, ctx->stream));
    } else {
        if ((rc = ensure(ctx, R.lat, (size_t)rows * 8)) || (rc = ensure(ctx, R.lon, (size_t)cols * 8)) ||
            (rc = ensure(ctx, R.slow, (size_t)n * 4)))
            return rc;
        unsigned long long *n_slow = (unsigned long long *)R.words.p;
        HIPCHK(ctx, hipMemcpyAsync(R.lat.p, lat, (size_t)rows * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(R.lon.p, lon, (size_t)cols * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(n_slow, 0, 8, ctx->stream));
        const unsigned long long mask = (unsigned long long)(nslots - 1);
        const int64_t nunits = (int64_t)rows * ((cols + 63) / 64);   // a wave each, four to a workgroup
        HIPCHK(ctx, hipEventRecord(R.ev[0], ctx->stream));
        hipLaunchKernelGGL(k_raster, dim3(read_grid(ctx->read_grid, nunits, 4, 256 * 32)), dim3(256), 0, ctx->stream, (const double *)R.lat.p, (int)rows,
                           (const double *)R.lon.p, (int)cols, (int)res, tab, mask, thr, d_counts, d_classes, (unsigned int *)R.slow.p,
                           n_slow);
        hipLaunchKernelGGL(k_raster_exact, dim3(256), dim3(256), 0, ctx->stream, (const double *)R.lat.p, (const double *)R.lon.p,
                           (int)cols, (int)res, tab, mask, thr, d_counts, d_classes, (const unsigned int *)R.slow.p,
                           (const unsigned long long *)n_slow);
        HIPCHK(ctx, hipEventRecord(R.ev[1], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        unsigned long long ne = 0;
        HIPCHK(ctx, hipMemcpyAsync(&ne, n_slow, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if ((int64_t)ne > n) return set_err(ctx, HM_E_STATE, "the raster's exception list holds %llu of %lld pixels", ne, (long long)n);
        R.info[1] = (int64_t)ne;
        float ms = 0;
        if (hipEventElapsedTime(&ms, R.ev[0], R.ev[1]) == hipSuccess) R.info[3] = (int64_t)(1e3 * ms);
    }
    if (out_memory == HM_MEM_HOST) {
        if ((rc = host_pinned(ctx, &R.h_counts, R.h_counts_cap, (size_t)n * 4)) ||
            (d_classes && (rc = host_pinned(ctx, &R.h_classes, R.h_classes_cap, (size_t)n))))
            return rc;
        HIPCHK(ctx, hipMemcpyAsync(R.h_counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (d_classes) HIPCHK(ctx, hipMemcpyAsync(R.h_classes, d_classes, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *counts = (const uint32_t *)R.h_counts;
        if (d_classes) *classes = (const uint8_t *)R.h_classes;
    } else {
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *counts = d_counts;
        if (d_classes) *classes = d_classes;
    }
    return HM_OK;
}

int hm_window_raster(hm_ctx *ctx, int64_t window_start_us, int32_t res, const double *lat, int32_t rows, const double *lon,
                     int32_t cols, const int64_t *thresholds, int32_t n_thresholds, int32_t out_memory, const uint32_t **counts,
                     const uint8_t **classes) {
    if (!ctx || !counts || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (const char *why = raster_grid_error(rows, cols)) return set_err(ctx, HM_E_INVALID, "hm_window_raster: %s", why);
    RasterThr thr;
    if (!raster_thresholds(thresholds, n_thresholds, thr))
        return set_err(ctx, HM_E_INVALID, "hm_window_raster: 0..%d thresholds, each >= 0, strictly ascending", RASTER_MAX_THRESHOLDS);
    if (n_thresholds > 0 && ctx->shard_count > 1)
        return set_err(ctx, HM_E_INVALID, "hm_window_raster: classes on a shard context (add the ranks' counts, then classify)");
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "raster resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_window_raster between stage calls");
    const int64_t n = (int64_t)rows * cols;
    if (n > 0 && (!lat || !lon)) return set_err(ctx, HM_E_INVALID, "bad argument");
    *counts = nullptr;
    if (classes) *classes = nullptr;
    hm_ctx::Raster &R = ctx->raster;
    R.info[0] = n;
    R.info[1] = R.info[2] = R.info[3] = 0;
    if (n == 0) return HM_OK;
    const bool want_classes = n_thresholds > 0 && classes;
    int64_t m = 0, nslots = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, "hm_window_raster", &m, &nslots))) return rc;
    return raster_from_table(ctx, (const GrowRec *)ctx->ru_tab.p, nslots, m, res, lat, rows, lon, cols, thr, want_classes, out_memory,
                             counts, classes);
}

// Host execution of the same per-pixel code: the fast path with its hand-over to the exact path, the cell-0 rule, a
// table of the roll-up's layout (GrowRec slots, home mix64(cell) & mask, linear probing, 0 = free) and raster_put.
// Records of equal cell add up (a caller may pass several ranks' records).
int hm_selftest_window_raster(const hm_state_rec *recs, int64_t n, int32_t res, const double *lat, int32_t rows, const double *lon,
                              int32_t cols, const int64_t *thresholds, int32_t n_thresholds, uint32_t *counts, uint8_t *classes) {
    RasterThr thr;
    if (n < 0 || (n > 0 && !recs) || res < 0 || res > 15 || raster_grid_error(rows, cols) ||
        !raster_thresholds(thresholds, n_thresholds, thr))
        return HM_E_INVALID;
    const int64_t npix = (int64_t)rows * cols;
    if (npix == 0) return HM_OK;
    if (!lat || !lon || !counts) return HM_E_INVALID;
    static const H3Tables T = make_tables();
    const uint64_t nslots = next_pow2((uint64_t)std::max<int64_t>(2 * n, 1024)), mask = nslots - 1;
    std::vector<GrowRec> tab((size_t)nslots);   // (value-initialised: every cell word 0)
    for (int64_t k = 0; k < n; k++) {
        if (recs[k].cell == 0) return HM_E_INVALID;
        uint64_t h = mix64(recs[k].cell) & mask;
        while (tab[h].cell != 0 && tab[h].cell != recs[k].cell) h = (h + 1) & mask;
        tab[h].cell = recs[k].cell;
        tab[h].count += (uint64_t)recs[k].count;
    }
    uint8_t *cls = n_thresholds > 0 ? classes : nullptr;
    for (int32_t r = 0; r < rows; r++)
        for (int32_t c = 0; c < cols; c++) {
            uint64_t cell;
            if (!latLngToCellFast(lat[r], lon[c], res, T, cell)) cell = latLngToCellDeg(lat[r], lon[c], res, T);
            unsigned long long count = 0;
            if (cell != 0)
                for (uint64_t h = mix64(cell) & mask; tab[h].cell != 0; h = (h + 1) & mask)
                    if (tab[h].cell == cell) { count = tab[h].count; break; }
            raster_put(count, thr, (int64_t)r * cols + c, counts, cls);
        }
    return HM_OK;
}

int hm_raster_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 4; i++) v[i] = ctx->raster.info[i];
    return HM_OK;
}
