// C ABI: the positions state aggregated into H3 density cells -- "how many vehicles are in each cell right now" at the
// resolution that fits the zoom, as records, for a viewport, and as a raster (k_density.h; the view is k_view_tiles, the
// raster k_raster on the density's own group table).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

static int density_init(hm_ctx *ctx) {
    hm_ctx::Density &D = ctx->dens;
    if (D.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, D.words, 256))) return rc;
    for (auto &e : D.ev) HIPCHK(ctx, hipEventCreate(&e));
    D.ready = true;
    return HM_OK;
}
// the slots of the group table for `keys` keys at res: 2^k >= max(2 * (distinct cells possible), 1024)
static int64_t density_slots(int64_t keys, int res) {
    return (int64_t)next_pow2((uint64_t)std::max<int64_t>(2 * std::min(keys, h3_cells_at(res)), 1024));
}

// The checks every density entry point shares, after its own argument checks (HM_E_INVALID comes first there).
static int density_state_ok(hm_ctx *ctx, const char *who) {
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank holds only the latest rows it received", who,
                       ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    return HM_OK;
}

// density(S, res, since_us) on the device: the groups' records in D.out, or -- with a view -- those whose cell is in
// view in D.vout; *recs = the records (device), *n their number, *nslots_out (optional) the slots of the group table in
// D.tab (0: no table), *groups_out (optional) the groups before the view.  Reads S only.
static int density_on_device(hm_ctx *ctx, int32_t res, int64_t since_us, const hm_view *view, const GrowRec **recs, int64_t *n,
                             int64_t *nslots_out = nullptr, int64_t *groups_out = nullptr) {
    static_assert(sizeof(hm_state_rec) == sizeof(GrowRec), "hm_state_rec mirrors GrowRec");
    hm_ctx::Positions &P = ctx->pos;
    hm_ctx::Density &D = ctx->dens;
    *recs = nullptr;
    *n = 0;
    if (nslots_out) *nslots_out = 0;
    if (groups_out) *groups_out = 0;
    for (int64_t &x : D.info) x = 0;
    D.info[0] = P.keys;
    if (P.keys == 0 || !P.tab) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t cap = (int64_t)P.cap, bound = std::min(P.keys, h3_cells_at(res)), nslots = density_slots(P.keys, res);
    int rc;
    if ((rc = density_init(ctx)) || (rc = ensure(ctx, D.cell_of, (size_t)cap * 8)) || (rc = ensure(ctx, D.slow, (size_t)cap * 4)) ||
        (rc = ensure(ctx, D.tab, (size_t)nslots * sizeof(GrowRec))) || (rc = ensure(ctx, D.out, (size_t)bound * sizeof(GrowRec))) ||
        (view && (rc = ensure(ctx, D.vout, (size_t)bound * sizeof(GrowRec)))))
        return rc;
    unsigned long long *words = (unsigned long long *)D.words.p;
    GrowRec *tab = (GrowRec *)D.tab.p;
    HIPCHK(ctx, hipMemsetAsync(tab, 0, (size_t)nslots * sizeof(GrowRec), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(words, 0, DW_WORDS * 8, ctx->stream));
    // one group-by workgroup per CU (its LDS table takes most of a CU's LDS), looping over the slots
    const int groups_grid = read_grid(ctx->read_grid, cap, RU_THREADS * DUMP_PER, std::max(ctx->n_cus, 1));
    HIPCHK(ctx, hipEventRecord(D.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_density_cells, dim3(read_grid(ctx->read_grid, cap, 256, 256 * 32)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab, cap,
                       (int)res, (long long)since_us, (uint64_t *)D.cell_of.p, (unsigned int *)D.slow.p, words + DW_SLOW);
    hipLaunchKernelGGL(k_density_exact, dim3(256), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab, (int)res, (uint64_t *)D.cell_of.p,
                       (const unsigned int *)D.slow.p, (const unsigned long long *)(words + DW_SLOW));
    hipLaunchKernelGGL(k_density_group, dim3(groups_grid), dim3(RU_THREADS), 0, ctx->stream, (const PosSlot *)P.tab, cap,
                       (const uint64_t *)D.cell_of.p, tab, (unsigned long long)(nslots - 1), words);
    hipLaunchKernelGGL(k_density_emit, dim3(read_grid(ctx->read_grid, nslots, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const GrowRec *)tab, nslots,
                       (GrowRec *)D.out.p, bound, words + DW_OUT);
    HIPCHK(ctx, hipEventRecord(D.ev[1], ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    unsigned long long w[DW_WORDS] = {};
    HIPCHK(ctx, hipMemcpyAsync(w, words, DW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    float ms = 0, view_ms = 0;
    if (hipEventElapsedTime(&ms, D.ev[0], D.ev[1]) != hipSuccess) ms = 0;
    if (w[DW_OVERFLOW]) return set_err(ctx, HM_E_OVERFLOW, "density group table of %lld slots overflowed", (long long)nslots);
    if ((int64_t)w[DW_OUT] > bound || (int64_t)w[DW_SLOW] > cap)
        return set_err(ctx, HM_E_STATE, "density found %llu groups (at most %lld expected), %llu exceptions of %lld slots", w[DW_OUT],
                       (long long)bound, w[DW_SLOW], (long long)cap);
    const int64_t m = (int64_t)w[DW_OUT];
    int64_t kept = m;
    const GrowRec *out = (const GrowRec *)D.out.p;
    if (view && m > 0) {   // (the view's validity is the caller's check)
        const ViewPoles &poles = view_poles();
        HIPCHK(ctx, hipEventRecord(D.ev[2], ctx->stream));
        hipLaunchKernelGGL(k_view_tiles, dim3(read_grid(ctx->read_grid, m, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, out, m, poles.north[res],
                           poles.south[res], *view, (GrowRec *)D.vout.p, words + DW_VIEW);
        HIPCHK(ctx, hipEventRecord(D.ev[3], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&w[DW_VIEW], words + DW_VIEW, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if (hipEventElapsedTime(&view_ms, D.ev[2], D.ev[3]) != hipSuccess) view_ms = 0;
        if ((int64_t)w[DW_VIEW] > m) return set_err(ctx, HM_E_STATE, "the view kept %llu of %lld groups", w[DW_VIEW], (long long)m);
        kept = (int64_t)w[DW_VIEW];
        out = (const GrowRec *)D.vout.p;
    }
    D.info[8] = (int64_t)(1e3 * (ms + view_ms));   // (the host's read of the group count between the two intervals is not in it)
    D.info[1] = (int64_t)w[DW_KEPT];
    D.info[2] = (int64_t)w[DW_UNSNAPPED];
    D.info[3] = m;
    D.info[4] = kept;
    D.info[5] = (int64_t)w[DW_SLOW];
    D.info[6] = (int64_t)w[DW_GADDS];
    D.info[7] = groups_grid;
    D.info[9] = nslots;
    *recs = out;
    *n = kept;
    if (nslots_out) *nslots_out = nslots;
    if (groups_out) *groups_out = m;
    return HM_OK;
}

int hm_positions_density(hm_ctx *ctx, int32_t res, int64_t since_us, const hm_view *view, int32_t out_memory,
                         const hm_state_rec **recs, int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (res < 0 || res > 15) return set_err(ctx, HM_E_INVALID, "density resolution %d outside 0..15", res);
    if (view && !view_valid(*view))
        return set_err(ctx, HM_E_INVALID, "view (%g, %g, %g, %g): finite, -90 <= south <= north <= 90, -180 <= west, east <= 180",
                       view->west, view->south, view->east, view->north);
    int rc;
    if ((rc = density_state_ok(ctx, "hm_positions_density"))) return rc;
    *recs = nullptr;
    *n = 0;
    const GrowRec *d = nullptr;
    int64_t m = 0;
    if ((rc = density_on_device(ctx, res, since_us, view, &d, &m))) return rc;
    if (m == 0) return HM_OK;
    if (out_memory == HM_MEM_HOST) {
        hm_ctx::Density &D = ctx->dens;
        if ((rc = host_pinned(ctx, &D.h_recs, D.h_recs_cap, (size_t)m * sizeof(GrowRec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(D.h_recs, d, (size_t)m * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *recs = (const hm_state_rec *)D.h_recs;
    } else {
        *recs = (const hm_state_rec *)d;
    }
    *n = m;
    return HM_OK;
}

int hm_positions_density_raster(hm_ctx *ctx, int32_t res, int64_t since_us, const double *lat, int32_t rows, const double *lon,
                                int32_t cols, const int64_t *thresholds, int32_t n_thresholds, int32_t out_memory,
                                const uint32_t **counts, const uint8_t **classes) {
    if (!ctx || !counts || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (const char *why = raster_grid_error(rows, cols)) return set_err(ctx, HM_E_INVALID, "hm_positions_density_raster: %s", why);
    RasterThr thr;
    if (!raster_thresholds(thresholds, n_thresholds, thr))
        return set_err(ctx, HM_E_INVALID, "hm_positions_density_raster: 0..%d thresholds, each >= 0, strictly ascending",
                       RASTER_MAX_THRESHOLDS);
    if (res < 0 || res > 15) return set_err(ctx, HM_E_INVALID, "density resolution %d outside 0..15", res);
    const int64_t n = (int64_t)rows * cols;
    if (n > 0 && (!lat || !lon)) return set_err(ctx, HM_E_INVALID, "bad argument");
    int rc;
    if ((rc = density_state_ok(ctx, "hm_positions_density_raster"))) return rc;
    *counts = nullptr;
    if (classes) *classes = nullptr;
    hm_ctx::Raster &R = ctx->raster;
    R.info[0] = n;
    R.info[1] = R.info[2] = R.info[3] = 0;
    if (n == 0) return HM_OK;
    const bool want_classes = n_thresholds > 0 && classes;
    const GrowRec *d = nullptr;
    int64_t m = 0, nslots = 0;
    if ((rc = density_on_device(ctx, res, since_us, nullptr, &d, &m, &nslots))) return rc;
    return raster_from_table(ctx, (const GrowRec *)ctx->dens.tab.p, nslots, m, res, lat, rows, lon, cols, thr, want_classes, out_memory,
                             counts, classes);
}

// Host execution of the same per-key code: the since compare, the fast path with its hand-over to the exact path, the
// cell-0 rule, a GrowRec table of the device's layout and size (home mix64(cell) & mask, linear probing, 0 = free), sums
// added in record order, the newest ts by dn_ts_enc's order.  Records leave in slot order.
int hm_selftest_positions_density(const hm_position_rec *recs, int64_t n, int32_t res, int64_t since_us, hm_state_rec *out,
                                  int64_t cap, int64_t *n_out, int64_t *unsnapped) {
    if (n < 0 || (n > 0 && !recs) || res < 0 || res > 15 || cap < 0 || (cap > 0 && !out) || !n_out) return HM_E_INVALID;
    static const H3Tables T = make_tables();
    *n_out = 0;
    if (unsnapped) *unsnapped = 0;
    const uint64_t nslots = (uint64_t)density_slots(n, res), mask = nslots - 1;
    std::vector<GrowRec> tab((size_t)nslots);   // (value-initialised: every word 0, as the device's memset)
    int64_t bad = 0, groups = 0;
    for (int64_t k = 0; k < n; k++) {
        if (!(recs[k].ts_us >= since_us)) continue;
        uint64_t cell;
        if (!latLngToCellFast(recs[k].lat, recs[k].lon, res, T, cell)) cell = latLngToCellDeg(recs[k].lat, recs[k].lon, res, T);
        if (cell == 0) { bad++; continue; }
        uint64_t h = mix64(cell) & mask;
        while (tab[h].cell != 0 && tab[h].cell != cell) h = (h + 1) & mask;
        if (tab[h].cell == 0) { tab[h].cell = cell; groups++; }
        tab[h].count += 1;
        tab[h].slat += recs[k].lat;
        tab[h].slon += recs[k].lon;
        const unsigned long long te = dn_ts_enc(recs[k].ts_us);
        if (te > (unsigned long long)tab[h].wstart) tab[h].wstart = (int64_t)te;
    }
    if (unsnapped) *unsnapped = bad;
    *n_out = groups;
    if (groups > cap) return HM_E_INVALID;
    int64_t at = 0;
    for (uint64_t h = 0; h < nslots; h++) {
        if (tab[h].cell == 0) continue;
        hm_state_rec r;
        memset(&r, 0, sizeof r);
        r.cell = tab[h].cell;
        r.window_start_us = dn_ts_dec((unsigned long long)tab[h].wstart);
        r.count = (int64_t)tab[h].count;
        r.sum_lat = tab[h].slat;
        r.sum_lon = tab[h].slon;
        out[at++] = r;
    }
    return HM_OK;
}

int hm_positions_density_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 10; i++) v[i] = ctx->dens.info[i];
    return HM_OK;
}
