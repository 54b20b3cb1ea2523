// C ABI: the read side for a map viewport -- which cells are in view (standalone, as hm_cells_to_boundary), and the two
// GeoJSON bodies of the tiles / positions in view (k_view.h; api_geojson.h encodes what the filter kept).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// the two pole cells of every resolution, from the host execution of latLngToCell (once per process)
static const ViewPoles &view_poles() {
    static const ViewPoles P = [] {
        const H3Tables T = make_tables();
        ViewPoles p;
        for (int r = 0; r < 16; r++) {
            p.north[r] = latLngToCellDeg(90.0, 0.0, r, T);
            p.south[r] = latLngToCellDeg(-90.0, 0.0, r, T);
        }
        return p;
    }();
    return P;
}

int hm_cells_in_view(const uint64_t *cells, int64_t n, int32_t memory, int32_t device, const hm_view *view, uint8_t *keep_u8) {
    if (n < 0 || n > (int64_t)UINT32_MAX || !view || !view_valid(*view) || (n > 0 && (!cells || !keep_u8)) ||
        (memory != HM_MEM_HOST && memory != HM_MEM_DEVICE))
        return HM_E_INVALID;
    if (n == 0) return HM_OK;
    const ViewPoles &poles = view_poles();
    std::lock_guard<std::mutex> lock(g_udf_mu);
    UdfState *S = nullptr;
    int rc;
    if ((rc = udf_begin(device, S))) return rc;
    const uint64_t *dcells = cells;
    uint8_t *dkeep = keep_u8;
    hipError_t e = hipSuccess;
    if (memory == HM_MEM_HOST) {
        if (udf_buf(S->in0, n * 8) || udf_buf(S->out2, n)) return HM_E_NOMEM;
        e = hipMemcpyAsync(S->in0.p, cells, n * 8, hipMemcpyHostToDevice, S->stream);
        dcells = (const uint64_t *)S->in0.p;
        dkeep = (uint8_t *)S->out2.p;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_cells_in_view, dim3(read_grid(udf_read_grid(), n, 256, 256 * 32)), dim3(256), 0, S->stream, dcells, n, poles, *view, dkeep);
        e = hipGetLastError();
    }
    if (e == hipSuccess && memory == HM_MEM_HOST) e = hipMemcpyAsync(keep_u8, dkeep, n, hipMemcpyDeviceToHost, S->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(S->stream);
    return e == hipSuccess ? HM_OK : HM_E_HIP;
}

int hm_selftest_cells_in_view(const uint64_t *cells, int64_t n, const hm_view *view, uint8_t *keep_u8) {
    if (n < 0 || !view || !view_valid(*view) || (n > 0 && (!cells || !keep_u8))) return HM_E_INVALID;
    static const H3Tables T = make_tables();
    const ViewPoles &poles = view_poles();
    for (int64_t i = 0; i < n; i++) {
        const int res = (int)((cells[i] >> 52) & 0xf);
        keep_u8[i] = cell_in_view(cells[i], T, poles.north[res], poles.south[res], *view) ? 1 : 0;
    }
    return HM_OK;
}

int hm_window_geojson_view(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                           const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs,
                           const hm_view *view) {
    if (!ctx || !cfg || !bytes || !offsets || !n || !view || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!view_valid(*view))
        return set_err(ctx, HM_E_INVALID, "view (%g, %g, %g, %g): finite, -90 <= south <= north <= 90, -180 <= west, east <= 180",
                       view->west, view->south, view->east, view->north);
    GjTexts T;
    if (gj_texts(cfg, T)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    *n = 0;
    if (recs) *recs = nullptr;
    int64_t m = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, "hm_window_geojson_view", &m))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hm_ctx::GeoJson &G = ctx->gj;
    if ((rc = gj_init(ctx))) return rc;
    G.candidates = m;
    G.view_us = 0;
    unsigned long long kept = 0;
    if (m > 0) {
        if ((rc = ensure(ctx, G.vrecs, (size_t)m * sizeof(GrowRec)))) return rc;
        const ViewPoles &poles = view_poles();
        unsigned long long *w = (unsigned long long *)G.words.p + GJW_OUT;
        HIPCHK(ctx, hipMemsetAsync(w, 0, 8, ctx->stream));
        HIPCHK(ctx, hipEventRecord(G.vev[0], ctx->stream));
        hipLaunchKernelGGL(k_view_tiles, dim3(read_grid(ctx->read_grid, m, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const GrowRec *)ctx->ru_out.p, m,
                           poles.north[res], poles.south[res], *view, (GrowRec *)G.vrecs.p, w);
        HIPCHK(ctx, hipEventRecord(G.vev[1], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&kept, w, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        float ms = 0;
        if (hipEventElapsedTime(&ms, G.vev[0], G.vev[1]) == hipSuccess) G.view_us = 1e3 * ms;
        if ((int64_t)kept > m) return set_err(ctx, HM_E_STATE, "the view kept %llu of %lld records", kept, (long long)m);
    }
    const int64_t k = (int64_t)kept;
    if (recs && k > 0) {   // the kept records in feature order
        if ((rc = host_pinned(ctx, &ctx->h_ru, ctx->h_ru_cap, (size_t)k * sizeof(GrowRec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_ru, G.vrecs.p, (size_t)k * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
        *recs = (const hm_state_rec *)ctx->h_ru;
    }
    if ((rc = gj_tiles(ctx, T, (const GrowRec *)G.vrecs.p, k, out_memory, bytes, offsets))) return rc;
    *n = k;
    return HM_OK;
}

int hm_positions_geojson_view(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                              const int64_t **offsets, int64_t *n, const hm_position_rec **recs, const hm_view *view) {
    if (!ctx || !view) return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!view_valid(*view))
        return set_err(ctx, HM_E_INVALID, "view (%g, %g, %g, %g): finite, -90 <= south <= north <= 90, -180 <= west, east <= 180",
                       view->west, view->south, view->east, view->north);
    return gj_positions(ctx, buckets, out_memory, bytes, offsets, n, recs, view, "hm_positions_geojson_view");
}
