// C ABI: the read side of the tile state -- the live windows, one window's tiles at any resolution r <= h3_res
// (the reference's /api/tiles/latest reads them from MongoDB, app.py:45-69; here they come from the state the engine holds).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

int hm_live_windows(hm_ctx *ctx, int64_t *window_start_us, int64_t *keys, int64_t cap, int64_t *n) {
    if (!ctx || !n || cap < 0) return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_live_windows between stage calls");
    std::vector<std::pair<int64_t, int64_t>> w;
    for (const auto &g : ctx->gens)
        if (g.keys > 0) w.emplace_back(wdec(g.wenc), g.keys);   // (a window whose table holds no key yet has no tile)
    std::sort(w.begin(), w.end());
    *n = (int64_t)w.size();
    for (int64_t i = 0; i < *n && i < cap; i++) {
        if (window_start_us) window_start_us[i] = w[i].first;
        if (keys) keys[i] = w[i].second;
    }
    return HM_OK;
}

// the live window that starts at window_start_us: its table if it holds a key, else nullptr (rollup_on_device, and the
// span's window selection, api_span.h)
static const hm_ctx::Gen *live_gen(const hm_ctx *ctx, int64_t window_start_us) {
    const hm_ctx::Gen *gen = nullptr;
    for (const auto &g : ctx->gens)
        if (g.wenc == wenc_of(window_start_us) && g.keys > 0) gen = &g;
    return gen;
}

// One pass over the window's table (k_rollup) into a zeroed parent table, then the compaction (k_rollup_emit); buffers
// of its own (ru_tab, ru_out, h_ru), so that a checkpoint dump waiting in parts_regrow stays as it is.
// Leaves *m_out records of window window_start_us at res in ctx->ru_out (0: the window is not live); `who` names the
// entry point in the errors (hm_window_rollup, and hm_window_geojson, which encodes the records where they are).
// nslots_out (optional): the slots of the parent table in ctx->ru_tab, which stays probe-able until the next roll-up
// (hm_window_raster looks the pixels' cells up there; a change call, api_change.h, counts as one: it rolls its current
// window up through ru_tab); 0 when the window is not live.
// tab / out (optional): the parent table and the record buffer to use instead of ctx->ru_tab / ctx->ru_out (the change's
// base window, api_change.h: its roll-up must survive the current window's).
static int rollup_on_device(hm_ctx *ctx, int64_t window_start_us, int32_t res, const char *who, int64_t *m_out,
                            int64_t *nslots_out = nullptr, DevBuf *tab = nullptr, DevBuf *out = nullptr) {
    static_assert(sizeof(hm_state_rec) == sizeof(GrowRec), "hm_state_rec mirrors GrowRec");
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    *m_out = 0;
    if (nslots_out) *nslots_out = 0;
    const hm_ctx::Gen *gen = live_gen(ctx, window_start_us);
    if (!gen) return HM_OK;
    DevBuf &ru_tab = tab ? *tab : ctx->ru_tab, &ru_out = out ? *out : ctx->ru_out;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // distinct parents possible: the window's keys, and the cells of the target resolution
    const int64_t bound = std::min(gen->keys, h3_cells_at(res));
    const int64_t nslots = (int64_t)next_pow2((uint64_t)std::max<int64_t>(2 * bound, 1024));
    int rc;
    if ((rc = ensure(ctx, ru_tab, (size_t)nslots * sizeof(GrowRec))) ||
        (rc = ensure(ctx, ru_out, (size_t)bound * sizeof(GrowRec))))
        return rc;
    unsigned long long *words = ctx->d_scratch + ROLLUP_WORD;   // parents emitted, overflow
    HIPCHK(ctx, hipMemsetAsync(ru_tab.p, 0, (size_t)nslots * sizeof(GrowRec), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(words, 0, 16, ctx->stream));
    const GenDesc d = gen_desc(*gen);
    // one workgroup per CU (its LDS table takes most of a CU's LDS), looping over the table
    const int grid = read_grid(ctx->read_grid, int64_t(1) << gen->log2cap, RU_THREADS * DUMP_PER, std::max(ctx->n_cus, 1));
    hipLaunchKernelGGL(k_rollup, dim3(grid), dim3(RU_THREADS), 0, ctx->stream, d, (int)res, (GrowRec *)ru_tab.p,
                       (unsigned long long)(nslots - 1), words + 1);
    hipLaunchKernelGGL(k_rollup_emit, dim3(read_grid(ctx->read_grid, nslots, 256 * DUMP_PER)), dim3(256), 0, ctx->stream,
                       (const GrowRec *)ru_tab.p, nslots, window_start_us, (GrowRec *)ru_out.p, bound, words);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long got[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(got, words, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if (got[1]) return set_err(ctx, HM_E_OVERFLOW, "roll-up parent table of %lld slots overflowed", (long long)nslots);
    if ((int64_t)got[0] > bound)
        return set_err(ctx, HM_E_STATE, "roll-up found %llu parents, at most %lld expected", got[0], (long long)bound);
    *m_out = (int64_t)got[0];
    if (nslots_out) *nslots_out = nslots;
    return HM_OK;
}

int hm_window_rollup(hm_ctx *ctx, int64_t window_start_us, int32_t res, int32_t out_memory, const hm_state_rec **recs,
                     int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    *recs = nullptr;
    *n = 0;
    int64_t m = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, "hm_window_rollup", &m))) return rc;
    if (m == 0) return HM_OK;
    if (out_memory == HM_MEM_HOST) {
        if ((rc = host_pinned(ctx, &ctx->h_ru, ctx->h_ru_cap, (size_t)std::max<int64_t>(m, 1) * sizeof(GrowRec)))) return rc;
        if (m > 0) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_ru, ctx->ru_out.p, (size_t)m * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        }
        *recs = (const hm_state_rec *)ctx->h_ru;
    } else {
        *recs = (const hm_state_rec *)ctx->ru_out.p;
    }
    *n = m;
    return HM_OK;
}

int hm_selftest_cell_to_parent(const uint64_t *cells, int64_t n, int32_t res, uint64_t *out) {
    if (n < 0 || res < 0 || res > 15 || (n > 0 && (!cells || !out))) return HM_E_INVALID;
    for (int64_t i = 0; i < n; i++) out[i] = h3_cell_to_parent(cells[i], res);
    return HM_OK;
}
