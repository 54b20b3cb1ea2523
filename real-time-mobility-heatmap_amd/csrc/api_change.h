// C ABI: the change between two live windows -- the pairs of their roll-up records joined on the cell, all of them or
// the k of a rising / falling / absolute order, as records or as the GeoJSON body (k_change.h; the roll-ups are
// rollup_on_device, the view k_view_tiles, the select top_run, the encoder gj_tiles).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

enum { CW_REST = 0, CW_VIEW, CW_WORDS };   // the change's device words: the unmatched base slots, the pairs in view

static int change_init(hm_ctx *ctx) {
    hm_ctx::Change &C = ctx->change;
    if (C.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, C.words, CW_WORDS * 8))) return rc;
    for (auto &e : C.ev) HIPCHK(ctx, hipEventCreate(&e));
    C.ready = true;
    return HM_OK;
}

// change(A, B, res) [cut to view] on the device: *out = the pairs (device), *n_out their number; ranked (k >= 0): the
// first min(k, n) of `order` in rank order instead.  The arguments but res and the stage are checked by the caller.
// Fills C.info.  Window B is rolled up first, into the change's own table and records; window A then goes through
// ru_tab / ru_out as any roll-up.
static int change_on_device(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view,
                            int32_t order, int64_t k, const char *who, const ChangeRec **out, int64_t *n_out) {
    hm_ctx::Change &C = ctx->change;
    hm_ctx::Top &T = ctx->top;
    *out = nullptr;
    *n_out = 0;
    for (int64_t &x : C.info) x = 0;
    int64_t mA = 0, mB = 0, slotsB = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, base_start_us, res, who, &mB, &slotsB, &C.tab, &C.recs)) ||
        (rc = rollup_on_device(ctx, window_start_us, res, who, &mA)))
        return rc;
    C.info[0] = mA;
    C.info[1] = mB;
    if (mA + mB == 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = change_init(ctx)) || (rc = ensure(ctx, C.out, (size_t)(mA + mB) * sizeof(ChangeRec)))) return rc;
    unsigned long long *words = (unsigned long long *)C.words.p;
    ChangeRec *pairs = (ChangeRec *)C.out.p;
    double us = 0;
    float ms = 0;
    // the join: A's records against B's table, then B's slots nobody matched
    HIPCHK(ctx, hipMemsetAsync(words, 0, CW_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipEventRecord(C.ev[0], ctx->stream));
    if (mA > 0)
        hipLaunchKernelGGL(k_change_match, dim3(read_grid(ctx->read_grid, mA, 256)), dim3(256), 0, ctx->stream, (const GrowRec *)ctx->ru_out.p, mA,
                           mB > 0 ? (GrowRec *)C.tab.p : nullptr, (unsigned long long)(mB > 0 ? slotsB - 1 : 0), base_start_us, pairs);
    if (mB > 0)
        hipLaunchKernelGGL(k_change_rest, dim3(read_grid(ctx->read_grid, slotsB, 256 * DUMP_PER)), dim3(256), 0, ctx->stream,
                           (const GrowRec *)C.tab.p, slotsB, window_start_us, base_start_us, pairs + mA, mB, words + CW_REST);
    HIPCHK(ctx, hipEventRecord(C.ev[1], ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    unsigned long long rest = 0;
    HIPCHK(ctx, hipMemcpyAsync(&rest, words + CW_REST, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if (hipEventElapsedTime(&ms, C.ev[0], C.ev[1]) == hipSuccess) us += 1e3 * ms;
    if ((int64_t)rest > mB || mB - (int64_t)rest > mA)
        return set_err(ctx, HM_E_STATE, "the change left %llu of %lld base cells unmatched against %lld current ones", rest, (long long)mB,
                       (long long)mA);
    int64_t n = mA + (int64_t)rest;
    C.info[2] = mB - (int64_t)rest;
    if (view) {
        if ((rc = ensure(ctx, C.vout, (size_t)n * sizeof(ChangeRec)))) return rc;
        const ViewPoles &poles = view_poles();
        unsigned long long kept = 0;
        HIPCHK(ctx, hipEventRecord(C.ev[2], ctx->stream));
        hipLaunchKernelGGL(k_view_tiles, dim3(read_grid(ctx->read_grid, n, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const ChangeRec *)pairs, n,
                           poles.north[res], poles.south[res], *view, (ChangeRec *)C.vout.p, words + CW_VIEW);
        HIPCHK(ctx, hipEventRecord(C.ev[3], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&kept, words + CW_VIEW, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if (hipEventElapsedTime(&ms, C.ev[2], C.ev[3]) == hipSuccess) us += 1e3 * ms;
        if ((int64_t)kept > n) return set_err(ctx, HM_E_STATE, "the view kept %llu of %lld pairs", kept, (long long)n);
        n = (int64_t)kept;
        pairs = (ChangeRec *)C.vout.p;
    }
    C.info[3] = n;
    if (k >= 0) {   // the first min(k, n) of the order, through the top's select on the change's key words
        const int64_t m = std::min(k, n);
        if (m > 0) {
            if ((rc = top_init(ctx)) || (rc = ensure(ctx, T.kc, (size_t)n * 8)) || (rc = ensure(ctx, T.cell, (size_t)n * 8)) ||
                (rc = top_select_buffers(ctx, m)) || (rc = ensure(ctx, C.ranked, (size_t)m * sizeof(ChangeRec))))
                return rc;
            unsigned long long *kc = (unsigned long long *)T.kc.p, *cell = (unsigned long long *)T.cell.p;
            const int max_grid = T.test_grid ? T.test_grid : 8 * std::max(ctx->n_cus, 1);
            const ChangeRec *src = pairs;
            int64_t passes[3] = {0, 0, 0}, tied = 0;
            rc = top_run(
                ctx, kc, cell, n, m, us, passes, &tied,
                [&] {
                    hipLaunchKernelGGL(k_change_keys, dim3(read_grid(ctx->read_grid, n, 256)), dim3(256), 0, ctx->stream, src, n, (int)order, kc, cell);
                    hipLaunchKernelGGL(k_near_vary, dim3(grid_for(n, 256, max_grid)), dim3(256), 0, ctx->stream, (const unsigned long long *)kc,
                                       (const unsigned long long *)cell, n, (unsigned long long *)T.words.p);
                },
                [&] {
                    hipLaunchKernelGGL(k_change_scatter, dim3(read_grid(ctx->read_grid, 8 * m, 256)), dim3(256), 0, ctx->stream, (const uint4 *)src, n,
                                       (const unsigned *)T.sidx.p, (const unsigned *)T.rank.p, (int)m, (uint4 *)C.ranked.p);
                });
            if (rc) return rc;
            pairs = (ChangeRec *)C.ranked.p;
        }
        n = m;
    }
    C.info[4] = n;
    C.info[5] = (int64_t)us;
    *out = n ? pairs : nullptr;
    *n_out = n;
    return HM_OK;
}

// the pairs handed out where they are, or copied to the change's pinned buffer
static int change_out(hm_ctx *ctx, const ChangeRec *d, int64_t n, int32_t out_memory, const hm_change_rec **recs) {
    hm_ctx::Change &C = ctx->change;
    *recs = (const hm_change_rec *)d;
    if (n == 0 || out_memory == HM_MEM_DEVICE) return HM_OK;
    int rc;
    if ((rc = host_pinned(ctx, &C.h_out, C.h_out_cap, (size_t)n * sizeof(ChangeRec)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(C.h_out, d, (size_t)n * sizeof(ChangeRec), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    *recs = (const hm_change_rec *)C.h_out;
    return HM_OK;
}

// the checks every change call shares, in hm_window_top's order: the arguments, the shard, the state
static int change_args(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view, bool ranked,
                       int32_t order, int64_t k, const char *who) {
    if (ranked && !top_k_ok(k)) return top_bad_k(ctx, who, k);
    if (ranked && !change_order_ok(order)) return set_err(ctx, HM_E_INVALID, "%s: order %d is none of HM_CHANGE_*", who, order);
    if (view && !view_valid(*view)) return top_bad_view(ctx, view);
    if (window_start_us == base_start_us)
        return set_err(ctx, HM_E_INVALID, "%s: the window and its base are the same window (%lld)", who, (long long)window_start_us);
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (ranked && ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank's ranking is not the global one (hm_window_change gives the rank's pairs)",
                       who, ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    return HM_OK;
}

int hm_window_change(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view, int32_t out_memory,
                     const hm_change_rec **recs, int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    int rc;
    if ((rc = change_args(ctx, window_start_us, base_start_us, res, view, false, 0, -1, "hm_window_change"))) return rc;
    *recs = nullptr;
    *n = 0;
    const ChangeRec *o = nullptr;
    int64_t m = 0;
    if ((rc = change_on_device(ctx, window_start_us, base_start_us, res, view, 0, -1, "hm_window_change", &o, &m)) ||
        (rc = change_out(ctx, o, m, out_memory, recs)))
        return rc;
    *n = m;
    return HM_OK;
}

int hm_window_change_top(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_view *view, int32_t order,
                         int64_t k, int32_t out_memory, const hm_change_rec **recs, int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    int rc;
    if ((rc = change_args(ctx, window_start_us, base_start_us, res, view, true, order, k, "hm_window_change_top"))) return rc;
    *recs = nullptr;
    *n = 0;
    const ChangeRec *o = nullptr;
    int64_t m = 0;
    if ((rc = change_on_device(ctx, window_start_us, base_start_us, res, view, order, k, "hm_window_change_top", &o, &m)) ||
        (rc = change_out(ctx, o, m, out_memory, recs)))
        return rc;
    *n = m;
    return HM_OK;
}

int hm_window_geojson_change(hm_ctx *ctx, int64_t window_start_us, int64_t base_start_us, int32_t res, const hm_geojson_cfg *cfg,
                             const hm_view *view, int32_t order, int64_t k, int32_t out_memory, const uint8_t **bytes,
                             const int64_t **offsets, int64_t *n, const hm_change_rec **recs) {
    if (!ctx || !cfg || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    GjTexts X;
    if (gj_texts(cfg, X)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    int rc;
    if ((rc = change_args(ctx, window_start_us, base_start_us, res, view, k >= 0, order, k, "hm_window_geojson_change"))) return rc;
    *n = 0;
    if (recs) *recs = nullptr;
    const ChangeRec *o = nullptr;
    int64_t m = 0;
    if ((rc = change_on_device(ctx, window_start_us, base_start_us, res, view, order, k < 0 ? -1 : k, "hm_window_geojson_change", &o, &m)))
        return rc;
    if (recs && (rc = change_out(ctx, o, m, HM_MEM_HOST, recs))) return rc;   // the pairs in feature order
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = gj_tiles(ctx, X, (const GrowRec *)o, m, out_memory, bytes, offsets, nullptr, true))) return rc;
    *n = m;
    return HM_OK;
}

// Host execution of the join with the kernels' HM_HD code (change_zero, change_key, the top's select and comparator)
int hm_selftest_window_change(const hm_state_rec *cur, int64_t n_cur, const hm_state_rec *base, int64_t n_base, int64_t window_start_us,
                              int64_t base_start_us, int32_t order, int64_t k, hm_change_rec *out, int64_t *n_out) {
    if (n_cur < 0 || n_base < 0 || n_cur + n_base > (int64_t(1) << 31) || (n_cur > 0 && !cur) || (n_base > 0 && !base) || !n_out ||
        window_start_us == base_start_us || (k >= 0 && (!top_k_ok(k) || !change_order_ok(order))))
        return HM_E_INVALID;
    *n_out = 0;
    const GrowRec *A = (const GrowRec *)cur, *B = (const GrowRec *)base;
    std::vector<int64_t> ib((size_t)n_base);   // B's records by cell
    for (int64_t j = 0; j < n_base; j++) ib[j] = j;
    std::sort(ib.begin(), ib.end(), [&](int64_t x, int64_t y) { return B[x].cell < B[y].cell; });
    std::vector<char> matched((size_t)n_base, 0);
    std::vector<ChangeRec> pairs;
    pairs.reserve((size_t)(n_cur + n_base));
    for (int64_t i = 0; i < n_cur; i++) {   // k_change_match
        ChangeRec p;
        memcpy(&p.cur, &A[i], sizeof(GrowRec));
        p.base = change_zero(A[i].cell, base_start_us);
        auto it = std::lower_bound(ib.begin(), ib.end(), A[i].cell, [&](int64_t x, uint64_t c) { return B[x].cell < c; });
        if (it != ib.end() && B[*it].cell == A[i].cell) {
            memcpy(&p.base, &B[*it], sizeof(GrowRec));
            matched[*it] = 1;
        }
        pairs.push_back(p);
    }
    for (int64_t j = 0; j < n_base; j++)   // k_change_rest
        if (!matched[j]) {
            ChangeRec p;
            p.cur = change_zero(B[j].cell, window_start_us);
            memcpy(&p.base, &B[j], sizeof(GrowRec));
            pairs.push_back(p);
        }
    const int64_t n = (int64_t)pairs.size();
    std::vector<unsigned> sel;
    if (k < 0) {
        sel.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) sel[i] = (unsigned)i;
        std::sort(sel.begin(), sel.end(), [&](unsigned x, unsigned y) { return pairs[x].cur.cell < pairs[y].cur.cell; });
    } else if (std::min(k, n) > 0) {
        std::vector<unsigned long long> kc((size_t)n), cell((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            kc[i] = change_key(pairs[i].cur, pairs[i].base, order);
            cell[i] = pairs[i].cur.cell;
        }
        if (int rc = top_select_host(kc.data(), cell.data(), n, std::min(k, n), sel)) return rc;
    }
    if (!sel.empty() && !out) return HM_E_INVALID;
    for (size_t j = 0; j < sel.size(); j++) memcpy(&out[j], &pairs[sel[j]], sizeof(ChangeRec));
    *n_out = (int64_t)sel.size();
    return HM_OK;
}

int hm_selftest_change_features(const hm_geojson_cfg *cfg, const hm_change_rec *pairs, int64_t n, uint8_t *bytes, int64_t cap,
                                int64_t *offsets) {
    GjTexts T;
    if (n < 0 || !bytes || !offsets || (n > 0 && !pairs) || cap < (int64_t)sizeof(GJ_EMPTY_BODY) - 1) return HM_E_INVALID;
    if (gj_texts(cfg, T)) return HM_E_INVALID;
    static const H3Tables H = make_tables();
    memcpy(bytes, GJ_EMPTY_BODY, GJ_PREFIX_LEN);
    int64_t o = GJ_PREFIX_LEN;
    for (int64_t i = 0; i < n; i++) {
        offsets[i] = o;
        const hm_state_rec &r = pairs[i].cur;
        const GjBase gb = {pairs[i].base.count, pairs[i].base.n_speed, pairs[i].base.sum_speed};
        double la[10], lo[10];
        const int nv = cellToBoundaryDeg(r.cell, H, la, lo);
        const int len = tile_feature(nullptr, T, r.cell, r.count, r.n_speed, r.sum_speed, nv, la, lo, 1, nullptr, &gb);
        if (o + len + 2 > cap) return HM_E_INVALID;
        tile_feature(bytes + o, T, r.cell, r.count, r.n_speed, r.sum_speed, nv, la, lo, 1, nullptr, &gb);
        o += len;
        bytes[o++] = i == n - 1 ? ']' : ',';
    }
    offsets[n] = o;
    if (n == 0) bytes[o++] = ']';
    bytes[o] = '}';
    return HM_OK;
}

int hm_change_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 6; i++) v[i] = ctx->change.info[i];
    return HM_OK;
}
