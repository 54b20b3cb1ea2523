// C ABI: the read side's response bodies as GeoJSON encoded on the GPU (reference app.py:45-88; geojson_docs.h, k_geojson.h).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

static const char GJ_EMPTY_BODY[] = HM_GJ_PREFIX "]}";   // 42 bytes

static int gj_texts(const hm_geojson_cfg *cfg, GjTexts &T) {
    if (!cfg || !gj_text_ok(cfg->window_start_text, cfg->start_len) || !gj_text_ok(cfg->window_end_text, cfg->end_len)) return HM_E_INVALID;
    memset(&T, 0, sizeof(T));
    if (cfg->start_len) memcpy(T.start, cfg->window_start_text, cfg->start_len);
    if (cfg->end_len) memcpy(T.end, cfg->window_end_text, cfg->end_len);
    T.start_len = cfg->start_len;
    T.end_len = cfg->end_len;
    return HM_OK;
}

static int gj_init(hm_ctx *ctx) {
    hm_ctx::GeoJson &G = ctx->gj;
    if (G.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, G.words, GJW_WORDS * 8))) return rc;
    for (auto &e : G.ev) HIPCHK(ctx, hipEventCreate(&e));
    for (auto &e : G.vev) HIPCHK(ctx, hipEventCreate(&e));
    G.ready = true;
    return HM_OK;
}

// the buffers of a scan over n features (n + 1 sizes: the prefix first)
static int gj_scan_buffers(hm_ctx *ctx, int64_t n) {
    hm_ctx::GeoJson &G = ctx->gj;
    const int64_t nb = (n + 1 + SC_PER - 1) / SC_PER;
    int rc;
    if ((rc = ensure(ctx, G.sizes, (size_t)(n + 1) * 4)) || (rc = ensure(ctx, G.off, (size_t)(n + 2) * 8)) ||
        (rc = ensure(ctx, G.btot, (size_t)nb * 4)) || (rc = ensure(ctx, G.boff, (size_t)nb * 8)))
        return rc;
    return HM_OK;
}
// G.sizes -> G.off: off[0] = 0, off[1 + i] = the caller's offsets[i], off[n + 1] = offsets[n]
static void gj_scan(hm_ctx *ctx, int64_t n) {
    hm_ctx::GeoJson &G = ctx->gj;
    const int64_t m = n + 1, nb = (m + SC_PER - 1) / SC_PER;
    unsigned long long *off = (unsigned long long *)G.off.p;
    hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(1024), 0, ctx->stream, (const unsigned *)G.sizes.p, m, off, (unsigned *)G.btot.p);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned *)G.btot.p, nb, (unsigned long long *)G.boff.p,
                       off + m);
    hipLaunchKernelGGL(k_scan_add, dim3(read_grid(ctx->read_grid, m, 256)), dim3(256), 0, ctx->stream, off, m, (const unsigned long long *)G.boff.p);
}
// the body without a feature
static int gj_empty(hm_ctx *ctx) {
    hm_ctx::GeoJson &G = ctx->gj;
    int rc;
    if ((rc = ensure(ctx, G.bytes, 64)) || (rc = ensure(ctx, G.off, 16))) return rc;
    static const unsigned long long off0[2] = {0, GJ_PREFIX_LEN};
    HIPCHK(ctx, hipMemcpyAsync(G.bytes.p, GJ_EMPTY_BODY, sizeof(GJ_EMPTY_BODY) - 1, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(G.off.p, off0, 16, hipMemcpyHostToDevice, ctx->stream));
    return HM_OK;
}
// the body in G.bytes / G.off handed out on the device or copied to the pinned host buffers
static int gj_out(hm_ctx *ctx, int64_t n, int64_t body_len, int32_t out_memory, const uint8_t **bytes, const int64_t **offsets) {
    hm_ctx::GeoJson &G = ctx->gj;
    G.last_bytes = body_len;
    if (out_memory == HM_MEM_DEVICE) {
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *bytes = (const uint8_t *)G.bytes.p;
        *offsets = (const int64_t *)G.off.p + 1;
    } else {
        int rc;
        if ((rc = host_pinned(ctx, &G.h_bytes, G.h_bytes_cap, (size_t)body_len)) ||
            (rc = host_pinned(ctx, &G.h_off, G.h_off_cap, (size_t)(n + 1) * 8)))
            return rc;
        HIPCHK(ctx, hipMemcpyAsync(G.h_bytes, G.bytes.p, (size_t)body_len, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(G.h_off, (const int64_t *)G.off.p + 1, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        *bytes = (const uint8_t *)G.h_bytes;
        *offsets = (const int64_t *)G.h_off;
    }
    float ms = 0;
    if (n > 0) {
        if (hipEventElapsedTime(&ms, G.ev[0], G.ev[1]) == hipSuccess) G.us[0] = 1e3 * ms;
        if (hipEventElapsedTime(&ms, G.ev[2], G.ev[3]) == hipSuccess) G.us[1] = 1e3 * ms;
        if (hipEventElapsedTime(&ms, G.ev[0], G.ev[3]) == hipSuccess) G.us[2] = 1e3 * ms;
    } else {
        G.us[0] = G.us[1] = G.us[2] = 0;
    }
    return HM_OK;
}

// the features of n device records: sizes -> scan -> write -> out.  dist_m (optional, device): a distance per record
// for the near bodies' distanceM.  pairs: recs are the change's n pairs (k_change.h) -- feature i is the cur half of pair i
// with its base half's three properties.  series / windows (optional, device): a span's series row per record
// (api_span.h) for the features' windows and counts; without one every byte is as it always was
static int gj_tiles(hm_ctx *ctx, const GjTexts &T, const GrowRec *recs, int64_t n, int32_t out_memory, const uint8_t **bytes,
                    const int64_t **offsets, const double *dist_m = nullptr, bool pairs = false, const int64_t *series = nullptr,
                    int windows = 0) {
    hm_ctx::GeoJson &G = ctx->gj;
    int rc;
    if ((rc = gj_init(ctx))) return rc;
    if (n == 0) {
        if ((rc = gj_empty(ctx))) return rc;
        return gj_out(ctx, 0, (int64_t)sizeof(GJ_EMPTY_BODY) - 1, out_memory, bytes, offsets);
    }
    if ((rc = gj_scan_buffers(ctx, n)) || (rc = ensure(ctx, G.verts, (size_t)n * 160)) || (rc = ensure(ctx, G.vn, (size_t)n * 4))) return rc;
    unsigned long long *words = (unsigned long long *)G.words.p;
    double *vlat = (double *)G.verts.p, *vlng = vlat + 10 * n;
    HIPCHK(ctx, hipMemsetAsync(words, 0, GJW_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipEventRecord(G.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_gj_tile_sizes, dim3(read_grid(ctx->read_grid, n, 256)), dim3(256), 0, ctx->stream, T, recs, n, vlat, vlng, (int *)G.vn.p,
                       (unsigned *)G.sizes.p, words, dist_m, pairs ? 2 : 1, pairs, series, windows);
    HIPCHK(ctx, hipEventRecord(G.ev[1], ctx->stream));
    gj_scan(ctx, n);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long total = 0, longest = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, (unsigned long long *)G.off.p + n + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&longest, words + GJW_MAX, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    const int tile_max = GJ_TILE_MAX + (dist_m ? GJ_DIST_MAX : 0) + (pairs ? GJ_BASE_MAX : 0) + (series ? GJ_SPAN_MAX : 0);
    if (longest == 0 || longest > (unsigned long long)tile_max)
        return set_err(ctx, HM_E_STATE, "a tile feature of %llu bytes (at most %d expected)", longest, tile_max);
    const int64_t body_len = (int64_t)total + 1;
    if ((rc = ensure(ctx, G.bytes, (size_t)body_len + 16))) return rc;
    // 64 x the longest feature + 64 B.  Without a series that is <= 64 x 992 + 64 B, below the 64-KB default; with one
    // tile_max is 1232, and a launch whose longest feature exceeds 1008 bytes (counts of 13 digits and more in most of 16
    // windows) is refused rather than given more than 64 KB (hm_span_geojson's contract, include/mobheat.h)
    const size_t lds = (size_t)GJ_THREADS * ((longest + 15) & ~15ull) + 64;
    if (lds > 65536)
        return set_err(ctx, HM_E_UNSUPPORTED, "a tile feature of %llu bytes: the encoder's workgroup holds features of at most 1008", longest);
    HIPCHK(ctx, hipEventRecord(G.ev[2], ctx->stream));
    hipLaunchKernelGGL(k_gj_tile_write, dim3(read_grid(ctx->read_grid, n, GJ_THREADS)), dim3(GJ_THREADS), lds, ctx->stream, T, recs, n,
                       (const double *)vlat, (const double *)vlng, (const int *)G.vn.p, (const unsigned long long *)G.off.p,
                       (uint8_t *)G.bytes.p, dist_m, pairs ? 2 : 1, pairs, series, windows);
    HIPCHK(ctx, hipEventRecord(G.ev[3], ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return gj_out(ctx, n, body_len, out_memory, bytes, offsets);
}

int hm_encode_tile_features(hm_ctx *ctx, const hm_geojson_cfg *cfg, int64_t n, int32_t memory, const hm_state_rec *recs,
                            int32_t out_memory, const uint8_t **bytes, const int64_t **offsets) {
    if (!ctx || !cfg || !bytes || !offsets || n < 0 || n > (int64_t(1) << 31) || (n > 0 && !recs) ||
        (memory != HM_MEM_HOST && memory != HM_MEM_DEVICE) || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    GjTexts T;
    if (gj_texts(cfg, T)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_encode_tile_features between stage calls");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const GrowRec *d = (const GrowRec *)recs;
    if (memory == HM_MEM_HOST && n > 0) {
        int rc;
        if ((rc = ensure(ctx, ctx->gj.in, (size_t)n * sizeof(GrowRec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->gj.in.p, recs, (size_t)n * sizeof(GrowRec), hipMemcpyHostToDevice, ctx->stream));
        d = (const GrowRec *)ctx->gj.in.p;
    }
    return gj_tiles(ctx, T, d, n, out_memory, bytes, offsets);
}

int hm_window_geojson(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, int32_t out_memory,
                      const uint8_t **bytes, const int64_t **offsets, int64_t *n, const hm_state_rec **recs) {
    if (!ctx || !cfg || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    GjTexts T;
    if (gj_texts(cfg, T)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    *n = 0;
    if (recs) *recs = nullptr;
    int64_t m = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, "hm_window_geojson", &m))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (recs && m > 0) {   // the records in feature order (the roll-up's pinned copy)
        if ((rc = host_pinned(ctx, &ctx->h_ru, ctx->h_ru_cap, (size_t)m * sizeof(GrowRec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_ru, ctx->ru_out.p, (size_t)m * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
        *recs = (const hm_state_rec *)ctx->h_ru;
    }
    if ((rc = gj_tiles(ctx, T, (const GrowRec *)ctx->ru_out.p, m, out_memory, bytes, offsets))) return rc;
    *n = m;
    return HM_OK;
}

int hm_selftest_tile_features_near(const hm_geojson_cfg *cfg, const hm_state_rec *recs, int64_t n, const double *dist_m,
                                   uint8_t *bytes, int64_t cap, int64_t *offsets) {
    GjTexts T;
    if (n < 0 || !bytes || !offsets || (n > 0 && !recs) || cap < (int64_t)sizeof(GJ_EMPTY_BODY) - 1) return HM_E_INVALID;
    if (gj_texts(cfg, T)) return HM_E_INVALID;
    static const H3Tables H = make_tables();
    memcpy(bytes, GJ_EMPTY_BODY, GJ_PREFIX_LEN);
    int64_t o = GJ_PREFIX_LEN;
    for (int64_t i = 0; i < n; i++) {
        offsets[i] = o;
        double la[10], lo[10];
        const int nv = cellToBoundaryDeg(recs[i].cell, H, la, lo);
        const double *d = dist_m ? dist_m + i : nullptr;
        const int len = tile_feature(nullptr, T, recs[i].cell, recs[i].count, recs[i].n_speed, recs[i].sum_speed, nv, la, lo, 1, d);
        if (o + len + 2 > cap) return HM_E_INVALID;
        tile_feature(bytes + o, T, recs[i].cell, recs[i].count, recs[i].n_speed, recs[i].sum_speed, nv, la, lo, 1, d);
        o += len;
        bytes[o++] = i == n - 1 ? ']' : ',';
    }
    offsets[n] = o;
    if (n == 0) bytes[o++] = ']';
    bytes[o] = '}';
    return HM_OK;
}

int hm_selftest_tile_features(const hm_geojson_cfg *cfg, const hm_state_rec *recs, int64_t n, uint8_t *bytes, int64_t cap,
                              int64_t *offsets) {
    return hm_selftest_tile_features_near(cfg, recs, n, nullptr, bytes, cap, offsets);
}

// ---- positions ----
static int gj_buckets_ok(hm_ctx *ctx, const hm_position_doc_cfg *c) {
    if (c->n_buckets < 0 || (c->n_buckets && (!c->bucket_ids || !c->bucket_offset_s))) return set_err(ctx, HM_E_INVALID, "bad time buckets");
    for (int64_t k = 1; k < c->n_buckets; k++)
        if (c->bucket_ids[k - 1] >= c->bucket_ids[k]) return set_err(ctx, HM_E_INVALID, "bucket ids not ascending");
    return HM_OK;
}

int hm_positions_buckets(hm_ctx *ctx, int64_t *bucket_ids, int64_t cap, int64_t *n) {
    if (!ctx || !n || cap < 0 || (cap > 0 && !bucket_ids)) return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "hm_positions_buckets on shard %d of %d", ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_positions_buckets between stage calls");
    hm_ctx::Positions &P = ctx->pos;
    hm_ctx::GeoJson &G = ctx->gj;
    *n = 0;
    if (P.keys == 0 || !P.tab) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = gj_init(ctx))) return rc;
    const unsigned long long scap = next_pow2((unsigned long long)std::max<int64_t>(2 * P.keys, 1024));
    if ((rc = ensure(ctx, G.bset, scap * 8)) || (rc = ensure(ctx, G.blist, (size_t)P.keys * 8))) return rc;
    unsigned long long *w = (unsigned long long *)G.words.p + GJW_BUCKETS;
    hipLaunchKernelGGL(k_fill_i64, dim3(read_grid(ctx->read_grid, (int64_t)scap, 256)), dim3(256), 0, ctx->stream, (long long *)G.bset.p, (int64_t)scap,
                       (long long)INT64_MIN);
    HIPCHK(ctx, hipMemsetAsync(w, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_gj_pos_buckets, dim3(read_grid(ctx->read_grid, (int64_t)P.cap, 256)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab,
                       (int64_t)P.cap, (long long *)G.bset.p, scap - 1, (long long *)G.blist.p, w);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long k = 0;
    HIPCHK(ctx, hipMemcpyAsync(&k, w, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if ((int64_t)k > P.keys) return set_err(ctx, HM_E_STATE, "%llu buckets of %lld keys", k, (long long)P.keys);
    std::vector<int64_t> ids(k);
    if (k) HIPCHK(ctx, hipMemcpy(ids.data(), G.blist.p, k * 8, hipMemcpyDeviceToHost));
    std::sort(ids.begin(), ids.end());
    *n = (int64_t)k;
    for (int64_t i = 0; i < (int64_t)k && i < cap; i++) bucket_ids[i] = ids[i];
    return HM_OK;
}

// device records to encode instead of the state's own emission, in feature order, with a distance each (the near body)
struct GjGiven {
    const hm_position_rec *recs;
    const double *dist_m;
    int64_t n;
};
// hm_positions_geojson (view nullptr: the whole state), hm_positions_geojson_view (api_view.h: the valid view's part) and
// hm_positions_geojson_near (api_near.h: `given`, the ranked records)
static int gj_positions(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                        const int64_t **offsets, int64_t *n, const hm_position_rec **recs, const hm_view *view, const char *who,
                        const GjGiven *given = nullptr) {
    if (!ctx || !buckets || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank holds only the latest rows it received", who,
                       ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    int rc;
    if ((rc = gj_buckets_ok(ctx, buckets))) return rc;
    hm_ctx::Positions &P = ctx->pos;
    hm_ctx::GeoJson &G = ctx->gj;
    *n = 0;
    if (recs) *recs = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = gj_init(ctx))) return rc;
    int64_t m = given ? given->n : P.tab ? P.keys : 0;
    const double *dist_m = given ? given->dist_m : nullptr;
    if (view) {
        G.candidates = m;
        G.view_us = 0;
    }
    if (m == 0) {
        if ((rc = gj_empty(ctx))) return rc;
        return gj_out(ctx, 0, (int64_t)sizeof(GJ_EMPTY_BODY) - 1, out_memory, bytes, offsets);
    }
    const int64_t nb = buckets->n_buckets;
    if ((rc = gj_scan_buffers(ctx, m)) || (!given && (rc = ensure(ctx, G.precs, (size_t)m * sizeof(hm_position_rec)))) ||
        (rc = ensure(ctx, G.params, (size_t)std::max<int64_t>(nb, 1) * 16)))
        return rc;
    unsigned long long *words = (unsigned long long *)G.words.p;
    HIPCHK(ctx, hipMemsetAsync(words, 0, GJW_WORDS * 8, ctx->stream));
    if (nb) {
        HIPCHK(ctx, hipMemcpyAsync(G.params.p, buckets->bucket_ids, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync((int64_t *)G.params.p + nb, buckets->bucket_offset_s, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    // the state's records in feature order (k_pos_emit's compaction, into a buffer of this call's own)
    if (given) {   // (nothing to emit: the caller's records)
    } else if (!view) {
        hipLaunchKernelGGL(k_pos_emit, dim3(read_grid(ctx->read_grid, (int64_t)P.cap, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab,
                           (int64_t)P.cap, (hm_position_rec *)G.precs.p, m, words + GJW_OUT);
    } else {   // the same compaction with the point test; the features run over what it kept
        unsigned long long kept = 0;
        HIPCHK(ctx, hipEventRecord(G.vev[0], ctx->stream));
        hipLaunchKernelGGL(k_pos_emit_view, dim3(read_grid(ctx->read_grid, (int64_t)P.cap, 256 * DUMP_PER)), dim3(256), 0, ctx->stream,
                           (const PosSlot *)P.tab, (int64_t)P.cap, *view, (hm_position_rec *)G.precs.p, m, words + GJW_OUT);
        HIPCHK(ctx, hipEventRecord(G.vev[1], ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&kept, words + GJW_OUT, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        float vms = 0;
        if (hipEventElapsedTime(&vms, G.vev[0], G.vev[1]) == hipSuccess) G.view_us = 1e3 * vms;
        if ((int64_t)kept > m) return set_err(ctx, HM_E_STATE, "positions state holds %llu keys, at most %lld expected", kept, (long long)m);
        m = (int64_t)kept;
        if (m == 0) {
            if ((rc = gj_empty(ctx))) return rc;
            return gj_out(ctx, 0, (int64_t)sizeof(GJ_EMPTY_BODY) - 1, out_memory, bytes, offsets);
        }
    }
    PosFeatParams F;
    F.p_off = P.prov.code_off;
    F.p_len = P.prov.code_len;
    F.p_arena = P.prov.arena;
    F.v_off = P.veh.code_off;
    F.v_len = P.veh.code_len;
    F.v_arena = P.veh.arena;
    F.n_p = P.prov.n_codes;
    F.n_v = P.veh.n_codes;
    F.n_buckets = nb;
    F.bucket_id = (const int64_t *)G.params.p;
    F.bucket_off = F.bucket_id + nb;
    const hm_position_rec *d = given ? given->recs : (const hm_position_rec *)G.precs.p;
    HIPCHK(ctx, hipEventRecord(G.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_gj_pos_sizes, dim3(read_grid(ctx->read_grid, m, 256)), dim3(256), 0, ctx->stream, F, d, m, (unsigned *)G.sizes.p, words, dist_m);
    HIPCHK(ctx, hipEventRecord(G.ev[1], ctx->stream));
    gj_scan(ctx, m);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long total = 0, hw[GJW_WORDS] = {};
    HIPCHK(ctx, hipMemcpyAsync(&total, (unsigned long long *)G.off.p + m + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hw, words, GJW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));   // (the bucket table is pageable host memory)
    if (!given && (int64_t)hw[GJW_OUT] != m) return set_err(ctx, HM_E_STATE, "positions state holds %llu keys, %lld expected", hw[GJW_OUT], (long long)m);
    if (hw[GJW_BAD])
        return set_err(ctx, HM_E_INVALID, "%llu positions outside the time buckets or years 1-9999, or with a string that is not UTF-8",
                       hw[GJW_BAD]);
    const int64_t body_len = (int64_t)total + 1;
    if ((rc = ensure(ctx, G.bytes, (size_t)body_len + 16))) return rc;
    HIPCHK(ctx, hipEventRecord(G.ev[2], ctx->stream));
    hipLaunchKernelGGL(k_gj_pos_write, dim3(read_grid(ctx->read_grid, m, 256)), dim3(256), 0, ctx->stream, F, d, m, (const unsigned long long *)G.off.p,
                       (uint8_t *)G.bytes.p, dist_m);
    HIPCHK(ctx, hipEventRecord(G.ev[3], ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    if (recs) {
        if ((rc = host_pinned(ctx, &G.h_recs, G.h_recs_cap, (size_t)m * sizeof(hm_position_rec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(G.h_recs, d, (size_t)m * sizeof(hm_position_rec), hipMemcpyDeviceToHost, ctx->stream));
        *recs = (const hm_position_rec *)G.h_recs;
    }
    if ((rc = gj_out(ctx, m, body_len, out_memory, bytes, offsets))) return rc;
    *n = m;
    return HM_OK;
}

int hm_positions_geojson(hm_ctx *ctx, const hm_position_doc_cfg *buckets, int32_t out_memory, const uint8_t **bytes,
                         const int64_t **offsets, int64_t *n, const hm_position_rec **recs) {
    return gj_positions(ctx, buckets, out_memory, bytes, offsets, n, recs, nullptr, "hm_positions_geojson");
}

int hm_selftest_position_features_near(const hm_position_doc_cfg *cfg, const hm_position_rec *recs, int64_t n, const double *dist_m,
                                       uint8_t *bytes, int64_t cap, int64_t *offsets) {
    if (!cfg || n < 0 || !bytes || !offsets || (n > 0 && !recs) || cap < (int64_t)sizeof(GJ_EMPTY_BODY) - 1) return HM_E_INVALID;
    if (cfg->n_providers < 0 || cfg->n_vehicles < 0 || cfg->n_buckets < 0 || (cfg->n_providers && (!cfg->provider_offsets || !cfg->provider_bytes)) ||
        (cfg->n_vehicles && (!cfg->vehicle_offsets || !cfg->vehicle_bytes)) || (cfg->n_buckets && (!cfg->bucket_ids || !cfg->bucket_offset_s)))
        return HM_E_INVALID;
    memcpy(bytes, GJ_EMPTY_BODY, GJ_PREFIX_LEN);
    int64_t o = GJ_PREFIX_LEN;
    for (int64_t i = 0; i < n; i++) {
        offsets[i] = o;
        const hm_position_rec &r = recs[i];
        int64_t off_s;
        if ((int64_t)r.provider >= cfg->n_providers || (int64_t)r.vehicle >= cfg->n_vehicles ||
            !gj_bucket_offset(cfg->bucket_ids, cfg->bucket_offset_s, cfg->n_buckets, r.ts_us, off_s))
            return HM_E_INVALID;
        const uint8_t *ps = (const uint8_t *)cfg->provider_bytes + cfg->provider_offsets[r.provider];
        const uint8_t *vs = (const uint8_t *)cfg->vehicle_bytes + cfg->vehicle_offsets[r.vehicle];
        const int pl = (int)(cfg->provider_offsets[r.provider + 1] - cfg->provider_offsets[r.provider]);
        const int vl = (int)(cfg->vehicle_offsets[r.vehicle + 1] - cfg->vehicle_offsets[r.vehicle]);
        const double *d = dist_m ? dist_m + i : nullptr;
        const int len = position_feature(nullptr, ps, pl, vs, vl, r.ts_us, off_s, r.lat, r.lon, d);
        if (len < 0 || o + len + 2 > cap) return HM_E_INVALID;
        position_feature(bytes + o, ps, pl, vs, vl, r.ts_us, off_s, r.lat, r.lon, d);
        o += len;
        bytes[o++] = i == n - 1 ? ']' : ',';
    }
    offsets[n] = o;
    if (n == 0) bytes[o++] = ']';
    bytes[o] = '}';
    return HM_OK;
}

int hm_selftest_position_features(const hm_position_doc_cfg *cfg, const hm_position_rec *recs, int64_t n, uint8_t *bytes,
                                  int64_t cap, int64_t *offsets) {
    return hm_selftest_position_features_near(cfg, recs, n, nullptr, bytes, cap, offsets);
}

int hm_geojson_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    const hm_ctx::GeoJson &G = ctx->gj;
    const int64_t w[6] = {(int64_t)G.us[0], (int64_t)G.us[1], (int64_t)G.us[2], G.last_bytes, G.candidates, (int64_t)G.view_us};
    for (int i = 0; i < n && i < 6; i++) v[i] = w[i];
    return HM_OK;
}
