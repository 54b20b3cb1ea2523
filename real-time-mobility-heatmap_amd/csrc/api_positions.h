// C ABI: the latest position per (provider, vehicleId) across batches -- the positions_latest collection the reference
// folds inside MongoDB (heatmap_stream.py:217-228) and serves from it (app.py:71-88), kept on the device (k_positions.h).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

constexpr int POS_USED_P = PW_WORDS, POS_USED_V = PW_WORDS + 2, POS_WORDS = PW_WORDS + 4;

// a device allocation of the positions state (counted like every other of the context)
static int pos_alloc(hm_ctx *ctx, void *pp, size_t bytes, const char *what) {
    void **p = (void **)pp;   // (the address of a typed device pointer)
    if (dev_malloc(ctx, p, std::max<size_t>(bytes, 256), what) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return set_err(ctx, HM_E_NOMEM, "hipMalloc(%zu) failed (%s)", bytes, what);
    }
    return HM_OK;
}
// (the stream has drained every kernel that reads p)
static int pos_release(hm_ctx *ctx, void *p) {
    if (!p) return HM_OK;
    { AllocTimer at_(ctx); HIPCHK(ctx, hipFree(p)); }
    ctx->n_frees++;
    return HM_OK;
}

// the control block and the timing events, at the first positions call that needs the device
static int positions_init(hm_ctx *ctx) {
    hm_ctx::Positions &P = ctx->pos;
    if (P.ready) return HM_OK;
    int rc;
    if ((rc = pos_alloc(ctx, &P.words, POS_WORDS * 8, "positions words"))) return rc;
    { AllocTimer at_(ctx); ctx->n_allocs++; HIPCHK(ctx, hipHostMalloc((void **)&P.h_words, POS_WORDS * 8, hipHostMallocDefault)); }
    HIPCHK(ctx, hipMemsetAsync(P.words, 0, POS_WORDS * 8, ctx->stream));
    for (auto &e : P.ev) HIPCHK(ctx, hipEventCreate(&e));
    P.ready = true;
    return HM_OK;
}
static bool positions_empty(const hm_ctx *ctx) {
    const hm_ctx::Positions &P = ctx->pos;
    return P.keys == 0 && P.prov.n_codes == 0 && P.veh.n_codes == 0;
}

// the dictionary's table, arena and code lists made large enough for need_codes strings of need_bytes bytes (load <= 1/2);
// a larger table is filled by k_pos_str_rehash, a larger arena by a device-to-device copy
static int pos_dict_grow(hm_ctx *ctx, hm_ctx::PosDict &d, int64_t need_codes, int64_t need_bytes) {
    hm_ctx::Positions &P = ctx->pos;
    int rc;
    if (need_codes > (int64_t)POS_MAX_CODES) return set_err(ctx, HM_E_OVERFLOW, "%lld strings in a positions dictionary", (long long)need_codes);
    const unsigned long long want = next_pow2((unsigned long long)std::max<int64_t>(2 * need_codes, 1024));
    std::vector<void *> old;
    if (!d.tab || d.cap < want) {
        PosStr *t = nullptr;
        if ((rc = pos_alloc(ctx, &t, want * sizeof(PosStr), "positions dictionary"))) return rc;
        HIPCHK(ctx, hipMemsetAsync(t, 0xff, want * sizeof(PosStr), ctx->stream));
        if (d.tab) {
            hipLaunchKernelGGL(k_pos_str_rehash, dim3(grid_for((int64_t)d.cap, 256)), dim3(256), 0, ctx->stream,
                               (const PosStr *)d.tab, (int64_t)d.cap, t, want - 1, P.words);
            HIPCHK(ctx, hipGetLastError());
            old.push_back(d.tab);
            P.regrows++;
        }
        d.tab = t;
        d.cap = want;
    }
    if (!d.arena || d.arena_cap < (size_t)need_bytes) {
        const size_t cap = std::max<size_t>({(size_t)need_bytes, d.arena_cap + d.arena_cap / 2, 4096});
        uint8_t *a = nullptr;
        if ((rc = pos_alloc(ctx, &a, cap, "positions arena"))) return rc;
        if (d.arena) {
            if (d.arena_used)
                HIPCHK(ctx, hipMemcpyAsync(a, d.arena, (size_t)d.arena_used, hipMemcpyDeviceToDevice, ctx->stream));
            old.push_back(d.arena);
            P.regrows++;
            d.arena_regrows++;
        }
        d.arena = a;
        d.arena_cap = cap;
    }
    if (!d.code_off || d.codes_cap < (size_t)need_codes) {
        const size_t cap = std::max<size_t>({(size_t)need_codes, d.codes_cap + d.codes_cap / 2, 1024});
        unsigned long long *co = nullptr;
        unsigned *cl = nullptr;
        if ((rc = pos_alloc(ctx, &co, cap * 8, "positions code spans")) || (rc = pos_alloc(ctx, &cl, cap * 4, "positions code lengths")))
            return rc;
        if (d.code_off) {
            if (d.n_codes) {
                HIPCHK(ctx, hipMemcpyAsync(co, d.code_off, (size_t)d.n_codes * 8, hipMemcpyDeviceToDevice, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(cl, d.code_len, (size_t)d.n_codes * 4, hipMemcpyDeviceToDevice, ctx->stream));
            }
            old.push_back(d.code_off);
            old.push_back(d.code_len);
            P.regrows++;
        }
        d.code_off = co;
        d.code_len = cl;
        d.codes_cap = cap;
    }
    if (!old.empty()) {
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        for (void *p : old)
            if ((rc = pos_release(ctx, p))) return rc;
    }
    return HM_OK;
}
// the pair table made large enough for need_keys keys (load <= 1/2), the old one's keys moved by k_pos_pair_put
static int pos_pairs_grow(hm_ctx *ctx, int64_t need_keys) {
    hm_ctx::Positions &P = ctx->pos;
    if (need_keys > (int64_t(1) << 30)) return set_err(ctx, HM_E_OVERFLOW, "%lld positions keys", (long long)need_keys);
    const unsigned long long want = next_pow2((unsigned long long)std::max<int64_t>(2 * need_keys, 1024));
    if (P.tab && P.cap >= want) return HM_OK;
    PosSlot *t = nullptr;
    int rc;
    if ((rc = pos_alloc(ctx, &t, want * (sizeof(PosSlot) + 4), "positions table"))) return rc;
    HIPCHK(ctx, hipMemsetAsync(t, 0xff, want * (sizeof(PosSlot) + 4), ctx->stream));   // (keys POS_EMPTY, candidates POS_NONE)
    PosSlot *old = P.tab;
    if (old) {
        hipLaunchKernelGGL(k_pos_pair_put, dim3(grid_for((int64_t)P.cap, 256)), dim3(256), 0, ctx->stream, (const PosSlot *)old,
                           (int64_t)P.cap, t, want - 1, P.words);
        HIPCHK(ctx, hipGetLastError());
        P.regrows++;
        P.pair_regrows++;
    }
    P.tab = t;
    P.cap = want;
    if (old) {
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if ((rc = pos_release(ctx, old))) return rc;
    }
    return HM_OK;
}
static unsigned *pos_cand(const hm_ctx::Positions &P) { return (unsigned *)(P.tab + P.cap); }
// the end of a call that counted into the control block (copied to h_words): HM_E_OVERFLOW if a probe bound ran out
static int pos_overflow_status(hm_ctx *ctx) {
    const unsigned long long lost = ctx->pos.h_words[PW_OVERFLOW];
    if (!lost) return HM_OK;
    return set_err(ctx, HM_E_OVERFLOW, "positions tables: %llu probes past the bound of %llu (colliding string hashes)", lost,
                   POS_PROBES);
}

// host-side shape of a caller's dictionaries (the offsets themselves are checked where they are read: on the device
// for a batch's, on the host for an import's)
static int pos_dicts_shape(hm_ctx *ctx, const hm_position_doc_cfg *c, int64_t &p_total, int64_t &v_total) {
    if (c->n_providers < 0 || c->n_vehicles < 0 || c->n_providers > (int64_t)POS_MAX_CODES || c->n_vehicles > (int64_t)POS_MAX_CODES ||
        (c->n_providers && (!c->provider_offsets || !c->provider_bytes)) || (c->n_vehicles && (!c->vehicle_offsets || !c->vehicle_bytes)))
        return set_err(ctx, HM_E_INVALID, "bad position dictionaries");
    p_total = c->n_providers ? c->provider_offsets[c->n_providers] : 0;
    v_total = c->n_vehicles ? c->vehicle_offsets[c->n_vehicles] : 0;
    if (p_total < 0 || v_total < 0 || p_total > (int64_t(1) << 40) || v_total > (int64_t(1) << 40))
        return set_err(ctx, HM_E_INVALID, "bad position dictionary offsets");
    return HM_OK;
}

int hm_positions_update(hm_ctx *ctx, const hm_position_doc_cfg *dicts) {
    if (!ctx || !dicts) return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "hm_positions_update on shard %d of %d: a rank holds only the latest rows it received",
                       ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_positions_update between stage calls");
    if (ctx->last_n_latest < 0) return set_err(ctx, HM_E_STATE, "no hm_process_batch latest rows to fold");
    hm_ctx::Positions &P = ctx->pos;
    const int64_t n = ctx->last_n_latest, np_ = dicts->n_providers, nv = dicts->n_vehicles;
    int64_t p_total = 0, v_total = 0;
    int rc;
    if ((rc = pos_dicts_shape(ctx, dicts, p_total, v_total))) return rc;
    if (n == 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = positions_init(ctx))) return rc;
    // one device block: the two offset lists (8-B aligned), then the bytes
    const size_t o_p = 0, o_v = o_p + (size_t)(np_ + 1) * 8, o_ps = o_v + (size_t)(nv + 1) * 8, o_vs = o_ps + (size_t)p_total;
    if ((rc = ensure(ctx, P.params, o_vs + (size_t)v_total + 8)) || (rc = ensure(ctx, P.p_code, std::max<int64_t>(np_, 1) * 4)) ||
        (rc = ensure(ctx, P.v_code, std::max<int64_t>(nv, 1) * 4)) || (rc = ensure(ctx, P.slot_of, n * 4)))
        return rc;
    HIPCHK(ctx, hipEventRecord(P.ev[0], ctx->stream));
    uint8_t *d = (uint8_t *)P.params.p;
    HIPCHK(ctx, hipMemsetAsync(d, 0, o_ps, ctx->stream));   // (an empty dictionary's single offset)
    if (np_) HIPCHK(ctx, hipMemcpyAsync(d + o_p, dicts->provider_offsets, (size_t)(np_ + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nv) HIPCHK(ctx, hipMemcpyAsync(d + o_v, dicts->vehicle_offsets, (size_t)(nv + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (p_total) HIPCHK(ctx, hipMemcpyAsync(d + o_ps, dicts->provider_bytes, (size_t)p_total, hipMemcpyHostToDevice, ctx->stream));
    if (v_total) HIPCHK(ctx, hipMemcpyAsync(d + o_vs, dicts->vehicle_bytes, (size_t)v_total, hipMemcpyHostToDevice, ctx->stream));
    const int64_t *p_off = (const int64_t *)(d + o_p), *v_off = (const int64_t *)(d + o_v);
    const uint8_t *p_bytes = d + o_ps, *v_bytes = d + o_vs;
    const int64_t *rows = (const int64_t *)ctx->rows.p;
    HIPCHK(ctx, hipEventRecord(P.ev[1], ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(P.words, 0, PW_WORDS * 8, ctx->stream));
    // 1. the rows' codes checked, the batch's dictionary entries checked and looked up (read only: S is untouched so far)
    hipLaunchKernelGGL(k_pos_check, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, np_, nv, rows, n, ctx->last_vk, P.words);
    hipLaunchKernelGGL(k_pos_str_find, dim3(grid_for(std::max<int64_t>(np_, 1), 256)), dim3(256), 0, ctx->stream, p_off, p_bytes, np_,
                       p_total, (const PosStr *)P.prov.tab, P.prov.cap - 1, (const uint8_t *)P.prov.arena, P.hash_bits,
                       (unsigned *)P.p_code.p, P.words, (int)PW_NEW_P);
    hipLaunchKernelGGL(k_pos_str_find, dim3(grid_for(std::max<int64_t>(nv, 1), 256)), dim3(256), 0, ctx->stream, v_off, v_bytes, nv,
                       v_total, (const PosStr *)P.veh.tab, P.veh.cap - 1, (const uint8_t *)P.veh.arena, P.hash_bits,
                       (unsigned *)P.v_code.p, P.words, (int)PW_NEW_V);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.words, PW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if (P.h_words[PW_BAD])
        return set_err(ctx, HM_E_INVALID, "%llu latest rows or dictionary offsets outside the provider/vehicle dictionaries", P.h_words[PW_BAD]);
    const int64_t new_p = (int64_t)P.h_words[PW_NEW_P], new_v = (int64_t)P.h_words[PW_NEW_V];
    // 2. capacity before anything is written: exactly the strings not found; for the pairs the worst case (every row a
    // new key) where the table already holds it, else the rows whose key k_pos_pair_count does not find -- a batch over
    // known vehicles then leaves the table as it is
    int64_t new_pairs = n;
    if (!P.tab || (unsigned long long)(2 * (P.keys + n)) > P.cap) {
        HIPCHK(ctx, hipMemsetAsync(P.words + PW_NEW_PAIRS, 0, 8, ctx->stream));
        hipLaunchKernelGGL(k_pos_pair_count, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, rows, n, ctx->last_vk, (uint64_t)nv,
                           (const unsigned *)P.p_code.p, (const unsigned *)P.v_code.p, (const PosSlot *)P.tab, P.cap - 1, P.words);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(P.h_words + PW_NEW_PAIRS, P.words + PW_NEW_PAIRS, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(P.words + PW_NEW_PAIRS, 0, 8, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        new_pairs = (int64_t)P.h_words[PW_NEW_PAIRS];
    }
    if ((rc = pos_dict_grow(ctx, P.prov, P.prov.n_codes + new_p, P.prov.arena_used + (int64_t)P.h_words[PW_BYTES_P])) ||
        (rc = pos_dict_grow(ctx, P.veh, P.veh.n_codes + new_v, P.veh.arena_used + (int64_t)P.h_words[PW_BYTES_V])) ||
        (rc = pos_pairs_grow(ctx, P.keys + new_pairs)))
        return rc;
    // 3. the new strings, then the two passes over the latest rows
    if (new_p)
        hipLaunchKernelGGL(k_pos_str_insert, dim3(grid_for(np_, 256)), dim3(256), 0, ctx->stream, p_off, p_bytes, np_, P.prov.tab,
                           P.prov.cap - 1, P.prov.arena, P.hash_bits, (unsigned *)P.p_code.p, P.words + POS_USED_P, P.prov.code_off,
                           P.prov.code_len, P.words);
    if (new_v)
        hipLaunchKernelGGL(k_pos_str_insert, dim3(grid_for(nv, 256)), dim3(256), 0, ctx->stream, v_off, v_bytes, nv, P.veh.tab,
                           P.veh.cap - 1, P.veh.arena, P.hash_bits, (unsigned *)P.v_code.p, P.words + POS_USED_V, P.veh.code_off,
                           P.veh.code_len, P.words);
    hipLaunchKernelGGL(k_pos_pair_pass1, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, rows, n, ctx->last_vk, ctx->last_ts,
                       (uint64_t)nv, (const unsigned *)P.p_code.p, (const unsigned *)P.v_code.p, P.tab, P.cap - 1, pos_cand(P),
                       (unsigned *)P.slot_of.p, P.words);
    hipLaunchKernelGGL(k_pos_pair_pass2, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, rows, n, ctx->last_ts, ctx->last_lat,
                       ctx->last_lon, P.tab, pos_cand(P), (const unsigned *)P.slot_of.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.words, POS_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(P.ev[2], ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    float ms = 0;
    if (hipEventElapsedTime(&ms, P.ev[0], P.ev[2]) == hipSuccess) P.us[0] = 1e3 * ms;
    if (hipEventElapsedTime(&ms, P.ev[1], P.ev[2]) == hipSuccess) P.us[1] = 1e3 * ms;
    P.keys += (int64_t)P.h_words[PW_NEW_PAIRS];
    P.prov.arena_used = (int64_t)P.h_words[POS_USED_P];
    P.prov.n_codes = (int64_t)P.h_words[POS_USED_P + 1];
    P.veh.arena_used = (int64_t)P.h_words[POS_USED_V];
    P.veh.n_codes = (int64_t)P.h_words[POS_USED_V + 1];
    return pos_overflow_status(ctx);
}

// exclusive scan of a dictionary's code lengths into Arrow offsets (n + 1 entries; the total is its arena's fill)
static int pos_export_dict(hm_ctx *ctx, const hm_ctx::PosDict &d, int which, int32_t out_memory, const int64_t **offs,
                           const char **bytes) {
    hm_ctx::Positions &P = ctx->pos;
    const int64_t m = d.n_codes, total = d.arena_used;
    int rc;
    if ((rc = ensure(ctx, P.x_off[which], (size_t)(m + 1) * 8)) || (rc = ensure(ctx, P.x_bytes[which], (size_t)std::max<int64_t>(total, 1))))
        return rc;
    unsigned long long *xo = (unsigned long long *)P.x_off[which].p;
    if (m > 0) {
        const int64_t nb = (m + SC_PER - 1) / SC_PER;
        if ((rc = ensure(ctx, P.x_btot, nb * 4)) || (rc = ensure(ctx, P.x_boff, nb * 8))) return rc;
        hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(1024), 0, ctx->stream, (const unsigned *)d.code_len, m, xo, (unsigned *)P.x_btot.p);
        hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned *)P.x_btot.p, nb,
                           (unsigned long long *)P.x_boff.p, xo + m);
        hipLaunchKernelGGL(k_scan_add, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, xo, m, (const unsigned long long *)P.x_boff.p);
        hipLaunchKernelGGL(k_pos_str_gather, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const unsigned long long *)d.code_off,
                           (const unsigned *)d.code_len, m, (const uint8_t *)d.arena, (const unsigned long long *)xo,
                           (uint8_t *)P.x_bytes[which].p);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemsetAsync(xo, 0, 8, ctx->stream));
    }
    if (out_memory == HM_MEM_DEVICE) {
        *offs = (const int64_t *)xo;
        *bytes = (const char *)P.x_bytes[which].p;
        return HM_OK;
    }
    if ((rc = host_pinned(ctx, &P.h_off[which], P.h_off_cap[which], (size_t)(m + 1) * 8)) ||
        (rc = host_pinned(ctx, &P.h_bytes[which], P.h_bytes_cap[which], (size_t)std::max<int64_t>(total, 1))))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(P.h_off[which], xo, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (total) HIPCHK(ctx, hipMemcpyAsync(P.h_bytes[which], P.x_bytes[which].p, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    *offs = (const int64_t *)P.h_off[which];
    *bytes = (const char *)P.h_bytes[which];
    return HM_OK;
}

int hm_positions_export(hm_ctx *ctx, int32_t out_memory, const hm_position_rec **recs, int64_t *n, hm_position_doc_cfg *dicts) {
    if (!ctx || !recs || !n || !dicts || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_positions_export between stage calls");
    hm_ctx::Positions &P = ctx->pos;
    *recs = nullptr;
    *n = 0;
    memset(dicts, 0, sizeof(*dicts));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = positions_init(ctx))) return rc;
    const int64_t m = P.keys;
    if ((rc = ensure(ctx, P.x_recs, (size_t)std::max<int64_t>(m, 1) * sizeof(hm_position_rec)))) return rc;
    HIPCHK(ctx, hipMemsetAsync(P.words + PW_OUT, 0, 8, ctx->stream));
    if (P.tab) {
        hipLaunchKernelGGL(k_pos_emit, dim3(read_grid(ctx->read_grid, (int64_t)P.cap, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, (const PosSlot *)P.tab,
                           (int64_t)P.cap, (hm_position_rec *)P.x_recs.p, m, P.words + PW_OUT);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(P.h_words + PW_OUT, P.words + PW_OUT, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = pos_export_dict(ctx, P.prov, 0, out_memory, &dicts->provider_offsets, &dicts->provider_bytes)) ||
        (rc = pos_export_dict(ctx, P.veh, 1, out_memory, &dicts->vehicle_offsets, &dicts->vehicle_bytes)))
        return rc;
    dicts->n_providers = P.prov.n_codes;
    dicts->n_vehicles = P.veh.n_codes;
    if (out_memory == HM_MEM_HOST) {
        if ((rc = host_pinned(ctx, &P.h_recs, P.h_recs_cap, (size_t)std::max<int64_t>(m, 1) * sizeof(hm_position_rec)))) return rc;
        if (m > 0)
            HIPCHK(ctx, hipMemcpyAsync(P.h_recs, P.x_recs.p, (size_t)m * sizeof(hm_position_rec), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    if ((int64_t)P.h_words[PW_OUT] != m)
        return set_err(ctx, HM_E_STATE, "positions export found %llu keys, %lld expected", P.h_words[PW_OUT], (long long)m);
    *recs = out_memory == HM_MEM_HOST ? (const hm_position_rec *)P.h_recs : (const hm_position_rec *)P.x_recs.p;
    *n = m;
    return HM_OK;
}

// an imported dictionary on the host: offsets ascending from 0 within the bytes, strings of at most 2^20 bytes, distinct
static bool pos_import_dict_ok(int64_t m, const int64_t *off, const char *bytes) {
    if (m == 0) return true;
    if (off[0] != 0) return false;
    std::unordered_set<std::string_view> seen;
    seen.reserve((size_t)m * 2);
    for (int64_t k = 0; k < m; k++) {
        if (off[k] > off[k + 1] || off[k + 1] - off[k] > (1 << 20)) return false;
        if (!seen.insert(std::string_view(bytes + off[k], (size_t)(off[k + 1] - off[k]))).second) return false;
    }
    return true;
}
static int pos_import_dict(hm_ctx *ctx, hm_ctx::PosDict &d, int64_t m, const int64_t *off, const char *bytes, int64_t total,
                           int64_t *dev_off, int used_word) {
    hm_ctx::Positions &P = ctx->pos;
    if (m == 0) return HM_OK;
    HIPCHK(ctx, hipMemcpyAsync(dev_off, off, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (total) HIPCHK(ctx, hipMemcpyAsync(d.arena, bytes, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pos_str_import, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const int64_t *)dev_off, m, d.tab, d.cap - 1,
                       (const uint8_t *)d.arena, P.hash_bits, d.code_off, d.code_len, P.words);
    HIPCHK(ctx, hipGetLastError());
    P.h_words[used_word] = (unsigned long long)total;
    P.h_words[used_word + 1] = (unsigned long long)m;
    HIPCHK(ctx, hipMemcpyAsync(P.words + used_word, P.h_words + used_word, 16, hipMemcpyHostToDevice, ctx->stream));
    return HM_OK;
}

int hm_positions_import(hm_ctx *ctx, const hm_position_rec *recs, int64_t n, const hm_position_doc_cfg *dicts) {
    if (!ctx || !dicts || n < 0 || (n > 0 && !recs)) return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_positions_import between stage calls");
    if (!positions_empty(ctx)) return set_err(ctx, HM_E_STATE, "hm_positions_import into a positions state that holds keys");
    hm_ctx::Positions &P = ctx->pos;
    const int64_t np_ = dicts->n_providers, nv = dicts->n_vehicles;
    int64_t p_total = 0, v_total = 0;
    int rc;
    if ((rc = pos_dicts_shape(ctx, dicts, p_total, v_total))) return rc;
    if (!pos_import_dict_ok(np_, dicts->provider_offsets, dicts->provider_bytes) ||
        !pos_import_dict_ok(nv, dicts->vehicle_offsets, dicts->vehicle_bytes))
        return set_err(ctx, HM_E_INVALID, "imported dictionaries: offsets not ascending from 0, or a string twice");
    std::vector<PosSlot> slots((size_t)n);
    std::vector<unsigned long long> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if ((int64_t)recs[i].provider >= np_ || (int64_t)recs[i].vehicle >= nv)
            return set_err(ctx, HM_E_INVALID, "imported record %lld: codes outside the dictionaries", (long long)i);
        keys[i] = ((unsigned long long)recs[i].provider << 32) | recs[i].vehicle;
        slots[i] = PosSlot{keys[i], (long long)recs[i].ts_us, recs[i].lat, recs[i].lon};
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return set_err(ctx, HM_E_INVALID, "imported records: a key twice");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = positions_init(ctx))) return rc;
    if ((rc = pos_dict_grow(ctx, P.prov, np_, p_total)) || (rc = pos_dict_grow(ctx, P.veh, nv, v_total)) || (rc = pos_pairs_grow(ctx, n)) ||
        (rc = ensure(ctx, P.params, (size_t)(np_ + nv + 2) * 8)) || (rc = ensure(ctx, P.imp, (size_t)std::max<int64_t>(n, 1) * sizeof(PosSlot))))
        return rc;
    HIPCHK(ctx, hipMemsetAsync(P.words, 0, PW_WORDS * 8, ctx->stream));
    int64_t *dp = (int64_t *)P.params.p;
    if ((rc = pos_import_dict(ctx, P.prov, np_, dicts->provider_offsets, dicts->provider_bytes, p_total, dp, POS_USED_P)) ||
        (rc = pos_import_dict(ctx, P.veh, nv, dicts->vehicle_offsets, dicts->vehicle_bytes, v_total, dp + np_ + 1, POS_USED_V)))
        return rc;
    if (n > 0) {
        HIPCHK(ctx, hipMemcpyAsync(P.imp.p, slots.data(), (size_t)n * sizeof(PosSlot), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pos_pair_put, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const PosSlot *)P.imp.p, n, P.tab, P.cap - 1,
                           P.words);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.words, PW_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    P.prov.n_codes = np_;
    P.prov.arena_used = p_total;
    P.veh.n_codes = nv;
    P.veh.arena_used = v_total;
    P.keys = n;
    return pos_overflow_status(ctx);
}

int hm_positions_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    const hm_ctx::Positions &P = ctx->pos;
    const int64_t w[10] = {P.keys, (int64_t)P.cap, P.prov.n_codes, P.veh.n_codes, P.prov.arena_used + P.veh.arena_used, P.regrows,
                           P.pair_regrows, P.veh.arena_regrows, (int64_t)P.us[0], (int64_t)P.us[1]};
    for (int i = 0; i < n && i < 10; i++) v[i] = w[i];
    return HM_OK;
}

int hm_positions_debug_hash_bits(hm_ctx *ctx, int32_t bits) {
    if (!ctx) return HM_E_INVALID;
    if (bits < 0 || bits > 64) return set_err(ctx, HM_E_INVALID, "hash bits %d outside 0..64", bits);
    if (!positions_empty(ctx)) return set_err(ctx, HM_E_STATE, "hm_positions_debug_hash_bits on a positions state that holds keys");
    ctx->pos.hash_bits = bits;
    return HM_OK;
}
