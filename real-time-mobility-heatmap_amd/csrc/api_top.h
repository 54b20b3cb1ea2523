// C ABI: top-k hotspots -- the k records with the largest count, in rank order, of caller records, of a live window's
// roll-up (with or without a view, as records or as the GeoJSON body) and of the positions density (k_top.h; the roll-up
// is rollup_on_device, the view k_view_tiles, the density density_on_device, the encoder gj_tiles).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

struct TopPass { int word, shift; };   // word 0 kc, 1 cell, 2 idx; shift = 8 * its byte
// The bytes that vary among n keys, from the most significant: those of kc and cell by their OR ^ AND, those of the
// index by n itself.  At most 20.
static int top_plan(unsigned long long vary_c, unsigned long long vary_cell, int64_t n, TopPass *p) {
    const unsigned long long vary[3] = {vary_c, vary_cell, n > 1 ? next_pow2((uint64_t)n) - 1 : 0};
    int np = 0;
    for (int w = 0; w < 3; w++)
        for (int shift = w == 2 ? 24 : 56; shift >= 0; shift -= 8)
            if ((vary[w] >> shift) & 0xff) p[np++] = {w, shift};
    return np;
}
static void top_examine(TopMasks &M, const TopPass &p) {
    if (p.word == 0) M.c |= 0xffull << p.shift;
    else if (p.word == 1) M.cell |= 0xffull << p.shift;
    else M.idx |= 0xffu << p.shift;
}

static int top_init(hm_ctx *ctx) {
    hm_ctx::Top &T = ctx->top;
    if (T.ready) return HM_OK;
    int rc;
    if ((rc = ensure(ctx, T.words, TW_WORDS * 8))) return rc;
    for (auto &e : T.ev) HIPCHK(ctx, hipEventCreate(&e));
    T.ready = true;
    return HM_OK;
}

// the top's kernels between two events; their time is added to `us` at the segment's end (after the caller's sync)
struct TopSegment {
    hm_ctx *ctx;
    bool open = false;
    explicit TopSegment(hm_ctx *c) : ctx(c) {}
    hipError_t begin() { open = true; return hipEventRecord(ctx->top.ev[0], ctx->stream); }
    hipError_t end() { return hipEventRecord(ctx->top.ev[1], ctx->stream); }
    void add(double &us) {
        float ms = 0;
        if (open && hipEventElapsedTime(&ms, ctx->top.ev[0], ctx->top.ev[1]) == hipSuccess) us += 1e3 * ms;
        open = false;
    }
};

// The select and the ordering on two device arrays of key words (kc[n], cell[n]; word 2 is the index), a step of
// top_run, which is how callers reach it: the control block is uploaded (top_control), the OR / NAND of both words
// reduced into it inside the open segment and that segment ended.  Leaves the m selected candidates' indices in T.sidx and their ranks in T.rank, with the last
// segment open: the caller launches its scatter and calls top_finish.  passes[3]: the passes per key word; *tied: the
// candidates still tied with the threshold when the walk stopped.
static int top_select(hm_ctx *ctx, const unsigned long long *kc, const unsigned long long *cell, int64_t n, int64_t m,
                      TopSegment &seg, double &us, int64_t *passes, int64_t *tied) {
    hm_ctx::Top &T = ctx->top;
    unsigned long long *words = (unsigned long long *)T.words.p;
    const int max_grid = T.test_grid ? T.test_grid : 8 * std::max(ctx->n_cus, 1);
    const int stream_grid = grid_for(n, 256, max_grid);
    unsigned long long w[4] = {};
    HIPCHK(ctx, hipMemcpyAsync(w, words + TW_OR_C, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    seg.add(us);
    TopPass plan[20];
    const int np = top_plan(w[0] ^ ~w[1], w[2] ^ ~w[3], n, plan);
    TopMasks M = {0, 0, 0};
    unsigned long long nt[2] = {(unsigned long long)m, (unsigned long long)n};   // need, tied
    for (int p = 0; p < np && nt[1] != nt[0]; p++) {
        HIPCHK(ctx, seg.begin());
        hipLaunchKernelGGL(k_top_hist, dim3(stream_grid), dim3(256), 0, ctx->stream, kc, cell, n, M, plan[p].word, plan[p].shift, words);
        hipLaunchKernelGGL(k_top_pick, dim3(1), dim3(64), 0, ctx->stream, words, plan[p].word, plan[p].shift);
        HIPCHK(ctx, seg.end());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(nt, words + TW_NEED, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        seg.add(us);
        top_examine(M, plan[p]);
        passes[plan[p].word]++;
        if (nt[0] < 1 || nt[0] > nt[1] || nt[1] > (unsigned long long)n)
            return set_err(ctx, HM_E_STATE, "top select: %llu needed of %llu tied after pass %d", nt[0], nt[1], p);
    }
    if (nt[1] != nt[0]) return set_err(ctx, HM_E_STATE, "top select: %llu needed of %llu tied with no byte left", nt[0], nt[1]);
    *tied = (int64_t)nt[1];
    // the selected and their ranks
    const int jblocks = (int)((m + 255) / 256);
    const int splits = std::max(1, std::min(jblocks, 4 * std::max(ctx->n_cus, 1) / jblocks));
    HIPCHK(ctx, seg.begin());
    hipLaunchKernelGGL(k_top_compact, dim3(grid_for(n, 256 * DUMP_PER, max_grid)), dim3(256), 0, ctx->stream, kc, cell, n, M, words,
                       (unsigned long long *)T.skc.p, (unsigned long long *)T.scell.p, (unsigned *)T.sidx.p, (unsigned long long)m);
    HIPCHK(ctx, hipMemsetAsync(T.rank.p, 0, (size_t)m * 4, ctx->stream));
    hipLaunchKernelGGL(k_top_rank, dim3(jblocks, splits), dim3(256), 0, ctx->stream, (const unsigned long long *)T.skc.p,
                       (const unsigned long long *)T.scell.p, (const unsigned *)T.sidx.p, (int)m, (unsigned *)T.rank.p);
    return HM_OK;
}
// the select's buffers for m selected of any number of candidates
static int top_select_buffers(hm_ctx *ctx, int64_t m) {
    hm_ctx::Top &T = ctx->top;
    int rc;
    if ((rc = ensure(ctx, T.skc, (size_t)m * 8)) || (rc = ensure(ctx, T.scell, (size_t)m * 8)) || (rc = ensure(ctx, T.sidx, (size_t)m * 4)) ||
        (rc = ensure(ctx, T.rank, (size_t)m * 4)))
        return rc;
    return HM_OK;
}
// the control block: everything 0 but the need and the tied group, which is every candidate
static hipError_t top_control(hm_ctx *ctx, int64_t n, int64_t m) {
    hm_ctx::Top &T = ctx->top;
    memset(T.h_words, 0, sizeof T.h_words);
    T.h_words[TW_NEED] = (unsigned long long)m;
    T.h_words[TW_TIED] = (unsigned long long)n;
    return hipMemcpyAsync(T.words.p, T.h_words, TW_WORDS * 8, hipMemcpyHostToDevice, ctx->stream);
}
// after the caller's scatter: the last segment's end, and k_top_compact's count against m
static int top_finish(hm_ctx *ctx, TopSegment &seg, double &us, int64_t m) {
    HIPCHK(ctx, seg.end());
    HIPCHK(ctx, hipGetLastError());
    unsigned long long got = 0;
    HIPCHK(ctx, hipMemcpyAsync(&got, (unsigned long long *)ctx->top.words.p + TW_OUT, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    seg.add(us);
    if ((int64_t)got != m) return set_err(ctx, HM_E_STATE, "top select kept %llu records, %lld expected", got, (long long)m);
    return HM_OK;
}
// The whole protocol in one place: the control block, `vary` (launches the kernel that reduces the OR / NAND of the key
// words into the control block -- k_top_keys while it extracts the keys, k_near_vary over keys that exist), the select
// and the ranks (top_select), `scatter` (launches the caller's kernel that copies its records by T.sidx / T.rank), and
// the final count (top_finish).  us gains the device time of all of it.
extern "C++" {
template <class Vary, class Scatter>
static int top_run(hm_ctx *ctx, const unsigned long long *kc, const unsigned long long *cell, int64_t n, int64_t m, double &us,
                   int64_t *passes, int64_t *tied, Vary vary, Scatter scatter) {
    TopSegment seg(ctx);
    HIPCHK(ctx, top_control(ctx, n, m));
    HIPCHK(ctx, seg.begin());
    vary();
    HIPCHK(ctx, seg.end());
    HIPCHK(ctx, hipGetLastError());
    int rc;
    if ((rc = top_select(ctx, kc, cell, n, m, seg, us, passes, tied))) return rc;
    scatter();
    return top_finish(ctx, seg, us, m);
}
}  // extern "C++"

// top(recs[0, n), k) on the device: *out = the first min(k, n) records of the order in T.out (device), *m_out their
// number.  recs: device memory, 16-byte aligned.  Fills T.info; reads recs only.
static int top_on_device(hm_ctx *ctx, const GrowRec *recs, int64_t n, int64_t k, const GrowRec **out, int64_t *m_out) {
    hm_ctx::Top &T = ctx->top;
    for (int64_t &x : T.info) x = 0;
    T.info[0] = n;
    *out = nullptr;
    *m_out = 0;
    const int64_t m = std::min(k, n);
    if (m <= 0) return HM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = top_init(ctx)) || (rc = ensure(ctx, T.kc, (size_t)n * 8)) || (rc = ensure(ctx, T.cell, (size_t)n * 8)) ||
        (rc = top_select_buffers(ctx, m)) || (rc = ensure(ctx, T.out, (size_t)m * sizeof(GrowRec))))
        return rc;
    unsigned long long *words = (unsigned long long *)T.words.p;
    unsigned long long *kc = (unsigned long long *)T.kc.p, *cell = (unsigned long long *)T.cell.p;
    const int max_grid = T.test_grid ? T.test_grid : 8 * std::max(ctx->n_cus, 1);
    double us = 0;
    rc = top_run(
        ctx, kc, cell, n, m, us, &T.info[2], &T.info[5],
        [&] { hipLaunchKernelGGL(k_top_keys, dim3(grid_for(n, 256, max_grid)), dim3(256), 0, ctx->stream, recs, n, kc, cell, words); },
        [&] {   // the records in rank order
            hipLaunchKernelGGL(k_top_scatter, dim3(grid_for(4 * m, 256)), dim3(256), 0, ctx->stream, (const uint4 *)recs, n,
                               (const unsigned *)T.sidx.p, (const unsigned *)T.rank.p, (int)m, (uint4 *)T.out.p);
        });
    if (rc) return rc;
    T.info[1] = m;
    T.info[6] = (int64_t)us;
    *out = (const GrowRec *)T.out.p;
    *m_out = m;
    return HM_OK;
}

// the device records handed out where they are, or copied to the top's pinned buffer
static int top_out(hm_ctx *ctx, const GrowRec *d, int64_t m, int32_t out_memory, const hm_state_rec **recs) {
    hm_ctx::Top &T = ctx->top;
    *recs = (const hm_state_rec *)d;
    if (m == 0 || out_memory == HM_MEM_DEVICE) return HM_OK;
    int rc;
    if ((rc = host_pinned(ctx, &T.h_out, T.h_out_cap, (size_t)m * sizeof(GrowRec)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(T.h_out, d, (size_t)m * sizeof(GrowRec), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, ctx_sync(ctx, __LINE__));
    *recs = (const hm_state_rec *)T.h_out;
    return HM_OK;
}

static bool top_k_ok(int64_t k) { return k >= 0 && k <= TOP_MAX; }
static int top_bad_k(hm_ctx *ctx, const char *who, int64_t k) {
    return set_err(ctx, HM_E_INVALID, "%s: k = %lld outside 0..%lld", who, (long long)k, (long long)TOP_MAX);
}
static int top_bad_view(hm_ctx *ctx, const hm_view *view) {
    return set_err(ctx, HM_E_INVALID, "view (%g, %g, %g, %g): finite, -90 <= south <= north <= 90, -180 <= west, east <= 180",
                   view->west, view->south, view->east, view->north);
}

int hm_top_records(hm_ctx *ctx, const hm_state_rec *recs, int64_t n, int32_t memory, int64_t k, int32_t out_memory,
                   const hm_state_rec **top, int64_t *n_top) {
    if (!ctx || !top || !n_top || n < 0 || n > (int64_t(1) << 31) || (n > 0 && !recs) ||
        (memory != HM_MEM_HOST && memory != HM_MEM_DEVICE) || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE) ||
        (memory == HM_MEM_DEVICE && ((uintptr_t)recs & 15)))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_top_records", k);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "hm_top_records between stage calls");
    *top = nullptr;
    *n_top = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const GrowRec *d = (const GrowRec *)recs;
    int rc;
    if (memory == HM_MEM_HOST && n > 0 && k > 0) {
        if ((rc = ensure(ctx, ctx->top.in, (size_t)n * sizeof(GrowRec)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->top.in.p, recs, (size_t)n * sizeof(GrowRec), hipMemcpyHostToDevice, ctx->stream));
        d = (const GrowRec *)ctx->top.in.p;
    }
    const GrowRec *o = nullptr;
    int64_t m = 0;
    if ((rc = top_on_device(ctx, d, n, k, &o, &m)) || (rc = top_out(ctx, o, m, out_memory, top))) return rc;
    *n_top = m;
    return HM_OK;
}

// hm_window_top's and hm_window_geojson_top's device part: roll up, filter by the view if there is one (into the top's
// own buffer), select; *out / *m_out as top_on_device's.  The arguments are checked by the caller.
static int top_window(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_view *view, int64_t k, const char *who,
                      const GrowRec **out, int64_t *m_out) {
    hm_ctx::Top &T = ctx->top;
    *out = nullptr;
    *m_out = 0;
    if (res < 0 || res > ctx->cfg.h3_res)
        return set_err(ctx, HM_E_INVALID, "roll-up resolution %d outside 0..%d", res, ctx->cfg.h3_res);
    if (ctx->shard_count > 1)
        return set_err(ctx, HM_E_UNSUPPORTED, "%s on shard %d of %d: a rank's top is not the global one (hm_top_records on the added records is)",
                       who, ctx->shard_rank, ctx->shard_count);
    if (ctx->stage != 0) return set_err(ctx, HM_E_STATE, "%s between stage calls", who);
    for (int64_t &x : T.info) x = 0;
    if (k == 0) return HM_OK;
    int64_t m = 0;
    int rc;
    if ((rc = rollup_on_device(ctx, window_start_us, res, who, &m))) return rc;
    const GrowRec *cand = (const GrowRec *)ctx->ru_out.p;
    if (view && m > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if ((rc = top_init(ctx)) || (rc = ensure(ctx, T.vrecs, (size_t)m * sizeof(GrowRec)))) return rc;
        const ViewPoles &poles = view_poles();
        unsigned long long *w = (unsigned long long *)T.words.p + TW_VIEW, kept = 0;
        HIPCHK(ctx, hipMemsetAsync(w, 0, 8, ctx->stream));
        hipLaunchKernelGGL(k_view_tiles, dim3(grid_for(m, 256 * DUMP_PER)), dim3(256), 0, ctx->stream, cand, m, poles.north[res],
                           poles.south[res], *view, (GrowRec *)T.vrecs.p, w);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&kept, w, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, ctx_sync(ctx, __LINE__));
        if ((int64_t)kept > m) return set_err(ctx, HM_E_STATE, "the view kept %llu of %lld records", kept, (long long)m);
        m = (int64_t)kept;
        cand = (const GrowRec *)T.vrecs.p;
    }
    return top_on_device(ctx, cand, m, k, out, m_out);
}

int hm_window_top(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_view *view, int64_t k, int32_t out_memory,
                  const hm_state_rec **recs, int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_window_top", k);
    if (view && !view_valid(*view)) return top_bad_view(ctx, view);
    const GrowRec *o = nullptr;
    int64_t m = 0;
    int rc;
    if ((rc = top_window(ctx, window_start_us, res, view, k, "hm_window_top", &o, &m))) return rc;
    *recs = nullptr;
    *n = 0;
    if ((rc = top_out(ctx, o, m, out_memory, recs))) return rc;
    *n = m;
    return HM_OK;
}

int hm_window_geojson_top(hm_ctx *ctx, int64_t window_start_us, int32_t res, const hm_geojson_cfg *cfg, const hm_view *view,
                          int64_t k, int32_t out_memory, const uint8_t **bytes, const int64_t **offsets, int64_t *n,
                          const hm_state_rec **recs) {
    if (!ctx || !cfg || !bytes || !offsets || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_window_geojson_top", k);
    if (view && !view_valid(*view)) return top_bad_view(ctx, view);
    GjTexts X;
    if (gj_texts(cfg, X)) return set_err(ctx, HM_E_INVALID, "window texts: at most %d bytes of 0x20-0x7e without '\"' and '\\'", GJ_TEXT_MAX);
    const GrowRec *o = nullptr;
    int64_t m = 0;
    int rc;
    if ((rc = top_window(ctx, window_start_us, res, view, k, "hm_window_geojson_top", &o, &m))) return rc;
    *n = 0;
    if (recs) {   // the records in feature order = rank order (the top's pinned copy)
        *recs = nullptr;
        if ((rc = top_out(ctx, o, m, HM_MEM_HOST, recs))) return rc;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = gj_tiles(ctx, X, o, m, out_memory, bytes, offsets))) return rc;
    *n = m;
    return HM_OK;
}

int hm_positions_density_top(hm_ctx *ctx, int32_t res, int64_t since_us, const hm_view *view, int64_t k, int32_t out_memory,
                             const hm_state_rec **recs, int64_t *n) {
    if (!ctx || !recs || !n || (out_memory != HM_MEM_HOST && out_memory != HM_MEM_DEVICE))
        return ctx ? set_err(ctx, HM_E_INVALID, "bad argument") : HM_E_INVALID;
    if (!top_k_ok(k)) return top_bad_k(ctx, "hm_positions_density_top", k);
    if (res < 0 || res > 15) return set_err(ctx, HM_E_INVALID, "density resolution %d outside 0..15", res);
    if (view && !view_valid(*view)) return top_bad_view(ctx, view);
    int rc;
    if ((rc = density_state_ok(ctx, "hm_positions_density_top"))) return rc;
    *recs = nullptr;
    *n = 0;
    for (int64_t &x : ctx->top.info) x = 0;
    if (k == 0) return HM_OK;
    const GrowRec *d = nullptr, *o = nullptr;
    int64_t g = 0, m = 0;
    if ((rc = density_on_device(ctx, res, since_us, view, &d, &g)) || (rc = top_on_device(ctx, d, g, k, &o, &m)) ||
        (rc = top_out(ctx, o, m, out_memory, recs)))
        return rc;
    *n = m;
    return HM_OK;
}

// Host execution of the select and the ordering with the kernels' HM_HD helpers on n keys of two words (word 2 is the
// index): the plan of varying bytes, the passes' digits (top_digit, top_tied), the selection (top_selected), and the
// order by the comparator the counting uses (top_before).  sel = the m selected indices in rank order.
static int top_select_host(const unsigned long long *kc, const unsigned long long *cell, int64_t n, int64_t m, std::vector<unsigned> &sel) {
    unsigned long long orc = 0, andc = ~0ull, orl = 0, andl = ~0ull;
    for (int64_t i = 0; i < n; i++) {
        orc |= kc[i];
        andc &= kc[i];
        orl |= cell[i];
        andl &= cell[i];
    }
    TopPass plan[20];
    const int np = top_plan(orc ^ andc, orl ^ andl, n, plan);
    TopMasks M = {0, 0, 0};
    unsigned long long prefix[3] = {0, 0, 0}, need = (unsigned long long)m, tied = (unsigned long long)n;
    for (int p = 0; p < np && tied != need; p++) {
        unsigned long long h[256] = {};
        for (int64_t i = 0; i < n; i++)
            if (top_tied(kc[i], cell[i], (unsigned)i, M, prefix[0], prefix[1], (unsigned)prefix[2])) {
                const unsigned long long word = plan[p].word == 0 ? kc[i] : plan[p].word == 1 ? cell[i] : (unsigned long long)(unsigned)i;
                h[top_digit(word, plan[p].shift)]++;
            }
        unsigned d = 0;
        while (h[d] < need) need -= h[d++];
        prefix[plan[p].word] |= (unsigned long long)d << plan[p].shift;
        tied = h[d];
        top_examine(M, plan[p]);
    }
    if (tied != need) return HM_E_STATE;
    sel.clear();
    sel.reserve((size_t)m);
    for (int64_t i = 0; i < n; i++)
        if (top_selected(kc[i], cell[i], (unsigned)i, M, prefix[0], prefix[1], (unsigned)prefix[2])) sel.push_back((unsigned)i);
    if ((int64_t)sel.size() != m) return HM_E_STATE;
    std::sort(sel.begin(), sel.end(), [&](unsigned a, unsigned b) { return top_before(kc[a], cell[a], a, kc[b], cell[b], b); });
    return HM_OK;
}

// Host execution of the top: the keys (top_key_count), then top_select_host.
int hm_selftest_top_records(const hm_state_rec *recs, int64_t n, int64_t k, hm_state_rec *out, int64_t *n_out) {
    if (n < 0 || n > (int64_t(1) << 31) || (n > 0 && !recs) || !top_k_ok(k) || !n_out) return HM_E_INVALID;
    const int64_t m = std::min(k, n);
    if (m > 0 && !out) return HM_E_INVALID;
    *n_out = 0;
    if (m == 0) return HM_OK;
    std::vector<unsigned long long> kc((size_t)n), cell((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        kc[i] = top_key_count(recs[i].count);
        cell[i] = recs[i].cell;
    }
    std::vector<unsigned> sel;
    if (int rc = top_select_host(kc.data(), cell.data(), n, m, sel)) return rc;
    for (int64_t j = 0; j < m; j++) out[j] = recs[sel[j]];
    *n_out = m;
    return HM_OK;
}

int hm_top_info(const hm_ctx *ctx, int64_t *v, int32_t n) {
    if (!ctx || !v || n < 0) return HM_E_INVALID;
    for (int i = 0; i < n && i < 7; i++) v[i] = ctx->top.info[i];
    return HM_OK;
}
