// Read side: a trailing span of live windows rolled up into one heatmap, with every parent's count per window of the
// span from the same pass (k_span + k_span_emit), and the series rows of records a view or a ranking moved (k_span_rows).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// The span is the roll-up's group-by (k_rollup.h) over up to SPAN_MAX windows' tables in ONE launch: the same liveness
// test (wenc), the same parent (h3_cell_to_parent), the same two levels -- the workgroup's RuTable in LDS in front of
// the global GrowRec table claimed with tab_probe -- and beside the global table a u64[nslots][windows] array, the
// series: word [h][j] is the count of the parent in slot h in the span's j-th window.
//  work        the tables' tiles of RU_THREADS x DUMP_PER slots, concatenated in window order (a table smaller than a
//              tile is one partial tile).  A workgroup takes a CONTIGUOUS block of that tile space, so it meets the
//              windows one after the other and its LDS table holds one window's partial sums at a time.
//  flush       at every window boundary the workgroup crosses, and at its end: each occupied LDS slot adds its sums to
//              the parent's global slot and its cnt to series[slot][window], then the LDS table is cleared (between
//              two barriers: a count is added once).  While a window's parents fit in LDS that is, per parent and
//              window, at most one CAS (the claim), four adds into the slot (n_speed, the three sums; two of them only
//              with a speed) and one into the series: six device-scope atomics.
//  direct      a record whose parent finds no LDS slot goes to the global slot and its series word itself, as in k_rollup.
// The global slot's count word is NOT added to by k_span: a parent's count is the sum of its series row, and k_span_emit,
// which reads the row anyway, stores it into the record and into the slot (the raster's lookup reads it there).
// =====================================================================================================
constexpr int SPAN_MAX = HM_SPAN_MAX_WINDOWS;
struct SpanDescs {
    GenDesc g[SPAN_MAX];          // the live windows of the span, ascending
    long long tile0[SPAN_MAX + 1];   // table i's first tile in the concatenated tile space; [n] = all tiles
    int col[SPAN_MAX];            // table i's column of the series (its window's index in the span)
    int n;
};

// span_global_add: ru_global_add without the count word; *slot = the parent's slot
__device__ __forceinline__ bool span_global_add(GrowRec *tab, unsigned long long mask, uint64_t p, unsigned long long ns, double ssp,
                                                double sla, double slo, unsigned long long *slot) {
    unsigned long long seen;
    const unsigned long long h = tab_probe<true>([tab](unsigned long long i) { return (unsigned long long *)&tab[i].cell; }, mask,
                                                 mix64(p) & mask, mask + 1, 0ull, p, TabKeyIs{p, 0ull}, seen);
    if (h == TAB_NONE) return false;
    GrowRec &s = tab[h];
    if (ns) {
        atomicAdd((unsigned long long *)&s.nspeed, ns);
        atomicAdd(&s.sspeed, ssp);
    }
    atomicAdd(&s.slat, sla);
    atomicAdd(&s.slon, slo);
    *slot = h;
    return true;
}

// the workgroup's LDS table into the global one and column `col` of the series, then cleared; every thread calls it
__device__ __forceinline__ bool span_flush(RuTable &T, GrowRec *tab, unsigned long long mask, unsigned long long *series, int windows,
                                           int col) {
    bool ok = true;
    __syncthreads();
    for (int s = threadIdx.x; s < RU_SLOTS; s += RU_THREADS) {
        if (T.key[s] == 0) continue;
        unsigned long long h;
        if (span_global_add(tab, mask, T.key[s], T.nsp[s], T.ssp[s], T.slat[s], T.slon[s], &h))
            atomicAdd(&series[h * (unsigned long long)windows + col], T.cnt[s]);
        else
            ok = false;
        T.key[s] = 0;
        T.cnt[s] = 0;
        T.nsp[s] = 0;
        T.ssp[s] = 0.0;
        T.slat[s] = 0.0;
        T.slon[s] = 0.0;
    }
    if (threadIdx.x == 0) T.occ = 0;
    __syncthreads();
    return ok;
}

__global__ __launch_bounds__(RU_THREADS) void k_span(SpanDescs D, int res, int windows, GrowRec *__restrict__ tab,
                                                     unsigned long long mask, unsigned long long *__restrict__ series,
                                                     unsigned long long *overflow) {
    __shared__ RuTable T;
    for (int s = threadIdx.x; s < RU_SLOTS; s += RU_THREADS) {
        T.key[s] = 0;
        T.cnt[s] = 0;
        T.nsp[s] = 0;
        T.ssp[s] = 0.0;
        T.slat[s] = 0.0;
        T.slon[s] = 0.0;
    }
    if (threadIdx.x == 0) T.occ = 0;
    __syncthreads();
    const long long total = D.tile0[D.n];
    const long long per = (total + gridDim.x - 1) / gridDim.x;
    const long long t0 = (long long)blockIdx.x * per, t1 = t0 + per < total ? t0 + per : total;
    const int64_t tile = (int64_t)RU_THREADS * DUMP_PER;
    bool ok = true;
    int w = 0;   // the table tile t0 lies in (all of this is uniform over the workgroup)
    while (w + 1 < D.n && D.tile0[w + 1] <= t0) w++;
    for (long long t = t0; t < t1; t++) {
        if (t >= D.tile0[w + 1]) {   // (every table has at least one tile: one step)
            ok &= span_flush(T, tab, mask, series, windows, D.col[w]);
            w++;
        }
        const GenDesc &g = D.g[w];
        const int col = D.col[w];
        const int64_t cap = (int64_t)((g.rmask + 1) << g.rbits);
        const int64_t base = (int64_t)(t - D.tile0[w]) * tile;
        bool live[DUMP_PER];
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * RU_THREADS + threadIdx.x;
            live[k] = i < cap && g.tab[i].wenc == g.wenc;
        }
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            if (!live[k]) continue;
            const TileSlot sl = g.tab[base + k * RU_THREADS + threadIdx.x];
            const uint64_t p = h3_cell_to_parent(sl.cell, res);
            if (ru_lds_add(T, p, sl.count, sl.nspeed, sl.sspeed, sl.slat, sl.slon)) continue;
            unsigned long long h;
            if (span_global_add(tab, mask, p, sl.nspeed, sl.sspeed, sl.slat, sl.slon, &h))
                atomicAdd(&series[h * (unsigned long long)windows + col], sl.count);
            else
                ok = false;
        }
    }
    if (t0 < t1) ok &= span_flush(T, tab, mask, series, windows, D.col[w]);
    if (__ballot(!ok) && lane_id() == 0) atomicAdd(overflow, 1ull);
}

// the claimed slots as records of window `first` (count = the sum of the slot's series row, also stored into the slot),
// compacted by block256_compact, and at the same positions their series rows; past out_cap: counted, not written
__global__ __launch_bounds__(256) void k_span_emit(GrowRec *__restrict__ tab, int64_t nslots, const unsigned long long *__restrict__ series,
                                                   int windows, int64_t first, GrowRec *__restrict__ out,
                                                   unsigned long long *__restrict__ rows, int64_t out_cap, unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < nslots && tab[i].cell != 0; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            GrowRec p = tab[i];
            unsigned long long sum = 0;
            for (int j = 0; j < windows; j++) {
                const unsigned long long c = series[i * windows + j];
                rows[at * windows + j] = c;
                sum += c;
            }
            tab[i].count = sum;
            p.count = sum;
            p.wstart = first;
            p.touched = 0;
            out[at] = p;
        });
    }
}

// rows[i] = the series row of record i's cell, found in the span's parent table (a view or a ranking moved the records)
__global__ __launch_bounds__(256) void k_span_rows(const GrowRec *__restrict__ recs, int64_t n, const GrowRec *__restrict__ tab,
                                                   unsigned long long mask, const unsigned long long *__restrict__ series, int windows,
                                                   unsigned long long *__restrict__ rows, unsigned long long *missing) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t cell = recs[i].cell;
        unsigned long long seen;
        const unsigned long long h = tab_probe<false>([tab](unsigned long long s) { return (const unsigned long long *)&tab[s].cell; }, mask,
                                                      mix64(cell) & mask, mask + 1, 0ull, 0ull, TabKeyIs{cell, 0ull}, seen);
        if (h == TAB_NONE) atomicAdd(missing, 1ull);
        for (int j = 0; j < windows; j++) rows[i * windows + j] = h == TAB_NONE ? 0ull : series[h * (unsigned long long)windows + j];
    }
}
