// Read side: the change between two live windows -- the roll-up records of window A joined on the cell with those of
// window B, one pair per cell of either (k_change_match, k_change_rest), the ranking key on the pair's count change
// (k_change_keys; the select is the top's, k_top.h) and the pairs moved into rank order (k_change_scatter).  The rule
// is DESIGN §5o's; the only arithmetic here is an int64 subtraction.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// A pair is 128 B: A's record of the cell, then B's, each exactly the record hm_window_rollup returns, or the zero
// record {cell, the window's start, 0, 0, 0.0, 0.0, 0.0, 0} when the window has none for the cell.
// The join never sorts: window B's roll-up leaves its parent table (open addressing on the cell word, load <= 1/2).
//  k_change_match  one thread per record of A probes B's table read-only (tab_probe<false>); a hit copies the slot's
//                  body as the base and sets the slot's `touched` word -- the roll-up leaves that word 0 in the table
//                  (k_rollup_emit writes 0 into the records' copy) and A's cells are distinct, so one thread at most
//                  marks a slot: a plain store.  Pair i goes to out[i].
//  k_change_rest   B's claimed slots that nobody marked, compacted behind them (block256_compact): out[mA + at].
// The order of a pair among the ranked: the top's three-word key (k_top.h) with word 0 = top_key_count of
// +change (rising), -change (falling) or |change| (abs), word 1 the cell, word 2 the pair's index.
// =====================================================================================================
struct alignas(64) ChangeRec {
    GrowRec cur, base;
};
static_assert(sizeof(ChangeRec) == 128, "ChangeRec is 128 B");
static_assert(sizeof(hm_change_rec) == sizeof(ChangeRec), "hm_change_rec mirrors ChangeRec");
HM_HD uint64_t rec_cell(const ChangeRec &r) { return r.cur.cell; }   // k_view_tiles' (both halves carry the cell)

// a window's record of a cell it does not hold
HM_HD GrowRec change_zero(uint64_t cell, int64_t wstart) {
    GrowRec z;
    z.cell = cell;
    z.wstart = wstart;
    z.count = 0;
    z.nspeed = 0;
    z.sspeed = 0.0;
    z.slat = 0.0;
    z.slon = 0.0;
    z.touched = 0;
    return z;
}
// countChange: library counts are >= 0, so the difference of two of them fits an int64
HM_HD long long change_of(const GrowRec &cur, const GrowRec &base) { return (long long)cur.count - (long long)base.count; }
HM_HD bool change_order_ok(int order) { return order == HM_CHANGE_RISING || order == HM_CHANGE_FALLING || order == HM_CHANGE_ABS; }
// key word 0 of a pair (the smaller key ranks first)
HM_HD unsigned long long change_key(const GrowRec &cur, const GrowRec &base, int order) {
    const long long d = change_of(cur, base);
    return top_key_count(order == HM_CHANGE_RISING ? d : order == HM_CHANGE_FALLING ? -d : d < 0 ? -d : d);
}

// a pair as eight 16-byte stores
__device__ __forceinline__ void change_store(ChangeRec *out, const GrowRec &cur, const GrowRec &base) {
    uint4 q[8];
    memcpy(q, &cur, 64);
    memcpy(q + 4, &base, 64);
    uint4 *o = (uint4 *)out;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = q[k];
}

// out[i] = (A's record i, B's record of its cell or the zero base); tab: B's parent table of mask + 1 slots, nullptr
// when B is not live.  Marks the slots it matched.
__global__ __launch_bounds__(256) void k_change_match(const GrowRec *__restrict__ recs, int64_t n, GrowRec *tab, unsigned long long mask,
                                                      int64_t base_start, ChangeRec *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const GrowRec a = recs[i];
        GrowRec b = change_zero(a.cell, base_start);
        if (tab) {
            unsigned long long seen;
            const unsigned long long h = tab_probe<false>([tab](unsigned long long s) { return (const unsigned long long *)&tab[s].cell; },
                                                          mask, mix64(a.cell) & mask, mask + 1, 0ull, 0ull, TabKeyIs{a.cell, 0ull}, seen);
            if (h != TAB_NONE) {
                b = tab[h];
                b.wstart = base_start;
                b.touched = 0;
                tab[h].touched = 1;
            }
        }
        change_store(out + i, a, b);
    }
}

// B's claimed and unmarked slots as pairs with the zero cur, compacted into out[0, cap) (the caller passes the pairs'
// buffer past A's records); *n_out counts them
__global__ __launch_bounds__(256) void k_change_rest(const GrowRec *__restrict__ tab, int64_t nslots, int64_t window_start,
                                                     int64_t base_start, ChangeRec *__restrict__ out, int64_t cap,
                                                     unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < nslots && tab[i].cell != 0 && tab[i].touched == 0; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)cap, [=](int64_t i, unsigned long long at) {
            GrowRec b = tab[i];
            b.wstart = base_start;
            change_store(out + at, change_zero(b.cell, window_start), b);
        });
    }
}

// the two key words of every pair into the top's key buffers (their OR / NAND: k_near_vary over them)
__global__ __launch_bounds__(256) void k_change_keys(const ChangeRec *__restrict__ pairs, int64_t n, int order,
                                                     unsigned long long *__restrict__ kc, unsigned long long *__restrict__ cell) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        kc[i] = change_key(pairs[i].cur, pairs[i].base, order);
        cell[i] = pairs[i].cur.cell;
    }
}

// out[rank[j]] = pairs[sidx[j]], whole: eight lanes per pair, 16 bytes each (a stale index or rank writes nothing)
__global__ __launch_bounds__(256) void k_change_scatter(const uint4 *__restrict__ pairs, int64_t n, const unsigned *__restrict__ sidx,
                                                        const unsigned *__restrict__ rank, int m, uint4 *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)m * 8; t += (int64_t)gridDim.x * 256) {
        const unsigned src = sidx[t >> 3], r = rank[t >> 3];
        if ((int64_t)src < n && r < (unsigned)m) out[(int64_t)r * 8 + (t & 7)] = pairs[(int64_t)src * 8 + (t & 7)];
    }
}
