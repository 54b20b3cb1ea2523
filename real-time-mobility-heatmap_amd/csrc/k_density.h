// Read side: the positions state aggregated into H3 density cells -- how many vehicles are in each cell of resolution
// res right now, among those seen since since_us (k_density_cells + k_density_exact + k_density_group + k_density_emit).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// Two phases over the pair table's slots (PosSlot, k_positions.h; the state is at rest: no POS_FRESH):
//  A  k_density_cells   one slot per thread: a live slot (key != POS_EMPTY) with ts >= since_us is snapped by
//                       latLngToCellFast; cell_of[slot] = its cell, DN_UNSNAPPED where the snap gives 0 (a NaN or
//                       out-of-range coordinate), 0 for a free or too old slot.  The fast path's misses go to an
//                       exception list (u32 slot indices, wave_append, room for every slot), and k_density_exact runs
//                       latLngToCellDeg on that list only -- the arrangement of k_cells / k_raster, so that the exact
//                       path's registers never limit the streaming kernel.
//  B  k_density_group   the group-by of k_rollup.h on (cell_of[slot], the slot's body): the per-workgroup LDS front
//                       table (ru_lds_add) with one more word per slot, the group's newest ts; what finds no slot
//                       there, and every LDS slot at the workgroup's end, goes to the zeroed global GrowRec table
//                       (ru_global_add) with an atomicMax into the slot's wstart word.  A whole fleet inside one
//                       res-0 cell costs LDS atomics and one global add per workgroup.
// A and B are separate kernels: A wants the fast path's ~60 VGPRs at full occupancy and no LDS, B is one workgroup
// per CU behind a 112-KB LDS table; fused, every snap would run at B's 4 waves per SIMD.
// The newest ts is kept as ts ^ 2^63 in an unsigned word (dn_ts_enc): unsigned order is then signed order, and the
// zeroed word of a fresh slot -- LDS or global -- is INT64_MIN, the identity of max, so a group of negative ts_us never
// reads a cleared word as a time.  k_density_emit decodes it into the record's window_start_us.
// =====================================================================================================
constexpr uint64_t DN_UNSNAPPED = 1;   // cell_of[] of a kept key without a cell (no H3 index is 1: mode bits 59-62 are 0)
HM_HD unsigned long long dn_ts_enc(long long ts) { return (unsigned long long)ts ^ (1ull << 63); }
HM_HD long long dn_ts_dec(unsigned long long w) { return (long long)(w ^ (1ull << 63)); }
// words of the density's control block (device; zeroed before every call)
enum { DW_OUT = 0, DW_OVERFLOW, DW_SLOW, DW_KEPT, DW_UNSNAPPED, DW_GADDS, DW_VIEW, DW_WORDS };

struct DnTable : RuTable {
    unsigned long long ts[RU_SLOTS];   // dn_ts_enc of the group's newest ts; 0 = none yet
};

// phase A: exceptions -> slow[] (room for nslots indices)
__global__ __launch_bounds__(256) void k_density_cells(const PosSlot *__restrict__ tab, int64_t nslots, int res, long long since,
                                                       uint64_t *__restrict__ cell_of, unsigned int *__restrict__ slow,
                                                       unsigned long long *n_slow) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nslots; base += stride) {   // (uniform trip count: ballots)
        const int64_t i = base + threadIdx.x;
        bool exc = false;
        if (i < nslots) {
            const PosSlot e = tab[i];
            uint64_t c = 0;
            if (e.key != POS_EMPTY && e.ts >= since) {
                exc = !latLngToCellFast(e.lat, e.lon, res, c_tab, c);
                if (c == 0) c = DN_UNSNAPPED;
            }
            cell_of[i] = c;   // (an exception's word is rewritten by k_density_exact)
        }
        const unsigned long long pos = wave_append(exc, n_slow);
        if (exc) slow[pos] = (unsigned int)i;
    }
}
// the exception list's slots by the exact path
__global__ __launch_bounds__(256) void k_density_exact(const PosSlot *__restrict__ tab, int res, uint64_t *__restrict__ cell_of,
                                                       const unsigned int *__restrict__ slow, const unsigned long long *n_slow) {
    const int64_t m = (int64_t)*n_slow;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (int64_t)gridDim.x * blockDim.x) {
        const unsigned i = slow[q];
        const uint64_t c = latLngToCellDeg(tab[i].lat, tab[i].lon, res, c_tab);
        cell_of[i] = c ? c : DN_UNSNAPPED;
    }
}

// one vehicle into group `cell` of the global table; counts the add
__device__ __forceinline__ bool dn_global_add(GrowRec *tab, unsigned long long mask, uint64_t cell, unsigned long long c,
                                              double sla, double slo, unsigned long long ts_enc) {
    unsigned long long h;
    if (!ru_global_add<true>(tab, mask, cell, c, 0ull, 0.0, sla, slo, &h)) return false;
    atomicMax((unsigned long long *)&tab[h].wstart, ts_enc);
    return true;
}

// phase B: tiles of DUMP_PER x RU_THREADS consecutive slots per workgroup iteration, as k_rollup's.  words: DW_KEPT,
// DW_UNSNAPPED and DW_GADDS gain one add per workgroup (from LDS counters), DW_OVERFLOW one per failing wave.
__global__ __launch_bounds__(RU_THREADS) void k_density_group(const PosSlot *__restrict__ slots, int64_t nslots,
                                                              const uint64_t *__restrict__ cell_of, GrowRec *__restrict__ tab,
                                                              unsigned long long mask, unsigned long long *words) {
    __shared__ DnTable T;
    __shared__ unsigned long long tally[3];   // kept, unsnapped, global adds
    for (int s = threadIdx.x; s < RU_SLOTS; s += RU_THREADS) {
        T.key[s] = 0;
        T.cnt[s] = 0;
        T.nsp[s] = 0;
        T.ssp[s] = 0.0;
        T.slat[s] = 0.0;
        T.slon[s] = 0.0;
        T.ts[s] = 0;
    }
    if (threadIdx.x == 0) T.occ = 0;
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    __syncthreads();
    const int64_t tile = (int64_t)RU_THREADS * DUMP_PER;
    bool ok = true;
    unsigned long long kept = 0, unsnapped = 0, gadds = 0;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        uint64_t cell[DUMP_PER];
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * RU_THREADS + threadIdx.x;
            cell[k] = i < nslots ? cell_of[i] : 0;
        }
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            if (cell[k] == 0) continue;
            kept++;
            if (cell[k] == DN_UNSNAPPED) { unsnapped++; continue; }
            const PosSlot e = slots[base + k * RU_THREADS + threadIdx.x];
            const unsigned long long te = dn_ts_enc(e.ts);
            unsigned h;
            if (ru_lds_add<true>(T, cell[k], 1ull, 0ull, 0.0, e.lat, e.lon, &h)) {
                atomicMax(&T.ts[h], te);
            } else {
                ok &= dn_global_add(tab, mask, cell[k], 1ull, e.lat, e.lon, te);
                gadds++;
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < RU_SLOTS; s += RU_THREADS)
        if (T.key[s]) {
            ok &= dn_global_add(tab, mask, T.key[s], T.cnt[s], T.slat[s], T.slon[s], T.ts[s]);
            gadds++;
        }
    kept = wave_sum(kept);
    unsnapped = wave_sum(unsnapped);
    gadds = wave_sum(gadds);
    if (lane_id() == 0) {
        if (kept) atomicAdd(&tally[0], kept);
        if (unsnapped) atomicAdd(&tally[1], unsnapped);
        if (gadds) atomicAdd(&tally[2], gadds);
    }
    if (__ballot(!ok) && lane_id() == 0) atomicAdd(&words[DW_OVERFLOW], 1ull);
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&words[DW_KEPT + threadIdx.x], tally[threadIdx.x]);
}

// k_rollup_emit keeping the table's newest ts: the claimed slots of the global table as records whose window_start_us
// is that ts, compacted by block256_compact; records past out_cap are counted, not written
__global__ __launch_bounds__(256) void k_density_emit(const GrowRec *__restrict__ tab, int64_t nslots, GrowRec *__restrict__ out,
                                                      int64_t out_cap, unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < nslots && tab[i].cell != 0; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            GrowRec p = tab[i];
            p.wstart = dn_ts_dec((unsigned long long)p.wstart);
            p.touched = 0;
            out[at] = p;
        });
    }
}
