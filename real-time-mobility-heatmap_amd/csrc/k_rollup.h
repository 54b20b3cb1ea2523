// Read side: one live window's tiles rolled up to a coarser H3 resolution (k_rollup + k_rollup_emit).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// upstream cellToParent for r <= the cell's resolution (the caller's guarantee): the resolution field (bits 52-55)
// becomes r, digits r+1..15 become 7 (unused), base cell and digits 1..r stay -- pentagons included: a cell's parent is
// a prefix of its digits, whatever the base cell.
HM_HD uint64_t h3_cell_to_parent(uint64_t cell, int r) {
    const uint64_t unused = (UINT64_C(1) << (3 * (15 - r))) - 1;
    return (cell & ~(UINT64_C(0xF) << 52)) | ((uint64_t)r << 52) | unused;
}

// =====================================================================================================
// The roll-up is a group-by of one window's table on h3_cell_to_parent(cell, r): count, non-null speed count and the
// three sums add up exactly across a parent's children.  Two levels, as table mode (k_table.h):
//  LDS front table   one per workgroup (1024 threads, one workgroup per CU), open addressing, linear probing with a
//                    probe bound, never more than half full.  While every parent the workgroup meets fits (res 0:
//                    122 cells, res 1: 842), every add is an LDS atomic and the workgroup adds each parent to the global
//                    table once, at its end.  A record whose parent finds no slot (table at its fill limit, or the
//                    probe bound) goes to the global table directly: exact, just not pre-aggregated.  Nothing is
//                    evicted, so a key is never behind an empty slot of its probe chain.
//  global table      2^k >= 2 * (distinct parents possible) slots of 64 B (a GrowRec each, zeroed before the launch):
//                    a slot is found or claimed by tab_probe (dev_table.h: a 64-bit CAS on its cell word, 0 = free),
//                    linear probing wraps over the whole table (load <= 1/2: it always ends), counts added with u64
//                    atomics, sums with fp64 atomic adds.
// k_rollup_emit compacts the claimed slots into hm_state_rec records (block256_compact, dev_table.h).
// =====================================================================================================
constexpr int RU_THREADS = 1024;
constexpr int RU_SLOTS = 2048;           // 48 B each: 96 KB of LDS
constexpr int RU_FILL = RU_SLOTS / 2;    // no new key from here on (>= the 842 cells of res 1)
constexpr int RU_PROBES = 16;
struct RuTable {
    unsigned long long key[RU_SLOTS];    // parent cell, 0 = free
    unsigned long long cnt[RU_SLOTS];    // (cumulative u64 counts: not packed with nsp as k_agg's per-batch ones are)
    unsigned long long nsp[RU_SLOTS];
    double ssp[RU_SLOTS];
    double slat[RU_SLOTS];
    double slon[RU_SLOTS];
    unsigned occ;
};

// add a child's aggregate to parent p in the LDS table; false: no slot for it (the caller adds it globally)
// SLOT (k_density.h, whose table has one more word per slot): *slot = the slot the aggregate went to
template <bool SLOT = false>
__device__ __forceinline__ bool ru_lds_add(RuTable &T, uint64_t p, unsigned long long c, unsigned long long ns, double ssp,
                                           double sla, double slo, unsigned *slot = nullptr) {
    unsigned h = (unsigned)(mix64(p) >> 32) & (RU_SLOTS - 1);
    for (int q = 0; q < RU_PROBES; q++) {
        unsigned long long cur = __hip_atomic_load(&T.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) {
            if (__hip_atomic_load(&T.occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (unsigned)RU_FILL) return false;
            cur = atomicCAS(&T.key[h], 0ull, (unsigned long long)p);
            if (cur == 0) atomicAdd(&T.occ, 1u);
        }
        if (cur == 0 || cur == p) {
            atomicAdd(&T.cnt[h], c);
            if (ns) {   // (only non-null speeds: Spark's sum skips nulls)
                atomicAdd(&T.nsp[h], ns);
                atomicAdd(&T.ssp[h], ssp);
            }
            atomicAdd(&T.slat[h], sla);
            atomicAdd(&T.slon[h], slo);
            if constexpr (SLOT) *slot = h;
            return true;
        }
        h = (h + 1) & (RU_SLOTS - 1);
    }
    return false;
}

// add an aggregate to parent p in the global table (mask + 1 slots); false: every slot belongs to another parent
// (cannot happen at load <= 1/2; the bound keeps a mis-sized table from spinning).  SLOT: *slot = the parent's slot
template <bool SLOT = false>
__device__ __forceinline__ bool ru_global_add(GrowRec *tab, unsigned long long mask, uint64_t p, unsigned long long c,
                                              unsigned long long ns, double ssp, double sla, double slo,
                                              unsigned long long *slot = nullptr) {
    unsigned long long seen;
    const unsigned long long h = tab_probe<true>([tab](unsigned long long i) { return (unsigned long long *)&tab[i].cell; }, mask,
                                                 mix64(p) & mask, mask + 1, 0ull, p, TabKeyIs{p, 0ull}, seen);
    if (h == TAB_NONE) return false;
    GrowRec &s = tab[h];
    atomicAdd((unsigned long long *)&s.count, c);
    if (ns) {
        atomicAdd((unsigned long long *)&s.nspeed, ns);
        atomicAdd(&s.sspeed, ssp);
    }
    atomicAdd(&s.slat, sla);
    atomicAdd(&s.slon, slo);
    if constexpr (SLOT) *slot = h;
    return true;
}

// scans window g's table in tiles of DUMP_PER x RU_THREADS consecutive slots per workgroup iteration (coalesced: slot
// k * RU_THREADS + tid); a slot is live iff its window word is g's (tables are reused without clearing)
__global__ __launch_bounds__(RU_THREADS) void k_rollup(GenDesc g, int res, GrowRec *__restrict__ tab, unsigned long long mask,
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
    const int64_t cap = (int64_t)((g.rmask + 1) << g.rbits);
    const int64_t tile = (int64_t)RU_THREADS * DUMP_PER;
    bool ok = true;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < cap; base += (int64_t)gridDim.x * tile) {
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
            if (!ru_lds_add(T, p, sl.count, sl.nspeed, sl.sspeed, sl.slat, sl.slon))
                ok &= ru_global_add(tab, mask, p, sl.count, sl.nspeed, sl.sspeed, sl.slat, sl.slon);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < RU_SLOTS; s += RU_THREADS)
        if (T.key[s]) ok &= ru_global_add(tab, mask, T.key[s], T.cnt[s], T.nsp[s], T.ssp[s], T.slat[s], T.slon[s]);
    if (__ballot(!ok) && lane_id() == 0) atomicAdd(overflow, 1ull);
}

// the claimed slots of the global table as records of window wstart, compacted by block256_compact (dev_table.h);
// records past out_cap are counted, not written (the host then fails the call)
__global__ __launch_bounds__(256) void k_rollup_emit(const GrowRec *__restrict__ tab, int64_t nslots, int64_t wstart,
                                                     GrowRec *__restrict__ out, int64_t out_cap, unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < nslots && tab[i].cell != 0; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            GrowRec p = tab[i];
            p.wstart = wstart;
            p.touched = 0;
            out[at] = p;
        });
    }
}
