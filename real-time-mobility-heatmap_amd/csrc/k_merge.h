// State-table kernels: census, growth dump, the region-owned merge into the update-mode state (heatmap_stream.py:111-133,243) and the row densification.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// census of a batch's partials per window (sizes the window tables before the merge)
__global__ __launch_bounds__(256) void k_census(const TilePartial *__restrict__ parts, int64_t n, WinCount *cmap, DevStats *st) {
    __shared__ WinLds WL;
    wl_init(WL);
    __syncthreads();
    const CensusSink sink{cmap};
    bool ok = true;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        const bool in = i < n;
        const unsigned long long we = in ? wenc_of(parts[i].wstart) : 0;
        ok &= wave_count_windows(in, we, 1ull, WL, sink);
    }
    __syncthreads();
    ok &= wl_flush(WL, sink);
    if (__ballot(!ok) && lane_id() == 0) atomicAdd(&st->overflow, 1ull);
}

// growth: the live keys of one window's old table as partial records (aux = the key's touched word), to be
// merged into its new table by k_merge_owned in rehash mode
// (only_seq != 0: only the keys whose touched word carries that batch sequence -- an incremental checkpoint)
// (clear_touched: a checkpoint export -- the touched word means nothing outside this context)
// compacted by block256_compact (dev_table.h): the record order in `out` is irrelevant to every caller
__global__ __launch_bounds__(256) void k_dump_gen(GenDesc g, GrowRec *__restrict__ out, unsigned long long *n_out,
                                                  unsigned only_seq = 0, bool clear_touched = false) {
    const int64_t cap = (int64_t)((g.rmask + 1) << g.rbits);
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < cap; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=, &g](int64_t i) {   // (g: the descriptor in the kernel's arguments, not copied)
            bool live = false;
            if (i < cap) {
                const unsigned long long we = g.tab[i].wenc;
                live = we == g.wenc && (only_seq == 0 || (unsigned)(g.tab[i].touched >> 32) == only_seq);
            }
            return live;
        };
        block256_compact<false>(base, is_live, n_out, 0, [=, &g](int64_t i, unsigned long long at) {
            const TileSlot sl = g.tab[i];
            GrowRec p;
            p.cell = sl.cell;
            p.wstart = wdec(sl.wenc);
            p.count = sl.count;
            p.nspeed = sl.nspeed;
            p.sspeed = sl.sspeed;
            p.slat = sl.slat;
            p.slon = sl.slon;
            p.touched = clear_touched ? 0ull : sl.touched;
            out[at] = p;
        });
    }
}

// =====================================================================================================
// K3': owner merge + emission. The workgroup of a bin is the only writer of the (window, region)s the partition
// sent it, so the state is updated with plain loads/stores instead of device-scope atomics. Per chunk of 512
// partials (one per lane), each lane finds its key's slot and claims it in an LDS claim set (MoClaims); a lane whose
// slot is already claimed by the same key in this chunk adds its values into the claimer's LDS staging entry and is
// done (in-chunk de-duplication without a separate hash table):
//  * resident windows (the bin's regions of the windows this batch merges into, while their tags fit in
//    tag_bytes of LDS): probing runs over the region's slot tags in LDS -- a new key reads nothing from HBM;
//    an occupied slot not claimed in this chunk is read only on a tag match;
//  * other windows (too many/too large regions, or growth): probing reads the slots' window words from HBM;
//    the tag byte of a created slot is stored to HBM.
// The update-mode output row of a key (cumulative count/avg, heatmap_stream.py:124-132,243) is written at its
// first touch in the batch to row b0 + k of the bin's segment (b0 = the bin's first partial, k = touch order
// in the bin; the slot's `touched` word keeps (batch seq, b0 + k)), and rewritten in place when a later chunk -- of
// this launch, or a later merge of the same batch -- updates the key again; k_fill_gaps closes the gaps left by keys
// that had several partials.
// rehash != 0: growth (k_dump_gen records, unique keys, into the window's new table): created slots keep the
// record's touched word, no rows are written.
// The kernel is its bin loop and chunk loop over these steps, each a function below:
//   per bin    0  mo_resident_regions (+ mo_load_segments), mo_fill_tags
//   per chunk  1  mo_rec_at, mrec_of, mo_stage          2  mo_probe / mo_probe_coop     3a mo_old_line
//              3  mo_touch_rows, mo_new_line            4  mo_store_lines, put_row      5  barrier, MoClaims::release
//   per bin    6  mo_tags_writeback
// =====================================================================================================
constexpr int MO_THREADS = 512;      // partials per chunk (one per lane)
// The LDS of a chunk's claim set holds MO_CLAIM 64-bit entries keyed by slot address (load <= 1/2) or, in the
// resident-only merge, MO_CLAIM32 32-bit entries keyed by tag index (load <= 1/4): MoClaims below.
constexpr int MO_CLAIM = 2 * MO_THREADS;
// LDS for resident region tags per workgroup: dynamic, sized per launch to the regions a bin can receive (the sum
// over the batch's windows of slots per region, 1 B each) up to MO_TAG_MAX -- 24 KB on the bench (3 windows x 8 K
// slots: two workgroups per CU), 32 KB for a res-7 window of 2^28 slots, which would otherwise probe through HBM
constexpr int MO_TAG_MAX = 90112;
constexpr int MO_RES_MAX = 16;                   // resident (window, region)s per bin

struct MoShared {
    // this chunk's records by lane; a duplicate key's values are added into its claimer's entry
    unsigned long long sc[MO_THREADS];
    unsigned long long sh[MO_THREADS];
    unsigned long long scnt[MO_THREADS];
    unsigned long long snsp[MO_THREADS];
    double sssp[MO_THREADS];
    double sslat[MO_THREADS];
    double sslon[MO_THREADS];
    unsigned long long claim[MO_CLAIM];   // the claim set (MoClaims); 0 = free
    unsigned n_touched;                   // keys of the current bin touched for the first time this batch
    int n_res;
    unsigned res_new[MO_RES_MAX];         // keys created in the resident region this bin
    unsigned long long res_we[MO_RES_MAX];
    TileSlot *res_slots[MO_RES_MAX];      // the region's first slot
    uint8_t *res_gtags[MO_RES_MAX];       // the region's tags in HBM
    unsigned res_off[MO_RES_MAX];         // byte offset of the region's tags in `tags`
    unsigned res_mask[MO_RES_MAX];        // slots per region - 1
    unsigned res_dirty[MO_RES_MAX];
    uint4 xline[MO_THREADS / 64][64];     // per wave: one round of the cooperative old-line loads (16 lines)
};

template <typename T>
__device__ __forceinline__ T ld_l2(const T *p) {   // bypass the CU's L1 (chunks of one workgroup re-read slots)
    // (a global-address-space access: the slot pointers come from LDS, and as generic pointers every access became a
    // flat instruction, which also counts on lgkmcnt -- so each later LDS wait waited for it to complete)
    return __hip_atomic_load((__attribute__((address_space(1))) const T *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The claim set of a chunk in S.claim: open addressing, an entry is ((key + kBias) << kLaneBits) | claimer lane, 0 = free.
//  * MoClaimsAddr: 64-bit entries keyed by the slot's address (the variants that may probe through HBM);
//  * MoClaimsTag: the resident-only merge keys its claims by the slot's tag index (< 2^17: MO_TAG_MAX) instead, so an
//    entry is 32 bits -- ((tag index + 1) << 9) | lane -- and the same LDS holds twice the entries.
template <typename E, int kLaneBits, int kEntries>
struct MoClaims {
    typedef E Key;
    static constexpr E kBias = sizeof(E) == 4 ? 1 : 0;   // (a tag index may be 0; an address is not)
    E *cl;
    static __device__ __forceinline__ unsigned home(E key) {
        if constexpr (sizeof(E) == 8) return (unsigned)(((key >> 6) * UINT64_C(0x9e3779b97f4a7c15)) >> 40) & (kEntries - 1);
        else return (key * 0x9e3779b1u) >> (32 - __builtin_ctz(kEntries));
    }
    // claim `key` for `lane`: -1 = claimed (entry index in ci), else the lane that already holds it (-2: the set is full)
    __device__ __forceinline__ int claim(E key, int lane, int &ci) const {
        const E packed = ((key + kBias) << kLaneBits) | (E)lane;
        unsigned h = home(key);
        for (int k = 0; k < kEntries; k++) {
            const E o = atomicCAS(&cl[h], (E)0, packed);
            if (o == 0) { ci = (int)h; return -1; }
            if ((o >> kLaneBits) == key + kBias) return (int)(o & ((E(1) << kLaneBits) - 1));
            h = (h + 1) & (kEntries - 1);
        }
        return -2;
    }
    // the lane holding `key`, -1 if none
    __device__ __forceinline__ int holder(E key) const {
        unsigned h = home(key);
        for (int k = 0; k < kEntries; k++) {
            const E o = __hip_atomic_load(&cl[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (o == 0) return -1;
            if ((o >> kLaneBits) == key + kBias) return (int)(o & ((E(1) << kLaneBits) - 1));
            h = (h + 1) & (kEntries - 1);
        }
        return -1;
    }
    __device__ __forceinline__ void release(int ci) const { cl[ci] = 0; }
};
constexpr int MO_CLAIM32 = 2 * MO_CLAIM;
static_assert(MO_TAG_MAX < (1 << 17) && MO_THREADS <= 512, "32-bit claim entries");
typedef MoClaims<unsigned long long, 16, MO_CLAIM> MoClaimsAddr;
typedef MoClaims<unsigned, 9, MO_CLAIM32> MoClaimsTag;
template <bool kResident> using MoClaimsOf = typename std::conditional<kResident, MoClaimsTag, MoClaimsAddr>::type;

// a merge input record, normalised: SortedRec (table mode / stage merge), GrowRec (growth), EventRec (direct path)
struct MRec {
    uint64_t cell;
    unsigned long long we;   // wenc of the window start
    uint64_t hk;             // tile_hash(cell, window start)
    unsigned long long cnt, nsp;
    double ssp, slat, slon;
    unsigned long long touched;   // GrowRec only
};
__device__ __forceinline__ MRec mrec_of(const SortedRec &p, const WInfo *, uint64_t) {
    return MRec{p.cell, wenc_of(p.wstart), p.hash, p.count, p.nspeed, p.sspeed, p.slat, p.slon, 0ull};
}
__device__ __forceinline__ MRec mrec_of(const GrowRec &p, const WInfo *, uint64_t) {
    return MRec{p.cell, wenc_of(p.wstart), tile_hash(p.cell, p.wstart), p.count, p.nspeed, p.sspeed, p.slat, p.slon, p.touched};
}
__device__ __forceinline__ MRec mrec_of_wi(const EventRec &p, const WInfo &wi, uint64_t cell_hi) {
    const uint64_t cell = (p.key & CELL_LO) | cell_hi;
    const bool sv = __builtin_bit_cast(uint64_t, p.speed) != SPEED_NULL_BITS;
    return MRec{cell, wi.wenc, mix64(cell ^ wi.inner), 1ull, sv ? 1ull : 0ull, sv ? p.speed : 0.0, p.lat, p.lon, 0ull};
}
__device__ __forceinline__ MRec mrec_of(const EventRec &p, const WInfo *winfo, uint64_t cell_hi) {
    return mrec_of_wi(p, winfo[ekey_widx(p.key)], cell_hi);   // (an LDS copy measured no faster here: the chunk loop hides it)
}
// a duplicate of lane x's key: add this record's values into x's staging entry
__device__ __forceinline__ void mo_add_into(MoShared &S, int x, const MRec &p) {
    atomicAdd(&S.scnt[x], p.cnt);
    if (p.nsp) {
        atomicAdd(&S.snsp[x], p.nsp);
        atomicAdd(&S.sssp[x], p.ssp);
    }
    atomicAdd(&S.sslat[x], p.slat);
    atomicAdd(&S.sslon[x], p.slon);
}

struct RowsOut {   // update-mode output rows (SoA), heatmap_stream.py:124-132
    uint64_t *cell;
    int64_t *ws;
    int64_t *cnt;
    double *sp;
    uint8_t *spnull;
    double *lon;
    double *lat;
};
// Spark Average: sum / count (count of non-null inputs) as double; null when that count is 0
__device__ __forceinline__ void put_row(const RowsOut &o, int64_t t, uint64_t cell, unsigned long long we,
                                        unsigned long long count, unsigned long long nspeed, double sspeed, double slat,
                                        double slon) {
    const bool null_sp = nspeed == 0;
    // x / 1.0 == x: a key's first row (count 1) skips the fp64 divisions
    double asp = null_sp ? 0.0 : sspeed, alon = slon, alat = slat;
    if (count != 1) {   // (a branch: a wave whose keys all have one row skips the three fp64 divisions)
        if (!null_sp && nspeed != 1) asp = sspeed / (double)nspeed;
        alon = slon / (double)count;
        alat = slat / (double)count;
    }
    o.cell[t] = cell;
    o.ws[t] = wdec(we);
    o.cnt[t] = (int64_t)count;
    o.sp[t] = asp;
    o.spnull[t] = null_sp;
    o.lon[t] = alon;
    o.lat[t] = alat;
}

// a state line's values (cell and window word are the key's), and the line as its four 16-B parts (TileSlot's layout:
// cell, wenc | count, nspeed | sspeed, slat | slon, touched)
struct MLine {
    unsigned long long count, nspeed;
    double sspeed, slat, slon;
    unsigned long long touched;
};
struct MoLineParts { uint4 q0, q1, q2, q3; };
__device__ __forceinline__ unsigned long long mo_u64(unsigned lo, unsigned hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); }
__device__ __forceinline__ uint4 mo_u4(unsigned long long a, unsigned long long b) { return make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)); }
__device__ __forceinline__ MLine mo_unpack_line(const MoLineParts &L) {
    return MLine{mo_u64(L.q1.x, L.q1.y), mo_u64(L.q1.z, L.q1.w), __builtin_bit_cast(double, mo_u64(L.q2.x, L.q2.y)),
                 __builtin_bit_cast(double, mo_u64(L.q2.z, L.q2.w)), __builtin_bit_cast(double, mo_u64(L.q3.x, L.q3.y)),
                 mo_u64(L.q3.z, L.q3.w)};
}
__device__ __forceinline__ MoLineParts mo_pack_line(uint64_t cell, unsigned long long we, const MLine &v) {
    return MoLineParts{mo_u4(cell, we), mo_u4(v.count, v.nspeed),
                       mo_u4(__builtin_bit_cast(uint64_t, v.sspeed), __builtin_bit_cast(uint64_t, v.slat)),
                       mo_u4(__builtin_bit_cast(uint64_t, v.slon), v.touched)};
}
// Whole lines per memory instruction, through LDS scratch of the wave (xa, xb: 32 16-B words each).  Every lane of the
// wave calls these (shuffles); ga = the lane's slot address, 0 for none.  In round k, lanes 16k..16k+15 own the lines
// and lane L moves part L & 3 of the line of lane 16k + L / 4: each 16-B instruction touches 16 whole 64-B lines
// instead of a quarter of 64.
// mo_gather_lines: the lanes' lines, loaded (16-B non-temporal loads: L2-served, like ld_l2); a round none of whose
// 16 lanes has a line is skipped (wave-uniform).
__device__ __forceinline__ MoLineParts mo_gather_lines(unsigned long long ga, uint4 *xa, uint4 *xb) {
    MoLineParts L{};
    const int ln = lane_id();
    const unsigned long long needm = __ballot(ga != 0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!((needm >> (16 * k)) & 0xffffull)) continue;   // (wave-uniform)
        const int src = k * 16 + (ln >> 2), part = ln & 3;
        const unsigned long long sa = __shfl(ga, src, 64);
        if (sa) {
            const hm_v4u v = __builtin_nontemporal_load((g_cv4u *)sa + part);
            ((part < 2) ? xa : xb)[(src & 15) * 2 + (part & 1)] = make_uint4(v.x, v.y, v.z, v.w);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (ga && (ln >> 4) == k) {
            const int e = (ln & 15) * 2;
            L = MoLineParts{xa[e], xa[e + 1], xb[e], xb[e + 1]};
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    return L;
}
// mo_scatter_lines: the lanes' lines L, stored (the mirror of the gather; each lane storing its own line would be four
// instructions, each touching 64 different lines)
__device__ __forceinline__ void mo_scatter_lines(unsigned long long ga, const MoLineParts &L, uint4 *xa, uint4 *xb) {
    const int ln = lane_id();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((ln >> 4) == k) {
            const int e = (ln & 15) * 2;
            xa[e] = L.q0; xa[e + 1] = L.q1;
            xb[e] = L.q2; xb[e + 1] = L.q3;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int src = k * 16 + (ln >> 2), part = ln & 3;
        const unsigned long long sa = __shfl(ga, src, 64);
        const uint4 val = ((part < 2) ? xa : xb)[(src & 15) * 2 + (part & 1)];
        if (sa) st_g16((uint4 *)sa + part, val);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

// Advance (s, scanned) over the tags of a resident region (tag bytes [off, off + rmask] of `tags`, in LDS) to the next
// slot whose tag is empty or tg: true with that slot in s and its tag in b, false when the region has none left.
// Tags are scanned 8 at a time (one 8-B LDS read): only slots whose tag is empty or this key's are visited one by one,
// so a wave's loop runs its lanes' longest count of such slots, not of probed slots.
// (regions are >= 256 slots and start at multiples of their size: a word never crosses a region)
__device__ __forceinline__ bool mo_tag_scan(const unsigned *tags, unsigned off, unsigned rmask, unsigned tg, unsigned &s,
                                            unsigned &scanned, unsigned &b) {
    const unsigned long long tgv = (unsigned long long)tg * UINT64_C(0x0101010101010101);
    const unsigned long long *tags64 = (const unsigned long long *)tags;
    while (scanned <= rmask) {
        const unsigned bw = off + s, p0 = bw & 7;
        const unsigned long long word = __hip_atomic_load(&tags64[bw >> 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        // high bit of each byte that is 0 (exact per byte: no borrow between bytes), or equal to tg
        constexpr unsigned long long LO7 = UINT64_C(0x7f7f7f7f7f7f7f7f);
        const unsigned long long y = word ^ tgv;
        unsigned long long cand = ~(((word & LO7) + LO7) | word | LO7) | ~(((y & LO7) + LO7) | y | LO7);
        cand &= ~UINT64_C(0) << (8 * p0);
        if (!cand) {   // no candidate in the rest of the word: the next word
            scanned += 8 - p0;
            s = (s + 8 - p0) & rmask;
            continue;
        }
        const unsigned pos = (unsigned)__builtin_ctzll(cand) >> 3;
        scanned += pos - p0 + 1;
        s = (s + pos - p0) & rmask;
        b = (unsigned)(word >> (8 * pos)) & 0xffu;
        return true;
    }
    return false;
}

// Rec = SortedRec: a batch's partials (partitioned); EventRec: the direct path's rows; GrowRec: growth (rehash).
// kResident: the host found every window of the batch resident in every bin (merge_sorted), so the variant carries
// no HBM-probing fallback (less code, fewer live registers); a record outside the resident windows sets overflow.
// kCoop (resident only): the wave-cooperative probe (mo_probe_coop) -- chosen when the last batch re-touched mostly
// existing keys (their lines then cost one cooperative round trip); a batch of mostly new keys runs the per-lane probe,
// which carries less machinery per probed slot (bench leg: 3.72-3.81 vs 4.03-4.11 ms; state-read leg: 6.86-6.89 vs
// 6.22-6.30 ms, profiles/r3/r3ab9/)
// kSeg (the multi-GPU owner): bin b's records are nseg segments, one per sender -- segment s at address SO[b * nseg + s]
// (the receive buffer, or the owner's own slab), after SP[b * nseg + s] records of the bin (k_stage_segments)
// The instantiations that are launched are listed once, in merge_variant (host_ctx.h).
constexpr int MO_SEG_MAX = 64;
// Debug build (make libmobheat_dbg.so: MOBHEAT_BOUNDS_CHECK=1): every segment read of the kSeg variant must lie in one
// of the two ranges the host declared for the launch (merge_sorted: the receive buffer, the owner's slabs) -- else the
// kernel prints the bin, segment and address and traps, so that a fault names its access
#ifndef MOBHEAT_BOUNDS_CHECK
#define MOBHEAT_BOUNDS_CHECK 0
#endif
struct SegBounds { unsigned long long lo[2], hi[2]; };
#if MOBHEAT_BOUNDS_CHECK
__device__ SegBounds g_seg_bounds;
#endif

// what the steps of one bin share (wave-uniform): the workgroup's LDS, the bin's records [b0, b1) and resident regions,
// the kSeg variant's segment tables (in LDS)
struct MoBin {
    MoShared &S;
    unsigned *tags;   // the resident regions' tags (dynamic LDS)
    int bin;
    int64_t b0, b1;
    int nres;
    const unsigned long long *seg_base;   // kSeg: segment s's first record, after seg_pre[s] records of the bin
    const unsigned *seg_pre;
    int nseg;
};

// 0. the bin's resident regions: windows merged into this batch whose region maps to this bin (one thread)
__device__ __forceinline__ void mo_resident_regions(MoShared &S, const GenCache &C, int bin, bool any, unsigned tag_bytes) {
    int nr = 0;
    unsigned off = 0;
    if (any && C.n >= 0) {
        for (int q = 0; q < C.n; q++) {
            const GenDesc &g = C.e[q];
            if (!g.batch_parts) continue;
            const unsigned sb = g.sb, smask = (1u << sb) - 1;
            if (((unsigned)bin & smask) != (window_salt(g.wenc) & smask)) continue;
            const unsigned reg = ((unsigned)bin >> sb) - g.rbase;   // (a shard's table: its range only)
            if (reg >= (1u << g.rbits)) continue;
            const unsigned slots = (unsigned)g.rmask + 1;
            if (nr == MO_RES_MAX || off + slots > tag_bytes) continue;
            const unsigned long long first = (unsigned long long)reg << g.rshift;
            S.res_we[nr] = g.wenc;
            S.res_slots[nr] = g.tab + first;
            S.res_gtags[nr] = gen_tags(g) + first;
            S.res_off[nr] = off;
            S.res_mask[nr] = slots - 1;
            S.res_dirty[nr] = 0;
            S.res_new[nr] = 0;
            off += slots;
            nr++;
        }
    }
    S.n_res = nr;
}
// the resident regions' tags into LDS (16-B words, regions >= 256 slots): every load of a thread in flight together
__device__ __forceinline__ void mo_fetch_tag_word(const MoShared &S, unsigned q, unsigned tot, uint4 &v, unsigned &a) {
    typedef __attribute__((address_space(1))) const hm_v4u gv4u;   // global loads (the pointers sit in LDS)
    if (q >= tot) return;
    unsigned w = q;
    int r = 0;
    while (w >= ((S.res_mask[r] + 1) >> 4)) { w -= (S.res_mask[r] + 1) >> 4; r++; }
    const hm_v4u x = ((gv4u *)S.res_gtags[r])[w];
    v = make_uint4(x.x, x.y, x.z, x.w);
    a = (S.res_off[r] >> 4) + w;
}
__device__ __forceinline__ void mo_fill_tags(const MoBin &B, int t) {
    const MoShared &S = B.S;
    unsigned tot = 0;
    for (int r = 0; r < B.nres; r++) tot += (S.res_mask[r] + 1) >> 4;
    for (unsigned q0 = t; q0 < tot; q0 += 4 * MO_THREADS) {
        uint4 v0, v1, v2, v3;
        unsigned a0 = ~0u, a1 = ~0u, a2 = ~0u, a3 = ~0u;
        mo_fetch_tag_word(S, q0, tot, v0, a0);
        mo_fetch_tag_word(S, q0 + MO_THREADS, tot, v1, a1);
        mo_fetch_tag_word(S, q0 + 2 * MO_THREADS, tot, v2, a2);
        mo_fetch_tag_word(S, q0 + 3 * MO_THREADS, tot, v3, a3);
        if (a0 != ~0u) ((uint4 *)B.tags)[a0] = v0;
        if (a1 != ~0u) ((uint4 *)B.tags)[a1] = v1;
        if (a2 != ~0u) ((uint4 *)B.tags)[a2] = v2;
        if (a3 != ~0u) ((uint4 *)B.tags)[a3] = v3;
    }
}

// 1. record i of the bin: [b0, b1) of the partitioned array or of the bin's slab (bp), or (kSeg) the record at bin
// index v = i - b0, in the last segment starting at or before v (binary search)
template <typename Rec, bool kSeg>
__device__ __forceinline__ const Rec *mo_rec_at(const MoBin &B, const Rec *__restrict__ bp, int64_t i) {
    if constexpr (kSeg) {
        const unsigned v = (unsigned)(i - B.b0);
        int lo = 0, hi = B.nseg;   // seg_pre[lo] <= v < seg_pre[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (B.seg_pre[mid] <= v) lo = mid; else hi = mid;
        }
        const Rec *rp = (const Rec *)(uintptr_t)B.seg_base[lo] + (v - B.seg_pre[lo]);
#if MOBHEAT_BOUNDS_CHECK
        const unsigned long long a = (unsigned long long)(uintptr_t)rp, e = a + sizeof(Rec);
        const SegBounds &G = g_seg_bounds;
        if (!((a >= G.lo[0] && e <= G.hi[0]) || (a >= G.lo[1] && e <= G.hi[1]))) {
            printf("k_merge_owned: bin %d segment %d record %u at 0x%llx outside [0x%llx, 0x%llx) and [0x%llx, 0x%llx)\n",
                   B.bin, lo, v, a, G.lo[0], G.hi[0], G.lo[1], G.hi[1]);
            __builtin_trap();
        }
#endif
        return rp;
    } else {
        return bp + i;
    }
}
// 1. lane t's record of this chunk, staged in LDS
__device__ __forceinline__ void mo_stage(MoShared &S, int t, const MRec &p) {
    S.sc[t] = p.cell; S.sh[t] = p.hk;
    S.scnt[t] = p.cnt; S.snsp[t] = p.nsp; S.sssp[t] = p.ssp;
    S.sslat[t] = p.slat; S.sslon[t] = p.slon;
}

// 2. what a lane's probe found
struct MoProbe {
    TileSlot *gslot = nullptr;   // the slot this lane claimed (nullptr: it joined the lane holding its key, or has no record)
    bool created = false;        // the slot was empty
    int r = -1, ci = -1;         // the key's resident region (-1: none), the lane's claim-set entry
    MLine pre{}; bool preloaded = false;   // mo_probe_coop: the existing line, already loaded
    bool lost = false;           // no slot found (a full region, a window without a table): overflow
    bool hbm = false;            // probed through HBM
};
__device__ __forceinline__ int mo_region_of(const MoBin &B, unsigned long long we) {
    int r = -1;
    for (int q = 0; q < B.nres; q++) r = B.S.res_we[q] == we ? q : r;
    return r;
}
// a claimed resident slot that was empty gets the key's tag
__device__ __forceinline__ void mo_tag_created(const MoBin &B, int r, unsigned bi, unsigned tg) {
    atomicOr(&B.tags[bi >> 2], tg << ((bi & 3) * 8));
    B.S.res_dirty[r] = 1;
}
// find (and claim) the slot of lane t's key p, or join the lane of this chunk that holds it
template <bool kResident>
__device__ __forceinline__ void mo_probe(const MoBin &B, const GenCache &C, GenDesc *gm, const MRec &p, int t, MoProbe &o) {
    typedef MoClaimsOf<kResident> Claims;
    MoShared &S = B.S;
    const Claims cl{(typename Claims::Key *)S.claim};
    const unsigned long long we = p.we;
    const uint64_t hk = p.hk;
    const unsigned tg = tag8(hk);
    bool done = false;
    const int r = o.r = mo_region_of(B, we);
    if (r >= 0) {
        const unsigned rmask = S.res_mask[r], off = S.res_off[r];
        TileSlot *const base = S.res_slots[r];
        unsigned s = (unsigned)inreg_slot(hk, rmask), scanned = 0, b = 0;
        while (!done && mo_tag_scan(B.tags, off, rmask, tg, s, scanned, b)) {
            TileSlot *const sl = base + s;
            const unsigned bi = off + s;
            const typename Claims::Key key = kResident ? (typename Claims::Key)bi : (typename Claims::Key)(unsigned long long)sl;
            int x = b == 0 ? -1 : cl.holder(key);
            bool old_match = false;
            if (b == tg && x < 0) old_match = ld_l2(&sl->cell) == p.cell && ld_l2(&sl->wenc) == we;
            if (b == 0 || old_match) {
                x = cl.claim(key, t, o.ci);
                if (x == -1) {
                    o.gslot = sl;
                    o.created = b == 0;
                    if (o.created) mo_tag_created(B, r, bi, tg);
                    done = true;
                }
            }
            if (!done && x >= 0 && S.sc[x] == p.cell && S.sh[x] == hk) {   // same key, this chunk
                mo_add_into(S, x, p);
                done = true;
            }
            s = (s + 1) & rmask;
        }
    } else if constexpr (!kResident) {
        o.hbm = true;
        const GenDesc *g = gen_lookup(C, gm, we);
        if (g) {
            TileSlot *const tab = g->tab;
            const unsigned long long rmask = g->rmask;
            unsigned long long sidx = home_slot(*g, hk);
            for (unsigned long long pr = 0; pr <= rmask && !done; pr++) {
                TileSlot *const sl = &tab[sidx];
                const bool free_here = ld_l2(&sl->wenc) != we;   // never used, or another window's key
                if (free_here || ld_l2(&sl->cell) == p.cell) {
                    const int x = cl.claim((unsigned long long)sl, t, o.ci);
                    if (x == -1) {
                        o.gslot = sl;
                        o.created = free_here;
                        if (o.created) ((__attribute__((address_space(1))) uint8_t *)gen_tags(*g))[sidx] = (uint8_t)tag8(hk);
                        done = true;
                    } else if (S.sc[x] == p.cell && S.sh[x] == hk) {
                        mo_add_into(S, x, p);
                        done = true;
                    }
                }
                sidx = next_slot(sidx, rmask);
            }
        }
    }
    if (!done) o.lost = true;
}
// The resident-only merge's probe, wave-cooperative: each round every lane still probing scans its region's
// tags to its next candidate slot (empty or its tag); the lanes whose candidate holds an older key of the same
// tag then load those lines TOGETHER, whole (mo_gather_lines), compare the key and keep the line: one round trip per
// existing key, and no second load of the line after the barrier.  Every lane of the wave calls it (has: with a record).
__device__ __forceinline__ void mo_probe_coop(const MoBin &B, const MRec &p, bool has, int t, MoProbe &o) {
    MoShared &S = B.S;
    const MoClaimsTag cl{(unsigned *)S.claim};
    const unsigned long long we = p.we;
    const uint64_t hk = p.hk;
    const unsigned tg = tag8(hk);
    const int r = o.r = has ? mo_region_of(B, we) : -1;
    bool done = !has || r < 0;
    o.lost = has && r < 0;
    unsigned rmask = 0, off = 0, s = 0, scanned = 0;
    TileSlot *base = nullptr;
    if (r >= 0) {
        rmask = S.res_mask[r];
        off = S.res_off[r];
        base = S.res_slots[r];
        s = (unsigned)inreg_slot(hk, rmask);
    }
    uint4 *const xa = &S.xline[t >> 6][0], *const xb = &S.xline[t >> 6][32];
    while (__ballot(!done)) {
        // 1. this lane's next candidate slot
        unsigned b = 0;
        bool found = false;
        if (!done) {
            found = mo_tag_scan(B.tags, off, rmask, tg, s, scanned, b);
            if (!found) { done = true; o.lost = true; }   // the region is full
        }
        const unsigned bi = off + s;
        TileSlot *const sl = base + s;
        // 2. a tag-matching slot: claimed in this chunk (its holder), else its line from HBM, loaded together
        int x = -1;
        if (found && b != 0) x = cl.holder(bi);
        const bool need = found && b == tg && x < 0;
        const MoLineParts L = mo_gather_lines(need ? (unsigned long long)sl : 0ull, xa, xb);
        const bool old_match = need && mo_u64(L.q0.x, L.q0.y) == p.cell && mo_u64(L.q0.z, L.q0.w) == we;
        // 3. claim an empty slot or the key's own
        if (found && (b == 0 || old_match)) {
            x = cl.claim(bi, t, o.ci);
            if (x == -1) {
                o.gslot = sl;
                o.created = b == 0;
                if (o.created) mo_tag_created(B, r, bi, tg);
                else { o.pre = mo_unpack_line(L); o.preloaded = true; }
                done = true;
            }
        }
        if (found && !done && x >= 0 && S.sc[x] == p.cell && S.sh[x] == hk) {   // same key, this chunk
            mo_add_into(S, x, p);
            done = true;
        }
        if (found && !done) s = (s + 1) & rmask;
    }
}

// 3a. the claimed slot's current line (created slots read nothing; mo_probe_coop's lanes have theirs): whole lines per
// load instruction through the wave's own scratch -- the lines are loaded before the barrier, while other waves'
// joiners still read this wave's staged keys in S.sc / S.sh.  Every lane of the wave calls it.
__device__ __forceinline__ MLine mo_old_line(MoShared &S, int t, const MoProbe &pr) {
    MLine o{};
    if (pr.preloaded) o = pr.pre;
    const bool need = pr.gslot && !pr.created && !pr.preloaded;
    const MoLineParts L = mo_gather_lines(need ? (unsigned long long)pr.gslot : 0ull, &S.xline[t >> 6][0], &S.xline[t >> 6][32]);
    if (need) o = mo_unpack_line(L);
    return o;
}
// 3. row index of a key's first touch in this batch: one LDS add per wave
__device__ __forceinline__ unsigned mo_touch_rows(MoShared &S, bool first) {
    const unsigned long long fb = __ballot(first);
    unsigned tbase = 0;
    if (lane_id() == 0 && fb) tbase = atomicAdd(&S.n_touched, (unsigned)__popcll(fb));
    tbase = __shfl(tbase, 0, 64);
    return tbase + (unsigned)__popcll(fb & ((1ull << lane_id()) - 1));
}
// 3. the new state line of a claimed slot: its old values (o) + the chunk's sums for the key in lane t's staging entry
template <bool rehash>
__device__ __forceinline__ MLine mo_new_line(const MoShared &S, int t, const MRec &p, const MLine &o, bool first, unsigned seq,
                                             unsigned krow) {
    MLine v;
    const unsigned long long acnt = S.scnt[t], ansp = S.snsp[t];
    v.count = o.count + acnt;
    v.nspeed = o.nspeed + ansp;
    v.sspeed = ansp ? o.sspeed + S.sssp[t] : o.sspeed;
    v.slat = o.slat + S.sslat[t];
    v.slon = o.slon + S.sslon[t];
    if constexpr (rehash) v.touched = p.touched;
    else v.touched = first ? ((unsigned long long)seq << 32) | krow : o.touched;
    return v;
}
// 4. this chunk's state lines, stored whole: the lanes' lines go through the wave's slices of S.sc / S.sh, unused
// after the probe.  Every lane of the wave calls it (gslot == nullptr: nothing to store).
__device__ __forceinline__ void mo_store_lines(MoShared &S, int t, TileSlot *gslot, const MRec &p, const MLine &v) {
    mo_scatter_lines((unsigned long long)gslot, mo_pack_line(p.cell, p.we, v), (uint4 *)&S.sc[t & ~63], (uint4 *)&S.sh[t & ~63]);
}
// 6. the bin's created keys counted for their windows, and the resident regions' tags written back
__device__ __forceinline__ bool mo_tags_writeback(const MoBin &B, GenDesc *gm, int t) {
    const MoShared &S = B.S;
    bool ok = true;
    if (t < B.nres && S.res_new[t] && !gmap_add(gm, S.res_we[t], S.res_new[t])) ok = false;
    for (int r = 0; r < B.nres; r++) {
        if (!S.res_dirty[r]) continue;
        uint4 *dst = (uint4 *)S.res_gtags[r];
        const unsigned w0 = S.res_off[r] >> 4, nw = (S.res_mask[r] + 1) >> 4;
        for (unsigned q = t; q < nw; q += MO_THREADS) st_g16(dst + q, ((const uint4 *)B.tags)[w0 + q]);
    }
    return ok;
}

template <typename Rec, bool kResident = false, bool kCoop = false, bool kSeg = false>
__global__ __launch_bounds__(MO_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_merge_owned(const Rec *__restrict__ parts, int64_t slab,
                                                            const unsigned long long *__restrict__ SO, const unsigned *__restrict__ SP, int nseg,
                                                            const unsigned long long *__restrict__ O, int64_t ntiles, int nbins,
                                                            GenDesc *gm, const GenDesc *glist, int n_glist,
                                                            const WInfo *__restrict__ winfo, uint64_t cell_hi,
                                                            unsigned seq, RowsOut rows, unsigned *bin_cnt, DevStats *st,
                                                            unsigned tag_bytes) {
    constexpr bool rehash = std::is_same<Rec, GrowRec>::value;
    constexpr bool kEv = std::is_same<Rec, EventRec>::value;
    __shared__ MoShared S;
    extern __shared__ unsigned mo_tags[];   // tag_bytes of resident region tags
    __shared__ WinLds WL;
    __shared__ GenCache C;
    __shared__ unsigned long long seg_base[kSeg ? MO_SEG_MAX : 1];
    __shared__ unsigned seg_pre[kSeg ? MO_SEG_MAX + 1 : 1];
    wl_init(WL);
    gc_load(C, glist, n_glist);
    const GenSink sink{gm};
    const int t = threadIdx.x;
    unsigned long long created_cnt = 0;
    bool overflow = false, hbm = false;
    for (int q = t; q < MO_CLAIM; q += MO_THREADS) S.claim[q] = 0;
    if (t == 0) S.n_touched = 0;
    __syncthreads();
    for (int bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
        const int64_t b0 = (int64_t)O[(int64_t)bin * ntiles];
        const int64_t b1 = (int64_t)O[(int64_t)(bin + 1) * ntiles];   // (digit nbins: the gaps, after every bin)
        // 0. the bin's resident regions, their tags, the kSeg variant's segments
        if (t == 0) mo_resident_regions(S, C, bin, !rehash && b1 > b0, tag_bytes);
        if constexpr (kSeg) {
            for (int q = t; q < nseg; q += MO_THREADS) {
                seg_base[q] = SO[(int64_t)bin * nseg + q];
                seg_pre[q] = SP[(int64_t)bin * nseg + q];
            }
            if (t == 0) seg_pre[nseg] = (unsigned)(b1 - b0);
        }
        lds_barrier();
        const MoBin B{S, mo_tags, bin, b0, b1, S.n_res, seg_base, seg_pre, nseg};
        mo_fill_tags(B, t);
        lds_barrier();
        // software pipeline: the next chunk's record is loaded while this chunk is merged
        Rec nxt;
        // the bin's records: [b0, b1) of the partitioned array, or (slab != 0: k_ingest's fused binning) the first
        // b1 - b0 records of the bin's slab; either way row k of the bin goes to b0 + k
        const Rec *__restrict__ bp = slab ? parts + ((int64_t)bin * slab - b0) : parts;
        // EventRec: the next chunk's window parameters are loaded with the chunk's store drain, so that the record's
        // hash needs no dependent load at the chunk's start (state-read leg's merge -0.27 ms, bench leg unchanged:
        // profiles/r4/r4v7/)
        WInfo nwi{};
        if (b0 + t < b1) nxt = ld_stream(mo_rec_at<Rec, kSeg>(B, bp, b0 + t));
        if constexpr (kEv) { if (b0 + t < b1) nwi = winfo[ekey_widx(nxt.key)]; }
        for (int64_t c0 = b0; c0 < b1; c0 += MO_THREADS) {
            // 1. stage this chunk's records in LDS
            const int64_t i = c0 + t;
            const bool has = i < b1;
            MRec p{};
            if (has) {
                if constexpr (kEv) p = mrec_of_wi(nxt, nwi, cell_hi);
                else p = mrec_of(nxt, winfo, cell_hi);
            }
            if (i + MO_THREADS < b1) nxt = ld_stream(mo_rec_at<Rec, kSeg>(B, bp, i + MO_THREADS));
            if (has) mo_stage(S, t, p);
            lds_barrier();
            // 2. find and claim the key's slot, or join the lane that holds it
            MoProbe pr;
            if constexpr (kResident && kCoop) mo_probe_coop(B, p, has, t, pr);
            else if (has) mo_probe<kResident>(B, C, gm, p, t, pr);
            overflow |= pr.lost;
            hbm |= pr.hbm;
            TileSlot *const gslot = pr.gslot;
            const bool created = pr.created;
            // (one LDS add per created key: a ballot per resident region measured 0.17 ms slower on the bench, r4j/)
            if (created && pr.r >= 0) atomicAdd(&S.res_new[pr.r], 1u);
            // 3a. the claimed existing lines, loaded before the barrier (their slots' last stores were drained by an
            // earlier chunk's barrier, and no store of this chunk precedes step 4): the round trip overlaps the wait
            const MLine o = mo_old_line(S, t, pr);
            lds_barrier();
            // 3. the claimers' new lines (old values read above: the slot's last store is visible) and row indices
            MLine v{};
            const bool retouch = !rehash && gslot && !created && (unsigned)(o.touched >> 32) == seq;
            const bool first = !rehash && gslot && !retouch;
            // (the row index is absolute -- the bin's first row b0 + its touch order -- so that a later merge of the same
            // batch, whose segment of the bin starts elsewhere, rewrites the row in place: a pipelined batch's chunks)
            unsigned krow = (unsigned)b0 + mo_touch_rows(S, first);
            if (!first) krow = (unsigned)o.touched;
            if (gslot) v = mo_new_line<rehash>(S, t, p, o, first, seq, krow);
            // 4. this chunk's stores: the state line (whole) and the key's row
            mo_store_lines(S, t, gslot, p, v);
            if (gslot) {
                if (created) created_cnt++;
                if (!rehash) put_row(rows, (int64_t)krow, p.cell, p.we, v.count, v.nspeed, v.sspeed, v.slat, v.slon);
            }
            // created keys of non-resident windows count for their window here (resident ones: res_new); rehash:
            // the host already carries the moved keys
            if constexpr (!kResident) {
                const bool count_here = created && !rehash && pr.r < 0;
                if (__ballot(count_here) && !wave_count_windows(count_here, p.we, 1ull, WL, sink)) overflow = true;
            }
            if constexpr (kEv) { if (i + MO_THREADS < b1) nwi = winfo[ekey_widx(nxt.key)]; }
            // 5. drain this chunk's stores (visible to the next chunk's probes: a full barrier waits for every store of
            // the wave -- measured: draining them a chunk later instead, deferring the keys the previous chunk wrote,
            // cost 1.5 ms on the bench and 4.5 ms on the state-read leg); release the claims
            __syncthreads();
            if (pr.ci >= 0) MoClaimsOf<kResident>{(typename MoClaimsOf<kResident>::Key *)S.claim}.release(pr.ci);
        }
        lds_barrier();
        // 6. write the resident regions' tags back
        if (!mo_tags_writeback(B, gm, t)) overflow = true;
        if (t == 0) { bin_cnt[bin] = S.n_touched; S.n_touched = 0; }
        lds_barrier();
    }
    if (!wl_flush(WL, sink)) overflow = true;
    created_cnt = wave_sum(created_cnt);
    unsigned long long ov = __ballot(overflow);
    if (lane_id() == 0) {
        if (created_cnt) atomicAdd(&st->n_state_new, created_cnt);
        if (ov) atomicAdd(&st->overflow, 1ull);
    }
    // (hm_last_counts [12], bit 8: once per wave that had a record probe through HBM; growth always does, uncounted)
    if constexpr (!kResident && !rehash) { if (__ballot(hbm) && lane_id() == 0) atomicAdd(&st->merge_hbm, 1ull); }
}

// =====================================================================================================
// Housekeeping kernels of a batch: zeroing released window tables' tags, the start-of-batch reset
// =====================================================================================================
// zero n16 16-B words (the window tables' tag bytes on pool reuse: hipMemsetAsync's fill kernel ran at ~0.3 TB/s
// on these 64-MB ranges, 0.68 ms per batch)
__global__ __launch_bounds__(256) void k_zero16(uint4 *__restrict__ p, int64_t n16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
// up to ZR_MAX ranges in one launch (blockIdx.y = range): a batch's released tables
constexpr int ZR_MAX = 8;
struct ZeroRanges {
    uint4 *p[ZR_MAX];
    int64_t n16[ZR_MAX];
};
__global__ __launch_bounds__(256) void k_zero16_ranges(ZeroRanges r) {
    uint4 *__restrict__ p = r.p[blockIdx.y];
    const int64_t n16 = r.n16[blockIdx.y], stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// the start of a batch in one launch (was six memsets and a copy): the batch statistics (max ts / min window start
// at their identities), the fast-path exception and dedup give-up words, the window registry and its census
__global__ __launch_bounds__(256) void k_batch_reset(unsigned long long *__restrict__ st, unsigned long long *__restrict__ slow_word,
                                                     unsigned long long *__restrict__ giveup_word, unsigned long long *__restrict__ wreg2,
                                                     int n_wreg2, unsigned *__restrict__ bin_cur, int n_bin) {
    static_assert(sizeof(DevStats) % 8 == 0 && offsetof(DevStats, min_wstart) == offsetof(DevStats, max_ts_ms) + 8, "DevStats");
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_wreg2) wreg2[i] = 0;
    if (i < n_bin) bin_cur[i] = 0;
    if (i < (int)(sizeof(DevStats) / 8)) {
        const int mx = (int)(offsetof(DevStats, max_ts_ms) / 8);
        st[i] = i == mx ? (unsigned long long)INT64_MIN : i == mx + 1 ? (unsigned long long)INT64_MAX : 0ull;
    }
    if (i == 0) { *slow_word = 0; *giveup_word = 0; }
}

// =====================================================================================================
// K4: close the gaps between the bins' row segments: bin b's rows [O(b), O(b) + cnt[b]) -> [off[b], ...)
// =====================================================================================================
// In-place densification of the per-bin row segments: bin b's merged rows are [s_b, s_b + c_b) of the staging
// arrays (s_b = the bin's first partial, c_b its touched keys), so the rows [0, T) (T = sum c_b) are dense except
// for the gaps left by keys with several partials; each gap below T takes one row from above T (gap i <- the i-th
// row at or above T, both counted in bin order).  Moves only the ~2% gap rows instead of every row.
__global__ __launch_bounds__(256) void k_gap_counts(const unsigned long long *__restrict__ O, int64_t ntiles, int nbins,
                                                    const unsigned *__restrict__ cnt, const unsigned long long *__restrict__ T_ptr,
                                                    unsigned *__restrict__ g, unsigned *__restrict__ v) {
    const unsigned long long T = *T_ptr;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nbins; b += gridDim.x * blockDim.x) {
        const unsigned long long s = O[(int64_t)b * ntiles], e = O[(int64_t)(b + 1) * ntiles], c = cnt[b];
        const unsigned long long glo = s + c, ghi = e < T ? e : T;
        g[b] = ghi > glo ? (unsigned)(ghi - glo) : 0u;
        const unsigned long long vlo = s > T ? s : T, vhi = s + c;
        v[b] = vhi > vlo ? (unsigned)(vhi - vlo) : 0u;
    }
}
__global__ __launch_bounds__(256) void k_fill_gaps(RowsOut r, const unsigned long long *__restrict__ O, int64_t ntiles, int nbins,
                                                   const unsigned *__restrict__ cnt, const unsigned long long *__restrict__ T_ptr,
                                                   const unsigned *__restrict__ g, const unsigned long long *__restrict__ goff,
                                                   const unsigned long long *__restrict__ voff) {
    const unsigned long long T = *T_ptr;
    for (int b = blockIdx.x; b < nbins; b += gridDim.x) {
        const unsigned ng = g[b];
        if (!ng) continue;
        const unsigned long long dst0 = O[(int64_t)b * ntiles] + cnt[b], g0 = goff[b];
        int lo = -1;   // the donor bin: the last bin with voff <= i
        for (unsigned k = threadIdx.x; k < ng; k += blockDim.x) {
            const unsigned long long i = g0 + k;
            if (lo < 0) {   // a thread's first row: binary search (13 dependent loads)
                lo = 0;
                int hi = nbins;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (voff[mid] <= i) lo = mid; else hi = mid;
                }
            } else {        // i grows by blockDim.x per row: the donor bin moves forward a few bins at most
                while (lo + 1 < nbins && voff[lo + 1] <= i) lo++;
            }
            const unsigned long long sb = O[(int64_t)lo * ntiles];
            const int64_t src = (int64_t)((sb > T ? sb : T) + (i - voff[lo])), dst = (int64_t)(dst0 + k);
            r.cell[dst] = r.cell[src];
            r.ws[dst] = r.ws[src];
            r.cnt[dst] = r.cnt[src];
            r.sp[dst] = r.sp[src];
            r.spnull[dst] = r.spnull[src];
            r.lon[dst] = r.lon[src];
            r.lat[dst] = r.lat[src];
        }
    }
}
