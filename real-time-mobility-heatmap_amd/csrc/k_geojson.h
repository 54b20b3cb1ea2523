// Read side: the GeoJSON response bodies of /api/tiles/latest and /api/positions/latest (geojson_docs.h), two kernels each:
// sizes -> (k_scan_blocks / k_cp_scan / k_scan_add) -> write.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
//
// Body layout (both): bytes[0, 40) = {"type":"FeatureCollection","features":[ ; feature i = bytes[off[i], off[i+1] - 1),
// followed by one ',' -- the last one by ']' -- and '}' at off[n].  The scan runs over n + 1 sizes, the prefix's 40
// first, so that its output is 0 | off[0..n] and the caller's offsets start at its second entry.
#pragma once

constexpr int GJ_THREADS = 64;   // k_gj_tile_write's workgroup: its LDS holds GJ_THREADS x (the launch's longest feature),
                                 // <= 64 x 872 B = 55 KB; typical res-8 features (~520 B) leave room for 4 workgroups per CU
enum { GJW_MAX = 0, GJW_BAD, GJW_OUT, GJW_BUCKETS, GJW_WORDS };   // the encoder's device words

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)v, o);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ GjBase gj_base_of(const GrowRec &b) { return GjBase{(int64_t)b.count, (int64_t)b.nspeed, b.sspeed}; }

// pass 1: the cell's boundary, once per feature (kept for pass 2: vertex k of feature i at vlat / vlng[k * n + i]), and the
// feature's size with its separator; sizes[0] = the prefix.  rstride: record i at recs[i * rstride] (1; 2: the cur halves
// of the change's pairs, with_base then takes the next GrowRec as the feature's base, k_change.h).  series (optional):
// record i's `windows` counts at series[i * windows] (a span's records, k_span.h)
__global__ __launch_bounds__(256) void k_gj_tile_sizes(GjTexts T, const GrowRec *__restrict__ recs, int64_t n,
                                                       double *__restrict__ vlat, double *__restrict__ vlng,
                                                       int *__restrict__ vn, unsigned *__restrict__ sizes,
                                                       unsigned long long *words, const double *__restrict__ dist_m = nullptr,
                                                       int rstride = 1, bool with_base = false,
                                                       const int64_t *__restrict__ series = nullptr, int windows = 0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const GrowRec r = recs[i * rstride];
        GjBase gb = {0, 0, 0.0};
        if (with_base) gb = gj_base_of(recs[i * rstride + 1]);
        double la[10], lo[10];
        const int nv = cellToBoundaryDeg(r.cell, c_tab, la, lo);
        vn[i] = nv;
        for (int k = 0; k < 10; k++) {
            vlat[(int64_t)k * n + i] = k < nv ? la[k] : 0.0;
            vlng[(int64_t)k * n + i] = k < nv ? lo[k] : 0.0;
        }
        const GjSpan gs = {windows, series ? series + i * windows : nullptr};
        const unsigned sz = (unsigned)tile_feature(nullptr, T, r.cell, (int64_t)r.count, (int64_t)r.nspeed, r.sspeed, nv, la, lo, 1,
                                                    dist_m ? dist_m + i : nullptr, with_base ? &gb : nullptr, series ? &gs : nullptr) + 1u;
        sizes[i + 1] = sz;
        mx = sz > mx ? sz : mx;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[0] = GJ_PREFIX_LEN;
    mx = wave_max_u32(mx);
    if (mx && lane_id() == 0) atomicMax(&words[GJW_MAX], (unsigned long long)mx);
}

// pass 2: each thread writes its feature into LDS at its final offset relative to the workgroup's first byte (shifted so
// that LDS and HBM agree modulo 16), then the workgroup stores its contiguous byte range with 16-B stores, bytes at
// the two edge lines (k_tile_docs' scheme).  off = the scan's output: off[0] = 0, feature i at off[i + 1].
__global__ __launch_bounds__(GJ_THREADS) void k_gj_tile_write(GjTexts T, const GrowRec *__restrict__ recs, int64_t n,
                                                              const double *__restrict__ vlat, const double *__restrict__ vlng,
                                                              const int *__restrict__ vn,
                                                              const unsigned long long *__restrict__ off,
                                                              uint8_t *__restrict__ out, const double *__restrict__ dist_m = nullptr,
                                                              int rstride = 1, bool with_base = false,
                                                              const int64_t *__restrict__ series = nullptr, int windows = 0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gj_buf[];   // GJ_THREADS x (the longest feature) + 64
    for (int64_t b0 = (int64_t)blockIdx.x * GJ_THREADS; b0 < n; b0 += (int64_t)gridDim.x * GJ_THREADS) {
        const int64_t b1 = b0 + GJ_THREADS < n ? b0 + GJ_THREADS : n;
        // the workgroup's bytes: its features, the prefix before the first one, the '}' after the last one
        const unsigned long long first = b0 == 0 ? 0ull : off[b0 + 1], last = off[b1 + 1] + (b1 == n ? 1ull : 0ull);
        const unsigned long long base = first & ~15ull;
        const int64_t i = b0 + threadIdx.x;
        if (i < b1) {
            const GrowRec r = recs[i * rstride];
            GjBase gb = {0, 0, 0.0};
            if (with_base) gb = gj_base_of(recs[i * rstride + 1]);
            uint8_t *at = gj_buf + (off[i + 1] - base);
            const GjSpan gs = {windows, series ? series + i * windows : nullptr};
            const int len = tile_feature(at, T, r.cell, (int64_t)r.count, (int64_t)r.nspeed, r.sspeed, vn[i], vlat + i, vlng + i, n,
                                         dist_m ? dist_m + i : nullptr, with_base ? &gb : nullptr, series ? &gs : nullptr);
            at[len] = i == n - 1 ? ']' : ',';
        }
        if (threadIdx.x == 0) {
            if (b0 == 0) {
                const char *pre = HM_GJ_PREFIX;
                for (int q = 0; q < GJ_PREFIX_LEN; q++) gj_buf[q] = (uint8_t)pre[q];
            }
            if (b1 == n) gj_buf[last - 1 - base] = '}';
        }
        __syncthreads();
        const unsigned long long endb = last - base;
        const unsigned long long nlines = (endb + 15) >> 4;
        for (unsigned long long L = threadIdx.x; L < nlines; L += GJ_THREADS) {
            const unsigned long long s = L << 4;
            if (s >= first - base && s + 16 <= endb) {
                *(uint4 *)(out + base + s) = *(const uint4 *)(gj_buf + s);
            } else {
                for (int k = 0; k < 16; k++) {
                    const unsigned long long x = s + k;
                    if (x >= first - base && x < endb) out[base + x] = gj_buf[x];
                }
            }
        }
        __syncthreads();
    }
}

// ---- positions ----
struct PosFeatParams {
    const unsigned long long *p_off;   // the persistent dictionaries (hm_ctx::PosDict): span of each code in its arena
    const unsigned *p_len;
    const uint8_t *p_arena;
    const unsigned long long *v_off;
    const unsigned *v_len;
    const uint8_t *v_arena;
    int64_t n_p, n_v;
    int64_t n_buckets;                 // 900-s buckets, ascending, and the local offset (s) of each
    const int64_t *bucket_id;
    const int64_t *bucket_off;
};

// the local offset of ts_us's 900-s bucket; false: the bucket is absent
HM_HD bool gj_bucket_offset(const int64_t *ids, const int64_t *offs, int64_t nb, int64_t ts_us, int64_t &off_s) {
    const int64_t b = floordiv(floordiv(ts_us, 1000000), 900);
    int64_t lo = 0, hi = nb;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nb || ids[lo] != b) return false;
    off_s = offs[lo];
    return true;
}

// one record's feature (dst nullptr: its size), -1: codes outside the dictionaries, bucket absent, bad UTF-8, year range
__device__ __forceinline__ int gj_position(uint8_t *dst, const PosFeatParams &P, const hm_position_rec &r, const double *dist_m) {
    if ((int64_t)r.provider >= P.n_p || (int64_t)r.vehicle >= P.n_v) return -1;
    int64_t off_s;
    if (!gj_bucket_offset(P.bucket_id, P.bucket_off, P.n_buckets, r.ts_us, off_s)) return -1;
    return position_feature(dst, P.p_arena + P.p_off[r.provider], (int)P.p_len[r.provider], P.v_arena + P.v_off[r.vehicle],
                            (int)P.v_len[r.vehicle], r.ts_us, off_s, r.lat, r.lon, dist_m);
}

__global__ __launch_bounds__(256) void k_gj_pos_sizes(PosFeatParams P, const hm_position_rec *__restrict__ recs, int64_t n,
                                                      unsigned *__restrict__ sizes, unsigned long long *words,
                                                      const double *__restrict__ dist_m = nullptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int len = gj_position(nullptr, P, recs[i], dist_m ? dist_m + i : nullptr);
        if (len < 0) atomicAdd(&words[GJW_BAD], 1ull);
        sizes[i + 1] = len < 0 ? 1u : (unsigned)len + 1u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[0] = GJ_PREFIX_LEN;
}
// (one thread per feature straight to HBM, as k_pos_docs: the strings make the lengths vary widely; runs only when
// k_gj_pos_sizes found no bad record)
__global__ __launch_bounds__(256) void k_gj_pos_write(PosFeatParams P, const hm_position_rec *__restrict__ recs, int64_t n,
                                                      const unsigned long long *__restrict__ off, uint8_t *__restrict__ out,
                                                      const double *__restrict__ dist_m = nullptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint8_t *at = out + off[i + 1];
        const int len = gj_position(at, P, recs[i], dist_m ? dist_m + i : nullptr);
        if (len < 0) continue;
        at[len] = i == n - 1 ? ']' : ',';
        if (i == n - 1) at[len + 1] = '}';
        if (i == 0) {
            const char *pre = HM_GJ_PREFIX;
            for (int q = 0; q < GJ_PREFIX_LEN; q++) out[q] = (uint8_t)pre[q];
        }
    }
}

// the distinct 900-s buckets of the positions state's ts (k_latest_buckets' reduction over the pair table's live slots)
__global__ __launch_bounds__(256) void k_gj_pos_buckets(const PosSlot *__restrict__ tab, int64_t nslots, long long *set,
                                                        unsigned long long mask, long long *list, unsigned long long *n_list) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += stride)
        if (tab[i].key != POS_EMPTY) bucket_set_add(tab[i].ts, set, mask, list, n_list);
}
