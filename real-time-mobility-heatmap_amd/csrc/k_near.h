// Read side: what is around a point, nearest first -- the great-circle distance of every position / tile centroid to a
// query point, the closed radius filter, and the compaction of the kept records with the two key words the top's select
// ranks them by (k_near_distances, k_pos_emit_near, k_near_tiles, k_near_vary, k_near_scatter).  The rule is DESIGN
// §5m's; nothing here has a tolerance.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// The distance (haversine on MongoDB's sphere), binary64, one rounding per operation in exactly this order (the
// translation unit is compiled with -ffp-contract=off):
//   D  = 0.017453292519943295          the double math.radians multiplies by
//   p0 = lat0 * D;  p1 = lat * D
//   s_h = sin((p1 - p0) * 0.5);  s_l = sin(((lon - lon0) * D) * 0.5);  c0 = cos(p0);  c1 = cos(p1)
//   a  = s_h * s_h + (c0 * c1) * (s_l * s_l)
//   r  = sqrt(a), clamped to 1;  d = (2 * HM_EARTH_RADIUS_M) * asin(r)
// sincos / asin are glibc's as restated in glibc_libm.h, sqrt the correctly rounded one.  The longitude difference is
// not normalised (sin^2 of its half is periodic).  d is +0.0 <= d <= pi R, or NaN when a coordinate is not finite (or
// a stored latitude lies so far outside [-90, 90] that a < 0).
// The order: nearest first, then key word 1 ascending (provider code << 32 | vehicle code, or the cell), then the
// candidate's index.  As the top's three-word key (k_top.h): word 0 = the bits of d -- non-negative doubles order as
// unsigned integers --, word 1 as above, word 2 the index; the select, the compaction of the selected and their ranks
// are the top's kernels unchanged.
// =====================================================================================================
constexpr double NEAR_DEG = 0.017453292519943295;
// what depends on the query point only: computed once per thread, not once per candidate
struct NearPoint { double p0, c0, lon0; };
HM_HD NearPoint near_point(double lat0, double lon0, const glm::Tables &G) {
    NearPoint q;
    double s0;
    q.p0 = lat0 * NEAR_DEG;
    glm::sincos(q.p0, s0, q.c0, G);
    q.lon0 = lon0;
    return q;
}
HM_HD double near_distance_m(const NearPoint &q, double lat, double lon, const glm::Tables &G) {
    const double p1 = lat * NEAR_DEG;
    double s_h, s_l, s1, c1, unused;
    glm::sincos((p1 - q.p0) * 0.5, s_h, unused, G);
    glm::sincos(((lon - q.lon0) * NEAR_DEG) * 0.5, s_l, unused, G);
    glm::sincos(p1, s1, c1, G);
    const double a = s_h * s_h + (q.c0 * c1) * (s_l * s_l);
    double r = sqrt(a);
    if (r > 1.0) r = 1.0;
    return (2.0 * HM_EARTH_RADIUS_M) * glm::asin(r, G);
}
HM_HD double near_distance_m(double lat0, double lon0, double lat, double lon, const glm::Tables &G) {
    return near_distance_m(near_point(lat0, lon0, G), lat, lon, G);
}
// valid: lat in [-90, 90], lon in [-180, 180], max_distance_m >= 0 or +inf (every comparison is false on a NaN)
HM_HD bool near_valid(const hm_near &q) {
    return q.lat >= -90.0 && q.lat <= 90.0 && q.lon >= -180.0 && q.lon <= 180.0 && q.max_distance_m >= 0.0;
}
HM_HD unsigned long long near_bits(double d) {
    union { double f; unsigned long long u; } v;
    v.f = d;
    return v.u;
}
// a tile's point: its centroid as the sink writes it, one division each, ahead of the distance
HM_HD double near_centroid(double sum, unsigned long long count) { return sum / (double)count; }

// words of the near's control block (device; zeroed before every scan)
enum { NW_SCANNED = 0, NW_SINCE, NW_NAN, NW_OUT, NW_WORDS };

// d[i] of caller coordinates: the numerics' own entry point
__global__ __launch_bounds__(256) void k_near_distances(hm_near q, const double *__restrict__ lat, const double *__restrict__ lon,
                                                        int64_t n, double *__restrict__ dist) {
    const NearPoint pt = near_point(q.lat, q.lon, g_glm);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dist[i] = near_distance_m(pt, lat[i], lon[i], g_glm);
}

// a workgroup's three counters into the control block: one atomic each (every thread of the 256 calls this once)
__device__ __forceinline__ void near_flush_counts(unsigned long long scanned, unsigned long long since, unsigned long long nan,
                                                  unsigned long long *words) {
    __shared__ unsigned long long part[4][3];
    scanned = wave_sum(scanned);
    since = wave_sum(since);
    nan = wave_sum(nan);
    if (lane_id() == 0) {
        part[threadIdx.x >> 6][0] = scanned;
        part[threadIdx.x >> 6][1] = since;
        part[threadIdx.x >> 6][2] = nan;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(&words[NW_SCANNED + threadIdx.x], v);
    }
}

// k_pos_emit_view's scan of the pair table with the live test key != POS_EMPTY && ts >= since && d == d && d <= max: the
// kept slots as hm_position_rec with their key words 0 (the bits of d) and 1 (the pair key), compacted (room for
// out_cap each; words[NW_OUT] counts them).  A thread computes the distances of its DUMP_PER slots of the iteration one
// after the other (one copy of the libm code), keeps the verdicts as bits and the distances in LDS; block256_compact
// then asks the same thread for the same slots.  No reject ahead of the exact distance.
__global__ __launch_bounds__(256) void k_pos_emit_near(const PosSlot *__restrict__ tab, int64_t nslots, hm_near q, long long since,
                                                       hm_position_rec *__restrict__ out, unsigned long long *__restrict__ k0,
                                                       unsigned long long *__restrict__ k1, int64_t out_cap,
                                                       unsigned long long *words) {
    __shared__ double sd[DUMP_PER][256];
    const NearPoint pt = near_point(q.lat, q.lon, g_glm);
    const int64_t tile = 256 * DUMP_PER;
    unsigned long long scanned = 0, kept_since = 0, nan = 0;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        unsigned bits = 0;
#pragma unroll 1
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i >= nslots) continue;
            scanned++;
            const PosSlot e = tab[i];
            if (e.key == POS_EMPTY) continue;
            if (!(e.ts >= since)) continue;
            kept_since++;
            const double d = near_distance_m(pt, e.lat, e.lon, g_glm);
            if (d != d) { nan++; continue; }
            if (d <= q.max_distance_m) {
                bits |= 1u << k;
                sd[k][threadIdx.x] = d;
            }
        }
        const auto is_live = [=](int64_t i) { return ((bits >> (unsigned)((i - base) >> 8)) & 1u) != 0; };
        block256_compact<true>(base, is_live, words + NW_OUT, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            const PosSlot e = tab[i];
            hm_position_rec r;
            r.provider = (uint32_t)(e.key >> 32);
            r.vehicle = (uint32_t)e.key;
            r.ts_us = e.ts;
            r.lat = e.lat;
            r.lon = e.lon;
            out[at] = r;
            k0[at] = near_bits(sd[(i - base) >> 8][threadIdx.x]);
            k1[at] = e.key;
        });
    }
    near_flush_counts(scanned, kept_since, nan, words);
}

// the same over the roll-up's n records: centroid, distance, filter, the record whole with its key words 0 (the bits
// of d) and 1 (the cell), compacted (room for n each)
__global__ __launch_bounds__(256) void k_near_tiles(const GrowRec *__restrict__ recs, int64_t n, hm_near q, GrowRec *__restrict__ out,
                                                    unsigned long long *__restrict__ k0, unsigned long long *__restrict__ k1,
                                                    unsigned long long *words) {
    __shared__ double sd[DUMP_PER][256];
    const NearPoint pt = near_point(q.lat, q.lon, g_glm);
    const int64_t tile = 256 * DUMP_PER;
    unsigned long long scanned = 0, nan = 0;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        unsigned bits = 0;
#pragma unroll 1
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i >= n) continue;
            scanned++;
            const unsigned long long c = recs[i].count;
            const double d = near_distance_m(pt, near_centroid(recs[i].slat, c), near_centroid(recs[i].slon, c), g_glm);
            if (d != d) { nan++; continue; }
            if (d <= q.max_distance_m) {
                bits |= 1u << k;
                sd[k][threadIdx.x] = d;
            }
        }
        const auto is_live = [=](int64_t i) { return ((bits >> (unsigned)((i - base) >> 8)) & 1u) != 0; };
        block256_compact<true>(base, is_live, words + NW_OUT, (unsigned long long)n, [=](int64_t i, unsigned long long at) {
            out[at] = recs[i];
            k0[at] = near_bits(sd[(i - base) >> 8][threadIdx.x]);
            k1[at] = recs[i].cell;
        });
    }
    near_flush_counts(scanned, scanned, nan, words);
}

// the OR of the candidates' two key words and of their complements into words[TW_OR_C .. TW_NAND_CELL] (k_top_keys'
// reduction over keys that exist already): the bytes that vary are the select's plan
__global__ __launch_bounds__(256) void k_near_vary(const unsigned long long *__restrict__ k0, const unsigned long long *__restrict__ k1,
                                                   int64_t n, unsigned long long *words) {
    __shared__ unsigned long long part[4][4];
    unsigned long long r[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned long long c = k0[i], l = k1[i];
        r[0] |= c;
        r[1] |= ~c;
        r[2] |= l;
        r[3] |= ~l;
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        for (int o = 32; o > 0; o >>= 1) r[q] |= __shfl_xor(r[q], o, 64);
    if (lane_id() == 0)
        for (int q = 0; q < 4; q++) part[threadIdx.x >> 6][q] = r[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][threadIdx.x] | part[1][threadIdx.x] | part[2][threadIdx.x] | part[3][threadIdx.x];
        if (v) atomicOr(&words[TW_OR_C + threadIdx.x], v);
    }
}

// out[rank[j]] = recs[sidx[j]], whole: Q lanes per record of Q 16-byte quarters (2: hm_position_rec, 4: GrowRec), and
// dist[rank[j]] = the distance whose bits are key word 0 (a stale index or rank writes nothing)
template <int Q>
__global__ __launch_bounds__(256) void k_near_scatter(const uint4 *__restrict__ recs, int64_t n, const unsigned long long *__restrict__ k0,
                                                      const unsigned *__restrict__ sidx, const unsigned *__restrict__ rank, int m,
                                                      uint4 *__restrict__ out, unsigned long long *__restrict__ dist) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)m * Q; t += (int64_t)gridDim.x * 256) {
        const int64_t j = t / Q;
        const int part = (int)(t % Q);
        const unsigned src = sidx[j], r = rank[j];
        if ((int64_t)src < n && r < (unsigned)m) {
            out[(int64_t)r * Q + part] = recs[(int64_t)src * Q + part];
            if (part == 0) dist[r] = k0[src];
        }
    }
}
