// Read side: polygon geofences -- which zones of a zone set contain a point, for caller points (k_points_in_zones), the
// positions state (k_pos_within) and the roll-up's records by their centroid (k_within_tiles): the kept records compacted
// with the lowest containing zone as their label, and per-zone totals.  The rule is DESIGN §5n's; nothing here has a
// tolerance.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// The rule.  A zone is a set of rings, edges straight in the (lon, lat) plane; a point is in the zone iff it crosses an
// odd number of the zone's edges (all rings together: holes need no case).  An edge is packed in its canonical
// direction a.lat <= b.lat (both coordinates swapped otherwise), with the two differences that depend on the edge alone:
//   w = b.lon - a.lon;  h = b.lat - a.lat            (binary64, one rounding each, on the host)
//   crossed = (a.lat <= lat) && (lat < b.lat) && (w * (lat - a.lat) > (lon - a.lon) * h)
// every operation rounded once in this order (-ffp-contract=off).  A horizontal edge (a.lat == b.lat) is never crossed:
// its half-open range is empty, so it needs no case either.  A NaN coordinate makes every comparison false.
// =====================================================================================================
HM_HD bool edge_crossed(double alat, double blat, double alon, double w, double h, double lat, double lon) {
    const bool straddles = (alat <= lat) && (lat < blat);
    return straddles && (w * (lat - alat) > (lon - alon) * h);
}

// A packed zone set in device (or, for the host execution, host) memory: n_edges edges as five arrays, zone z's edges
// [eoff[z], eoff[z + 1]) with its box: every edge has zmin <= a.lat, b.lat <= zmax and a.lon, b.lon <= zlon.
struct ZoneSet {
    int n_zones, n_edges;
    const double *alat, *blat, *alon, *w, *h;
    const double *zmin, *zmax, *zlon;
    const int *eoff;
};
// The rejects ahead of a zone's edges (DESIGN §5n proves that a rejected point crosses none of them):
//   lat outside [zmin, zmax): no edge's half-open range holds it;  lon > zlon: w * t <= u * h by monotone rounding.
HM_HD bool zone_box_may_hold(double zmin, double zmax, double zlon, double lat, double lon) {
    return (zmin <= lat) && (lat < zmax) && (lon <= zlon);
}
// host execution of the rule, no reject: the lowest zone that contains the point (-1: none) and how many do
static inline void zones_of_point_host(const ZoneSet &zs, double lat, double lon, int &first, unsigned &hits) {
    first = -1;
    hits = 0;
    for (int z = 0; z < zs.n_zones; z++) {
        unsigned par = 0;
        for (int e = zs.eoff[z]; e < zs.eoff[z + 1]; e++)
            par ^= edge_crossed(zs.alat[e], zs.blat[e], zs.alon[e], zs.w[e], zs.h[e], lat, lon) ? 1u : 0u;
        if (par) {
            hits++;
            if (first < 0) first = z;
        }
    }
}

constexpr int WITHIN_STAGE = 512;    // edges a workgroup holds in LDS at a time (5 doubles each: 20 KB)
constexpr int WITHIN_ZLDS = 1024;    // zones whose totals a workgroup accumulates in LDS (more: straight to memory)
struct WithinStage {
    double alat[WITHIN_STAGE], blat[WITHIN_STAGE], alon[WITHIN_STAGE], w[WITHIN_STAGE], h[WITHIN_STAGE];
};

// The workgroup's 256 x P points (P per thread, in registers) against every zone: first[p] = the lowest zone that
// contains point p (-1: none), hits[p] = how many do; hit(p, z) is called once per containing zone.  The edges reach the
// lanes from LDS, WITHIN_STAGE at a time, read at wave-uniform addresses (a broadcast; a zone's description through
// wave-uniform loads); a zone whose edges span two stages keeps its parity bits across them.  A wave skips the edges of
// a zone whose box rejects all of its points.  Every thread of the workgroup calls this together (barriers inside).
template <int P, class Hit>
__device__ __forceinline__ void zones_classify(const ZoneSet &zs, WithinStage &S, const double (&lat)[P], const double (&lon)[P],
                                               int (&first)[P], unsigned (&hits)[P], Hit hit) {
#pragma unroll
    for (int p = 0; p < P; p++) {
        first[p] = -1;
        hits[p] = 0;
    }
    unsigned par = 0;   // bit p: point p has crossed an odd number of the current zone's edges so far
    int z = 0;
    for (int s0 = 0; s0 < zs.n_edges; s0 += WITHIN_STAGE) {
        const int s1 = min(s0 + WITHIN_STAGE, zs.n_edges);
        __syncthreads();   // (the previous stage's readers are done)
        for (int e = s0 + (int)threadIdx.x; e < s1; e += 256) {
            S.alat[e - s0] = zs.alat[e];
            S.blat[e - s0] = zs.blat[e];
            S.alon[e - s0] = zs.alon[e];
            S.w[e - s0] = zs.w[e];
            S.h[e - s0] = zs.h[e];
        }
        __syncthreads();
        while (z < zs.n_zones && zs.eoff[z] < s1) {
            const int zend = zs.eoff[z + 1];
            const int e0 = max(zs.eoff[z], s0) - s0, e1 = min(zend, s1) - s0;
            const double zmin = zs.zmin[z], zmax = zs.zmax[z], zlon = zs.zlon[z];
            bool may = false;
#pragma unroll
            for (int p = 0; p < P; p++) may |= zone_box_may_hold(zmin, zmax, zlon, lat[p], lon[p]);
            if (__any(may)) {
                for (int e = e0; e < e1; e++) {
                    const double alat = S.alat[e], blat = S.blat[e], alon = S.alon[e], w = S.w[e], h = S.h[e];
#pragma unroll
                    for (int p = 0; p < P; p++) par ^= (edge_crossed(alat, blat, alon, w, h, lat[p], lon[p]) ? 1u : 0u) << p;
                }
            }
            if (zend > s1) break;   // the zone goes on in the next stage
            if (par) {
#pragma unroll
                for (int p = 0; p < P; p++)
                    if ((par >> p) & 1u) {
                        hits[p]++;
                        if (first[p] < 0) first[p] = z;
                        hit(p, z);
                    }
            }
            par = 0;
            z++;
        }
    }
}

// first[i] / hits[i] of caller points: the numerics' own entry point
__global__ __launch_bounds__(256) void k_points_in_zones(ZoneSet zs, const double *__restrict__ lat, const double *__restrict__ lon, int64_t n,
                                                         int *__restrict__ first_out, unsigned *__restrict__ hits_out) {
    __shared__ WithinStage S;
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        double la[DUMP_PER], lo[DUMP_PER];
        int first[DUMP_PER];
        unsigned hits[DUMP_PER];
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            la[k] = i < n ? lat[i] : NAN;
            lo[k] = i < n ? lon[i] : NAN;
        }
        zones_classify<DUMP_PER>(zs, S, la, lo, first, hits, [](int, int) {});
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i < n) {
                first_out[i] = first[k];
                hits_out[i] = hits[k];
            }
        }
    }
}

// Per-zone totals on the device: WT_WORDS words per zone -- n, the summed count, the summed n_speed, sum_speed (the bits
// of a double, added as one), the newest ts_us as wenc_of (unsigned order = signed order; 0 = INT64_MIN = none), 0 --
// zeroed before every scan; the host turns them into hm_zone_rec.
enum { WT_N = 0, WT_COUNT, WT_NSPEED, WT_SSPEED, WT_NEWEST, WT_RESERVED, WT_WORDS };
static_assert(WT_WORDS * 8 == sizeof(hm_zone_rec), "a zone's device totals mirror hm_zone_rec");
// words of the within's control block (device; zeroed before every scan): near_flush_counts' three, then the compaction's
enum { WW_SCANNED = 0, WW_SINCE, WW_IN, WW_OUT, WW_WORDS };
static_assert(WW_SCANNED == NW_SCANNED && WW_IN == NW_NAN && WW_OUT == NW_OUT, "near_flush_counts writes words 0..2");

// The pair table's live slots with ts >= since against the zones (k_pos_emit_view's scan): those in at least one zone as
// hm_position_rec with their label, compacted (out == nullptr: totals only; room for out_cap, words[WW_OUT] counts
// them), and every containing zone's n and newest ts_us.  A slot that is free or too old enters as a NaN point: in no zone.
__global__ __launch_bounds__(256) void k_pos_within(const PosSlot *__restrict__ tab, int64_t nslots, ZoneSet zs, long long since,
                                                    hm_position_rec *__restrict__ out, int *__restrict__ zone, int64_t out_cap,
                                                    unsigned long long *tot, unsigned long long *words) {
    __shared__ WithinStage S;
    __shared__ int s_first[DUMP_PER][256];
    __shared__ unsigned long long s_tot[WITHIN_ZLDS][2];   // n, newest
    const bool tot_lds = zs.n_zones <= WITHIN_ZLDS;
    if (tot_lds)
        for (int z = threadIdx.x; z < zs.n_zones; z += 256) s_tot[z][0] = s_tot[z][1] = 0;
    const int64_t tile = 256 * DUMP_PER;
    unsigned long long scanned = 0, kept_since = 0, in_zone = 0;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        double la[DUMP_PER], lo[DUMP_PER];
        int first[DUMP_PER];
        unsigned hits[DUMP_PER];
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            la[k] = lo[k] = NAN;
            if (i >= nslots) continue;
            scanned++;
            const PosSlot e = tab[i];
            if (e.key == POS_EMPTY || !(e.ts >= since)) continue;
            kept_since++;
            la[k] = e.lat;
            lo[k] = e.lon;
        }
        zones_classify<DUMP_PER>(zs, S, la, lo, first, hits, [&](int p, int z) {
            const unsigned long long ts = wenc_of(tab[base + p * 256 + threadIdx.x].ts);
            if (tot_lds) {
                atomicAdd(&s_tot[z][0], 1ull);
                atomicMax(&s_tot[z][1], ts);
            } else {
                atomicAdd(&tot[(int64_t)z * WT_WORDS + WT_N], 1ull);
                atomicMax(&tot[(int64_t)z * WT_WORDS + WT_NEWEST], ts);
            }
        });
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            s_first[k][threadIdx.x] = first[k];
            if (first[k] >= 0) {
                bits |= 1u << k;
                in_zone++;
            }
        }
        if (out) {
            const auto is_live = [=](int64_t i) { return ((bits >> (unsigned)((i - base) >> 8)) & 1u) != 0; };
            block256_compact<true>(base, is_live, words + WW_OUT, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
                const PosSlot e = tab[i];
                hm_position_rec r;
                r.provider = (uint32_t)(e.key >> 32);
                r.vehicle = (uint32_t)e.key;
                r.ts_us = e.ts;
                r.lat = e.lat;
                r.lon = e.lon;
                out[at] = r;
                zone[at] = s_first[(i - base) >> 8][threadIdx.x];
            });
        }
    }
    near_flush_counts(scanned, kept_since, in_zone, words);   // (its barrier: every thread's LDS totals are in)
    if (tot_lds)
        for (int z = threadIdx.x; z < zs.n_zones; z += 256)
            if (s_tot[z][0]) {
                atomicAdd(&tot[(int64_t)z * WT_WORDS + WT_N], s_tot[z][0]);
                atomicMax(&tot[(int64_t)z * WT_WORDS + WT_NEWEST], s_tot[z][1]);
            }
}

// The same over the roll-up's n records by their centroid (near_centroid): those in at least one zone whole with their
// label, compacted (out == nullptr: totals only; room for n), and every containing zone's n, count, n_speed and sum_speed
// (an fp64 sum in atomic order).
struct WithinTileTot {
    unsigned long long n, count, nspeed;
    double sspeed;
};
__global__ __launch_bounds__(256) void k_within_tiles(const GrowRec *__restrict__ recs, int64_t n, ZoneSet zs, GrowRec *__restrict__ out,
                                                      int *__restrict__ zone, unsigned long long *tot, unsigned long long *words) {
    __shared__ WithinStage S;
    __shared__ int s_first[DUMP_PER][256];
    __shared__ WithinTileTot s_tot[WITHIN_ZLDS];
    const bool tot_lds = zs.n_zones <= WITHIN_ZLDS;
    if (tot_lds)
        for (int z = threadIdx.x; z < zs.n_zones; z += 256) {
            s_tot[z].n = s_tot[z].count = s_tot[z].nspeed = 0;
            s_tot[z].sspeed = 0.0;
        }
    const int64_t tile = 256 * DUMP_PER;
    unsigned long long scanned = 0, in_zone = 0;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        double la[DUMP_PER], lo[DUMP_PER];
        int first[DUMP_PER];
        unsigned hits[DUMP_PER];
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            la[k] = lo[k] = NAN;
            if (i >= n) continue;
            scanned++;
            const unsigned long long c = recs[i].count;
            la[k] = near_centroid(recs[i].slat, c);
            lo[k] = near_centroid(recs[i].slon, c);
        }
        zones_classify<DUMP_PER>(zs, S, la, lo, first, hits, [&](int p, int z) {
            const GrowRec &r = recs[base + p * 256 + threadIdx.x];
            const unsigned long long c = r.count, ns = r.nspeed;
            const double ss = r.sspeed;
            if (tot_lds) {
                atomicAdd(&s_tot[z].n, 1ull);
                atomicAdd(&s_tot[z].count, c);
                if (ns) {
                    atomicAdd(&s_tot[z].nspeed, ns);
                    atomicAdd(&s_tot[z].sspeed, ss);
                }
            } else {
                unsigned long long *t = tot + (int64_t)z * WT_WORDS;
                atomicAdd(&t[WT_N], 1ull);
                atomicAdd(&t[WT_COUNT], c);
                if (ns) {
                    atomicAdd(&t[WT_NSPEED], ns);
                    atomicAdd((double *)&t[WT_SSPEED], ss);
                }
            }
        });
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < DUMP_PER; k++) {
            s_first[k][threadIdx.x] = first[k];
            if (first[k] >= 0) {
                bits |= 1u << k;
                in_zone++;
            }
        }
        if (out) {
            const auto is_live = [=](int64_t i) { return ((bits >> (unsigned)((i - base) >> 8)) & 1u) != 0; };
            block256_compact<true>(base, is_live, words + WW_OUT, (unsigned long long)n, [=](int64_t i, unsigned long long at) {
                out[at] = recs[i];
                zone[at] = s_first[(i - base) >> 8][threadIdx.x];
            });
        }
    }
    near_flush_counts(scanned, scanned, in_zone, words);   // (its barrier: every thread's LDS totals are in)
    if (tot_lds)
        for (int z = threadIdx.x; z < zs.n_zones; z += 256)
            if (s_tot[z].n) {
                unsigned long long *t = tot + (int64_t)z * WT_WORDS;
                atomicAdd(&t[WT_N], s_tot[z].n);
                atomicAdd(&t[WT_COUNT], s_tot[z].count);
                if (s_tot[z].nspeed) {
                    atomicAdd(&t[WT_NSPEED], s_tot[z].nspeed);
                    atomicAdd((double *)&t[WT_SSPEED], s_tot[z].sspeed);
                }
            }
}
