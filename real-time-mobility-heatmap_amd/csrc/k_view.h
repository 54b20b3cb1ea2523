// Read side: a map viewport (west, south, east, north in degrees) applied on the device -- which cells' boundary boxes
// meet it (k_cells_in_view), the roll-up's records of those cells compacted (k_view_tiles), the positions state's
// records inside it (k_pos_emit_view).  The rule is DESIGN §5i's; nothing here has a tolerance.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// valid: all four finite, -90 <= south <= north <= 90, -180 <= west, east <= 180 (every comparison is false on a NaN)
HM_HD bool view_valid(const hm_view &v) {
    return v.south >= -90.0 && v.south <= v.north && v.north <= 90.0 && v.west >= -180.0 && v.west <= 180.0 &&
           v.east >= -180.0 && v.east <= 180.0;
}
// a set of longitudes: one closed interval, or two when it crosses the antimeridian
struct LngSet {
    double lo[2], hi[2];
    int n;
};
HM_HD LngSet view_lngs(const hm_view &v) {
    LngSet s;
    if (v.west <= v.east) {
        s.n = 1;
        s.lo[0] = v.west; s.hi[0] = v.east;
        s.lo[1] = v.west; s.hi[1] = v.east;
    } else {
        s.n = 2;
        s.lo[0] = v.west; s.hi[0] = 180.0;
        s.lo[1] = -180.0; s.hi[1] = v.east;
    }
    return s;
}
HM_HD bool lngs_meet(const LngSet &a, const LngSet &b) {
    for (int i = 0; i < a.n; i++)
        for (int j = 0; j < b.n; j++)
            if (a.lo[i] <= b.hi[j] && b.lo[j] <= a.hi[i]) return true;
    return false;
}
HM_HD bool point_in_view(double lat, double lon, const hm_view &v) {
    if (!(v.south <= lat && lat <= v.north)) return false;
    if (v.west <= v.east) return v.west <= lon && lon <= v.east;
    return (v.west <= lon && lon <= 180.0) || (-180.0 <= lon && lon <= v.east);
}
// the ring of nv vertices against the view: the latitude ranges intersect and the longitude sets meet.  A ring whose
// longitudes span more than 180 degrees wraps: its set is [the least positive one, 180] U [-180, the greatest of the
// others].  north_pole / south_pole: the ring's cell contains that pole (every longitude, latitudes up to the pole).
HM_HD bool ring_in_view(int nv, const double *lat, const double *lng, bool north_pole, bool south_pole, const hm_view &v) {
    if (nv <= 0) return false;
    double la0 = lat[0], la1 = lat[0], lo0 = lng[0], lo1 = lng[0];
    for (int k = 1; k < nv; k++) {
        la0 = lat[k] < la0 ? lat[k] : la0;
        la1 = lat[k] > la1 ? lat[k] : la1;
        lo0 = lng[k] < lo0 ? lng[k] : lo0;
        lo1 = lng[k] > lo1 ? lng[k] : lo1;
    }
    if (north_pole) la1 = 90.0;
    if (south_pole) la0 = -90.0;
    if (!(la0 <= v.north && v.south <= la1)) return false;
    LngSet r;
    r.n = 1;
    r.lo[0] = r.lo[1] = lo0;
    r.hi[0] = r.hi[1] = lo1;
    if (north_pole || south_pole) {
        r.lo[0] = r.lo[1] = -180.0;
        r.hi[0] = r.hi[1] = 180.0;
    } else if (lo1 - lo0 > 180.0) {
        double pos = 180.0, neg = -180.0;   // (both groups are non-empty: lo1 > 0 > lo0)
        for (int k = 0; k < nv; k++) {
            if (lng[k] > 0.0) pos = lng[k] < pos ? lng[k] : pos;
            else neg = lng[k] > neg ? lng[k] : neg;
        }
        r.n = 2;
        r.lo[0] = pos; r.hi[0] = 180.0;
        r.lo[1] = -180.0; r.hi[1] = neg;
    }
    return lngs_meet(r, view_lngs(v));
}
// the two cells of each resolution that contain a pole: latLngToCell(+-90, 0, res), computed once on the host
struct ViewPoles {
    uint64_t north[16], south[16];
};
// one cell against the view: its boundary once, then the rule; np / sp = the pole cells of the cell's resolution
HM_HD bool cell_in_view(uint64_t cell, const H3Tables &T, uint64_t np, uint64_t sp, const hm_view &v) {
    double la[10], lo[10];
    const int nv = cellToBoundaryDeg(cell, T, la, lo);
    return ring_in_view(nv, la, lo, cell == np, cell == sp, v);
}

// one thread per candidate cell (any mix of resolutions): a one-byte verdict
__global__ __launch_bounds__(256) void k_cells_in_view(const uint64_t *__restrict__ cells, int64_t n, ViewPoles poles, hm_view v,
                                                       uint8_t *__restrict__ keep) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t c = cells[i];
        const int res = (int)((c >> 52) & 0xf);
        keep[i] = cell_in_view(c, c_tab, poles.north[res], poles.south[res], v) ? 1 : 0;
    }
}

// the roll-up's n records (one resolution: its two pole cells as two words) whose cell is in view, compacted into out
// (room for n); *n_out counts them.  A thread tests its DUMP_PER records of the iteration one after the other (one copy
// of the boundary code) and keeps the verdicts as bits; block256_compact then asks the same thread for the same records.
// No reject ahead of the exact boundary: none was proved never to drop a tile the rule keeps.
// Rec: the record kept whole, GrowRec (every caller but one) or the change's pair of them (k_change.h); rec_cell gives
// its cell.
HM_HD uint64_t rec_cell(const GrowRec &r) { return r.cell; }
template <class Rec = GrowRec>
__global__ __launch_bounds__(256) void k_view_tiles(const Rec *__restrict__ recs, int64_t n, uint64_t north_pole,
                                                    uint64_t south_pole, hm_view v, Rec *__restrict__ out,
                                                    unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        unsigned bits = 0;
#pragma unroll 1
        for (int k = 0; k < DUMP_PER; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i < n && cell_in_view(rec_cell(recs[i]), c_tab, north_pole, south_pole, v)) bits |= 1u << k;
        }
        const auto is_live = [=](int64_t i) { return ((bits >> (unsigned)((i - base) >> 8)) & 1u) != 0; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)n,
                               [=](int64_t i, unsigned long long at) { out[at] = recs[i]; });
    }
}

// k_pos_emit with the point test: the pair table's live slots whose stored (lat, lon) lie in the view
__global__ __launch_bounds__(256) void k_pos_emit_view(const PosSlot *__restrict__ tab, int64_t nslots, hm_view v,
                                                       hm_position_rec *__restrict__ out, int64_t out_cap,
                                                       unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) {
            return i < nslots && tab[i].key != POS_EMPTY && point_in_view(tab[i].lat, tab[i].lon, v);
        };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            const PosSlot e = tab[i];
            hm_position_rec r;
            r.provider = (uint32_t)(e.key >> 32);
            r.vehicle = (uint32_t)e.key;
            r.ts_us = e.ts;
            r.lat = e.lat;
            r.lon = e.lon;
            out[at] = r;
        });
    }
}
