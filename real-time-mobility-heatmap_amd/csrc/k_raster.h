// Read side: one live window as a raster -- a pixel's value is the count of the roll-up record whose hexagon contains the
// pixel's centre (k_raster + k_raster_exact).  The grid is separable: lat[rows] x lon[cols] in degrees, pixel (r, c) at
// r * cols + c; the caller projects (mobheat/readside.py tile_grid for slippy-map tiles), the device never does.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// A pixel's cell is latLngToCell(lat[r], lon[c], res) at the roll-up's resolution -- not the parent of the pixel's
// h3_res cell: an H3 parent does not contain its children geometrically, and the pixel has to show the record whose
// hexagon the GeoJSON body draws at that spot.  As in K1 (k_ingest.h), the streaming kernel runs latLngToCellFast and
// appends the pixels it cannot decide to an exception list (u32 pixel indices, wave_append); k_raster_exact runs
// latLngToCellDeg (~170 VGPRs) on that list only.  The cell is looked up read-only in the parent table rollup_on_device
// left (GrowRec slots, home mix64(cell) & mask, tab_probe<false>): that table is at most half full, so a chain ends.
// Cell 0 (a NaN or out-of-range coordinate) is the table's free-slot marker and is never probed: count 0.
//
// k_raster: a wave takes 64 consecutive columns of one row, so lat[r] is wave-uniform and the stores coalesce (256 B of
// counts, 64 B of classes per wave).  63 VGPRs, no scratch, 7 waves per SIMD by the compiler's count -- k_cells' figures:
// the fast path is the footprint, the lookup adds nothing to it -- so no occupancy attribute beyond the block size;
// k_raster_exact takes 118 VGPRs (4 waves per SIMD) and runs on the exception list only.  Lanes of one wave that share
// a cell -- most of them at high zoom -- read the same slot's line; their probes are not deduplicated across lanes.
// =====================================================================================================
constexpr int RASTER_MAX_THRESHOLDS = 15;
constexpr int RASTER_MAX_DIM = 16384;
constexpr int64_t RASTER_MAX_PIXELS = int64_t(1) << 26;
struct RasterThr {   // strictly ascending, >= 0; n = 0: no classes
    unsigned long long t[RASTER_MAX_THRESHOLDS];
    int n;
};
// 0..15, every threshold >= 0, strictly ascending
static bool raster_thresholds(const int64_t *thresholds, int32_t n, RasterThr &T) {
    if (n < 0 || n > RASTER_MAX_THRESHOLDS || (n > 0 && !thresholds)) return false;
    for (int i = 0; i < RASTER_MAX_THRESHOLDS; i++) T.t[i] = ~0ull;
    T.n = n;
    for (int i = 0; i < n; i++) {
        if (thresholds[i] < 0 || (i > 0 && thresholds[i] <= thresholds[i - 1])) return false;
        T.t[i] = (unsigned long long)thresholds[i];
    }
    return true;
}
// the two outputs of a pixel from its record's 64-bit count (0: no record): the count saturated at 2^32 - 1, and the
// number of thresholds strictly below the unsaturated count
HM_HD uint32_t raster_count(unsigned long long count) { return count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)count; }
HM_HD uint8_t raster_class(unsigned long long count, const RasterThr &T) {
    int k = 0;
    for (int i = 0; i < T.n; i++) k += count > T.t[i];
    return (uint8_t)k;
}
HM_HD void raster_put(unsigned long long count, const RasterThr &T, int64_t i, uint32_t *counts, uint8_t *classes) {
    counts[i] = raster_count(count);
    if (classes) classes[i] = raster_class(count, T);
}

// the count of `cell` in the roll-up's parent table of mask + 1 slots; 0 where the window has no tile at that cell
__device__ __forceinline__ unsigned long long raster_lookup(const GrowRec *__restrict__ tab, unsigned long long mask, uint64_t cell) {
    if (cell == 0) return 0;   // (0 = a free slot's key word: it would "match" the first free slot)
    unsigned long long seen;
    const unsigned long long h = tab_probe<false>([tab](unsigned long long i) { return (const unsigned long long *)&tab[i].cell; },
                                                  mask, mix64(cell) & mask, mask + 1, 0ull, 0ull, TabKeyIs{cell, 0ull}, seen);
    return h == TAB_NONE ? 0ull : (unsigned long long)tab[h].count;
}

// one wave per (row, 64-column segment), grid-stride over the rows x ceil(cols / 64) segments; exceptions -> slow[]
// (room for rows x cols indices)
__global__ __launch_bounds__(256) void k_raster(const double *__restrict__ lat, int rows, const double *__restrict__ lon, int cols,
                                                int res, const GrowRec *__restrict__ tab, unsigned long long mask, RasterThr thr,
                                                uint32_t *__restrict__ counts, uint8_t *__restrict__ classes,
                                                unsigned int *__restrict__ slow, unsigned long long *n_slow) {
    const int nseg = (cols + 63) >> 6;
    const int64_t nunits = (int64_t)rows * nseg;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < nunits; u += stride) {
        const int r = (int)(u / nseg);
        const int c = (int)(u - (int64_t)r * nseg) * 64 + lane_id();
        const int64_t i = (int64_t)r * cols + c;
        bool exc = false;
        if (c < cols) {
            uint64_t cell;
            exc = !latLngToCellFast(lat[r], lon[c], res, c_tab, cell);
            if (!exc) raster_put(raster_lookup(tab, mask, cell), thr, i, counts, classes);
        }
        const unsigned long long pos = wave_append(exc, n_slow);
        if (exc) slow[pos] = (unsigned int)i;
    }
}
// the exception list's pixels by the exact path
__global__ __launch_bounds__(256) void k_raster_exact(const double *__restrict__ lat, const double *__restrict__ lon, int cols, int res,
                                                      const GrowRec *__restrict__ tab, unsigned long long mask, RasterThr thr,
                                                      uint32_t *__restrict__ counts, uint8_t *__restrict__ classes,
                                                      const unsigned int *__restrict__ slow, const unsigned long long *n_slow) {
    const int64_t m = (int64_t)*n_slow;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (int64_t)gridDim.x * blockDim.x) {
        const unsigned i = slow[q];
        const uint64_t cell = latLngToCellDeg(lat[i / (unsigned)cols], lon[i % (unsigned)cols], res, c_tab);
        raster_put(raster_lookup(tab, mask, cell), thr, i, counts, classes);
    }
}
