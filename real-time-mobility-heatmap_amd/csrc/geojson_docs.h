// The read side's GeoJSON responses, encoded on the GPU (reference app.py:45-88: api_tiles_latest / api_positions_latest
// build one dict per tile / vehicle in a Python loop and json.dumps walks them).  This file writes exactly the bytes of
//   json.dumps(feature, separators=(",", ":"))
// for the features mobheat/readside.py builds (tiles_latest_collection, positions_latest_collection), one encoder for
// host and device (HM_HD), as bson_docs.h does for the sink's statements.  Measure mode (dst == nullptr) only counts.
//
// Tile feature:
//   {"type":"Feature","geometry":{"type":"Polygon","coordinates":[[[lng,lat],...]]},"properties":{"cellId":"<hex>",
//    "count":<int>,"avgSpeedKmh":<repr>,"windowStart":"<text>","windowEnd":"<text>"}}
//   ring: cellToBoundary's vertices (h3_boundary.h) in upstream order, degrees, each [repr(lng),repr(lat)], the first one
//   repeated at the end iff there is one and it differs from the last by value (readside.rings); no vertex: [[]];
//   cellId = format(cell, "x"); avgSpeedKmh = 0.0 without a speed, else sum_speed / n_speed (IEEE fp64 division);
//   the two window texts are the caller's (one window per call).
// Position feature:
//   {"type":"Feature","geometry":{"type":"Point","coordinates":[lon,lat]},"properties":{"provider":"..","vehicleId":"..",
//    "ts":"YYYY-MM-DDTHH:MM:SS[.ffffff]"}}
//   strings escaped as json.dumps(ensure_ascii=True) escapes them; ts = datetime.isoformat() of the naive local wall time.
#pragma once
#include <stdint.h>

#include "bson_docs.h"    // floordiv, civil_from_days, PosDocParams / position_bucket
#include "float_repr.h"

namespace hm {

constexpr int GJ_TEXT_MAX = 40;      // a window text
constexpr int GJ_PREFIX_LEN = 40;    // {"type":"FeatureCollection","features":[
#define HM_GJ_PREFIX "{\"type\":\"FeatureCollection\",\"features\":["
// the longest tile feature: 63 + 11 x 51 + 10 + 18 + 27 + 29 + 39 + 57 + 55 + 2 bytes, and its separator; with the near's
// distance (,"distanceM": and at most 24 bytes of number) GJ_DIST_MAX more; with the change's base
// (,"baseCount": ,"baseAvgSpeedKmh": ,"countChange": -- 13 + 19 + 15 bytes -- and at most 20 + 24 + 20 bytes of numbers)
// GJ_BASE_MAX more
constexpr int GJ_DIST_MAX = 38;
constexpr int GJ_BASE_MAX = 111;
// with a span's series (,"windows": ,"counts":[ ] -- 11 + 11 + 1 bytes -- and at most 2 + 16 x 20 + 15 bytes of numbers and
// commas) GJ_SPAN_MAX more
constexpr int GJ_SPAN_MAX = 360;
constexpr int GJ_TILE_MAX = 872;

// the two window texts of a call, by value (a kernel argument)
struct GjTexts {
    uint8_t start[GJ_TEXT_MAX], end[GJ_TEXT_MAX];
    int32_t start_len, end_len;
};

struct JsonW {
    uint8_t *p;
    int n;
    HM_HD void u8(uint8_t v) { if (p) p[n] = v; n++; }
    HM_HD void lit(const char *s) { for (int q = 0; s[q]; q++) u8((uint8_t)s[q]); }
    HM_HD void bytes(const uint8_t *s, int len) { for (int q = 0; q < len; q++) u8(s[q]); }
    HM_HD void f64(double v) { n += float_repr(v, p ? p + n : nullptr); }
    HM_HD void i64(int64_t v) {
        uint64_t u = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
        if (v < 0) u8('-');
        int nd = 1;
        for (uint64_t t = 10; nd < 20 && u >= t; t *= 10) nd++;
        if (p) for (int i = nd - 1; i >= 0; i--) { p[n + i] = (uint8_t)('0' + u % 10); u /= 10; }
        n += nd;
    }
    HM_HD void hex(uint64_t v) {   // format(v, "x")
        int nd = 1;
        while (nd < 16 && (v >> (4 * nd))) nd++;
        for (int q = nd - 1; q >= 0; q--) {
            const unsigned d = (unsigned)(v >> (4 * q)) & 15u;
            u8((uint8_t)(d < 10 ? '0' + d : 'a' + d - 10));
        }
    }
    HM_HD void dec2(int v) { u8((uint8_t)('0' + v / 10)); u8((uint8_t)('0' + v % 10)); }
    HM_HD void hex4(unsigned v) {
        for (int q = 3; q >= 0; q--) {
            const unsigned d = (v >> (4 * q)) & 15u;
            u8((uint8_t)(d < 10 ? '0' + d : 'a' + d - 10));
        }
    }
    HM_HD void u_escape(unsigned v) { u8('\\'); u8('u'); hex4(v); }
    // a string's content as json.dumps(ensure_ascii=True) writes it; false: not valid UTF-8 (Python's strict decoder)
    HM_HD bool escaped(const uint8_t *s, int len) {
        for (int i = 0; i < len;) {
            const unsigned c = s[i];
            if (c < 0x80) {
                i++;
                if (c == '"') { u8('\\'); u8('"'); }
                else if (c == '\\') { u8('\\'); u8('\\'); }
                else if (c == '\n') { u8('\\'); u8('n'); }
                else if (c == '\r') { u8('\\'); u8('r'); }
                else if (c == '\t') { u8('\\'); u8('t'); }
                else if (c == 8) { u8('\\'); u8('b'); }
                else if (c == 12) { u8('\\'); u8('f'); }
                else if (c < 0x20 || c == 0x7f) u_escape(c);
                else u8((uint8_t)c);
                continue;
            }
            int need;
            unsigned lo = 0x80, hi = 0xBF, cp;
            if (c >= 0xC2 && c <= 0xDF) { need = 1; cp = c & 0x1f; }
            else if (c == 0xE0) { need = 2; lo = 0xA0; cp = 0; }
            else if (c >= 0xE1 && c <= 0xEF) { need = 2; cp = c & 0x0f; if (c == 0xED) hi = 0x9F; }
            else if (c == 0xF0) { need = 3; lo = 0x90; cp = 0; }
            else if (c >= 0xF1 && c <= 0xF3) { need = 3; cp = c & 0x07; }
            else if (c == 0xF4) { need = 3; hi = 0x8F; cp = 4; }
            else return false;
            if (i + need >= len) return false;   // the sequence runs past the string
            for (int k = 1; k <= need; k++) {
                const unsigned b = s[i + k];
                if (b < (k == 1 ? lo : 0x80u) || b > (k == 1 ? hi : 0xBFu)) return false;
                cp = (cp << 6) | (b & 0x3f);
            }
            i += need + 1;
            if (cp < 0x10000) {
                u_escape(cp);
            } else {
                const unsigned v = cp - 0x10000;
                u_escape(0xD800 | (v >> 10));
                u_escape(0xDC00 | (v & 0x3ff));
            }
        }
        return true;
    }
};

// the base half of a change pair, as tile_feature appends it
struct GjBase {
    int64_t count, n_speed;
    double sum_speed;
};
// a span record's series row, as tile_feature appends it: the record's count in each of the span's windows
struct GjSpan {
    int windows;
    const int64_t *counts;
};

// one tile feature from the record's fields and its boundary (vertex k at lat[k * stride], lng[k * stride]); returns
// its length (without the separator that follows it in the body).  dist_m (optional): the record's distance from a near
// query's point, appended as the last property ,"distanceM":<repr>; nullptr: the feature as it always was.  base
// (optional): the cell's record in a change's base window, appended after windowEnd as
// ,"baseCount":<int>,"baseAvgSpeedKmh":<repr>,"countChange":<int> (the average by avgSpeedKmh's rule, the change
// count - base count as int64); nullptr: every byte as without it.  span (optional): the record's series row, appended
// after windowEnd as ,"windows":<int>,"counts":[<int>,...]; nullptr: every byte as without it
HM_HD int tile_feature(uint8_t *dst, const GjTexts &T, uint64_t cell, int64_t count, int64_t n_speed, double sum_speed,
                       int nv, const double *lat, const double *lng, int64_t stride, const double *dist_m = nullptr,
                       const GjBase *base = nullptr, const GjSpan *span = nullptr) {
    JsonW w{dst, 0};
    w.lit("{\"type\":\"Feature\",\"geometry\":{\"type\":\"Polygon\",\"coordinates\":[[");
    for (int k = 0; k < nv; k++) {
        if (k) w.u8(',');
        w.u8('[');
        w.f64(lng[k * stride]);
        w.u8(',');
        w.f64(lat[k * stride]);
        w.u8(']');
    }
    if (nv > 0) {
        const double lng0 = lng[0], lat0 = lat[0], lngl = lng[(nv - 1) * stride], latl = lat[(nv - 1) * stride];
        if (!(lng0 == lngl && lat0 == latl)) {   // ring[0] != ring[-1], by value
            w.lit(",[");
            w.f64(lng0);
            w.u8(',');
            w.f64(lat0);
            w.u8(']');
        }
    }
    w.lit("]]},\"properties\":{\"cellId\":\"");
    w.hex(cell);
    w.lit("\",\"count\":");
    w.i64(count);
    w.lit(",\"avgSpeedKmh\":");
    w.f64(n_speed == 0 ? 0.0 : sum_speed / (double)n_speed);
    w.lit(",\"windowStart\":\"");
    w.bytes(T.start, T.start_len);
    w.lit("\",\"windowEnd\":\"");
    w.bytes(T.end, T.end_len);
    w.u8('"');
    if (base) {
        w.lit(",\"baseCount\":");
        w.i64(base->count);
        w.lit(",\"baseAvgSpeedKmh\":");
        w.f64(base->n_speed == 0 ? 0.0 : base->sum_speed / (double)base->n_speed);
        w.lit(",\"countChange\":");
        w.i64(count - base->count);
    }
    if (span) {
        w.lit(",\"windows\":");
        w.i64(span->windows);
        w.lit(",\"counts\":[");
        for (int j = 0; j < span->windows; j++) {
            if (j) w.u8(',');
            w.i64(span->counts[j]);
        }
        w.u8(']');
    }
    if (dist_m) {
        w.lit(",\"distanceM\":");
        w.f64(*dist_m);
    }
    w.lit("}}");
    return w.n;
}

// a window text: at most GJ_TEXT_MAX bytes of 0x20-0x7e without '"' and '\'
HM_HD bool gj_text_ok(const char *s, int len) {
    if (len < 0 || len > GJ_TEXT_MAX || (len > 0 && !s)) return false;
    for (int q = 0; q < len; q++) {
        const unsigned c = (uint8_t)s[q];
        if (c < 0x20 || c > 0x7e || c == '"' || c == '\\') return false;
    }
    return true;
}

// one position feature; ts_us shifted by off_s seconds of local offset.  -1: a string is not valid UTF-8, or the local
// year lies outside 1..9999.  dist_m (optional): as tile_feature's
HM_HD int position_feature(uint8_t *dst, const uint8_t *ps, int pl, const uint8_t *vs, int vl, int64_t ts_us, int64_t off_s,
                           double lat, double lon, const double *dist_m = nullptr) {
    const int64_t s = floordiv(ts_us, 1000000);
    const int us = (int)(ts_us - s * 1000000);
    const int64_t local = s + off_s;
    const int64_t days = floordiv(local, 86400);
    const int sod = (int)(local - days * 86400);
    int64_t y;
    int mo, d;
    civil_from_days(days, y, mo, d);
    if (y < 1 || y > 9999) return -1;
    JsonW w{dst, 0};
    w.lit("{\"type\":\"Feature\",\"geometry\":{\"type\":\"Point\",\"coordinates\":[");
    w.f64(lon);
    w.u8(',');
    w.f64(lat);
    w.lit("]},\"properties\":{\"provider\":\"");
    if (!w.escaped(ps, pl)) return -1;
    w.lit("\",\"vehicleId\":\"");
    if (!w.escaped(vs, vl)) return -1;
    w.lit("\",\"ts\":\"");
    w.dec2((int)(y / 100));
    w.dec2((int)(y % 100));
    w.u8('-');
    w.dec2(mo);
    w.u8('-');
    w.dec2(d);
    w.u8('T');
    w.dec2(sod / 3600);
    w.u8(':');
    w.dec2(sod / 60 % 60);
    w.u8(':');
    w.dec2(sod % 60);
    if (us) {
        w.u8('.');
        w.dec2(us / 10000);
        w.dec2(us / 100 % 100);
        w.dec2(us % 100);
    }
    w.u8('"');
    if (dist_m) {
        w.lit(",\"distanceM\":");
        w.f64(*dist_m);
    }
    w.lit("}}");
    return w.n;
}

}  // namespace hm
