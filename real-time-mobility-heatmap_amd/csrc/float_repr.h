// binary64 -> the text json.dumps writes for it (the read side's GeoJSON bodies, geojson_docs.h): CPython's
// float.__repr__ -- the shortest digits that round-trip, the nearest of them to the value, interval ends admitted for an
// even mantissa (David Gay's mode 0) -- in format 'r' layout, plus JSON's words NaN / Infinity / -Infinity.
// The inverse of json_decode.h's decimal_to_double_bits.  Host-callable too (HM_HD): the CPU tests run this same code
// against repr().
//
// Digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020), in the arrangement of A. Bolz's
// Drachennest schubfach_64: the value v = c * 2^q and its rounding interval's ends are scaled by 10^-k (one 128-bit
// power of ten rounded up, pow10_table.inc) into integers that keep a sticky bit (fr_round_to_odd), k chosen so that
// the interval holds at most one multiple of 10 and at least one integer; the shortest candidate inside wins, then the
// nearer of the two neighbouring integers, ties to even.  Integer arithmetic only: three 64 x 128-bit products.
//
// Layout (format_float_short 'r'): decpt = digits + exponent; fixed notation for -4 < decpt <= 16, always with a ".0"
// or a fraction; else d[.ddd]e+-XX with at least two exponent digits.  At most 24 bytes (-1.7976931348623157e+308).
#pragma once
#include <stdint.h>

#include "json_decode.h"   // mul64x64
#include "pow10_table.inc"

namespace hm {

#if defined(__HIPCC__)
__constant__ const unsigned long long c_pow10[] = {HM_POW10_ENTRIES};
#endif
static const unsigned long long h_pow10[] = {HM_POW10_ENTRIES};
HM_HD const unsigned long long *pow10_table() {
#if defined(__HIP_DEVICE_COMPILE__)
    return c_pow10;
#else
    return h_pow10;
#endif
}

constexpr int FLOAT_REPR_MAX = 24;

// floor(log2 10^e), floor(log10 2^e), floor(log10 (3/4 2^e)) for the arguments used here (tools/gen_pow10.py checks them)
HM_HD int fr_floor_log2_pow10(int e) { return (e * 1741647) >> 19; }
HM_HD int fr_floor_log10_pow2(int e) { return (e * 1262611) >> 22; }
HM_HD int fr_floor_log10_34_pow2(int e) { return (e * 1262611 - 524031) >> 22; }

// the top 64 bits of cp * g / 2^64 (g = ghi:glo), their lowest bit set if any lower bit of the product is
HM_HD uint64_t fr_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    uint64_t xh, xl, yh, yl;
    mul64x64(cp, glo, xh, xl);
    mul64x64(cp, ghi, yh, yl);
    const uint64_t y0 = yl + xh;
    const uint64_t y1 = yh + (uint64_t)(y0 < yl);
    return y1 | (uint64_t)(y0 > 1);
}

// a finite, non-zero binary64 (fraction field frac, biased exponent be) -> shortest decimal dig * 10^k
HM_HD void fr_to_decimal(uint64_t frac, int be, uint64_t &dig, int &k) {
    uint64_t c;
    int q;
    if (be != 0) { c = frac | (UINT64_C(1) << 52); q = be - 1075; }
    else { c = frac; q = -1074; }
    const bool even = (c & 1) == 0;
    const bool closer = frac == 0 && be > 1;   // a power of two: the lower neighbour is half as far
    const uint64_t cbl = 4 * c - 2 + (uint64_t)closer, cb = 4 * c, cbr = 4 * c + 2;
    k = closer ? fr_floor_log10_34_pow2(q) : fr_floor_log10_pow2(q);
    const int h = q + fr_floor_log2_pow10(-k) + 1;   // 1..4
    const unsigned long long *T = pow10_table() + 2 * (-k - HM_POW10_KMIN);
    const uint64_t ghi = T[0], glo = T[1];
    const uint64_t vbl = fr_round_to_odd(ghi, glo, cbl << h);
    const uint64_t vb = fr_round_to_odd(ghi, glo, cb << h);
    const uint64_t vbr = fr_round_to_odd(ghi, glo, cbr << h);
    const uint64_t lower = vbl + (uint64_t)!even, upper = vbr - (uint64_t)!even;
    const uint64_t s = vb / 4;
    if (s >= 10) {   // a multiple of 10 inside the interval is shorter than anything else
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) { dig = sp + (uint64_t)wp_in; k++; return; }
    }
    const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
    if (u_in != w_in) { dig = s + (uint64_t)w_in; return; }
    const uint64_t mid = 4 * s + 2;
    dig = s + (uint64_t)(vb > mid || (vb == mid && (s & 1)));
}

// writes json.dumps(x) to out (nullptr: only measures); returns its length (<= FLOAT_REPR_MAX)
HM_HD int float_repr(double x, uint8_t *out) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    const uint64_t frac = bits & ((UINT64_C(1) << 52) - 1);
    const int be = (int)((bits >> 52) & 0x7ff);
    int n = 0;
    auto lit = [&](const char *s) { for (int q = 0; s[q]; q++) { if (out) out[n] = (uint8_t)s[q]; n++; } };
    if (be == 0x7ff && frac) { lit("NaN"); return n; }
    if (bits >> 63) { if (out) out[n] = '-'; n++; }
    if (be == 0x7ff) { lit("Infinity"); return n; }
    if (be == 0 && frac == 0) { lit("0.0"); return n; }
    uint64_t dig;
    int k;
    fr_to_decimal(frac, be, dig, k);
    while (dig % 10 == 0) { dig /= 10; k++; }   // (the shortest candidate may still end in zeros: 1e22, 42.0)
    int nd = 1;
    for (uint64_t p = 10; nd < 17 && dig >= p; p *= 10) nd++;
    const int decpt = nd + k;
    const int start = n;
    if (-4 < decpt && decpt <= 16) {
        // digit i of nd goes to start + at(i)
        int len;
        if (decpt <= 0) len = 2 - decpt + nd;          // 0.000ddd
        else if (decpt < nd) len = nd + 1;             // dd.ddd
        else len = decpt + 2;                          // ddd000.0
        if (out) {
            if (decpt <= 0) {
                for (int i = 0; i < 2 - decpt; i++) out[start + i] = '0';
                out[start + 1] = '.';
                for (int i = nd - 1; i >= 0; i--) { out[start + 2 - decpt + i] = (uint8_t)('0' + dig % 10); dig /= 10; }
            } else if (decpt < nd) {
                for (int i = nd - 1; i >= 0; i--) { out[start + i + (i >= decpt)] = (uint8_t)('0' + dig % 10); dig /= 10; }
                out[start + decpt] = '.';
            } else {
                for (int i = nd - 1; i >= 0; i--) { out[start + i] = (uint8_t)('0' + dig % 10); dig /= 10; }
                for (int i = nd; i < decpt; i++) out[start + i] = '0';
                out[start + decpt] = '.';
                out[start + decpt + 1] = '0';
            }
        }
        return start + len;
    }
    // d[.ddd]e+-XX
    const int e = decpt - 1, ae = e < 0 ? -e : e;
    const int mant = nd > 1 ? nd + 1 : 1;
    const int len = mant + 2 + (ae >= 100 ? 3 : 2);
    if (out) {
        for (int i = nd - 1; i >= 1; i--) { out[start + 1 + i] = (uint8_t)('0' + dig % 10); dig /= 10; }
        out[start] = (uint8_t)('0' + dig);
        if (nd > 1) out[start + 1] = '.';
        int p = start + mant;
        out[p++] = 'e';
        out[p++] = e < 0 ? '-' : '+';
        if (ae >= 100) out[p++] = (uint8_t)('0' + ae / 100);
        out[p++] = (uint8_t)('0' + ae / 10 % 10);
        out[p++] = (uint8_t)('0' + ae % 10);
    }
    return start + len;
}

}  // namespace hm
