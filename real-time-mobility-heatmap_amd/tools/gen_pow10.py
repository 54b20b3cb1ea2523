#!/usr/bin/env python3
"""Writes real-time-mobility-heatmap_amd/csrc/pow10_table.inc: the 128-bit powers of ten 10^k, k in [-292, 324],
rounded UP, that the shortest binary64 -> decimal conversion of csrc/float_repr.h multiplies by (Schubfach: R. Giulietti,
"The Schubfach way to render doubles", 2020, section 9.2).  For every k there are unique beta and r with
10^k = beta * 2^r and 2^127 <= beta < 2^128 (r = floor(log2 10^k) - 127); the entry is g = ceil(beta), so that
(g - 1) * 2^r < 10^k <= g * 2^r.  Entry k occupies two words: [2 (k + 292)] = the high 64 bits, [2 (k + 292) + 1] = the
low 64 bits.  pow5_table.inc will not do: it covers another range and rounds as Eisel-Lemire needs (down for q >= 0).

Python integers are exact, so the table is checked here against its definition before it is written, and the whole
conversion, restated with Python integers on this table, is checked against float.__repr__ on a sample.
"""
import os
import random
import struct

K_MIN, K_MAX = -292, 324
M64 = (1 << 64) - 1


def entry(k):
    """(g, r) with g = ceil(10^k / 2^r), 2^127 <= g < 2^128."""
    if k >= 0:
        p = 10 ** k
        r = p.bit_length() - 128
        g = -((-p) >> r) if r >= 0 else p << -r          # ceil(p / 2^r)
    else:
        q = 10 ** -k
        r = -(q.bit_length() - 1) - 128                   # a first guess: 2^-r / q has 128 or 129 bits
        while True:
            g = -((-(1 << -r)) // q)                      # ceil(2^-r / q)
            if g >= (1 << 128):
                r += 1
            elif g < (1 << 127):
                r -= 1
            else:
                break
    return g, r


def check_entry(k, g, r):
    assert (1 << 127) <= g < (1 << 128), k
    # (g - 1) * 2^r < 10^k <= g * 2^r, in integers
    if k >= 0:
        lo, hi, p = (g - 1, g, 10 ** k)
        if r >= 0:
            assert (lo << r) < p <= (hi << r), k
        else:
            assert lo < (p << -r) <= hi, k
    else:
        q = 10 ** -k
        assert r < 0
        assert (g - 1) * q < (1 << -r) <= g * q, k
    assert r == floor_log2_pow10(k) - 127, k


# the three integer logarithms of float_repr.h, checked over the arguments it uses
def floor_log2_pow10(e):
    return (e * 1741647) >> 19


def floor_log10_pow2(e):
    return (e * 1262611) >> 22


def floor_log10_three_quarters_pow2(e):
    return (e * 1262611 - 524031) >> 22


def check_logs():
    for e in range(K_MIN, K_MAX + 1):
        want = (10 ** e).bit_length() - 1 if e >= 0 else -((10 ** -e - 1).bit_length())
        assert floor_log2_pow10(e) == want, e
    for e in range(-1074, 972):
        # floor(log10(2^e)) and floor(log10(3/4 * 2^e)) by exact comparison
        def flog10(num, den):   # floor(log10(num / den))
            k = 0
            while num >= 10 * den:
                den *= 10
                k += 1
            while num < den:
                num *= 10
                k -= 1
            return k
        n, d = (1 << e, 1) if e >= 0 else (1, 1 << -e)
        assert floor_log10_pow2(e) == flog10(n, d), e
        assert floor_log10_three_quarters_pow2(e) == flog10(3 * n, 4 * d), e


def round_to_odd(g, cp):
    """float_repr.h's fr_round_to_odd on a 128-bit g: the top 64 bits of cp * g / 2^64, sticky bit in bit 0."""
    ghi, glo = g >> 64, g & M64
    x = cp * glo
    y = cp * ghi
    y0 = (y & M64) + (x >> 64)
    y1 = (y >> 64) + (y0 >> 64)
    y0 &= M64
    return (y1 | (1 if y0 > 1 else 0)) & M64


def to_decimal(table, bits):
    """(digits, exponent) of a finite non-zero binary64 by the algorithm of float_repr.h, in Python integers."""
    frac, be = bits & ((1 << 52) - 1), (bits >> 52) & 0x7ff
    if be:
        c, q = frac | (1 << 52), be - 1075
    else:
        c, q = frac, -1074
    even = c % 2 == 0
    closer = frac == 0 and be > 1
    cbl, cb, cbr = 4 * c - 2 + closer, 4 * c, 4 * c + 2
    k = floor_log10_three_quarters_pow2(q) if closer else floor_log10_pow2(q)
    h = q + floor_log2_pow10(-k) + 1
    assert 1 <= h <= 4
    g = table[-k - K_MIN]
    vbl, vb, vbr = round_to_odd(g, cbl << h), round_to_odd(g, cb << h), round_to_odd(g, cbr << h)
    lower, upper = vbl + (not even), vbr - (not even)
    s = vb // 4
    if s >= 10:
        sp = s // 10
        up_in, wp_in = lower <= 40 * sp, 40 * sp + 40 <= upper
        if up_in != wp_in:
            return sp + wp_in, k + 1
    u_in, w_in = lower <= 4 * s, 4 * s + 4 <= upper
    if u_in != w_in:
        return s + w_in, k
    mid = 4 * s + 2
    up = vb > mid or (vb == mid and s % 2 == 1)
    return s + up, k


def check_conversion(table, n=20000):
    rng = random.Random(20240607)
    vals = [rng.getrandbits(63) for _ in range(n)]
    vals += [1, (1 << 52) - 1, 1 << 52, 0x7fefffffffffffff, struct.unpack("<Q", struct.pack("<d", 9007199254740993.0))[0]]
    vals += [struct.unpack("<Q", struct.pack("<d", float(f"1e{e}")))[0] for e in range(-323, 309)]
    vals += [(e << 52) for e in range(1, 2047)]
    for b in vals:
        if (b >> 52) & 0x7ff == 0x7ff or b == 0:
            continue
        x = struct.unpack("<d", struct.pack("<Q", b))[0]
        d, k = to_decimal(table, b)
        while d % 10 == 0:
            d //= 10
            k += 1
        m, _, e = f"{x!r}".partition("e")
        ip, _, fp = m.partition(".")
        want_d = int(ip + fp)
        want_k = (int(e) if e else 0) - len(fp)
        while want_d % 10 == 0:
            want_d //= 10
            want_k += 1
        assert (d, k) == (want_d, want_k), (x, d, k)


def main():
    check_logs()
    table = []
    for k in range(K_MIN, K_MAX + 1):
        g, r = entry(k)
        check_entry(k, g, r)
        table.append(g)
    check_conversion(table)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "pow10_table.inc")
    lines = ["// generated by tools/gen_pow10.py: 128-bit powers of ten 10^k rounded up, k in [-292, 324]",
             "// (entry k: words 2(k+292) = high 64 bits, 2(k+292)+1 = low 64 bits); float_repr.h instantiates it",
             f"#define HM_POW10_KMIN ({K_MIN})",
             f"#define HM_POW10_KMAX ({K_MAX})",
             "#define HM_POW10_ENTRIES \\"]
    for v in table:
        lines.append(f"    0x{v >> 64:016x}ull, 0x{v & M64:016x}ull, \\")
    lines.append("")
    text = "\n".join(lines) + "\n"
    old = open(out).read() if os.path.exists(out) else None
    if old != text:
        open(out, "w").write(text)
        print("wrote", os.path.normpath(out))
    else:
        print("unchanged", os.path.normpath(out))


if __name__ == "__main__":
    main()
