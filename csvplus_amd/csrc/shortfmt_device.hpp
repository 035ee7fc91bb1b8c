// shortfmt_device.hpp — strconv.FormatFloat(v, fmt, -1, 64) for fmt = 'e' 'E' 'f' 'g' 'G' for the Map kernels (map_device.hpp:
// a CPH_MAP_FLOAT64_SHORTEST piece): the shortest decimal digits that read back to the same double, the character count of
// each layout, and its bytes.  The length pass and the copy pass share the split, so a count and the bytes behind it cannot
// disagree.
//
// Plain C++ behind CPH_SHORTFMT_HD, depending on nothing else in the tree: hipcc compiles it for the device, g++ for the host
// (tests/cpp/test_shortfmt.cpp runs it against std::to_chars).
//
// Digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020).  v = c * 2^q.  With k = floor(log10(2^q))
// (floor(log10(3/4 * 2^q)) at a power of two, where the interval's lower half is narrower) the three numbers 4c - 2 (4c - 1
// at a power of two), 4c and 4c + 2 — the rounding interval's ends and v itself, times four — are scaled by 10^-k with one
// 64 x 128-bit multiply each by a tabulated 128-bit power of ten (pow10_table.inc, written by tools/gen_pow10_table.py,
// rounded up), the bits below the integer kept as one sticky bit.  Among the at most four candidates floor and ceil of v's
// scaled value at 10^k and at 10^(k+1), the paper proves that one of the coarser pair lies in the interval if any shorter
// digit string does, and otherwise the closer one of the finer pair does: exact for every double, nothing is left undecided.
// The ends belong to the interval exactly when c is even (round-half-even reads them back to v).  Trailing zeros of the
// result come off, which leaves the shortest digits.
//
// The table is 617 x 16 bytes in global memory; every lane indexes it with its own exponent, one 16-byte vector load per
// value, served by the vector cache / L2 (floatparse_device.hpp reads its table the same way).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CPH_SHORTFMT_HD __host__ __device__ __forceinline__
#define CPH_SHORTFMT_TABLE __device__ const
#else
#define CPH_SHORTFMT_HD inline
#define CPH_SHORTFMT_TABLE static const
#endif

namespace cph {

constexpr int32_t kPow10MinE = -292, kPow10MaxE = 324;

// Maximum characters per format.  'e': sign, 17 digits, point, 'e', sign, 3 exponent digits.  'g': the 'e' form outside
// 1e-4 <= |v| < 1e6, inside at most sign, "0.000", 17 digits = 23.  'f': below 1 the text is "0." and the decimals up to
// the last digit's place.  An interval of width 2^-1074 or more holds a multiple of 10^-324 < 2^-1074, so no shortest
// digit string of a double reaches beyond the 324th decimal: sign + "0." + 324 = 327 (reached by -2.2250738585072014e-308).
// From 1 up the longest is sign + 309 digits.
constexpr uint32_t kShortMaxCharsE = 24;
constexpr uint32_t kShortMaxCharsG = 24;
constexpr uint32_t kShortMaxCharsF = 327;

enum { SHORT_FINITE = 0, SHORT_NAN = 1, SHORT_INF = 2 };

struct alignas(16) Pow10 {
    uint64_t hi, lo;
};

CPH_SHORTFMT_TABLE Pow10 kPow10Table[kPow10MaxE - kPow10MinE + 1] = {
#include "pow10_table.inc"
};

// The value is 0.d1...dnd * 10^dp (Go's decimalSlice); zero is the one digit 0 with dp = 1.
struct ShortParts {
    uint64_t digits;   // d1...dnd as an integer, no trailing zero (but zero itself)
    int32_t nd;        // 1..17
    int32_t dp;        // -323..309
    uint32_t kind;     // SHORT_*
    uint32_t neg;      // the sign bit
};

CPH_SHORTFMT_HD bool short_fmt_ok(int32_t fmt) { return fmt == 'e' || fmt == 'E' || fmt == 'f' || fmt == 'g' || fmt == 'G'; }

// floor(g * cp / 2^128), and bit 0 set when bits were lost below it (cp < 2^64, g = hi:lo)
CPH_SHORTFMT_HD uint64_t short_round_to_odd(Pow10 g, uint64_t cp) {
    const unsigned __int128 x = (unsigned __int128)g.lo * cp;
    const unsigned __int128 y = (unsigned __int128)g.hi * cp + (uint64_t)(x >> 64);
    return (uint64_t)(y >> 64) | ((uint64_t)y > 1ull ? 1ull : 0ull);
}

// decimal digits of m < 10^17: 1..17 (compares against 10^1 .. 10^16)
CPH_SHORTFMT_HD int32_t short_digits(uint64_t m) {
    int32_t d = 1;
    uint64_t p = 10;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k <= 16; k++) {
        d += m >= p ? 1 : 0;
        p *= 10;
    }
    return d;
}

CPH_SHORTFMT_HD ShortParts short_split(double v) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, sizeof bits);
    ShortParts r;
    r.digits = 0, r.nd = 1, r.dp = 1, r.kind = SHORT_FINITE, r.neg = (uint32_t)(bits >> 63);
    const uint32_t ef = (uint32_t)(bits >> 52) & 0x7FFu;
    const uint64_t mant = bits & ((1ull << 52) - 1);
    if (ef == 0x7FFu) {
        r.kind = mant ? SHORT_NAN : SHORT_INF;
        return r;
    }
    if ((ef | mant) == 0) return r;
    const uint64_t c = ef ? mant | (1ull << 52) : mant;
    const int32_t q = (ef ? (int32_t)ef : 1) - 1075;              // -1074..971
    const bool even = (c & 1ull) == 0;
    const bool narrow = mant == 0 && ef > 1u;                       // a power of two with a full-width binade below it
    const uint64_t cbl = 4 * c - 2 + (narrow ? 1u : 0u), cb = 4 * c, cbr = 4 * c + 2;
    // floor(log10(2^q)) and floor(log10(3/4 * 2^q)); floor(log2(10^-k)): fixed-point constants exact over these ranges
    const int32_t k = narrow ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;   // -324..292
    const int32_t h = q + ((-k * 1741647) >> 19) + 1;                                 // 1..4
    const Pow10 g = kPow10Table[-k - kPow10MinE];
    const uint64_t vbl = short_round_to_odd(g, cbl << h);
    const uint64_t vb = short_round_to_odd(g, cb << h);
    const uint64_t vbr = short_round_to_odd(g, cbr << h);
    const uint64_t lower = vbl + (even ? 0u : 1u), upper = vbr - (even ? 0u : 1u);
    const uint64_t s = vb >> 2;                                     // < 10^17
    uint64_t d = 0;
    int32_t e10 = k;                                                // the value is d * 10^e10
    bool found = false;
    if (s >= 10) {                                                  // one digit fewer: floor or ceil at 10^(k+1)
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) d = sp + (wp_in ? 1u : 0u), e10 = k + 1, found = true;
    }
    if (!found) {
        const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
        if (u_in != w_in) {
            d = s + (w_in ? 1u : 0u);
        } else {                                                    // both or neither: the closer one, ties to even
            const uint64_t mid = 4 * s + 2;
            d = s + ((vb > mid || (vb == mid && (s & 1ull))) ? 1u : 0u);
        }
    }
    // trailing zeros off: eight at a time while the 64-bit division lasts, then in 32 bits
    while (d >= 100000000ull) {
        const uint64_t t = d / 100000000ull;
        if (d - t * 100000000ull != 0) break;
        d = t, e10 += 8;
    }
    if (d < (1ull << 32)) {
        uint32_t d32 = (uint32_t)d;
        for (;;) {
            const uint32_t t = d32 / 10u;
            if (d32 - t * 10u != 0) break;
            d32 = t, e10++;
        }
        d = d32;
    } else {
        for (;;) {
            const uint64_t t = d / 10;
            if (d - t * 10 != 0) break;
            d = t, e10++;
        }
    }
    r.digits = d;
    r.nd = short_digits(d);
    r.dp = e10 + r.nd;
    return r;
}

// true: fmt writes r in the exponent form ('g' picks it as Go does for the shortest digits: eprec = 6)
CPH_SHORTFMT_HD bool short_exp_form(const ShortParts& r, int32_t fmt) {
    const int32_t exp = r.dp - 1;
    return fmt == 'e' || fmt == 'E' || (fmt != 'f' && (exp < -4 || exp >= 6));
}

// characters of the result
CPH_SHORTFMT_HD uint32_t short_chars(const ShortParts& r, int32_t fmt) {
    if (r.kind != SHORT_FINITE) return r.kind == SHORT_NAN ? 3u : 4u;
    const uint32_t nd = (uint32_t)r.nd;
    if (short_exp_form(r, fmt)) {
        const int32_t exp = r.dp - 1;
        return r.neg + nd + (nd > 1u ? 1u : 0u) + 2u + ((exp <= -100 || exp >= 100) ? 3u : 2u);
    }
    if (r.dp <= 0) return r.neg + 2u + (uint32_t)-r.dp + nd;
    if (r.dp < r.nd) return r.neg + nd + 1u;
    return r.neg + (uint32_t)r.dp;
}

// up to 24 characters assembled in registers, three 8-byte chunks
struct ShortChars {
    uint64_t c0, c1, c2;
    CPH_SHORTFMT_HD void set(uint32_t pos, uint32_t ch) {
        const uint64_t sh = (uint64_t)ch << (8u * (pos & 7u));
        if (pos < 8u) c0 |= sh;
        else if (pos < 16u) c1 |= sh;
        else c2 |= sh;
    }
    template <class Sink>
    CPH_SHORTFMT_HD void put(Sink& s, uint32_t len) const {
        s.put8(c0, len < 8u ? len : 8u);
        if (len > 8u) s.put8(c1, len < 16u ? len - 8u : 8u);
        if (len > 16u) s.put8(c2, len - 16u);
    }
};

// the nd digits of m from position `first` on, a '.' after the `point`-th of them (0: none); returns the position behind them.
// The digits come off nine at a time, so that the inner divisions are 32-bit.
CPH_SHORTFMT_HD uint32_t short_set_digits(ShortChars& c, uint64_t m, uint32_t nd, uint32_t first, uint32_t point) {
    const uint32_t end = first + nd + (point ? 1u : 0u);
    uint32_t j = nd;   // digits left, from the last
    while (j) {
        const uint64_t q = m / 1000000000u;
        uint32_t r = (uint32_t)(m - q * 1000000000u);
        m = q;
        for (int k = 0; k < 9 && j; k++) {
            const uint32_t q10 = r / 10u;
            const uint32_t dig = r - q10 * 10u;
            r = q10;
            j--;
            c.set(first + j + (point && j >= point ? 1u : 0u), (uint32_t)'0' + dig);
        }
    }
    if (point) c.set(first + point, (uint32_t)'.');
    return end;
}

template <class Sink>
CPH_SHORTFMT_HD void short_put_zeros(Sink& s, uint32_t n) {
    const uint64_t zeros = 0x3030303030303030ull;
    for (; n >= 8u; n -= 8u) s.put8(zeros, 8u);
    if (n) s.put8(zeros, n);
}

// the bytes of the result, short_chars of them
template <class Sink>
CPH_SHORTFMT_HD void short_put(Sink& s, const ShortParts& r, int32_t fmt) {
    if (r.kind != SHORT_FINITE) {
        if (r.kind == SHORT_NAN) s.put8((uint64_t)'N' | (uint64_t)'a' << 8 | (uint64_t)'N' << 16, 3u);
        else s.put8((uint64_t)(r.neg ? '-' : '+') | (uint64_t)'I' << 8 | (uint64_t)'n' << 16 | (uint64_t)'f' << 24, 4u);
        return;
    }
    const uint32_t nd = (uint32_t)r.nd;
    ShortChars c;
    c.c0 = r.neg ? (uint64_t)'-' : 0, c.c1 = 0, c.c2 = 0;
    if (short_exp_form(r, fmt)) {   // d[.ddd]e±XX[X]
        uint32_t pos = short_set_digits(c, r.digits, nd, r.neg, nd > 1u ? 1u : 0u);
        const int32_t exp = r.dp - 1;
        uint32_t a = (uint32_t)(exp < 0 ? -exp : exp);   // <= 323
        c.set(pos++, (fmt == 'E' || fmt == 'G') ? (uint32_t)'E' : (uint32_t)'e');
        c.set(pos++, exp < 0 ? (uint32_t)'-' : (uint32_t)'+');
        if (a >= 100u) {
            const uint32_t h = a / 100u;
            c.set(pos++, (uint32_t)'0' + h);
            a -= h * 100u;
        }
        const uint32_t t = a / 10u;
        c.set(pos++, (uint32_t)'0' + t);
        c.set(pos++, (uint32_t)'0' + (a - t * 10u));
        c.put(s, pos);
    } else if (r.dp <= 0) {         // 0.000ddd
        c.set(r.neg, (uint32_t)'0');
        c.set(r.neg + 1u, (uint32_t)'.');
        s.put8(c.c0, r.neg + 2u);
        short_put_zeros(s, (uint32_t)-r.dp);
        c.c0 = 0;
        c.put(s, short_set_digits(c, r.digits, nd, 0u, 0u));
    } else if (r.dp < r.nd) {       // dd.ddd
        c.put(s, short_set_digits(c, r.digits, nd, r.neg, (uint32_t)r.dp));
    } else {                        // ddd000
        c.put(s, short_set_digits(c, r.digits, nd, r.neg, 0u));
        short_put_zeros(s, (uint32_t)(r.dp - r.nd));
    }
}

}  // namespace cph
