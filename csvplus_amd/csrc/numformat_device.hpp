// numformat_device.hpp — strconv.FormatFloat(v, 'f', prec, 64) for the Map kernels (map_format.hip): the split of a double
// into the decimal integer part and the prec rounded fraction digits, the character count of the result, and its bytes.
// The length pass and the copy pass share the split, so a count and the bytes behind it cannot disagree.
//
// Plain C++ behind CPH_NUMFMT_HD: hipcc compiles it for the device, g++ for the host (tests/cpp/test_numformat.cpp runs it
// against glibc's exact "%.*f").
//
// Exact inside two limits, with 128-bit integers and no big-number loop:
//   |v| < 2^128    v = m * 2^e, m < 2^53.  e >= 0: the integer part m << e fits 128 bits.
//   prec <= 22     e < 0: the integer part is m >> -e, the fraction (m mod 2^-e) / 2^-e.  Its prec digits are
//                  (m mod 2^-e) * 10^prec >> -e, rounded to nearest, ties to even, by the bits shifted out; the product is
//                  below 2^53 * 10^22 < 2^127.  A shift of 128 or more leaves less than a half: zero.  A fraction that
//                  rounds up to 10^prec carries into the integer part (9.995 at prec 2 -> 10.00).
// Beyond either limit the exact digits need more than 128 bits: such values are reported (FIXED_RANGE), not formatted.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CPH_NUMFMT_HD __host__ __device__ __forceinline__
#else
#define CPH_NUMFMT_HD inline
#endif

namespace cph {

typedef unsigned __int128 u128;

constexpr int kFixedMaxPrec = 22;
constexpr int kFixedMaxExp = 128;          // finite |v| >= 2^128 is not formatted
constexpr uint32_t kFixedMaxChars = 63;    // sign, 39 digits, point, 22 digits
constexpr uint64_t kTen19 = 10000000000000000000ull;

enum { FIXED_FINITE = 0, FIXED_NAN = 1, FIXED_INF = 2, FIXED_RANGE = 3 };

struct FixedParts {
    u128 ip;         // the integer part, after the fraction's carry
    u128 frac;       // the prec fraction digits as a number < 10^prec
    uint32_t kind;   // FIXED_*
    uint32_t neg;    // the sign bit (kept when the result rounds to zero)
};

CPH_NUMFMT_HD u128 fixed_pow10(int prec) {
    u128 p = 1;
    for (int k = 0; k < prec; k++) p *= 10;
    return p;
}

CPH_NUMFMT_HD FixedParts fixed_split(double v, int prec) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, sizeof bits);
    FixedParts r;
    r.ip = 0, r.frac = 0, r.kind = FIXED_FINITE, r.neg = (uint32_t)(bits >> 63);
    const uint32_t ef = (uint32_t)(bits >> 52) & 0x7FFu;
    const uint64_t mant = bits & ((1ull << 52) - 1);
    if (ef == 0x7FFu) {
        r.kind = mant ? FIXED_NAN : FIXED_INF;
        return r;
    }
    if (ef >= 1023u + kFixedMaxExp) {
        r.kind = FIXED_RANGE;
        return r;
    }
    const uint64_t m = ef ? mant | (1ull << 52) : mant;
    const int e = (ef ? (int)ef : 1) - 1075;
    if (e >= 0) {   // e <= 75
        r.ip = (u128)m << e;
        return r;
    }
    const uint32_t s = (uint32_t)-e;   // 1..1074
    uint64_t fm = m;
    if (s < 53u) {
        r.ip = m >> s;
        fm = m & ((1ull << s) - 1);
    }
    if (fm == 0 || s >= 128u) return r;
    const u128 p10 = fixed_pow10(prec);
    const u128 prod = (u128)fm * p10;
    u128 q = prod >> s;
    const u128 rem = prod & (((u128)1 << s) - 1);
    const u128 half = (u128)1 << (s - 1);
    // the last digit written: of the fraction, or with prec 0 (q is 0 then) of the integer part
    const uint32_t odd = (prec ? (uint32_t)q : (uint32_t)r.ip) & 1u;
    if (rem > half || (rem == half && odd)) q++;
    if (q >= p10) {
        q -= p10;
        r.ip++;
    }
    r.frac = q;
    return r;
}

// decimal digits of m: 1..20 (compares against 10^1 .. 10^19)
CPH_NUMFMT_HD uint32_t dec_digits64(uint64_t m) {
    uint32_t d = 1;
    uint64_t p = 10;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k <= 19; k++) {
        d += m >= p ? 1u : 0u;
        p *= 10;   // 10^19 < 2^64; the product behind it is never compared
    }
    return d;
}

// characters of the result; 0 for FIXED_RANGE
CPH_NUMFMT_HD uint32_t fixed_chars(const FixedParts& r, int prec) {
    if (r.kind != FIXED_FINITE) return r.kind == FIXED_NAN ? 3u : r.kind == FIXED_INF ? 4u : 0u;
    uint32_t d;
    if ((uint64_t)(r.ip >> 64) == 0) {
        d = dec_digits64((uint64_t)r.ip);
    } else {
        const u128 q = r.ip / kTen19;
        d = q < kTen19 ? 19u + dec_digits64((uint64_t)q) : 38u + dec_digits64((uint64_t)(q / kTen19));
    }
    return r.neg + d + (prec > 0 ? 1u + (uint32_t)prec : 0u);
}

// `lead` (0: none) and then m as exactly ndig (1..20) digits, zero-padded: at most 21 characters, three 8-byte chunks
// assembled in registers.  The digits come off nine at a time, so that the inner divisions are 32-bit.
template <class Sink>
CPH_NUMFMT_HD void put_dec(Sink& s, uint64_t m, uint32_t ndig, uint32_t lead) {
    const uint64_t zeros = 0x3030303030303030ull;
    const uint32_t first = lead ? 1u : 0u, len = ndig + first;
    uint64_t c0 = lead ? (zeros & ~0xFFull) | lead : zeros, c1 = zeros, c2 = zeros;
    uint32_t pos = len;
    while (m && pos > first) {
        const uint64_t q = m / 1000000000u;
        uint32_t r = (uint32_t)(m - q * 1000000000u);
        m = q;
        for (int k = 0; k < 9 && pos > first && (r || m); k++) {
            const uint32_t q10 = r / 10u;
            const uint64_t dig = r - q10 * 10u;
            r = q10;
            pos--;
            const uint64_t sh = dig << (8u * (pos & 7u));
            if (pos < 8u) c0 += sh;
            else if (pos < 16u) c1 += sh;
            else c2 += sh;
        }
    }
    s.put8(c0, len < 8u ? len : 8u);
    if (len > 8u) s.put8(c1, len < 16u ? len - 8u : 8u);
    if (len > 16u) s.put8(c2, len - 16u);
}

// the bytes of the result, fixed_chars of them
template <class Sink>
CPH_NUMFMT_HD void fixed_put(Sink& s, const FixedParts& r, int prec) {
    if (r.kind != FIXED_FINITE) {
        if (r.kind == FIXED_NAN) s.put8((uint64_t)'N' | (uint64_t)'a' << 8 | (uint64_t)'N' << 16, 3u);
        else if (r.kind == FIXED_INF) s.put8((uint64_t)(r.neg ? '-' : '+') | (uint64_t)'I' << 8 | (uint64_t)'n' << 16 | (uint64_t)'f' << 24, 4u);
        return;
    }
    const uint32_t sign = r.neg ? (uint32_t)'-' : 0u;
    if ((uint64_t)(r.ip >> 64) == 0) {
        put_dec(s, (uint64_t)r.ip, dec_digits64((uint64_t)r.ip), sign);
    } else {   // limbs of 19 digits: at most three below 2^128
        const u128 q = r.ip / kTen19;
        const uint64_t a0 = (uint64_t)(r.ip - q * kTen19);
        if (q < kTen19) {
            put_dec(s, (uint64_t)q, dec_digits64((uint64_t)q), sign);
        } else {
            const uint64_t a2 = (uint64_t)(q / kTen19);
            put_dec(s, a2, dec_digits64(a2), sign);
            put_dec(s, (uint64_t)(q - (u128)a2 * kTen19), 19u, 0u);
        }
        put_dec(s, a0, 19u, 0u);
    }
    if (prec > 19) {
        const uint64_t fh = (uint64_t)(r.frac / kTen19);
        put_dec(s, fh, (uint32_t)prec - 19u, (uint32_t)'.');
        put_dec(s, (uint64_t)(r.frac - (u128)fh * kTen19), 19u, 0u);
    } else if (prec > 0) {
        put_dec(s, (uint64_t)r.frac, (uint32_t)prec, (uint32_t)'.');
    }
}

}  // namespace cph
