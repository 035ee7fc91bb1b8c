// timeparse_device.hpp — RFC 3339 text <-> Unix time on the device: `time.Parse(time.RFC3339, s)` followed by t.Unix() /
// t.UnixNano() (numparse.hip: CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO; filter.hip: the literal of a CPH_PRED_TIME_* term) and
// `time.Unix(v, 0).In(time.FixedZone("", 60 * zone)).Format(time.RFC3339)` (map_device.hpp: CPH_MAP_TIME).  The accepted
// set and the order in which a value's status is decided are stated in include/csvplus_hip.h (cph_col_to_number).
//
// A well-formed value never loops over its bytes.  Its first 16 bytes are exactly `YYYY-MM-DDTHH:MM`: XORed with the
// pattern `0000-00-00T00:00` every digit becomes its value and every separator zero, so one carry-free range test per
// word and one mask decide the shape, and one multiply per word turns the digit pairs into month, day, hour, minute and
// the two halves of the year.  Bytes 16.. (`:SS`, the fraction, the zone: 4..19 bytes) are at most three more words; the
// zone is read from the value's END (`Z`, or the last six bytes), the fraction is what lies between.  Only a value that
// misses this shape takes the byte loop that tells the stated relaxations (UNSUPPORTED) from everything else (SYNTAX).
// Days from the civil date and back are the era / year-of-era / day-of-year arithmetic on 32-bit unsigned numbers,
// shifted by one era so that year 0000 stays non-negative: divisions by constants only, no table, no scratch.
//
// Everything is __host__ __device__ (the idiom of strpred_device.hpp), so the same code compiles with a plain host
// compiler (tests/cpp/test_timeparse.cpp).  The value is seen through
//   V   uint64_t v(int j): bytes [8j, 8j + 8) of the value, little-endian; bytes past the value's end are unspecified and
//       the functor is only called for a j with 8j < len.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CPH_TIME_HD __host__ __device__ __forceinline__
#else
#define CPH_TIME_HD inline
#endif

namespace cph {

// the CPH_NUM_* codes this file returns (include/csvplus_hip.h; restated so that the file needs no other header)
constexpr uint32_t kTimeOk = 0, kTimeSyntax = 1, kTimeRange = 2, kTimeUnsupported = 3;

constexpr int64_t kTimeMinSeconds = -62167219200ll;   // 0000-01-01T00:00:00Z
constexpr int64_t kTimeMaxSeconds = 253402300799ll;   // 9999-12-31T23:59:59Z
constexpr int32_t kTimeMaxZone = 1439;                // minutes east or west of UTC

// x = 8 bytes ^ '0' (or ^ a pattern of '0's and separators): every byte is 0..9
CPH_TIME_HD bool time_digits8(uint64_t x) { return (((x + 0x0606060606060606ull) | x) & 0xF0F0F0F0F0F0F0F0ull) == 0; }

// 8 digit values, the first in the lowest byte -> byte 2k = 10 * d(2k) + d(2k + 1) (no carry: a pair is at most 99)
CPH_TIME_HD uint64_t time_pairs(uint64_t x) { return (x * 2561ull) >> 8; }

// 8 digit values, the first in the lowest byte -> their number
CPH_TIME_HD uint32_t time_digits8_value(uint64_t x) {
    x = time_pairs(x);
    x = ((x & 0x00FF00FF00FF00FFull) * 6553601ull) >> 16;
    return (uint32_t)(((x & 0x0000FFFF0000FFFFull) * 42949672960001ull) >> 32);
}

CPH_TIME_HD uint64_t time_low_bytes(uint32_t n) { return n >= 8u ? ~0ull : ((1ull << (8u * n)) - 1ull); }

// days since 1970-01-01 of a proleptic Gregorian date: y 0..9999, m 1..12, d 1..31
CPH_TIME_HD int32_t days_from_civil(uint32_t y, uint32_t m, uint32_t d) {
    const uint32_t ys = y + 400u - (m <= 2u ? 1u : 0u);   // the year starts in March; one era added: never negative
    const uint32_t era = ys / 400u, yoe = ys - era * 400u;
    const uint32_t doy = (153u * (m > 2u ? m - 3u : m + 9u) + 2u) / 5u + d - 1u;
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
    return (int32_t)(era * 146097u + doe) - (719468 + 146097);
}

CPH_TIME_HD uint32_t days_in_month(uint32_t y, uint32_t m) {
    const bool leap = (y % 4u == 0u && y % 100u != 0u) || y % 400u == 0u;
    return m == 2u ? (leap ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u);
}

// the inverse: days since 1970-01-01 (within years 0000..9999) -> y, m, d
CPH_TIME_HD void civil_from_days(int32_t days, uint32_t* y, uint32_t* m, uint32_t* d) {
    const uint32_t z = (uint32_t)(days + 719468 + 146097);
    const uint32_t era = z / 146097u, doe = z - era * 146097u;
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const uint32_t mp = (5u * doy + 2u) / 153u;
    *d = doy - (153u * mp + 2u) / 5u + 1u;
    *m = mp < 10u ? mp + 3u : mp - 9u;
    *y = yoe + era * 400u - 400u + (*m <= 2u ? 1u : 0u);
}

// one byte of the value for the byte loop below (i < len)
template <class V>
CPH_TIME_HD uint32_t time_byte_at(const V& v, uint64_t i) { return (uint32_t)(v((int)(i >> 3)) >> (8u * (uint32_t)(i & 7u))) & 0xFFu; }

// A value that missed the strict shape: UNSUPPORTED when it matches the grammar with the hour written with one digit, ','
// for the fraction's '.', or more than 9 fraction digits (any of them, together too); SYNTAX otherwise.  Byte by byte:
// only malformed values come here.
template <class V>
CPH_TIME_HD uint32_t time_classify_relaxed(const V& v, uint64_t len) {
    uint64_t i = 0;
    // n digits at i
    auto digits = [&](uint32_t n) -> bool {
        for (uint32_t k = 0; k < n; k++, i++)
            if (i >= len || time_byte_at(v, i) - (uint32_t)'0' > 9u) return false;
        return true;
    };
    auto byte_is = [&](uint32_t c) -> bool {
        if (i >= len || time_byte_at(v, i) != c) return false;
        i++;
        return true;
    };
    if (!digits(4) || !byte_is('-') || !digits(2) || !byte_is('-') || !digits(2) || !byte_is('T') || !digits(1)) return kTimeSyntax;
    if (i < len && time_byte_at(v, i) - (uint32_t)'0' <= 9u) i++;   // the hour's second digit
    if (!byte_is(':') || !digits(2) || !byte_is(':') || !digits(2)) return kTimeSyntax;
    if (i < len && (time_byte_at(v, i) == '.' || time_byte_at(v, i) == ',')) {
        i++;
        if (!digits(1)) return kTimeSyntax;
        while (i < len && time_byte_at(v, i) - (uint32_t)'0' <= 9u) i++;
    }
    if (i >= len) return kTimeSyntax;
    const uint32_t z = time_byte_at(v, i);
    i++;
    if (z == 'Z') return i == len ? kTimeUnsupported : kTimeSyntax;
    if (z != '+' && z != '-') return kTimeSyntax;
    if (!digits(2) || !byte_is(':') || !digits(2)) return kTimeSyntax;
    return i == len ? kTimeUnsupported : kTimeSyntax;
}

// RFC 3339 text -> t.Unix() (nano false) or t.UnixNano() (nano true).  c0, c1: the value's first 16 bytes with the bytes past
// its end ZERO (numparse_device.hpp: load_head16); t0, t1: its bytes 16..23 and 24..31 where it has such bytes (anything
// else otherwise); v: the functor above, called for the value's bytes 32.. and by the byte loop of a malformed value.
// Returns CPH_NUM_*; *out = the result, 0 at every error.
template <class V>
CPH_TIME_HD uint32_t parse_rfc3339(uint64_t len, uint64_t c0, uint64_t c1, uint64_t t0, uint64_t t1, const V& v, bool nano, int64_t* out) {
    *out = 0;
    if (len == 0) return kTimeSyntax;
    if (len < 20 || len > 35) return time_classify_relaxed(v, len);
    // `0000-00-00T00:00` as two little-endian words
    const uint64_t x0 = c0 ^ 0x2D30302D30303030ull, x1 = c1 ^ 0x30303A3030543030ull;
    const uint64_t seps = (x0 & 0xFF0000FF00000000ull) | (x1 & 0x0000FF0000FF0000ull);
    // bytes 16..18 are `:SS`; byte 19 opens the zone or the fraction
    const uint32_t tl = (uint32_t)len - 16u;                       // 4..19 bytes behind the minute
    const uint64_t xs = (t0 & 0xFFFFFFull) ^ 0x30303Aull;          // 0, s1, s2
    // the tail's bytes [p, p + 8), p <= 18; the words past the value's end are never selected for a byte that counts
    const uint64_t t2 = len > 32 ? v(4) : 0ull;
    const uint32_t last = tl - 1u;
    const uint32_t lastb = (uint32_t)((last < 8u ? t0 : last < 16u ? t1 : t2) >> (8u * (last & 7u))) & 0xFFu;
    const uint32_t zl = lastb == 'Z' ? 1u : 6u;                    // the zone: `Z`, or the last six bytes `+HH:MM`
    if (tl < 3u + zl) return time_classify_relaxed(v, len);
    uint32_t zsign = 0, zh = 0, zm = 0;
    bool shape = time_digits8(x0) && time_digits8(x1) && seps == 0 && time_digits8(xs) && (xs & 0xFFull) == 0;
    if (zl == 6u) {
        const uint32_t p = tl - 6u, k = p >> 3, s = (p & 7u) * 8u;  // p = 3..13
        const uint64_t lo = k == 0u ? t0 : t1, hi = k == 0u ? t1 : t2;
        const uint64_t z = (s ? (lo >> s) | (hi << (64u - s)) : lo) & 0xFFFFFFFFFFFFull;
        zsign = (uint32_t)z & 0xFFu;
        const uint64_t xz = (z >> 8) ^ 0x30303A3030ull;             // h1 h2 0 m1 m2
        shape = shape && (zsign == '+' || zsign == '-') && time_digits8(xz) && (xz & 0xFF0000ull) == 0;
        const uint64_t zp = time_pairs((xz & 0xFFFFull) | ((xz >> 24) << 16));
        zh = (uint32_t)zp & 0xFFu;
        zm = (uint32_t)(zp >> 16) & 0xFFu;
    }
    const uint32_t fl = tl - 3u - zl;                              // the fraction with its '.': 0, or 2..10 bytes
    uint32_t frac = 0;                                             // nanoseconds
    if (fl) {
        const uint32_t nd = fl - 1u;
        const uint64_t f8 = ((t0 >> 32) | (t1 << 32)) ^ 0x3030303030303030ull;   // bytes 20..27: the first 8 digits
        const uint64_t xf = f8 & time_low_bytes(nd);
        const uint32_t d9 = nd > 8u ? ((uint32_t)(t1 >> 32) & 0xFFu) ^ 0x30u : 0u;   // byte 28: the ninth
        shape = shape && ((uint32_t)(t0 >> 24) & 0xFFu) == '.' && nd >= 1u && nd <= 9u && time_digits8(xf) && d9 <= 9u;
        frac = time_digits8_value(xf) * 10u + d9;                  // digits stand left-aligned: the masked bytes are the zeros behind them
    }
    if (!shape) return time_classify_relaxed(v, len);
    const uint64_t dp = time_pairs((x0 & 0xFFFFFFFFull) | (((x0 >> 40) & 0xFFFFull) << 32));          // y y y y m m
    const uint64_t tp = time_pairs((x1 & 0xFFFFull) | (((x1 >> 24) & 0xFFFFull) << 16) | ((x1 >> 48) << 32));   // d d h h m m
    const uint32_t year = ((uint32_t)dp & 0xFFu) * 100u + ((uint32_t)(dp >> 16) & 0xFFu), month = (uint32_t)(dp >> 32) & 0xFFu;
    const uint32_t day = (uint32_t)tp & 0xFFu, hour = (uint32_t)(tp >> 16) & 0xFFu, minute = (uint32_t)(tp >> 32) & 0xFFu;
    const uint32_t second = (uint32_t)(time_pairs(xs >> 8)) & 0xFFu;
    if (month < 1u || month > 12u || day < 1u || day > days_in_month(year, month) || hour > 23u || minute > 59u || second > 59u) return kTimeRange;
    if (zh > 23u || zm > 59u) return kTimeUnsupported;
    const int32_t off = (int32_t)(zh * 3600u + zm * 60u);
    const int64_t secs = (int64_t)days_from_civil(year, month, day) * 86400ll + (int64_t)(hour * 3600u + minute * 60u + second) -
                         (int64_t)(zsign == '-' ? -off : off);
    if (!nano) {
        *out = secs;   // the fraction only adds: the floor
        return kTimeOk;
    }
    // INT64_MIN ns = -9223372037 s + 145224192 ns, INT64_MAX ns = 9223372036 s + 854775807 ns
    if (secs < -9223372037ll || secs > 9223372036ll || (secs == -9223372037ll && frac < 145224192u) || (secs == 9223372036ll && frac > 854775807u))
        return kTimeUnsupported;
    *out = (int64_t)((uint64_t)secs * 1000000000ull + (uint64_t)frac);
    return kTimeOk;
}

// what a CPH_MAP_TIME piece writes for seconds v in the zone `zone` minutes east of UTC: 20 bytes (zone 0) or 25
CPH_TIME_HD uint32_t rfc3339_chars(int32_t zone) { return zone == 0 ? 20u : 25u; }

// the local year lies in 0000..9999
CPH_TIME_HD bool rfc3339_in_range(int64_t v, int32_t zone) {
    if (v < kTimeMinSeconds - 86400ll || v > kTimeMaxSeconds + 86400ll) return false;   // v + 60 * zone cannot overflow behind this
    const int64_t local = v + 60ll * (int64_t)zone;
    return local >= kTimeMinSeconds && local <= kTimeMaxSeconds;
}

CPH_TIME_HD uint64_t time_two(uint32_t x) {   // x < 100 as two characters, the first in the lowest byte
    const uint32_t t = x / 10u;
    return (uint64_t)(0x3030u + t + ((x - t * 10u) << 8));
}

// The characters as four little-endian words: w[0] = `YYYY-MM-`, w[1] = `DDTHH:MM`, w[2] = `:SSZ` or `:SS+HH:M`, w[3] = `M`.
// v must be rfc3339_in_range.
CPH_TIME_HD void rfc3339_words(int64_t v, int32_t zone, uint64_t* w0, uint64_t* w1, uint64_t* w2, uint64_t* w3) {
    const int64_t local = v + 60ll * (int64_t)zone - kTimeMinSeconds;   // seconds since 0000-01-01T00:00:00: never negative
    const uint32_t dz = (uint32_t)((uint64_t)local / 86400ull);          // < 3652425
    const uint32_t sod = (uint32_t)((uint64_t)local - (uint64_t)dz * 86400ull);
    uint32_t y, m, d;
    civil_from_days((int32_t)dz - 719528, &y, &m, &d);
    const uint32_t hh = sod / 3600u, mi = (sod - hh * 3600u) / 60u, ss = sod - hh * 3600u - mi * 60u;
    const uint32_t yh = y / 100u;
    *w0 = time_two(yh) | (time_two(y - yh * 100u) << 16) | ((uint64_t)'-' << 32) | (time_two(m) << 40) | ((uint64_t)'-' << 56);
    *w1 = time_two(d) | ((uint64_t)'T' << 16) | (time_two(hh) << 24) | ((uint64_t)':' << 40) | (time_two(mi) << 48);
    if (zone == 0) {
        *w2 = (uint64_t)':' | (time_two(ss) << 8) | ((uint64_t)'Z' << 24);
        *w3 = 0;
        return;
    }
    const uint32_t az = (uint32_t)(zone < 0 ? -zone : zone), zh = az / 60u;
    const uint64_t zmm = time_two(az - zh * 60u);
    *w2 = (uint64_t)':' | (time_two(ss) << 8) | ((uint64_t)(zone < 0 ? '-' : '+') << 24) | (time_two(zh) << 32) | ((uint64_t)':' << 48) | ((zmm & 0xFFull) << 56);
    *w3 = zmm >> 8;
}

}  // namespace cph
