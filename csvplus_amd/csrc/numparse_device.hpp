// numparse_device.hpp — string -> int64 / float64 on the device with Go's strconv semantics (Row.ValueAsInt /
// Row.ValueAsFloat64, csvplus.go:165-205): the per-value pieces numparse.hip (whole columns) and filter.hip (numeric
// compare terms) share.  The rules are restated from strconv's published behaviour in include/csvplus_hip.h
// (cph_col_to_number) and DESIGN.md; the reference tree itself only pins the two error strings.
//
// A value of at most 16 bytes — the common case — never loops over its bytes: its two 8-byte chunks are XORed with
// 0x30 per byte (for the digits '0'..'9' that IS the subtraction of 0x30, and it cannot borrow into the neighbour),
// one carry-free range test per chunk says whether every byte is a digit, and three multiply-and-shift steps per
// chunk turn 8 digits into their number.  Longer values (leading zeros, 17+ digits, exponents) take a byte loop over
// the value's chunks.
#pragma once

#include "materialize_device.hpp"

namespace cph {

constexpr uint8_t kNumDeferred = 0x80;   // float: valid syntax, but not decided on the device (never leaves the library)

constexpr uint64_t kAscii0x8 = 0x3030303030303030ull;

__device__ __forceinline__ uint64_t low_bytes_mask(uint32_t n) { return n >= 8u ? ~0ull : ((1ull << (8u * n)) - 1ull); }

// x = 8 bytes ^ '0': every byte is 0..9
__device__ __forceinline__ bool all_digits8(uint64_t x) {
    return (((x + 0x0606060606060606ull) | x) & 0xF0F0F0F0F0F0F0F0ull) == 0;
}

// 8 digit VALUES (0..9 per byte, the first digit in the lowest byte) -> their number
__device__ __forceinline__ uint64_t digits8_value(uint64_t x) {
    x = (x * 2561ull) >> 8;                                          // pairs:  10 * d0 + d1
    x = ((x & 0x00FF00FF00FF00FFull) * 6553601ull) >> 16;            // quads: 100 * p0 + p1
    return ((x & 0x0000FFFF0000FFFFull) * 42949672960001ull) >> 32;  // 10000 * q0 + q1
}

// nd (1..16) digit values in the low bytes of lo:hi (first digit lowest, the bytes above them zero) -> their number (< 10^16)
__device__ __forceinline__ uint64_t digits16_value(uint64_t lo, uint64_t hi, uint32_t nd) {
    const uint32_t s = 16u - nd, sh = (s & 7u) * 8u;   // leading zeros in front: the digits move up by s bytes
    const uint64_t a = lo << sh, b = (hi << sh) | (sh ? lo >> (64u - sh) : 0ull);
    const uint64_t first = s >= 8u ? 0ull : a, second = s >= 8u ? a : b;
    return digits8_value(first) * 100000000ull + digits8_value(second);
}

// The first 16 bytes of a value with two unconditional loads (device_utils.hpp: load_chunk_nobranch); the bytes past the
// value's end are zero.
__device__ __forceinline__ void load_head16(const DevCol& col, uint64_t begin, uint64_t len, uint64_t* c0, uint64_t* c1) {
    const uint64_t p = (uint64_t)(uintptr_t)col.data;
    const uint8_t* base8 = (const uint8_t*)(uintptr_t)(p & ~7ull);
    const uint32_t delta = (uint32_t)(p & 7ull);
    const uint32_t l32 = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    const uint64_t a = load_chunk_nobranch<uint64_t>(base8, delta, begin, l32, 0);
    const uint64_t b = load_chunk_nobranch<uint64_t>(base8, delta, begin, l32, 1);
    *c0 = l32 > 0u ? a & low_bytes_mask(l32) : 0ull;
    *c1 = l32 > 8u ? b & low_bytes_mask(l32 - 8u) : 0ull;
}

// A value's bytes one at a time: chunks 0 and 1 come from the head, later ones from memory as the reader gets there.
struct ByteReader {
    const DevCol& col;
    uint64_t begin, len, c0, c1, cur;
    uint64_t curj;
    __device__ __forceinline__ ByteReader(const DevCol& c, uint64_t b, uint64_t l, uint64_t h0, uint64_t h1)
        : col(c), begin(b), len(l), c0(h0), c1(h1), cur(h0), curj(0) {}
    __device__ __forceinline__ uint64_t chunk(uint64_t j) {
        if (j != curj) {
            cur = j == 0 ? c0 : j == 1 ? c1 : load_value_chunk(col.data, begin, len, (int)j);
            curj = j;
        }
        return cur;
    }
    __device__ __forceinline__ uint32_t at(uint64_t i) { return (uint32_t)(chunk(i >> 3) >> (8u * (uint32_t)(i & 7u))) & 0xFFu; }   // i < len
};

// strconv.Atoi on a 64-bit int.  Returns CPH_NUM_*; *out = what Go returns beside the error.
__device__ __forceinline__ uint32_t parse_int64(const DevCol& col, uint64_t begin, uint64_t len, uint64_t c0, uint64_t c1, int64_t* out) {
    *out = 0;
    if (len == 0) return CPH_NUM_ERR_SYNTAX;
    const uint32_t b0 = (uint32_t)c0 & 0xFFu;
    const bool neg = b0 == '-';
    const uint32_t sg = (neg || b0 == '+') ? 1u : 0u;
    if (len <= 16) {
        const uint32_t nd = (uint32_t)len - sg;
        if (nd == 0) return CPH_NUM_ERR_SYNTAX;
        const uint64_t lo = sg ? (c0 >> 8) | (c1 << 56) : c0, hi = sg ? c1 >> 8 : c1;
        const uint64_t xl = (lo ^ kAscii0x8) & low_bytes_mask(nd), xh = (hi ^ kAscii0x8) & low_bytes_mask(nd > 8u ? nd - 8u : 0u);
        if (!all_digits8(xl) || !all_digits8(xh)) return CPH_NUM_ERR_SYNTAX;
        const uint64_t mag = digits16_value(xl, xh, nd);   // < 10^16: always in range
        *out = neg ? -(int64_t)mag : (int64_t)mag;
        return CPH_NUM_OK;
    }
    // the unsigned accumulator of strconv.ParseUint: a byte that is no digit is a syntax error unless the accumulator
    // has overflowed 2^64 in front of it
    ByteReader rd(col, begin, len, c0, c1);
    uint64_t n = 0;
    for (uint64_t i = sg; i < len; i++) {
        const uint32_t d = rd.at(i) - (uint32_t)'0';
        if (d > 9u) return CPH_NUM_ERR_SYNTAX;
        const uint64_t n10 = n * 10ull, n1 = n10 + d;
        if (n > 0xFFFFFFFFFFFFFFFFull / 10ull || n1 < n10) {
            *out = neg ? INT64_MIN : INT64_MAX;
            return CPH_NUM_ERR_RANGE;
        }
        n = n1;
    }
    if (!neg && n >= (1ull << 63)) {
        *out = INT64_MAX;
        return CPH_NUM_ERR_RANGE;
    }
    if (neg && n > (1ull << 63)) {
        *out = INT64_MIN;
        return CPH_NUM_ERR_RANGE;
    }
    *out = neg ? (int64_t)(0ull - n) : (int64_t)n;
    return CPH_NUM_OK;
}

__device__ __forceinline__ double pow10_exact(int k) {   // 0..22: the powers of ten a double holds exactly
    static constexpr double p[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return p[k];
}

// Clinger's exact cases (strconv's atof64exact): mant != 0, not truncated.  One correctly rounded IEEE operation each
// (this file must not be built with fast-math or reciprocal division).  false: the caller defers the value.
__device__ __forceinline__ bool float_exact(uint64_t mant, int exp10, bool neg, double* out) {
    if (mant >> 53) return false;
    double f = (double)mant;
    if (neg) f = -f;
    if (exp10 == 0) {
        *out = f;
        return true;
    }
    if (exp10 > 0 && exp10 <= 15 + 22) {
        if (exp10 > 22) {
            f *= pow10_exact(exp10 - 22);
            exp10 = 22;
        }
        if (f > 1e15 || f < -1e15) return false;
        *out = f * pow10_exact(exp10);
        return true;
    }
    if (exp10 < 0 && exp10 >= -22) {
        *out = f / pow10_exact(-exp10);
        return true;
    }
    return false;
}

__device__ __forceinline__ double signed_zero(bool neg) { return neg ? -0.0 : 0.0; }
__device__ __forceinline__ double signed_inf(bool neg) { return __longlong_as_double(neg ? 0xFFF0000000000000ll : 0x7FF0000000000000ll); }

// What becomes of a valid value outside Clinger's exact cases — (first <= 19 significant digits != 0, decimal exponent, non-zero
// digits dropped behind them, sign) -> CPH_NUM_* with *out set, or kNumDeferred.  This one defers them all.
struct FloatBeyondDefer {
    __device__ __forceinline__ uint32_t operator()(uint64_t, int, bool, bool, double*) const { return kNumDeferred; }
};

// strconv.ParseFloat(s, 64).  Returns CPH_NUM_* or kNumDeferred (valid syntax; the library's host side finishes the value);
// *out = what Go returns beside the error (0 for a deferred row until it is patched).  `beyond` decides the values Clinger's
// cases leave (numparse.hip: the Eisel-Lemire conversion of floatparse_device.hpp).
template <class Beyond = FloatBeyondDefer>
__device__ __forceinline__ uint32_t parse_float64(const DevCol& col, uint64_t begin, uint64_t len, uint64_t c0, uint64_t c1, double* out,
                                                  const Beyond beyond = Beyond{}) {
    *out = 0.0;
    if (len == 0) return CPH_NUM_ERR_SYNTAX;
    const uint32_t b0 = (uint32_t)c0 & 0xFFu;
    const bool neg = b0 == '-';
    const uint32_t sg = (neg || b0 == '+') ? 1u : 0u;
    if (len <= 16) {   // digits with at most one '.', nothing else: the '.' is squeezed out and the digits are one number
        const uint32_t nd = (uint32_t)len - sg;
        if (nd == 0) return CPH_NUM_ERR_SYNTAX;
        const uint64_t lo = sg ? (c0 >> 8) | (c1 << 56) : c0, hi = sg ? c1 >> 8 : c1;
        const uint64_t ml = low_bytes_mask(nd), mh = low_bytes_mask(nd > 8u ? nd - 8u : 0u);
        const uint64_t xl = (lo ^ kAscii0x8) & ml, xh = (hi ^ kAscii0x8) & mh;
        const uint64_t dotpat = 0x1E1E1E1E1E1E1E1Eull;   // '.' ^ '0'
        const uint64_t dl = eq_mask8(xl, dotpat) & ml, dh = eq_mask8(xh, dotpat) & mh;
        const uint32_t ndots = (uint32_t)__popcll(dl) + (uint32_t)__popcll(dh);
        if (ndots <= 1u) {
            const uint32_t p = !ndots ? nd : dl ? (uint32_t)__builtin_ctzll(dl) >> 3 : 8u + ((uint32_t)__builtin_ctzll(dh) >> 3);
            uint64_t yl = xl, yh = xh;
            if (ndots) {   // bytes in front of p stay, the bytes behind it move down by one
                const uint64_t sl = (xl >> 8) | (xh << 56), sh = xh >> 8;   // everything moved down by one byte
                const uint64_t keep_l = low_bytes_mask(p), keep_h = low_bytes_mask(p > 8u ? p - 8u : 0u);
                yl = (xl & keep_l) | (sl & ~keep_l);
                yh = p >= 8u ? (xh & keep_h) | (sh & ~keep_h) : sh;
            }
            const uint32_t k = nd - ndots;
            if (k == 0) return CPH_NUM_ERR_SYNTAX;   // "." alone
            if (all_digits8(yl) && all_digits8(yh)) {
                const uint64_t mant = digits16_value(yl, yh, k);
                if (mant == 0) {
                    *out = signed_zero(neg);
                    return CPH_NUM_OK;
                }
                const int exp10 = ndots ? -(int)(nd - 1u - p) : 0;   // at least -15
                return float_exact(mant, exp10, neg, out) ? CPH_NUM_OK : beyond(mant, exp10, false, neg, out);
            }
        }
    }
    // the general grammar, byte by byte (strconv's readFloat)
    ByteReader rd(col, begin, len, c0, c1);
    for (uint64_t j = 0; 8 * j < len; j++) {
        const uint64_t nb = len - 8 * j;
        if (eq_mask8(rd.chunk(j), 0x5F5F5F5F5F5F5F5Full) & low_bytes_mask(nb >= 8 ? 8u : (uint32_t)nb)) return CPH_NUM_ERR_UNSUPPORTED;   // '_'
    }
    uint64_t i = sg;
    const uint64_t rem = len - i;
    if (rem >= 2 && rd.at(i) == '0' && (rd.at(i + 1) | 0x20u) == 'x') return CPH_NUM_ERR_UNSUPPORTED;
    if (rem == 3 || rem == 8) {   // inf, infinity, nan (no sign), ASCII case-insensitive
        const uint64_t w = ((sg ? (c0 >> 8) | (c1 << 56) : c0) | 0x2020202020202020ull) & low_bytes_mask((uint32_t)rem);
        if (w == (rem == 3 ? 0x666E69ull : 0x7974696E69666E69ull)) {   // "inf" / "infinity", little-endian
            *out = signed_inf(neg);
            return CPH_NUM_OK;
        }
        if (rem == 3 && !sg && w == 0x6E616Eull) {   // "nan"
            *out = __longlong_as_double(0x7FF8000000000001ll);   // the bits of Go's math.NaN()
            return CPH_NUM_OK;
        }
    }
    bool sawdot = false, sawdigits = false, trunc = false;
    int nd = 0, ndmant = 0, dp = 0;
    uint64_t mant = 0;
    for (; i < len; i++) {
        const uint32_t c = rd.at(i);
        if (c == '.') {
            if (sawdot) break;
            sawdot = true;
            dp = nd;
            continue;
        }
        const uint32_t d = c - (uint32_t)'0';
        if (d > 9u) break;
        sawdigits = true;
        if (d == 0 && nd == 0) {   // leading zeros are not significant
            dp--;
            continue;
        }
        if (nd < 0x3FFFFFFF) nd++;
        if (ndmant < 19) {
            mant = mant * 10ull + d;
            ndmant++;
        } else if (d != 0) {
            trunc = true;
        }
    }
    if (!sawdigits) return CPH_NUM_ERR_SYNTAX;
    if (!sawdot) dp = nd;
    if (i < len && (rd.at(i) | 0x20u) == 'e') {
        i++;
        if (i >= len) return CPH_NUM_ERR_SYNTAX;
        int esign = 1;
        const uint32_t c = rd.at(i);
        if (c == '+' || c == '-') {
            esign = c == '-' ? -1 : 1;
            i++;
        }
        if (i >= len || rd.at(i) - (uint32_t)'0' > 9u) return CPH_NUM_ERR_SYNTAX;
        int e = 0;
        for (; i < len; i++) {
            const uint32_t d = rd.at(i) - (uint32_t)'0';
            if (d > 9u) break;
            if (e < 10000) e = e * 10 + (int)d;
        }
        dp += e * esign;
    }
    if (i != len) return CPH_NUM_ERR_SYNTAX;
    if (mant == 0) {
        *out = signed_zero(neg);
        return CPH_NUM_OK;
    }
    if (trunc) return beyond(mant, dp - ndmant, true, neg, out);
    return float_exact(mant, dp - ndmant, neg, out) ? CPH_NUM_OK : beyond(mant, dp - ndmant, false, neg, out);
}

}  // namespace cph
