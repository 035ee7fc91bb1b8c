// strpred_device.hpp — the string conditions that look INSIDE a value (filter.hip: CPH_PRED_STR_* / HAS_PREFIX / HAS_SUFFIX /
// CONTAINS) and the span of a slice (map_device.hpp: CPH_MAP_SLICE), as plain byte routines: strings.Compare, HasPrefix,
// HasSuffix, Contains and s[a:b] are byte operations, nothing here knows about runes.
//
// Everything is __host__ __device__ and written over two small functors, so that the very same code compiles with a plain
// host compiler (tests/cpp/test_strpred.cpp) and inside k_pred_eval:
//   V   uint64_t v(uint64_t off, uint64_t len, int j): bytes [off + 8j, off + 8j + 8) of the VALUE, little-endian, where
//       [off, off + len) is a span inside the value; bytes past the span are unspecified, and the functor reads nothing
//       but the aligned 8-byte words that hold a byte of the span (device_utils.hpp: load_value_chunk's contract);
//   L   uint64_t lit(uint64_t j): word j of the LITERAL, little-endian, zero padded to whole words.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CPH_HD __host__ __device__ __forceinline__
#else
#define CPH_HD inline
#endif

namespace cph {

// the low nb (1..) bytes of a chunk
CPH_HD uint64_t str_valid_mask(uint64_t nb) { return nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1); }

// 0x80 in every byte of w that equals the byte replicated in pat (exact: no carry crosses a byte)
CPH_HD uint64_t str_eq_mask8(uint64_t w, uint64_t pat) {
    const uint64_t x = w ^ pat, k = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & k) + k) | x | k);
}

// value bytes [off, off + len) == the literal's first len bytes
template <class V, class L>
CPH_HD bool str_equal_at(const V& v, uint64_t off, uint64_t len, const L& lit) {
    for (uint64_t j = 0; 8 * j < len; j++) {
        const uint64_t chunk = v(off, len, (int)j);
        if ((chunk ^ lit(j)) & str_valid_mask(len - 8 * j)) return false;
    }
    return true;
}

// strings.Compare(value, literal): -1 / 0 / +1, bytewise and unsigned.  The first chunk that differs inside the common
// length decides by its big-endian words (the chunks are little-endian: the first byte is the lowest); no such chunk: the
// shorter one is the smaller.
template <class V, class L>
CPH_HD int str_compare(const V& v, uint64_t vlen, const L& lit, uint64_t llen) {
    const uint64_t m = vlen < llen ? vlen : llen;
    for (uint64_t j = 0; 8 * j < m; j++) {
        const uint64_t valid = str_valid_mask(m - 8 * j);
        const uint64_t a = v(0, m, (int)j) & valid, b = lit(j) & valid;
        if (a != b) return __builtin_bswap64(a) < __builtin_bswap64(b) ? -1 : 1;
    }
    return vlen < llen ? -1 : vlen > llen ? 1 : 0;
}

template <class V, class L>
CPH_HD bool str_has_prefix(const V& v, uint64_t vlen, const L& lit, uint64_t llen) {
    return llen <= vlen && str_equal_at(v, 0, llen, lit);
}

// the literal against the value's last llen bytes: an unaligned start, read as the span (vlen - llen, llen)
template <class V, class L>
CPH_HD bool str_has_suffix(const V& v, uint64_t vlen, const L& lit, uint64_t llen) {
    return llen <= vlen && str_equal_at(v, vlen - llen, llen, lit);
}

// strings.Contains(value, literal).  The vlen - llen + 1 start positions are filtered 8 at a time with the byte-equality
// mask on the literal's first byte; every candidate is verified against the whole literal.  Quadratic on a value that
// repeats the literal's first byte and mismatches late ("aaaa…a" against "aa…ab"): every step still advances — the
// candidate mask loses a bit, or the position moves on by 8 — so it terminates.
template <class V, class L>
CPH_HD bool str_contains(const V& v, uint64_t vlen, const L& lit, uint64_t llen) {
    if (llen == 0) return true;
    if (llen > vlen) return false;
    const uint64_t npos = vlen - llen + 1;
    const uint64_t pat = (lit(0) & 0xFFull) * 0x0101010101010101ull;
    for (uint64_t p = 0; p < npos; p += 8) {
        const uint64_t cnt = npos - p < 8 ? npos - p : 8;
        uint64_t cand = str_eq_mask8(v(p, cnt, 0), pat) & str_valid_mask(cnt);
        while (cand) {
            const uint64_t k = (uint64_t)__builtin_ctzll(cand) >> 3;
            cand &= cand - 1;
            if (str_equal_at(v, p + k, llen, lit)) return true;
        }
    }
    return false;
}

// bytes [from, to) of a value of `len` bytes under Python's slice rules: a negative index counts from the end, both ends are
// clamped into [0, len], from >= to is empty (to == INT64_MAX: to the end, by the clamp).  *off, *n: the span inside the value.
CPH_HD void slice_span(uint64_t len, int64_t from, int64_t to, uint64_t* off, uint64_t* n) {
    const int64_t l = len > 0x7FFFFFFFFFFFFFFFull ? 0x7FFFFFFFFFFFFFFFll : (int64_t)len;
    const int64_t f = from < 0 ? (from + l < 0 ? 0 : from + l) : (from < l ? from : l);
    const int64_t t = to < 0 ? (to + l < 0 ? 0 : to + l) : (to < l ? to : l);
    *off = (uint64_t)f;
    *n = t > f ? (uint64_t)(t - f) : 0;
}

}  // namespace cph
