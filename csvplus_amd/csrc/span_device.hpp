// span_device.hpp — the operations of a CPH_MAP_SPAN piece (map_device.hpp): a column value NARROWED to a sub-span of itself
// by a short program — strings.TrimSpace / TrimLeft / TrimRight / Trim / TrimPrefix / TrimSuffix, one field of strings.Split /
// SplitN (strings.Cut falls out of it) and s[a:b].  No byte changes: every routine takes a span (off, len) inside the value and
// leaves a span inside that one.  Plain byte routines; the only thing here that knows about runes is the list of the 25 byte
// sequences that are unicode.IsSpace.
//
// Everything is __host__ __device__ and written over the functors of strpred_device.hpp, so that the very same code compiles
// with a plain host compiler (tests/cpp/test_span.cpp, the host row model of csvplus.hpp) and inside the Map kernels:
//   V   uint64_t v(uint64_t off, uint64_t len, int j): bytes [off + 8j, off + 8j + 8) of the VALUE, where [off, off + len) is a
//       span inside the value; nothing but the aligned 8-byte words that hold a byte of that span is read (load_value_chunk's
//       contract).  No routine asks for a chunk of an empty span, and none reads a byte outside the value;
//   LB  L lb(uint32_t off, uint32_t len): the literal of `len` bytes at byte `off` of the plan's literal block, as a functor L
//       with uint64_t lit(uint64_t j) = its word j, 8 j < len (bytes past its end are unspecified and masked here).
//
// One lane runs one row's whole program: correct for any value length, and tuned for CSV-sized values (tens of bytes: a value
// is a handful of 8-byte chunks, a trim looks at one chunk per end, a field search at one chunk per 8 positions).  A value of
// kilobytes keeps one lane busy for its whole length while its wave waits.
#pragma once

#include "strpred_device.hpp"

namespace cph {

enum : int32_t { kSpanTrimSpace = 1, kSpanTrimCutset = 2, kSpanTrimPrefix = 3, kSpanTrimSuffix = 4, kSpanField = 5, kSpanSlice = 6 };   // CPH_SPAN_*
enum : int32_t { kSpanLeft = 1, kSpanRight = 2 };   // the bits of a trim's mode

// One operation as the kernels see it: 24 bytes, and a plan carries at most 16.
struct SpanOp {
    int32_t op;     // kSpan*
    int32_t mode;   // TRIM_SPACE / TRIM_CUTSET: kSpanLeft | kSpanRight; FIELD: the limit (-1, or >= 1)
    int64_t a;      // SLICE: from; FIELD: the index k; TRIM_CUTSET: bits 0..63 of the set's bitmap
    union {
        int64_t b;                        // SLICE: to; TRIM_CUTSET: bits 64..127
        struct { uint32_t lit_off, lit_len; };   // TRIM_PREFIX / TRIM_SUFFIX / FIELD: the literal's bytes in the literal block
    };
};

constexpr uint64_t kSpanHi = 0x8080808080808080ull;

// 0x80 in every byte of w that is one of \t \n \v \f \r ' ' (exact: the sums stay inside their bytes)
CPH_HD uint64_t span_ascii_space_mask(uint64_t w) {
    const uint64_t x = w & 0x7F7F7F7F7F7F7F7Full;
    const uint64_t ge9 = x + 0x7777777777777777ull;     // bit 7: x >= 9
    const uint64_t gt13 = x + 0x7272727272727272ull;    // bit 7: x >= 14
    return ((ge9 & ~gt13 & ~w) | str_eq_mask8(w, 0x2020202020202020ull)) & kSpanHi;
}

// bytes of the non-ASCII space whose encoding starts the word t (byte 0 first; nb = the bytes of t that count): 0, 2 or 3
CPH_HD uint32_t span_wide_space(uint64_t t, uint64_t nb) {
    const uint32_t b0 = (uint32_t)(t & 0xFFu), b1 = (uint32_t)((t >> 8) & 0xFFu), b2 = (uint32_t)((t >> 16) & 0xFFu);
    if (nb >= 2 && b0 == 0xC2u) return (b1 == 0x85u || b1 == 0xA0u) ? 2u : 0u;
    if (nb < 3) return 0u;
    if (b0 == 0xE2u) {
        if (b1 == 0x80u) return ((b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu) ? 3u : 0u;
        return (b1 == 0x81u && b2 == 0x9Fu) ? 3u : 0u;
    }
    if (b0 == 0xE1u) return (b1 == 0x9Au && b2 == 0x80u) ? 3u : 0u;
    if (b0 == 0xE3u) return (b1 == 0x80u && b2 == 0x80u) ? 3u : 0u;
    return 0u;
}

// strings.TrimLeftFunc(s, unicode.IsSpace) on the span: the longest run of space sequences at its head goes
template <class V>
CPH_HD void span_trim_left_space(const V& v, uint64_t* off, uint64_t* len) {
    while (*len) {
        const uint64_t n = *len < 8 ? *len : 8;
        const uint64_t w = v(*off, *len, 0);
        const uint64_t stop = (~span_ascii_space_mask(w) & kSpanHi) & str_valid_mask(n);   // 0x80 in every byte that is no ASCII space
        const uint64_t c = stop ? (uint64_t)__builtin_ctzll(stop) >> 3 : n;
        if (c) {
            *off += c, *len -= c;
            if (c < n && ((w >> (8 * c)) & 0xFFu) < 0xC2u) return;   // the byte that stopped the run starts no space
            continue;                                               // a new chunk, with that byte in front
        }
        const uint32_t m = span_wide_space(w, n);
        if (!m) return;
        *off += m, *len -= m;
    }
}

// strings.TrimRightFunc(s, unicode.IsSpace): at the tail a sequence matches only with its start byte, utf8.DecodeLastRune's decision
template <class V>
CPH_HD void span_trim_right_space(const V& v, uint64_t off, uint64_t* len) {
    while (*len) {
        const uint64_t n = *len < 8 ? *len : 8;
        const uint64_t w = v(off + *len - n, n, 0);   // the last n bytes: the last one is byte n - 1
        const uint64_t stop = (~span_ascii_space_mask(w) & kSpanHi) & str_valid_mask(n);
        const uint64_t c = stop ? n - 1 - ((63u - (uint64_t)__builtin_clzll(stop)) >> 3) : n;
        if (c) {
            *len -= c;
            if (c < n && ((w >> (8 * (n - 1 - c))) & 0xFFu) < 0x80u) return;   // an ASCII byte that is no space
            continue;                                                         // a new chunk that ends at that byte
        }
        if (n >= 2) {
            const uint64_t t2 = (w >> (8 * (n - 2))) & 0xFFFFu;
            if (t2 == 0x85C2u || t2 == 0xA0C2u) {
                *len -= 2;
                continue;
            }
        }
        if (n >= 3 && span_wide_space(w >> (8 * (n - 3)), 3) == 3u) {
            *len -= 3;
            continue;
        }
        return;
    }
}

CPH_HD bool span_in_set(uint64_t lo, uint64_t hi, uint32_t byte) {
    return byte < 0x80u && (((byte < 64u ? lo : hi) >> (byte & 63u)) & 1ull);
}

// strings.TrimLeft(s, cutset) for an ASCII cutset, the 128-bit bitmap (lo, hi): bytewise is Go's result for every byte string
template <class V>
CPH_HD void span_trim_left_set(const V& v, uint64_t lo, uint64_t hi, uint64_t* off, uint64_t* len) {
    while (*len) {
        const uint64_t n = *len < 8 ? *len : 8;
        const uint64_t w = v(*off, *len, 0);
        uint64_t c = 0;
        while (c < n && span_in_set(lo, hi, (uint32_t)((w >> (8 * c)) & 0xFFu))) c++;
        *off += c, *len -= c;
        if (c < n) return;
    }
}

template <class V>
CPH_HD void span_trim_right_set(const V& v, uint64_t lo, uint64_t hi, uint64_t off, uint64_t* len) {
    while (*len) {
        const uint64_t n = *len < 8 ? *len : 8;
        const uint64_t w = v(off + *len - n, n, 0);
        uint64_t c = 0;
        while (c < n && span_in_set(lo, hi, (uint32_t)((w >> (8 * (n - 1 - c))) & 0xFFu))) c++;
        *len -= c;
        if (c < n) return;
    }
}

// the value seen from a span's first byte: what the affix tests and the search of strpred_device.hpp take
template <class V>
struct SpanView {
    const V& v;
    uint64_t base;
    CPH_HD uint64_t operator()(uint64_t off, uint64_t len, int j) const { return v(base + off, len, j); }
};

// the first position >= from at which the literal (llen >= 1 bytes) lies inside the span of `len` bytes, or UINT64_MAX.
// Candidates 8 positions at a time by the byte-equality mask on the literal's first byte; a literal of several bytes is
// verified at each (str_contains' search, with the position kept).
template <class V, class L>
CPH_HD uint64_t span_find(const V& v, uint64_t off, uint64_t len, uint64_t from, const L& lit, uint64_t llen) {
    if (llen > len) return UINT64_MAX;
    const uint64_t npos = len - llen + 1;
    const uint64_t pat = (lit(0) & 0xFFull) * 0x0101010101010101ull;
    const SpanView<V> sv{v, off};
    for (uint64_t p = from; p < npos; p += 8) {
        const uint64_t cnt = npos - p < 8 ? npos - p : 8;
        uint64_t cand = str_eq_mask8(v(off + p, cnt, 0), pat) & str_valid_mask(cnt);
        while (cand) {
            const uint64_t k = (uint64_t)__builtin_ctzll(cand) >> 3;
            cand &= cand - 1;
            if (llen == 1 || str_equal_at(sv, p + k, llen, lit)) return p + k;
        }
    }
    return UINT64_MAX;
}

// the separators strings.SplitN would consume in the span, at most `cap` of them: left to right, non-overlapping
template <class V, class L>
CPH_HD uint64_t span_count_seps(const V& v, uint64_t off, uint64_t len, const L& lit, uint64_t llen, uint64_t cap) {
    uint64_t count = 0;
    if (llen == 1) {   // every equal byte is a separator: count them a word at a time
        const uint64_t pat = (lit(0) & 0xFFull) * 0x0101010101010101ull;
        for (uint64_t p = 0; p < len && count < cap; p += 8) {
            const uint64_t cnt = len - p < 8 ? len - p : 8;
            count += (uint64_t)__builtin_popcountll(str_eq_mask8(v(off + p, cnt, 0), pat) & str_valid_mask(cnt));
        }
        return count < cap ? count : cap;
    }
    for (uint64_t p = 0; count < cap;) {
        const uint64_t at = span_find(v, off, len, p, lit, llen);
        if (at == UINT64_MAX) break;
        count++;
        p = at + llen;
    }
    return count;
}

// parts = strings.Split(s, sep) (limit -1) or strings.SplitN(s, sep, limit) (limit >= 1): the span becomes parts[k], or
// parts[len(parts) + k] for k < 0; an index outside parts gives the empty span (where Go panics).
template <class V, class L>
CPH_HD void span_field(const V& v, const L& lit, uint64_t llen, int64_t k, int32_t limit, uint64_t* off, uint64_t* len) {
    const uint64_t max_seps = limit < 0 ? UINT64_MAX : (uint64_t)(limit - 1);   // the last part keeps the rest
    if (k < 0) {
        const uint64_t nparts = span_count_seps(v, *off, *len, lit, llen, max_seps) + 1;
        if ((uint64_t)(-(k + 1)) >= nparts) {
            *len = 0;
            return;
        }
        k = (int64_t)(nparts - (uint64_t)(-(k + 1)) - 1);
    }
    if ((uint64_t)k > max_seps) {
        *len = 0;
        return;
    }
    uint64_t start = 0;
    for (uint64_t seen = 0; seen < (uint64_t)k; seen++) {
        const uint64_t at = span_find(v, *off, *len, start, lit, llen);
        if (at == UINT64_MAX) {
            *len = 0;
            return;
        }
        start = at + llen;
    }
    uint64_t end = *len;
    if ((uint64_t)k < max_seps) {
        const uint64_t at = span_find(v, *off, *len, start, lit, llen);
        if (at != UINT64_MAX) end = at;
    }
    *off += start;
    *len = end - start;
}

// the program ops[0 .. nops) on a value of vlen bytes, left to right: (*off, *len) = the span that is left
template <class V, class LB>
CPH_HD void span_run(const SpanOp* ops, int nops, const V& v, uint64_t vlen, const LB& lb, uint64_t* off, uint64_t* len) {
    uint64_t o = 0, l = vlen;
    for (int q = 0; q < nops; q++) {
        const SpanOp& op = ops[q];
        if (op.op == kSpanTrimSpace) {
            if (op.mode & kSpanLeft) span_trim_left_space(v, &o, &l);
            if (op.mode & kSpanRight) span_trim_right_space(v, o, &l);
        } else if (op.op == kSpanTrimCutset) {
            if (op.mode & kSpanLeft) span_trim_left_set(v, (uint64_t)op.a, (uint64_t)op.b, &o, &l);
            if (op.mode & kSpanRight) span_trim_right_set(v, (uint64_t)op.a, (uint64_t)op.b, o, &l);
        } else if (op.op == kSpanTrimPrefix) {
            if (op.lit_len && str_has_prefix(SpanView<V>{v, o}, l, lb(op.lit_off, op.lit_len), op.lit_len)) o += op.lit_len, l -= op.lit_len;
        } else if (op.op == kSpanTrimSuffix) {
            if (op.lit_len && str_has_suffix(SpanView<V>{v, o}, l, lb(op.lit_off, op.lit_len), op.lit_len)) l -= op.lit_len;
        } else if (op.op == kSpanField) {
            span_field(v, lb(op.lit_off, op.lit_len), op.lit_len, op.a, op.mode, &o, &l);
        } else {   // kSpanSlice
            uint64_t so, sn;
            slice_span(l, op.a, op.b, &so, &sn);
            o += so, l = sn;
        }
    }
    *off = o, *len = l;
}

}  // namespace cph
