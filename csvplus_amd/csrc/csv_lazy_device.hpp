// csv_lazy_device.hpp — the byte automaton that finds the record separators of a CSV text under Go's LazyQuotes rules
// (encoding/csv readRecord with LazyQuotes = true), as csv_ingest.hip's lazy passes run it.  Everything here compiles for
// the host as well (tests/cpp/test_csv_lazy.cpp walks texts with it on the CPU and the Python line model checks the result).
//
// Under lazy rules a quote toggles nothing by itself (`a"b,c` holds no quoted field, `"a"b` does not close its field), so the
// strict passes' quote PARITY cannot say which newlines end a record.  Seven states can:
//   RS record start   FS field start   UQ in an unquoted field   QD in a quoted field   QS a quote seen inside a quoted field
//   QC QS followed by '\r'             CM comment line
// A '\n' is a record separator iff the state in front of it is not QD; behind a separator the state is RS.
//
// A stretch of text acts on the state as a MAP state -> state; maps compose associatively (not commutatively), which is what
// lets lanes, waves, tiles and the whole text be scanned in parallel.  A map lives in registers as EIGHT BYTES (byte s = where
// state s goes; byte 7 stays 7), because then  (a then b)[s] = b[a[s]]  is two v_perm_b32: the map's own bytes are the
// selectors.  A packed lookup per state in one 32-bit word (7 nibbles) costs a shift, an extract and an insert per state —
// about 30 instructions per composition where this takes 2; the nibble form is kept for the one word per tile that goes through
// global memory.  The per-byte step is the same composition with the byte's CLASS map (quote, Comma, '\r', space, comment
// character, newline, anything else: seven maps the host derives from the options, held in scalar registers), so a chunk of
// 16 bytes costs 16 x (class selection + 2 v_perm_b32) whatever its start state, and the SAME walk, started from a map whose
// bytes all hold the one true entry state, yields that state in front of every byte — the separators.
#pragma once

#include <cstdint>

#ifndef CPH_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CPH_HD __host__ __device__ __forceinline__
#else
#define CPH_HD inline
#endif
#endif

namespace cph {

enum : uint32_t { kLzRS = 0, kLzFS = 1, kLzUQ = 2, kLzQD = 3, kLzQS = 4, kLzQC = 5, kLzCM = 6, kLzStates = 7 };
enum : int { kLzQuote = 0, kLzComma, kLzCR, kLzSpace, kLzComment, kLzNewline, kLzOther, kLzClasses };

struct LzMap {
    uint32_t lo, hi;   // byte s of (hi:lo) = the state that state s goes to
};
struct LzTable {
    LzMap cls[kLzClasses];
    uint32_t comma;
    uint32_t comment;   // 0x100 = none (no byte equals it)
    uint32_t trim;
};

// v_perm_b32: byte i of the result = byte sel[i] (0..7) of the eight bytes hi:lo
CPH_HD uint32_t lz_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= (uint32_t)((src >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
#endif
}
CPH_HD LzMap lz_identity() { return LzMap{0x03020100u, 0x07060504u}; }
CPH_HD LzMap lz_constant(uint32_t s) { return LzMap{s * 0x01010101u, s * 0x01010101u}; }   // every state (and byte 7) -> s
// a first, then b
CPH_HD LzMap lz_compose(const LzMap& a, const LzMap& b) { return LzMap{lz_perm(b.hi, b.lo, a.lo), lz_perm(b.hi, b.lo, a.hi)}; }
CPH_HD uint32_t lz_apply(const LzMap& m, uint32_t s) { return ((s < 4 ? m.lo : m.hi) >> (8 * (s & 3))) & 0xFFu; }
// seven nibbles in one word: the form a tile's map has in global memory
CPH_HD uint32_t lz_pack(const LzMap& m) {
    uint32_t r = 0;
    for (uint32_t s = 0; s < kLzStates; s++) r |= lz_apply(m, s) << (4 * s);
    return r;
}
CPH_HD LzMap lz_unpack(uint32_t p) {
    LzMap m{0, 0x07000000u};
    for (uint32_t s = 0; s < 4; s++) m.lo |= ((p >> (4 * s)) & 7u) << (8 * s);
    for (uint32_t s = 4; s < kLzStates; s++) m.hi |= ((p >> (4 * s)) & 7u) << (8 * (s - 4));
    return m;
}

// The transition table (host): TrimLeadingSpace makes ASCII spaces and '\r' in front of a field part of "field start"; the
// comment character opens a comment only at a record's first byte.  (The multi-byte spaces of unicode.IsSpace are not in here:
// csv_ingest.hip detects the one case where that matters.)
inline uint32_t lz_next(uint32_t s, int cls, bool trim) {
    if (cls == kLzNewline) return s == kLzQD ? kLzQD : kLzRS;
    switch (s) {
    case kLzRS:
    case kLzFS:
        if (cls == kLzQuote) return kLzQD;
        if (cls == kLzComma) return kLzFS;
        if (cls == kLzCR || cls == kLzSpace) return trim ? kLzFS : kLzUQ;
        if (cls == kLzComment && s == kLzRS) return kLzCM;
        return kLzUQ;
    case kLzUQ: return cls == kLzComma ? kLzFS : kLzUQ;
    case kLzQD: return cls == kLzQuote ? kLzQS : kLzQD;
    case kLzQS:
        if (cls == kLzQuote) return kLzQD;   // "" = one literal quote
        if (cls == kLzComma) return kLzFS;   // the field ends
        if (cls == kLzCR) return kLzQC;      // ends field and record if a newline follows
        return kLzQD;                        // a literal quote, the field stays quoted
    case kLzQC: return cls == kLzQuote ? kLzQS : kLzQD;   // the quote and the '\r' were content; this byte is read in QD
    default: return kLzCM;
    }
}
inline LzTable lz_table(uint8_t comma, uint8_t comment, bool trim) {
    LzTable t{};
    for (int c = 0; c < kLzClasses; c++) {
        LzMap m{0, 0x07000000u};
        for (uint32_t s = 0; s < kLzStates; s++) {
            const uint32_t n = lz_next(s, c, trim);
            if (s < 4) m.lo |= n << (8 * s);
            else m.hi |= n << (8 * (s - 4));
        }
        t.cls[c] = m;
    }
    t.comma = comma;
    t.comment = comment ? comment : 0x100u;
    t.trim = trim ? 1u : 0u;
    return t;
}

// The 16 bytes w[0..3] (little-endian words, text order) act on `cur`; returns cur followed by them.  SEPS: *seps gets bit i
// for every '\n' at byte i that ends a record when byte 0 of cur is the state in front of the chunk (lz_constant of it).
// Class precedence as in readRecord: newline, quote, Comma, '\r', comment character, space.
template <bool TRIM, bool CMT, bool SEPS>
CPH_HD LzMap lz_walk16(const uint32_t (&w)[4], const LzTable& t, LzMap cur, uint32_t* seps) {
    uint32_t sep = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 16; i++) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        LzMap m = t.cls[kLzOther];
        if (TRIM && (c == ' ' || c - 9u <= 4u)) m = t.cls[kLzSpace];
        if (CMT && c == t.comment) m = t.cls[kLzComment];
        if (c == '\r') m = t.cls[kLzCR];
        if (c == t.comma) m = t.cls[kLzComma];
        if (c == '"') m = t.cls[kLzQuote];
        if (c == '\n') m = t.cls[kLzNewline];
        if (SEPS && c == '\n' && (cur.lo & 0xFFu) != kLzQD) sep |= 1u << i;
        cur = lz_compose(cur, m);
    }
    if (SEPS) *seps = sep;
    return cur;
}

}  // namespace cph
