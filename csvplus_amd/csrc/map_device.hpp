// map_device.hpp — the device pieces the two Map entry points share (map_format.hip: one template per column;
// map_switch.hip: the template of the first case that holds): a template piece as the kernels see it, FormatInt's digit
// count and characters, the field of a loaded record, the bytes one piece adds to a row (map_piece_bytes: the length pass)
// and the loop that puts a run of pieces into a byte sink (map_put_record: the copy pass).  The kernels keep their row and
// tile loops and what tells a row its run of pieces; what the entry points share on the host is in map_plan.hpp.  A SPAN piece
// (span_device.hpp: a column's value narrowed by a program of span operations) computes its span in both passes (map_span_of).
#pragma once

#include "materialize_device.hpp"
#include "numformat_device.hpp"
#include "shortfmt_device.hpp"
#include "span_device.hpp"
#include "strpred_device.hpp"
#include "timeparse_device.hpp"

namespace cph {

struct MapPiece {
    int32_t kind;          // CPH_MAP_*
    int32_t col;           // COLUMN / SLICE / SPAN: the column; FLOAT64: prec; TIME: the zone, minutes east of UTC; FLOAT64_SHORTEST: the format byte
    union {
        struct {
            uint32_t off, len;   // LITERAL: its bytes in the plan's literal block; SPAN: its operations [off, off + len) of the plan's
        };
        int64_t from;            // SLICE: bytes [from, to) of the value, Python's slice rules (strpred_device.hpp: slice_span)
    };
    union {
        const int64_t* ints;    // INT64 / TIME: one value per output row, on the device
        const double* floats;   // FLOAT64 / FLOAT64_SHORTEST: likewise
        int64_t to;             // SLICE
    };
};

// The piece kinds an instantiation of the Map kernels carries code for.  A template launches the smallest set that holds
// its pieces, so one of LITERAL / COLUMN / INT64 pieces alone launches the kernels it always launched.
enum : int { kPiecesBase = 0,     // LITERAL, COLUMN, INT64
             kPiecesSlice = 1,    // + SLICE
             kPiecesFloat = 2,    // + SLICE, FLOAT64 (the formatter's registers) and TIME: the pieces whose values can be refused
             kPiecesShortest = 3 };  // + all of those and FLOAT64_SHORTEST (shortfmt_device.hpp: the digit generator's registers)
__host__ __device__ constexpr int pieces_set(bool has_shortest, bool has_float, bool has_slice) {
    return has_shortest ? kPiecesShortest : has_float ? kPiecesFloat : has_slice ? kPiecesSlice : kPiecesBase;
}

// A SPAN piece (span_device.hpp) is no member of those sets: an instantiation carries its code where the second template
// parameter SP is set, and the entry points instantiate SP only over kPiecesSlice (a span-only template does not pay the
// float formatters' registers) and over kPiecesShortest (SPAN beside any other piece).  Without SP nothing changes.
__host__ __device__ constexpr int span_pieces_set(int pk) { return pk >= kPiecesFloat ? kPiecesShortest : kPiecesSlice; }

// a column's value and the plan's literal block as span_device.hpp reads them
struct SpanValue {
    const uint8_t* data;
    uint64_t begin;
    __device__ __forceinline__ uint64_t operator()(uint64_t off, uint64_t len, int j) const { return load_value_chunk(data, begin + off, len, j); }
};
struct SpanLiteral {
    const uint8_t* lits;
    uint32_t off, len;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return load_value_chunk(lits, off, len, (int)j); }
};
struct SpanLiterals {
    const uint8_t* lits;
    __device__ __forceinline__ SpanLiteral operator()(uint32_t off, uint32_t len) const { return SpanLiteral{lits, off, len}; }
};

__device__ __forceinline__ uint64_t int_magnitude(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }

// characters of strconv.FormatInt(v, 10): the digits of the unsigned magnitude (compares against 10^1 .. 10^19) + the sign
__device__ __forceinline__ uint32_t int_chars(int64_t v) {
    const uint64_t m = int_magnitude(v);
    uint32_t d = 1;
    uint64_t p = 10;
#pragma unroll
    for (int k = 1; k <= 19; k++) {
        d += m >= p ? 1u : 0u;
        p *= 10;   // 10^19 < 2^64; the product behind it is never compared
    }
    return d + (v < 0 ? 1u : 0u);
}

// the characters assembled in registers — at most 20, three 8-byte chunks — and put 8 at a time
template <class Sink>
__device__ __forceinline__ void put_int(Sink& s, int64_t v) {
    uint64_t m = int_magnitude(v);
    const uint32_t len = int_chars(v);
    uint64_t c0 = v < 0 ? (uint64_t)'-' : 0, c1 = 0, c2 = 0;
    uint32_t pos = len;
    do {
        const uint64_t q = m / 10;
        const uint64_t ch = (uint64_t)'0' + (m - q * 10);
        m = q;
        pos--;
        const uint64_t sh = ch << (8u * (pos & 7u));
        if (pos < 8u) c0 |= sh;
        else if (pos < 16u) c1 |= sh;
        else c2 |= sh;
    } while (m);
    s.put8(c0, len < 8u ? len : 8u);
    if (len > 8u) s.put8(c1, len < 16u ? len - 8u : 8u);
    if (len > 16u) s.put8(c2, len - 16u);
}

// the 20 or 25 characters of a CPH_MAP_TIME piece (timeparse_device.hpp), assembled in registers
template <class Sink>
__device__ __forceinline__ void put_time(Sink& s, int64_t v, int32_t zone) {
    uint64_t w0, w1, w2, w3;
    rfc3339_words(v, zone, &w0, &w1, &w2, &w3);
    s.put8(w0, 8u);
    s.put8(w1, 8u);
    s.put8(w2, zone == 0 ? 4u : 8u);
    if (zone != 0) s.put8(w3, 1u);
}

// (begin, length, first chunk) of column c's value in the loaded record; the arrays stay in registers (c is uniform in
// map_format.hip and may differ from lane to lane in map_switch.hip: a chain of selects either way)
template <int NC>
__device__ __forceinline__ void pick_field(const RecordFields<NC>& f, int c, uint64_t* b, uint64_t* l, uint64_t* c0) {
    *b = 0, *l = 0, *c0 = 0;
#pragma unroll
    for (int k = 0; k < NC; k++)
        if (k == c) *b = f.b[k], *l = f.l[k], *c0 = f.c0[k];
}

// the span (begin in the column's bytes, length) a SPAN piece leaves of its column's value in row i: both passes compute it
template <int NC>
__device__ __forceinline__ void map_span_of(const ColsArg& cols, const ColIds& ids, const uint8_t* lits, const SpanOp* ops, const MapPiece& p,
                                            const RecordFields<NC>& f, uint64_t i, uint64_t* begin, uint64_t* len) {
    uint64_t b, l, c0, so, sn;
    if constexpr (NC > 0) pick_field(f, p.col, &b, &l, &c0);
    else value_span(cols.c[p.col], source_row(ids.ids[p.col], i), &b, &l);
    span_run(ops + p.off, (int)p.len, SpanValue{cols.c[p.col].data, b}, l, SpanLiterals{lits}, &so, &sn);
    *begin = b + so, *len = sn;
}

// bytes a COLUMN or SLICE piece adds to row i: from the value's span alone, no data read
template <int NC, int PK>
__device__ __forceinline__ uint64_t map_field_bytes(const ColsArg& cols, const ColIds& ids, const MapPiece& p, const RecordFields<NC>& f, uint64_t i) {
    uint64_t b, l, c0;
    if constexpr (NC > 0) pick_field(f, p.col, &b, &l, &c0);
    else value_span(cols.c[p.col], source_row(ids.ids[p.col], i), &b, &l);
    if (PK >= kPiecesSlice && p.kind == CPH_MAP_SLICE) {
        uint64_t so, sn;
        slice_span(l, p.from, p.to, &so, &sn);
        return sn;
    }
    return l;
}

// The length pass of one piece: the bytes piece p adds to output row i besides its literal (digit counts by compares, spans
// from offsets alone).  PK >= kPiecesFloat: *refused, preset to UINT64_MAX, takes the lowest row with a value the FLOAT64 or
// TIME formatter refuses.
// SP: the plan may hold SPAN pieces, whose length is the span their program leaves: the one piece whose length reads value bytes.
template <int NC, int PK, bool SP = false>
__device__ __forceinline__ uint64_t map_piece_bytes(const ColsArg& cols, const ColIds& ids, const MapPiece& p, const RecordFields<NC>& f, uint64_t i,
                                                    uint64_t* refused, const uint8_t* lits = nullptr, const SpanOp* ops = nullptr) {
    uint64_t bytes = 0;
    if (SP && p.kind == CPH_MAP_SPAN) {
        uint64_t b;
        map_span_of<NC>(cols, ids, lits, ops, p, f, i, &b, &bytes);
    } else if (p.kind == CPH_MAP_INT64) {
        bytes = int_chars(p.ints[i]);
    } else if (PK >= kPiecesShortest && p.kind == CPH_MAP_FLOAT64_SHORTEST) {   // no value is refused
        bytes = short_chars(short_split(p.floats[i]), p.col);
    } else if (PK >= kPiecesFloat && p.kind == CPH_MAP_FLOAT64) {
        const FixedParts r = fixed_split(p.floats[i], p.col);
        bytes = fixed_chars(r, p.col);
        if (r.kind == FIXED_RANGE) atomicMin(reinterpret_cast<unsigned long long*>(refused), (unsigned long long)i);
    } else if (PK >= kPiecesFloat && p.kind == CPH_MAP_TIME) {   // the length needs no look at the value; the refusal does
        bytes = rfc3339_chars(p.col);
        if (!rfc3339_in_range(p.ints[i], p.col)) atomicMin(reinterpret_cast<unsigned long long*>(refused), (unsigned long long)i);
    } else if (p.kind == CPH_MAP_COLUMN || (PK >= kPiecesSlice && p.kind == CPH_MAP_SLICE)) {
        bytes = map_field_bytes<NC, PK>(cols, ids, p, f, i);
    }
    return bytes;
}

// pieces [k0, k1) of `pieces` for output row i, in order, into the sink; literals lie in `lits` (k0 and k1 may differ from lane
// to lane)
template <int NC, int PK, bool SP = false, class Sink>
__device__ __forceinline__ void map_put_record(Sink& s, const ColsArg& cols, const ColIds& ids, const uint8_t* lits, const MapPiece* pieces,
                                               int k0, int k1, const RecordFields<NC>& f, uint64_t i, const SpanOp* ops = nullptr) {
    for (int k = k0; k < k1; k++) {
        const MapPiece& p = pieces[k];
        if (SP && p.kind == CPH_MAP_SPAN) {   // the span again, then a slice's copy
            const uint8_t* data = cols.c[p.col].data;
            uint64_t sb, sn;
            map_span_of<NC>(cols, ids, lits, ops, p, f, i, &sb, &sn);
            for (uint64_t q = 0; q < sn; q += 8) s.put8(load_value_chunk(data, sb, sn, (int)(q >> 3)), (uint32_t)(sn - q < 8 ? sn - q : 8));
        } else if (p.kind == CPH_MAP_LITERAL) {
            for (uint32_t q = 0; q < p.len; q += 8)
                s.put8(load_value_chunk(lits, p.off, p.len, (int)(q >> 3)), p.len - q < 8u ? p.len - q : 8u);
        } else if (p.kind == CPH_MAP_INT64) {
            put_int(s, p.ints[i]);
        } else if (PK >= kPiecesShortest && p.kind == CPH_MAP_FLOAT64_SHORTEST) {
            short_put(s, short_split(p.floats[i]), p.col);
        } else if (PK >= kPiecesFloat && p.kind == CPH_MAP_FLOAT64) {
            fixed_put(s, fixed_split(p.floats[i], p.col), p.col);
        } else if (PK >= kPiecesFloat && p.kind == CPH_MAP_TIME) {
            put_time(s, p.ints[i], p.col);
        } else if (PK >= kPiecesSlice && p.kind == CPH_MAP_SLICE) {   // the record's preloaded first chunk is the whole field's: a slice loads its own
            const uint8_t* data = cols.c[p.col].data;
            uint64_t b, l, c0, so, sn;
            if constexpr (NC > 0) pick_field(f, p.col, &b, &l, &c0);
            else value_span(cols.c[p.col], source_row(ids.ids[p.col], i), &b, &l);
            slice_span(l, p.from, p.to, &so, &sn);
            for (uint64_t q = 0; q < sn; q += 8) s.put8(load_value_chunk(data, b + so, sn, (int)(q >> 3)), (uint32_t)(sn - q < 8 ? sn - q : 8));
        } else {
            const uint8_t* data = cols.c[p.col].data;
            uint64_t b, l, c0;
            if constexpr (NC > 0) {
                pick_field(f, p.col, &b, &l, &c0);
            } else {
                value_span(cols.c[p.col], source_row(ids.ids[p.col], i), &b, &l);
                c0 = l ? load_value_chunk(data, b, l, 0) : 0;
            }
            for (uint64_t q = 0; q < l; q += 8) {
                const uint64_t chunk = q ? load_value_chunk(data, b, l, (int)(q >> 3)) : c0;
                s.put8(chunk, (uint32_t)(l - q < 8 ? l - q : 8));
            }
        }
    }
}

}  // namespace cph
