// num_report.hpp — "which value was bad first, and how many were?": the error report of the typed-value passes (k_num_parse,
// k_expr_eval, k_order_key_num, k_jt_errors, k_resolve_tile).  A bad value is data, not a failure: a pass counts them and keeps the
// lowest (row, tag, kind) with ONE 64-bit atomicMin per wave; the host reads both words in the call's single wait and unpacks them
// with the functions the kernels packed them with.
//
//   ErrWord            the device accumulator: nerrors, and first = err_pack(row, tag, kind) of the lowest one (~0: none)
//   err_pack / err_*   row << 16 | tag << 8 | kind: words compare by row, then tag, then kind.  tag = what a pass tells apart inside a
//                      row (the op of an expression, the key of an OrderBy, the spec of Totals over a Join; 0 elsewhere), kind = the
//                      status byte (CPH_NUM_*)
//   WaveErr            the tally a kernel keeps in registers, fed by ballots (rows on lanes, wave-uniform) or lane by lane
//   ErrReport          host: the accumulator's block — preset on the stream, read in one wait
//
// The first part is plain C++: hipcc compiles it for both sides, g++ for the host (tests/cpp/test_num_report.cpp).
#pragma once

#include <stdint.h>

#include "../../include/csvplus_hip.h"

#if defined(__HIPCC__)
#include "cph_internal.hpp"
#define CPH_ERR_HD __host__ __device__ inline
#else
#define CPH_ERR_HD inline
#endif

namespace cph {

struct ErrWord {
    unsigned long long nerrors, first;   // first == kErrNone: no error
};
constexpr unsigned long long kErrNone = ~0ull;

// 48 bits of row: more rows than the device's memory holds status bytes for (2^48 of them are 256 TiB), and no pass admits more.
// kErrNone is the word of row 2^48 - 1, tag 255, kind 255: above every word a pass can produce.
constexpr int kErrTagShift = 8, kErrRowShift = 16;
static_assert(CPH_EXPR_MAX_OPS <= 256 && CPH_ORDER_MAX_KEYS <= 256 && CPH_AGG_MAX_SPECS <= 256, "a tag is 8 bits");

CPH_ERR_HD uint32_t err_tag_kind(uint32_t tag, uint32_t kind) { return (tag << kErrTagShift) | kind; }   // tag, kind < 256
CPH_ERR_HD unsigned long long err_pack(uint64_t row, uint32_t tag, uint32_t kind) {
    return ((unsigned long long)row << kErrRowShift) | (unsigned long long)err_tag_kind(tag, kind);
}
CPH_ERR_HD uint64_t err_row(unsigned long long w) { return (uint64_t)(w >> kErrRowShift); }
CPH_ERR_HD uint32_t err_tag(unsigned long long w) { return (uint32_t)(w >> kErrTagShift) & 0xFFu; }
CPH_ERR_HD uint32_t err_kind(unsigned long long w) { return (uint32_t)w & 0xFFu; }

// an ErrWord as the host hands it on
struct ErrFirst {
    uint64_t nerrors = 0, row = UINT64_MAX;
    int32_t tag = 0, kind = 0;
};
inline ErrFirst err_unpack(const ErrWord& w) {
    ErrFirst f;
    f.nerrors = w.nerrors;
    if (w.nerrors) f.row = err_row(w.first), f.tag = (int32_t)err_tag(w.first), f.kind = (int32_t)err_kind(w.first);
    return f;
}

#if defined(__HIPCC__)

// One wave's tally across a tile or a grid-stride loop.  Ballot form: first and nerr are wave-uniform from the start.  Lane form:
// they are the lane's own until reduce().  flush() is the wave's one pair of atomics.
struct WaveErr {
    unsigned long long first = kErrNone;
    uint32_t nerr = 0;
    // 64 rows on the lanes, lane 0 holding row0; bad = the ballot of the lanes whose row failed, tag_kind = the lane's err_tag_kind
    __device__ __forceinline__ void note_ballot(uint64_t bad, uint64_t row0, uint32_t tag_kind) {
        if (bad) {   // uniform
            const int fl = __builtin_ctzll(bad);
            const unsigned long long key = ((unsigned long long)(row0 + (uint64_t)fl) << kErrRowShift) | (unsigned long long)__shfl(tag_kind, fl, kWave);
            if (key < first) first = key;
            nerr += (uint32_t)__popcll(bad);
        }
    }
    __device__ __forceinline__ void note_lane(uint64_t row, uint32_t tag, uint32_t kind) {
        nerr++;
        const unsigned long long e = err_pack(row, tag, kind);
        first = e < first ? e : first;
    }
    __device__ __forceinline__ void reduce() {   // every lane of the wave
        nerr = wave_sum(nerr);
        first = wave_min(first);
    }
    __device__ __forceinline__ void flush(ErrWord* e) const {
        if (lane_id() == 0 && nerr) {
            atomicAdd(&e->nerrors, (unsigned long long)nerr);
            atomicMin(&e->first, first);
        }
    }
};

// The accumulator on the host.  C = ErrWord, or a pass's counters struct whose FIRST MEMBER is its ErrWord: one block, one preset,
// one read.
template <class C = ErrWord>
struct ErrReport {
    static_assert(sizeof(C) >= sizeof(ErrWord) && alignof(C) >= alignof(ErrWord), "the ErrWord comes first");
    DevBuf buf;
    C* counters() const { return buf.as<C>(); }
    ErrWord* word() const { return buf.as<ErrWord>(); }
    Status init(cph_ctx* ctx) {   // zeroes, no error yet; on the stream
        C zero{};
        const ErrWord none{0ull, kErrNone};
        memcpy(&zero, &none, sizeof none);
        return upload_block(ctx, zero, &buf);
    }
    Status read(cph_ctx* ctx, ErrFirst* f, C* all = nullptr) const {   // a host wait
        C got{};
        CPH_TRY(read_device_value(ctx, counters(), &got));
        ErrWord w;
        memcpy(&w, &got, sizeof w);
        *f = err_unpack(w);
        if (all) *all = got;
        return {};
    }
};

#endif   // __HIPCC__

}  // namespace cph
