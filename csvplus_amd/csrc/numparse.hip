// numparse.hip — Row.ValueAsInt / Row.ValueAsFloat64 (csvplus.go:165-205) for a whole column: strings -> int64 / float64
// with Go's strconv semantics (and RFC 3339 timestamps -> Unix time, the third typed value), plus the error report the reference's callers act on (which row failed first, and how).
//
//   cph_col_to_number   one column read through an optional row selection -> values, one status byte per row, the
//                       number of errors, the first error row and its kind
//   convert_rows        the same for a caller inside the library (filter.hip: float compare terms)
//
//   k_num_parse    rows on lanes (row = tile + 64 k + lane, 8 rows per lane and tile, 4 in flight, the geometry of
//                  k_pred_eval): span -> the value's first 16 bytes with two branch-free loads -> the SWAR conversion of
//                  numparse_device.hpp.  Values and status bytes leave as coalesced stores.  A wave that saw an error
//                  adds its count and sends ONE 64-bit atomicMin (the report of num_report.hpp, tag = 0), so the first
//                  error row and its kind arrive together; a wave that deferred float rows adds their count.
//                  The time instantiation (CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO: RFC 3339 text -> t.Unix() / t.UnixNano(),
//                  timeparse_device.hpp) loads bytes 16..31 with two more unbranched loads per row, issued for the phase's rows
//                  together; it defers nothing.
//   The device decides every row's syntax and every value Clinger's exact cases cover.  The float rows it DEFERS (19+
//   significant digits, a mantissa >= 2^53, exponents outside the exact range) are rare:
//   k_num_collect  (only when there are any) gathers position, span and the first bytes of each deferred row into 128-byte
//                  slots; the host converts those with a correctly rounded routine and
//   k_num_patch    writes the values and status bytes back.
//   With cph_ctx_set_option "float_device" = 1 the float conversion runs the kParseFloatFull instantiation: behind Clinger's
//   cases it converts with Eisel-Lemire (floatparse_device.hpp, one out-of-line body) and defers only what that leaves
//   undecided, so collect / host / patch see a few rows per thousand truncated values instead of every 17-digit one.
#include <algorithm>
#include <cerrno>
#include <charconv>
#include <clocale>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include <locale.h>

#include "floatparse_device.hpp"
#include "num_report.hpp"
#include "numparse_device.hpp"
#include "timeparse_device.hpp"

namespace cph {

// the instantiations of k_num_parse; kParseFloatFull (cph_ctx_set_option "float_device" = 1) is kParseFloat with the
// Eisel-Lemire conversion behind Clinger's cases: it defers only what that cannot decide
constexpr int kParseInt = 0, kParseFloat = 1, kParseTime = 2, kParseFloatFull = 3;

// A valid value outside Clinger's exact cases, decided on the device where Eisel-Lemire can (floatparse_device.hpp).  One
// out-of-line body per kernel: k_num_parse unrolls 8 rows per lane, and the two call sites in parse_float64 would make
// sixteen copies of it.  +-Inf is a range error, as the host route reports it; underflow to +-0 or a subnormal is no error.
// Arguments and result travel in registers (no pointer: an address would need a stack).
struct FloatBeyondResult {
    uint64_t bits;   // 0 for a deferred row until it is patched
    uint32_t st;
};
__device__ __noinline__ FloatBeyondResult float_beyond_exact(uint64_t mant, int exp10, uint32_t trunc, uint32_t neg) {
    uint64_t bits = 0;
    if (!float_eisel_lemire(mant, (int32_t)exp10, trunc != 0u, &bits)) return {0ull, (uint32_t)kNumDeferred};
    return {bits | ((uint64_t)neg << 63), bits == kFloatInfBits ? (uint32_t)CPH_NUM_ERR_RANGE : (uint32_t)CPH_NUM_OK};
}
struct FloatBeyondDevice {
    __device__ __forceinline__ uint32_t operator()(uint64_t mant, int exp10, bool trunc, bool neg, double* out) const {
        const FloatBeyondResult r = float_beyond_exact(mant, exp10, trunc ? 1u : 0u, neg ? 1u : 0u);
        *out = __longlong_as_double((long long)r.bits);
        return r.st;
    }
};

constexpr int kNumRows  = 8;                          // rows per lane and tile
constexpr int kNumPhase = 4;                          // ... of which this many are in flight at once
constexpr int kNumTile  = kMatThreads * kNumRows;     // 2048 rows
constexpr int kNumWaveRows = kNumRows;                // 64-row groups per wave and tile
constexpr uint32_t kSlotBytes = 104;                  // value bytes a deferred row's slot holds

struct NumCounters {   // preset by the host in front of k_num_parse (ErrReport)
    ErrWord err;       // first
    unsigned long long ndeferred, collected;
};
struct NumSlot {       // one deferred row on its way to the host
    uint64_t pos, begin, len;
    uint8_t bytes[kSlotBytes];
};
static_assert(sizeof(NumSlot) == 128, "NumSlot is 128 bytes");
struct NumPatch {
    uint64_t pos, bits;
    uint32_t status, pad_;
};

// bytes 32.. of a value for parse_rfc3339 (and every chunk for the byte loop of a malformed value)
struct TimeChunks {
    const uint8_t* data;
    uint64_t begin, len;
    __device__ __forceinline__ uint64_t operator()(int j) const { return load_value_chunk(data, begin, len, j); }
};

// bytes 16..23 and 24..31 of a value, unbranched like the head (a chunk past the value's end reads the word at the value's
// own first byte and is not used)
__device__ __forceinline__ void load_tail16(const DevCol& col, uint64_t begin, uint64_t len, uint64_t* t0, uint64_t* t1) {
    const uint64_t p = (uint64_t)(uintptr_t)col.data;
    const uint8_t* base8 = (const uint8_t*)(uintptr_t)(p & ~7ull);
    const uint32_t delta = (uint32_t)(p & 7ull);
    const uint32_t l32 = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    *t0 = load_chunk_nobranch<uint64_t>(base8, delta, begin, l32, 2);
    *t1 = load_chunk_nobranch<uint64_t>(base8, delta, begin, l32, 3);
}

// KIND: kParseInt / kParseFloat / kParseFloatFull / kParseTime; nano (kParseTime alone): UnixNano instead of Unix
template <int KIND>
__global__ __launch_bounds__(kMatThreads) void k_num_parse(DevCol col, RowIds rid, uint64_t first_row, uint64_t n,
                                                          uint64_t* __restrict__ values, uint8_t* __restrict__ status, NumCounters* cnt,
                                                          uint32_t nano) {
    constexpr bool FLT = KIND == kParseFloat || KIND == kParseFloatFull;
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = (n + kNumTile - 1) / kNumTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kNumTile;
        WaveErr we;          // wave-uniform: the wave's errors in this tile
        uint32_t ndef = 0;   // wave-uniform
#pragma unroll
        for (int ph = 0; ph < kNumRows / kNumPhase; ph++) {
            uint64_t b[kNumPhase], l[kNumPhase], c0[kNumPhase], c1[kNumPhase];
            bool live[kNumPhase];
#pragma unroll
            for (int k = 0; k < kNumPhase; k++) {
                const uint64_t i = t0 + (uint64_t)((wave * kNumWaveRows + ph * kNumPhase + k) * 64 + lane);
                live[k] = i < n;   // rows past the end look at the last row; their result is dropped
                value_span(col, source_row(rid, first_row + (live[k] ? i : n - 1)), &b[k], &l[k]);
            }
#pragma unroll
            for (int k = 0; k < kNumPhase; k++) load_head16(col, b[k], l[k], &c0[k], &c1[k]);
            uint64_t c2[KIND == kParseTime ? kNumPhase : 1], c3[KIND == kParseTime ? kNumPhase : 1];   // bytes 16..31
            if constexpr (KIND == kParseTime) {
#pragma unroll
                for (int k = 0; k < kNumPhase; k++) load_tail16(col, b[k], l[k], &c2[k], &c3[k]);
            }
#pragma unroll
            for (int k = 0; k < kNumPhase; k++) {
                const uint64_t g0 = t0 + (uint64_t)((wave * kNumWaveRows + ph * kNumPhase + k) * 64);
                uint64_t bits;
                uint32_t st;
                if constexpr (KIND == kParseTime) {
                    int64_t v;
                    st = parse_rfc3339(l[k], c0[k], c1[k], c2[k], c3[k], TimeChunks{col.data, b[k], l[k]}, nano != 0, &v);
                    bits = (uint64_t)v;
                } else if constexpr (FLT) {
                    double v;
                    if constexpr (KIND == kParseFloatFull) st = parse_float64(col, b[k], l[k], c0[k], c1[k], &v, FloatBeyondDevice{});
                    else st = parse_float64(col, b[k], l[k], c0[k], c1[k], &v);
                    bits = (uint64_t)__double_as_longlong(v);
                } else {
                    int64_t v;
                    st = parse_int64(col, b[k], l[k], c0[k], c1[k], &v);
                    bits = (uint64_t)v;
                }
                if (live[k]) {
                    values[g0 + lane] = bits;
                    status[g0 + lane] = (uint8_t)st;
                }
                we.note_ballot(__ballot(live[k] && st != CPH_NUM_OK && st != kNumDeferred), g0, err_tag_kind(0u, st));
                if constexpr (FLT) ndef += (uint32_t)__popcll(__ballot(live[k] && st == kNumDeferred));
            }
        }
        we.flush(&cnt->err);
        if (lane == 0 && ndef) atomicAdd(&cnt->ndeferred, (unsigned long long)ndef);
    }
}

// slots[q] = row, span and first bytes of the q-th deferred row (in no particular order)
__global__ __launch_bounds__(kMatThreads) void k_num_collect(DevCol col, RowIds rid, uint64_t first_row, uint64_t n,
                                                            const uint8_t* __restrict__ status, NumCounters* cnt, NumSlot* __restrict__ slots,
                                                            uint64_t nslots) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        if (status[i] != kNumDeferred) continue;
        const uint64_t q = atomicAdd(&cnt->collected, 1ull);
        if (q >= nslots) continue;   // cannot happen: nslots is the count k_num_parse left
        uint64_t b, l;
        value_span(col, source_row(rid, first_row + i), &b, &l);
        NumSlot& s = slots[q];
        s.pos = i;
        s.begin = b;
        s.len = l;
        const uint64_t take = l < kSlotBytes ? l : kSlotBytes;
        for (uint64_t j = 0; 8 * j < take; j++) {
            const uint64_t chunk = load_value_chunk(col.data, b, l, (int)j);
            memcpy(s.bytes + 8 * j, &chunk, 8);   // kSlotBytes is a multiple of 8: a whole chunk always fits
        }
    }
}

__global__ __launch_bounds__(kMatThreads) void k_num_patch(const NumPatch* __restrict__ patch, uint64_t np, uint64_t* __restrict__ values,
                                                          uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x;
    if (i >= np) return;
    values[patch[i].pos] = patch[i].bits;
    status[patch[i].pos] = (uint8_t)patch[i].status;
}

namespace {


// One syntactically valid decimal value the device deferred: correctly rounded, locale independent.  A finite result
// is never an error (underflow to 0 or a denormal included, as in Go); +-HUGE_VAL is a range error with value +-Inf.
uint32_t host_parse_float(const char* s, size_t len, double* out) {
    bool neg = false;
    size_t i = 0;
    if (len && (s[0] == '+' || s[0] == '-')) {
        neg = s[0] == '-';
        i = 1;
    }
    double v = 0.0;
    bool done = false;
#if defined(__cpp_lib_to_chars) && __cpp_lib_to_chars >= 201611L
    {
        const std::from_chars_result r = std::from_chars(s + i, s + len, v, std::chars_format::general);
        done = r.ec == std::errc() && r.ptr == s + len;   // out of range: from_chars does not say which way
    }
#endif
    if (!done) {
        static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
        const std::string z(s + i, len - i);
        v = c_locale ? strtod_l(z.c_str(), nullptr, c_locale) : strtod(z.c_str(), nullptr);
    }
    if (neg) v = -v;
    *out = v;
    return std::isinf(v) ? CPH_NUM_ERR_RANGE : CPH_NUM_OK;
}

}  // namespace

Status convert_rows(cph_ctx* ctx, const DevCol& col, const RowIds& ids, uint64_t first_row, uint64_t n, int32_t kind, DevBuf* values,
                    DevBuf* status, NumColStats* st) {
    *st = NumColStats{};
    if (n == 0) return {};
    const bool flt = kind == CPH_NUM_FLOAT64;
    const bool tim = kind == CPH_NUM_TIME_UNIX || kind == CPH_NUM_TIME_UNIXNANO;
    CPH_TRY(values->alloc(&ctx->pool, (size_t)n * 8));
    CPH_TRY(status->alloc(&ctx->pool, (size_t)n));
    ErrReport<NumCounters> cnt;
    CPH_TRY(cnt.init(ctx));
    const uint64_t ntiles = (n + kNumTile - 1) / kNumTile;
    {
        // byte model: offsets (or nothing for a fixed width) + row ids + ~8 value bytes in, 9 bytes out per row
        const double in_row = (col.fixed_width ? (double)col.fixed_width : (double)(col.offset_bits / 8) + 8.0) + (ids.ptr ? (double)(ids.bits / 8) : 0.0);
        // (a timestamp: 20..35 value bytes, counted as 25)
        const double in_time = tim && !col.fixed_width ? 17.0 : 0.0;
        const bool full = flt && ctx->float_device;
        ProfScope ps(ctx, tim ? "k_num_parse_time" : full ? "k_num_parse_f64_full" : flt ? "k_num_parse_f64" : "k_num_parse_i64",
                     (in_row + in_time + 9.0) * (double)n);
        if (tim)
            hipLaunchKernelGGL(k_num_parse<kParseTime>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, col, ids, first_row, n,
                               values->as<uint64_t>(), status->as<uint8_t>(), cnt.counters(), kind == CPH_NUM_TIME_UNIXNANO ? 1u : 0u);
        else if (full)
            hipLaunchKernelGGL(k_num_parse<kParseFloatFull>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, col, ids, first_row, n,
                               values->as<uint64_t>(), status->as<uint8_t>(), cnt.counters(), 0u);
        else if (flt)
            hipLaunchKernelGGL(k_num_parse<kParseFloat>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, col, ids, first_row, n,
                               values->as<uint64_t>(), status->as<uint8_t>(), cnt.counters(), 0u);
        else
            hipLaunchKernelGGL(k_num_parse<kParseInt>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, col, ids, first_row, n,
                               values->as<uint64_t>(), status->as<uint8_t>(), cnt.counters(), 0u);
    }
    CPH_HIP_TRY(hipGetLastError());
    NumCounters got{};
    ErrFirst e;
    CPH_TRY(cnt.read(ctx, &e, &got));   // the call's host wait
    st->nerrors = e.nerrors;
    st->first_error = e.row;
    st->first_kind = e.kind;
    st->host_rows = got.ndeferred;
    if (!got.ndeferred) return {};

    // the deferred rows: their bytes come back, the host converts them, the results are patched in
    const uint64_t nd = got.ndeferred;
    DevBuf slots;
    CPH_TRY(slots.alloc(&ctx->pool, (size_t)nd * sizeof(NumSlot)));
    hipLaunchKernelGGL(k_num_collect, dim3(grid_rows(n)), dim3(kMatThreads), 0, ctx->stream, col, ids, first_row, n, status->as<uint8_t>(),
                       cnt.counters(), slots.as<NumSlot>(), nd);
    CPH_HIP_TRY(hipGetLastError());
    std::vector<NumSlot> hs((size_t)nd);
    CPH_HIP_TRY(hipMemcpyAsync(hs.data(), slots.get(), (size_t)nd * sizeof(NumSlot), hipMemcpyDeviceToHost, ctx->stream));
    CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<NumPatch> hp((size_t)nd);
    std::string longv;
    for (uint64_t q = 0; q < nd; q++) {
        const NumSlot& s = hs[(size_t)q];
        const char* bytes = reinterpret_cast<const char*>(s.bytes);
        if (s.len > kSlotBytes) {   // a value longer than a slot: straight from the column
            longv.resize((size_t)s.len);
            CPH_HIP_TRY(hipMemcpyAsync(&longv[0], col.data + s.begin, (size_t)s.len, hipMemcpyDeviceToHost, ctx->stream));
            CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
            bytes = longv.data();
        }
        double v = 0.0;
        const uint32_t k = host_parse_float(bytes, (size_t)s.len, &v);
        NumPatch& p = hp[(size_t)q];
        p.pos = s.pos;
        memcpy(&p.bits, &v, 8);
        p.status = k;
        p.pad_ = 0;
        if (k != CPH_NUM_OK) {
            st->nerrors++;
            if (s.pos < st->first_error) {
                st->first_error = s.pos;
                st->first_kind = (int32_t)k;
            }
        }
    }
    DevBuf patch;
    CPH_TRY(patch.alloc(&ctx->pool, (size_t)nd * sizeof(NumPatch)));
    CPH_HIP_TRY(hipMemcpyAsync(patch.get(), hp.data(), (size_t)nd * sizeof(NumPatch), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_num_patch, dim3((unsigned)((nd + kMatThreads - 1) / kMatThreads)), dim3(kMatThreads), 0, ctx->stream,
                       patch.as<NumPatch>(), nd, values->as<uint64_t>(), status->as<uint8_t>());
    CPH_HIP_TRY(hipGetLastError());
    CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));   // hp and the patch block stay alive until the kernel has read them
    return {};
}

}  // namespace cph

using namespace cph;

extern "C" {

CPH_API int32_t cph_col_to_number(cph_ctx* ctx, const cph_strcol* col, const cph_rowsel* sel, uint64_t nrows, int32_t kind,
                                  int32_t out_mem, cph_numcol** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!col) return fail_with(ctx, {CPH_ERR_INVALID, "cph_col_to_number: col must not be NULL"});
    if (kind != CPH_NUM_INT64 && kind != CPH_NUM_FLOAT64 && kind != CPH_NUM_TIME_UNIX && kind != CPH_NUM_TIME_UNIXNANO)
        return fail_with(ctx, {CPH_ERR_INVALID, "cph_col_to_number: kind must be CPH_NUM_INT64, CPH_NUM_FLOAT64, CPH_NUM_TIME_UNIX or CPH_NUM_TIME_UNIXNANO"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    {
        Status s = check_row_sources(col, sel, 1, 0, nrows, true);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_numcol_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.nrows = nrows;
    r->pub.kind = kind;
    r->pub.mem = out_mem;
    r->pub.first_error_row = UINT64_MAX;
    auto run = [&]() -> Status {
        if (nrows == 0) return {};
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, col, sel, nullptr, 1, 0, nrows, &staged, &arg, &ids));
        NumColStats st;
        CPH_TRY(convert_rows(ctx, arg.c[0], ids.ids[0], 0, nrows, kind, &r->d_values, &r->d_status, &st));
        r->pub.nerrors = st.nerrors;
        r->pub.first_error_row = st.first_error;
        r->pub.first_error_kind = st.first_kind;
        r->pub.host_rows = st.host_rows;
        const ResultPart parts[2] = {{&r->d_values, (size_t)nrows * 8, &r->pub.values}, {&r->d_status, (size_t)nrows, &r->pub.status}};
        return deliver(ctx, &r->own, parts, 2, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API void cph_numcol_release(cph_numcol* pub) { release_result<cph_numcol_impl>(pub); }

}  // extern "C"
