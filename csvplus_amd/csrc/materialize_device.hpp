// materialize_device.hpp — the device pieces the writers share (materialize.hip: gather and ToCsv; json_write.hip: ToJSON;
// filter.hip: Filter; map_format.hip and map_switch.hip: Map): the row-id lookup, the byte sinks, the LDS stage, the record loader, the column-count dispatch and the
// length scan.  Their host side is shared too and lives in cph_internal.hpp / capi.hip: RowIds / ColIds, check_row_sources and
// stage_row_sources (columns + row ids onto the device), deliver / finish_call / release_result (the result handed out).
#pragma once

#include "lds_stage.hpp"

namespace cph {

constexpr int kMatThreads = 256;
constexpr int kMatStage   = 16 * 1024;   // LDS bytes for one tile's output (small: more workgroups per CU hide the barriers)

__device__ __forceinline__ uint64_t source_row(const RowIds& ids, uint64_t i) {
    if (!ids.ptr) return i;
    return (ids.bits == 32 ? (uint64_t) reinterpret_cast<const uint32_t*>(ids.ptr)[i]
                           : reinterpret_cast<const uint64_t*>(ids.ptr)[i]) - ids.base;
}

// ---- byte sinks -------------------------------------------------------------------------------------
struct LdsSink {
    CPH_LDS uint8_t* p;
    __device__ __forceinline__ void put(uint8_t b) { *p++ = b; }
};
struct GlobalSink {
    uint8_t* p;
    __device__ __forceinline__ void put(uint8_t b) { *p++ = b; }
    __device__ __forceinline__ void put8(uint64_t chunk, uint32_t n) {
        for (uint32_t j = 0; j < n; j++) put((uint8_t)(chunk >> (8u * j)));
    }
};

// (round 6) A tile's bytes assembled WORD-wise: a thread appends its record's bytes to a 64-bit accumulator and ORs whole 32-bit
// words into the (zeroed) LDS stage — atomically, because the first and last word of a record are shared with its neighbours.
// Byte puts (extract, ds_write_b8 per byte) were ~10 instructions per output byte and what k_csv_copy spent its 3 ms on; this
// is ~2.5 per byte for unquoted values (8 at a time).
struct WordSink {
    uint32_t* words;   // the stage as 32-bit words (a plain pointer into the dynamic LDS block: atomicOr -> ds_or_b32)
    uint32_t w;        // next word
    uint32_t fill;     // bytes pending in acc (< 4)
    uint64_t acc;
    __device__ __forceinline__ WordSink(uint32_t* stage_words, uint32_t byte_pos) : words(stage_words), w(byte_pos >> 2), fill(byte_pos & 3u), acc(0) {}
    // the low n (1..4) bytes of v; the bytes above them must be zero
    __device__ __forceinline__ void put4(uint32_t v, uint32_t n) {
        acc |= (uint64_t)v << (8u * fill);
        fill += n;
        if (fill >= 4u) {
            atomicOr(&words[w], (uint32_t)acc);
            w++;
            acc >>= 32;
            fill -= 4u;
        }
    }
    __device__ __forceinline__ void put(uint8_t b) { put4(b, 1u); }
    // the low n (1..8) bytes of chunk (whatever lies above them)
    __device__ __forceinline__ void put8(uint64_t chunk, uint32_t n) {
        const uint32_t nlo = n < 4u ? n : 4u, nhi = n - nlo;
        const uint32_t lo = (uint32_t)chunk, hi = (uint32_t)(chunk >> 32);
        put4(nlo < 4u ? lo & ((1u << (8u * nlo)) - 1u) : lo, nlo);
        if (nhi) put4(nhi < 4u ? hi & ((1u << (8u * nhi)) - 1u) : hi, nhi);
    }
    __device__ __forceinline__ void finish() {
        if (fill) atomicOr(&words[w], (uint32_t)acc);
    }
};
__device__ __forceinline__ void copy_value_words(WordSink& out, const DevCol& col, uint64_t begin, uint64_t len) {
    for (uint64_t q = 0; q < len; q += 8) {
        const uint64_t chunk = load_value_chunk(col.data, begin, len, (int)(q >> 3));
        out.put8(chunk, (uint32_t)(len - q < 8 ? len - q : 8));
    }
}
// zero the first `bytes` (+ slack for the phase shift and the last word) of the stage; the caller synchronises
__device__ __forceinline__ void stage_clear(CPH_LDS uint8_t* stage, uint64_t bytes) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 z = {0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < (uint32_t)((bytes + 47) >> 4); i += blockDim.x) ((CPH_LDS u32x4*)stage)[i] = z;
}

template <class Sink>
__device__ __forceinline__ void copy_value(Sink& out, const DevCol& col, uint64_t begin, uint64_t len) {
    uint64_t chunk = 0;
    for (uint64_t q = 0; q < len; q++) {
        if ((q & 7) == 0) chunk = load_value_chunk(col.data, begin, len, (int)(q >> 3));
        out.put((uint8_t)(chunk >> (8 * (q & 7))));
    }
}

// 0x80 in every byte of w that equals the byte replicated in pat
__device__ __forceinline__ uint64_t eq_mask8(uint64_t w, uint64_t pat) {
    const uint64_t x = w ^ pat, k = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & k) + k) | x | k);
}

// One record's fields: row ids, then offsets, then the first chunk of every value — three rounds of independent
// loads instead of a dependent chain per column.  NC > 0: compile-time column count (arrays stay in registers);
// NC == 0: any count up to kMaxKeyCols, one column at a time.
// The first 8 bytes of a value with ONE unconditional load (device_utils.hpp: load_chunk_nobranch): the loads of a
// record's columns overlap instead of each waiting behind the branch of the one before.
__device__ __forceinline__ uint64_t first_chunk_nobranch(const DevCol& col, uint64_t begin, uint64_t len) {
    const uint64_t p = (uint64_t)(uintptr_t)col.data;
    const uint32_t l32 = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    const uint64_t v = load_chunk_nobranch<uint64_t>((const uint8_t*)(uintptr_t)(p & ~7ull), (uint32_t)(p & 7ull), begin, l32, 0);
    return l32 ? v : 0;
}

template <int NC>
struct RecordFields {
    uint64_t b[NC ? NC : 1], l[NC ? NC : 1], c0[NC ? NC : 1];
    // data_mask bit c: the bytes of column c are needed (a RAW column's length pass needs only its offsets)
    __device__ __forceinline__ void load(const ColsArg& cols, const ColIds& ids, uint64_t i, uint32_t data_mask) {
        uint64_t row[NC ? NC : 1];
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = source_row(ids.ids[c], i);
#pragma unroll
        for (int c = 0; c < NC; c++) value_span(cols.c[c], row[c], &b[c], &l[c]);
#pragma unroll
        for (int c = 0; c < NC; c++)
            c0[c] = ((data_mask >> c) & 1u) ? first_chunk_nobranch(cols.c[c], b[c], l[c]) : 0;   // data_mask is uniform
    }
};

// launches kernel<NC> for ncols in 1..8, the generic kernel<0> above that
#define CPH_CSV_DISPATCH(KERNEL, NCOLS, GRID, SMEM, STREAM, ...)                                                     \
    switch (NCOLS) {                                                                                                 \
        case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 5: hipLaunchKernelGGL(KERNEL<5>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 6: hipLaunchKernelGGL(KERNEL<6>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 7: hipLaunchKernelGGL(KERNEL<7>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        case 8: hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;            \
        default: hipLaunchKernelGGL(KERNEL<0>, GRID, dim3(kMatThreads), SMEM, STREAM, __VA_ARGS__); break;           \
    }

static unsigned grid_rows(uint64_t n) {
    uint64_t b = (n + kMatThreads - 1) / kMatThreads;
    if (b > 4096) b = 4096;
    return (unsigned)(b ? b : 1);
}

// lens[n] -> offs[n+1] in place (offs[n] = total), total also read back
static Status scan_lengths(cph_ctx* ctx, uint64_t* lens, uint64_t n, uint64_t* total) {
    CPH_TRY(exclusive_scan_u64(ctx, lens, n, lens + n));
    return read_device_value(ctx, lens + n, total);
}

}  // namespace cph

// the library-owned string column behind cph_colbuf (cph_colbuf_release frees whichever call made it: the gather, Map)
struct cph_colbuf_impl {
    cph_colbuf pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_data, d_offs;
};

// the library-owned byte buffer behind cph_bytes (cph_bytes_release frees whichever writer made it)
struct cph_bytes_impl {
    cph_bytes pub;    // first
    cph::ResultOwner own;
    cph::DevBuf d_data;
};
