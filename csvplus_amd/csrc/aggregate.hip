// aggregate.hip — Totals: Count and Sum / Min / Max per KEY of an index (cph_index_aggregate), the reduction the reference's
// TestSimpleTotals (csvplus_test.go:516-571) accumulates in a Go closure.  The index already holds the rows grouped (equal keys
// are adjacent in the sorted codes, input order inside a run), so the reduction is segmented, not hashed:
//
//   k_agg_heads    one pass over the sorted codes, kResRows CONSECUTIVE rows per lane (equal_flags, runs_device.hpp): the bitmap
//                  of RUN STARTS (a run of one row is a group here) and the starts per tile, in the layout of tile_bitmap.hpp.
//   exclusive scan of the tile counts (TileBitmap::scan): offs[tile] = groups in front of the tile, offs[ntiles] = ngroups.
//   k_agg_emit     the rank walker of tile_bitmap.hpp: first_position[rank], first_row[rank] = perm[position].
//   k_agg_counts   count[g] = first_position[g + 1] - first_position[g] (n for the last group): no reduction needed.
//   per spec:
//   convert_rows   (col specs, numparse.hip) the column read through perm: values in SORTED order, read coalesced below.
//   k_agg_reduce   reads the bitmap, not the codes again; 8 values per lane (16-byte loads; `numbers` specs are gathered through
//                  perm here); a segmented scan: serial in the lane, 64-lane shuffles, LDS across the 4 waves.  A run that
//                  starts AND is followed by another start inside the tile is written to its group slot; the tile leaves one
//                  head partial (its rows in front of its first start) and one tail partial (its last run, or all its rows).
//   k_agg_carry    one wave per tile that has a start: the tile's LAST run = its tail partial, then the tail partials of the
//                  tiles without a start behind it, then the head partial of the next tile with one — folded in ascending
//                  tile order, 64 tiles per step (a run may span every tile).
// Run starts and group slots are computed once and shared by all specs.  Nothing here is atomic and nothing depends on
// scheduling: the association order of a float sum is a function of the positions alone, so the sums are bit-reproducible.
#include <algorithm>
#include <cstring>
#include <new>

#include "runs_device.hpp"

namespace cph {

// The aggregates over the 8-byte patterns of int64 / double.  Every one has a true identity, so the scan needs no "empty" state.
template <int OP, bool FLT>
__host__ __device__ constexpr uint64_t agg_identity() {
    if constexpr (OP == CPH_AGG_SUM) return FLT ? 0x8000000000000000ull : 0ull;   // -0.0 + x == x for every x, +0 included
    else if constexpr (OP == CPH_AGG_MIN) return FLT ? 0x7FF0000000000000ull : 0x7FFFFFFFFFFFFFFFull;
    else return FLT ? 0xFFF0000000000000ull : 0x8000000000000000ull;
}
template <int OP, bool FLT>
__device__ __forceinline__ uint64_t agg_join(uint64_t a, uint64_t b) {
    if constexpr (!FLT) {
        if constexpr (OP == CPH_AGG_SUM) return a + b;   // wraps
        else if constexpr (OP == CPH_AGG_MIN) return (int64_t)a < (int64_t)b ? a : b;
        else return (int64_t)a > (int64_t)b ? a : b;
    } else {
        const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
        if constexpr (OP == CPH_AGG_SUM) {
            return (uint64_t)__double_as_longlong(x + y);
        } else {
            if (x != x || y != y) return 0x7FF8000000000001ull;                       // the bits of Go's math.NaN()
            if (x == 0.0 && y == 0.0) return OP == CPH_AGG_MIN ? (a | b) : (a & b);   // Min(-0, +0) = -0, Max(-0, +0) = +0
            if constexpr (OP == CPH_AGG_MIN) return x < y ? a : b;
            else return x > y ? a : b;
        }
    }
}

// one element of the segmented scan: the aggregate since the last run start at or before this point, and whether there was one
struct AggSeg {
    uint64_t v;
    uint32_t start;
};
template <int OP, bool FLT>
__device__ __forceinline__ AggSeg agg_seg_join(const AggSeg left, const AggSeg right) {
    AggSeg r;
    r.v = right.start ? right.v : agg_join<OP, FLT>(left.v, right.v);
    r.start = left.start | right.start;
    return r;
}

// bit = a run starts at that sorted position (tile_bitmap.hpp).  n >= 1.
template <bool KEY32>
__global__ __launch_bounds__(kMatThreads) void k_agg_heads(const void* __restrict__ codes, uint64_t n, int nwords, uint64_t* __restrict__ bitmap,
                                                          uint32_t* __restrict__ counts) {
    __shared__ uint64_t s_word[kResWords];
    uint8_t* s_byte = reinterpret_cast<uint8_t*>(s_word);   // kResRows == 8: one byte per lane
    const uint64_t ntiles = tile_count(n);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kResTile;
        const uint64_t tend = t0 + kResTile < n ? t0 + kResTile : n;
        const uint64_t base = t0 + (uint64_t)threadIdx.x * kResRows;
        const uint32_t e = base < n ? equal_flags<KEY32>(codes, n, nwords, base) : 0u;
        s_byte[threadIdx.x] = (uint8_t)(tile_live_rows(base, tend) & ~e);
        tile_store_words(s_word, tile, bitmap, counts);
    }
}

// offs[tile] = run starts in front of the tile; first_position[rank] = the start's sorted position, first_row[rank] = its table row
__global__ __launch_bounds__(kMatThreads) void k_agg_emit(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ perm, uint64_t ntiles, uint64_t* __restrict__ first_position,
                                                         uint32_t* __restrict__ first_row) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t o0 = offs[tile], o1 = offs[tile + 1];
        if (o0 == o1) continue;   // uniform
        tile_for_each_set(bitmap, tile, o0, [&](uint64_t rank, int r) {
            const uint64_t pos = tile * kResTile + (uint64_t)r;
            first_position[rank] = pos;
            first_row[rank] = perm[pos];
        });
    }
}

// count[g] = the distance to the next run start
__global__ __launch_bounds__(kMatThreads) void k_agg_counts(const uint64_t* __restrict__ first_position, uint64_t ngroups, uint64_t n,
                                                           uint64_t* __restrict__ count) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t g = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; g < ngroups; g += stride)
        count[g] = (g + 1 < ngroups ? first_position[g + 1] : n) - first_position[g];
}

// src: GATHER ? one 8-byte value per TABLE row (read through perm) : one per SORTED position.  out[g] for every run that starts
// in the tile and is followed by another start in it; head[tile] = the aggregate of the rows in front of the tile's first start
// (the identity when its first row is one; unwritten and unused when the tile has no start); tail[tile] = the aggregate of the
// tile's last run over this tile's rows (all its rows when it has no start).
template <int OP, bool FLT, bool GATHER>
__global__ __launch_bounds__(kMatThreads) void k_agg_reduce(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs,
                                                           const uint64_t* __restrict__ src, const uint32_t* __restrict__ perm, uint64_t n,
                                                           uint64_t* __restrict__ out, uint64_t* __restrict__ head, uint64_t* __restrict__ tail) {
    __shared__ uint64_t s_word[kResWords];
    __shared__ uint32_t s_pre[kResWords];
    __shared__ uint64_t s_wave_v[kResWaves];
    __shared__ uint32_t s_wave_start[kResWaves];
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = tile_count(n);
    constexpr uint64_t ident = agg_identity<OP, FLT>();
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kResTile;
        const uint64_t tend = t0 + kResTile < n ? t0 + kResTile : n;   // one past the tile's last row
        tile_load_words(bitmap, tile, s_word, s_pre);
        const uint32_t r0 = threadIdx.x * kResRows;   // the lane's first row inside the tile
        const uint64_t base = t0 + r0;
        uint32_t starts, before;                      // the lane's run starts, and the tile's in front of the lane
        tile_lane_bits(s_word, s_pre, r0, &starts, &before);
        const uint32_t rn = r0 + kResRows;
        const uint32_t next_start = rn < (uint32_t)kResTile ? (uint32_t)(s_word[rn >> 6] >> (rn & 63u)) & 1u : 0u;
        const uint32_t live = tile_live_rows(base, tend);

        uint64_t v[kResRows];
        if (live == (1u << kResRows) - 1) {   // 16-byte streams: 4 loads of values, or 2 of perm
            if constexpr (GATHER) {
                const uint4* p = reinterpret_cast<const uint4*>(perm + base);
                const uint4 a = p[0], b = p[1];
                v[0] = src[a.x]; v[1] = src[a.y]; v[2] = src[a.z]; v[3] = src[a.w];
                v[4] = src[b.x]; v[5] = src[b.y]; v[6] = src[b.z]; v[7] = src[b.w];
            } else {
                const ulonglong2* p = reinterpret_cast<const ulonglong2*>(src + base);
#pragma unroll
                for (int k = 0; k < kResRows / 2; k++) {
                    const ulonglong2 a = p[k];
                    v[2 * k] = a.x;
                    v[2 * k + 1] = a.y;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kResRows; k++) {
                v[k] = ident;
                if ((live >> k) & 1u) {
                    const uint64_t pos = base + (uint64_t)k;
                    v[k] = GATHER ? src[perm[pos]] : src[pos];
                }
            }
        }
        // the lane's own rows: loc[k] = the aggregate since the last run start inside the lane (or since its first row)
        uint64_t loc[kResRows];
        uint64_t cur = ident;
        uint32_t started = 0;   // bit k: a run starts at one of the lane's rows 0..k
#pragma unroll
        for (int k = 0; k < kResRows; k++) {
            const bool st = (starts >> k) & 1u;
            cur = st ? v[k] : agg_join<OP, FLT>(cur, v[k]);
            if (st) started |= 1u << k;
            if (k > 0) started |= ((started >> (k - 1)) & 1u) << k;
            loc[k] = cur;
        }
        // across the lanes of the wave, then across the waves: incl = everything up to and including this lane
        AggSeg incl{cur, started >> (kResRows - 1)};
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            AggSeg up;
            up.v = __shfl_up(incl.v, d, kWave);
            up.start = __shfl_up(incl.start, d, kWave);
            if (lane >= d) incl = agg_seg_join<OP, FLT>(up, incl);
        }
        if (lane == kWave - 1) {
            s_wave_v[wave] = incl.v;
            s_wave_start[wave] = incl.start;
        }
        AggSeg excl;
        excl.v = __shfl_up(incl.v, 1, kWave);
        excl.start = __shfl_up(incl.start, 1, kWave);
        if (lane == 0) excl = AggSeg{ident, 0u};
        __syncthreads();
        AggSeg front{ident, 0u};   // the waves in front of this one
        for (int w = 0; w < wave; w++) front = agg_seg_join<OP, FLT>(front, AggSeg{s_wave_v[w], s_wave_start[w]});
        excl = agg_seg_join<OP, FLT>(front, excl);
        const uint64_t o0 = offs[tile];
#pragma unroll
        for (int k = 0; k < kResRows; k++) {
            if (!((live >> k) & 1u)) continue;
            const bool ends = k + 1 < kResRows ? (starts >> (k + 1)) & 1u : next_start != 0u;   // the next row of the tile starts a run
            const bool is_last = base + (uint64_t)k + 1 == tend;
            if (!ends && !is_last) continue;
            const bool own = (started >> k) & 1u;   // the row's run started inside this lane
            const uint64_t val = own ? loc[k] : agg_join<OP, FLT>(excl.v, loc[k]);
            const uint32_t nstarts = before + (uint32_t)__popc(starts & ((2u << k) - 1u));   // starts of the tile at or in front of the row
            if (ends) {
                if (nstarts) out[o0 + nstarts - 1] = val;   // o0 + nstarts - 1 < offs[tile + 1] <= ngroups
                else head[tile] = val;
            }
            if (is_last) tail[tile] = val;
        }
        if (threadIdx.x == 0 && (starts & 1u)) head[tile] = ident;
        __syncthreads();
    }
}

// One wave per tile that has a run start: the tile's last run, folded forward over the tiles it spans.
template <int OP, bool FLT>
__global__ __launch_bounds__(kMatThreads) void k_agg_carry(const uint32_t* __restrict__ offs, const uint64_t* __restrict__ head,
                                                          const uint64_t* __restrict__ tail, uint64_t ntiles, uint64_t* __restrict__ out) {
    const int lane = lane_id();
    constexpr uint64_t ident = agg_identity<OP, FLT>();
    const uint64_t nwaves = (uint64_t)gridDim.x * kResWaves;
    for (uint64_t t = (uint64_t)blockIdx.x * kResWaves + (uint64_t)wave_id(); t < ntiles; t += nwaves) {
        const uint32_t o1 = offs[t + 1];
        if (o1 == offs[t]) continue;   // uniform: no start, some tile in front owns the run
        uint64_t acc = tail[t];
        for (uint64_t j = t + 1; j < ntiles; j += kWave) {   // tiles j .. j+63 on the lanes
            const uint64_t u = j + (uint64_t)lane;
            const bool valid = u < ntiles;
            const bool has = valid && offs[u + 1] != offs[u];
            const uint64_t stop = __ballot(!valid || has);   // the first tile with a start closes the run; so does the end of the index
            const int first = stop ? __builtin_ctzll(stop) : kWave;
            uint64_t x = ident;
            if (valid && lane < first) x = tail[u];                // a tile without a start: all its rows
            else if (has && lane == first) x = head[u];            // the rows in front of that tile's first start
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {   // lane 0 ends with x0 . x1 . ... . x63, operands in ascending tile order
                const uint64_t o = __shfl_down(x, d, kWave);
                if (lane + d < kWave) x = agg_join<OP, FLT>(x, o);
            }
            acc = agg_join<OP, FLT>(acc, __shfl(x, 0, kWave));
            if (stop) break;
        }
        if (lane == 0) out[o1 - 1] = acc;
    }
}

}  // namespace cph

using namespace cph;

// the library-owned result behind cph_aggregated
struct cph_aggregated_impl {
    cph_aggregated pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_pos, d_row, d_cnt, d_val[CPH_AGG_MAX_SPECS];
};

namespace cph {

void agg_launch_heads(cph_ctx* ctx, const void* codes, bool key32, int nwords, uint64_t n, double code_bytes, uint64_t* bitmap, uint32_t* counts) {
    const uint64_t ntiles = tile_count(n);
    ProfScope ps(ctx, "k_agg_heads", (double)n * (code_bytes + 1.0 / 8.0) + 4.0 * (double)ntiles);
    if (key32)
        hipLaunchKernelGGL(k_agg_heads<true>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, codes, n, nwords, bitmap, counts);
    else
        hipLaunchKernelGGL(k_agg_heads<false>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, codes, n, nwords, bitmap, counts);
}

void agg_launch_emit(cph_ctx* ctx, const uint64_t* bitmap, const uint32_t* offs, const uint32_t* perm, uint64_t n, uint64_t ngroups,
                     uint64_t* first_position, uint32_t* first_row) {
    const uint64_t ntiles = tile_count(n);
    ProfScope ps(ctx, "k_agg_emit", (double)n / 8.0 + 4.0 * (double)ntiles + 16.0 * (double)ngroups);
    hipLaunchKernelGGL(k_agg_emit, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, bitmap, offs, perm, ntiles, first_position, first_row);
}

namespace {

template <int OP, bool FLT>
void launch_reduce(cph_ctx* ctx, bool gather, const AggReduceArgs& a) {
    {
        // byte model: 8 B per row (+ 4 B of perm and a sector per row for a gathered spec), 1 bit of bitmap, 8 B per group out
        ProfScope ps(ctx, gather ? "k_agg_reduce_gather" : "k_agg_reduce", (double)a.n * (8.0 + (gather ? 4.0 : 0.0) + 1.0 / 8.0) + 20.0 * (double)a.ntiles);
        if (gather)
            hipLaunchKernelGGL((k_agg_reduce<OP, FLT, true>), dim3(tile_grid(a.ntiles)), dim3(kMatThreads), 0, ctx->stream, a.bitmap, a.offs, a.src, a.perm,
                               a.n, a.out, a.head, a.tail);
        else
            hipLaunchKernelGGL((k_agg_reduce<OP, FLT, false>), dim3(tile_grid(a.ntiles)), dim3(kMatThreads), 0, ctx->stream, a.bitmap, a.offs, a.src, a.perm,
                               a.n, a.out, a.head, a.tail);
    }
    ProfScope ps(ctx, "k_agg_carry", 24.0 * (double)a.ntiles);
    const unsigned grid = (unsigned)std::min<uint64_t>((a.ntiles + kResWaves - 1) / kResWaves, 4096);
    hipLaunchKernelGGL((k_agg_carry<OP, FLT>), dim3(grid), dim3(kMatThreads), 0, ctx->stream, a.offs, a.head, a.tail, a.ntiles, a.out);
}

template <bool FLT>
void launch_reduce_op(cph_ctx* ctx, int32_t op, bool gather, const AggReduceArgs& a) {
    if (op == CPH_AGG_SUM) launch_reduce<CPH_AGG_SUM, FLT>(ctx, gather, a);
    else if (op == CPH_AGG_MIN) launch_reduce<CPH_AGG_MIN, FLT>(ctx, gather, a);
    else launch_reduce<CPH_AGG_MAX, FLT>(ctx, gather, a);
}

}  // namespace

void agg_launch_reduce(cph_ctx* ctx, int32_t op, bool flt, bool gather, const AggReduceArgs& a) {
    if (flt) launch_reduce_op<true>(ctx, op, gather, a);
    else launch_reduce_op<false>(ctx, op, gather, a);
}

}  // namespace cph

namespace {

Status check_specs(const cph_index* ix, const cph_agg_spec* specs, int32_t nspecs) {
    if (nspecs < 0 || nspecs > CPH_AGG_MAX_SPECS) return {CPH_ERR_INVALID, "cph_index_aggregate: nspecs must be 0..CPH_AGG_MAX_SPECS"};
    if (nspecs && !specs) return {CPH_ERR_INVALID, "cph_index_aggregate: specs is NULL"};
    for (int32_t s = 0; s < nspecs; s++) {
        const cph_agg_spec& sp = specs[s];
        if (sp.op != CPH_AGG_SUM && sp.op != CPH_AGG_MIN && sp.op != CPH_AGG_MAX)
            return {CPH_ERR_INVALID, "cph_index_aggregate: unknown op (CPH_AGG_SUM, CPH_AGG_MIN or CPH_AGG_MAX)"};
        if (sp.kind != CPH_NUM_INT64 && sp.kind != CPH_NUM_FLOAT64)
            return {CPH_ERR_INVALID, "cph_index_aggregate: kind must be CPH_NUM_INT64 or CPH_NUM_FLOAT64"};
        if ((sp.col != nullptr) == (sp.numbers != nullptr))
            return {CPH_ERR_INVALID, "cph_index_aggregate: a spec takes exactly one of col / numbers"};
        if (sp.col) {
            CPH_TRY(validate_cols(sp.col, 1));
            if (sp.col->nrows < ix->table_rows)
                return {CPH_ERR_INVALID, "cph_index_aggregate: a value column has fewer rows than the index's build table"};
        } else if (sp.numbers_mem != CPH_MEM_HOST && sp.numbers_mem != CPH_MEM_DEVICE) {
            return {CPH_ERR_INVALID, "cph_index_aggregate: bad numbers_mem"};
        }
    }
    return {};
}

}  // namespace

extern "C" {

CPH_API int32_t cph_index_aggregate(cph_ctx* ctx, const cph_index* ix, const cph_agg_spec* specs, int32_t nspecs, int32_t out_mem,
                                    cph_aggregated** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!ix) return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_aggregate: index must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    {
        const Status s = check_specs(ix, specs, nspecs);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_aggregated_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.mem = out_mem;
    r->pub.nspecs = nspecs;
    r->pub.first_error_position = r->pub.first_error_row = UINT64_MAX;
    auto run = [&]() -> Status {
        const uint64_t n = ix->nrows;
        if (!n) return {};   // no rows, no groups: every array stays NULL
        const uint32_t* perm = ix->perm.as<uint32_t>();
        // the values of every spec on the device: col specs converted through perm (sorted order), host numbers uploaded
        std::vector<DevBuf> staged;
        DevBuf values[CPH_AGG_MAX_SPECS], status[CPH_AGG_MAX_SPECS], uploaded[CPH_AGG_MAX_SPECS];
        const uint64_t* src[CPH_AGG_MAX_SPECS] = {nullptr};
        NumColStats all;   // the col specs' reports, merged
        for (int32_t s = 0; s < nspecs; s++) {
            const cph_agg_spec& sp = specs[s];
            if (sp.col) {
                DevCol col;
                CPH_TRY(stage_cols(ctx, sp.col, 1, &staged, &col));
                RowIds ids;
                ids.ptr = perm;
                ids.bits = 32;
                NumColStats st;
                CPH_TRY(convert_rows(ctx, col, ids, 0, n, sp.kind, &values[s], &status[s], &st));
                all.merge(st, s);
                src[s] = values[s].as<uint64_t>();
            } else {
                CPH_TRY(device_array(ctx, static_cast<const uint64_t*>(sp.numbers), sp.numbers_mem, (size_t)ix->table_rows, &uploaded[s], &src[s]));
            }
        }
        r->pub.host_rows = all.host_rows;
        r->pub.nerrors = all.nerrors;
        if (all.nerrors) {   // data, not a failure: no arrays
            r->pub.first_error_position = all.first_error;
            r->pub.first_error_kind = all.first_kind;
            r->pub.first_error_spec = all.first_tag;
            uint32_t row = 0;
            CPH_TRY(read_device_value(ctx, perm + r->pub.first_error_position, &row));
            r->pub.first_error_row = row;
            return {};
        }
        // run starts, group slots
        TileBitmap tb;
        CPH_TRY(tb.alloc(ctx, n));
        const uint64_t ntiles = tb.ntiles;
        agg_launch_heads(ctx, ix->sorted_codes.get(), ix->codec.key32, ix->total_words(), n, (double)index_code_bytes(ix), tb.words(), tb.counts());
        CPH_HIP_TRY(hipGetLastError());
        CPH_TRY(tb.scan(ctx));
        uint32_t total = 0;
        CPH_TRY(tb.read_total(ctx, &total));   // the call's host wait (beside the conversions')
        const uint64_t ng = total;
        if (ng == 0 || ng > n) return {CPH_ERR_HIP, "cph_index_aggregate: the run count is out of range"};   // n >= 1 has a run
        CPH_TRY(r->d_pos.alloc(&ctx->pool, ng * sizeof(uint64_t)));
        CPH_TRY(r->d_row.alloc(&ctx->pool, ng * sizeof(uint32_t)));
        CPH_TRY(r->d_cnt.alloc(&ctx->pool, ng * sizeof(uint64_t)));
        agg_launch_emit(ctx, tb.words(), tb.counts(), perm, n, ng, r->d_pos.as<uint64_t>(), r->d_row.as<uint32_t>());
        CPH_HIP_TRY(hipGetLastError());
        {
            ProfScope ps(ctx, "k_agg_counts", 16.0 * (double)ng);
            hipLaunchKernelGGL(k_agg_counts, dim3(grid_for_items(ng)), dim3(kMatThreads), 0, ctx->stream, r->d_pos.as<uint64_t>(), ng, n,
                               r->d_cnt.as<uint64_t>());
        }
        CPH_HIP_TRY(hipGetLastError());
        DevBuf partials;   // head[ntiles], tail[ntiles]: every spec's kernels run one behind the other on the stream and reuse them
        if (nspecs) CPH_TRY(partials.alloc(&ctx->pool, 2 * ntiles * sizeof(uint64_t)));
        for (int32_t s = 0; s < nspecs; s++) {
            CPH_TRY(r->d_val[s].alloc(&ctx->pool, ng * sizeof(uint64_t)));
            const AggReduceArgs a{tb.words(), tb.counts(), src[s], perm, n, ntiles, r->d_val[s].as<uint64_t>(), partials.as<uint64_t>(),
                               partials.as<uint64_t>() + ntiles};
            agg_launch_reduce(ctx, specs[s].op, specs[s].kind == CPH_NUM_FLOAT64, specs[s].col == nullptr, a);
            CPH_HIP_TRY(hipGetLastError());
        }
        r->pub.ngroups = ng;
        ResultPart parts[3 + CPH_AGG_MAX_SPECS];
        parts[0] = ResultPart{&r->d_pos, (size_t)ng * sizeof(uint64_t), &r->pub.first_position};
        parts[1] = ResultPart{&r->d_row, (size_t)ng * sizeof(uint32_t), &r->pub.first_row};
        parts[2] = ResultPart{&r->d_cnt, (size_t)ng * sizeof(uint64_t), &r->pub.count};
        for (int32_t s = 0; s < nspecs; s++) parts[3 + s] = ResultPart{&r->d_val[s], (size_t)ng * sizeof(uint64_t), &r->pub.values[s]};
        return deliver(ctx, &r->own, parts, 3 + nspecs, out_mem);   // waits for the stream: the staged values may go after it
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API void cph_aggregated_release(cph_aggregated* pub) { release_result<cph_aggregated_impl>(pub); }

}  // extern "C"

// Loads this translation unit's code object now (cph_ctx_create) instead of inside the first timed call.
namespace cph {
void warm_aggregate() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_agg_emit));
    (void)hipGetLastError();
}
}  // namespace cph
