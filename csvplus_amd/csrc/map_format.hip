// map_format.hip — Map (csvplus.go:290-296) with a ROW TEMPLATE instead of a closure: one computed string column.
//
//   cph_map_format  value i of the new column = the template's pieces in order: literal bytes, the value of a column in
//                   row i (read through that column's row ids, as the writers read a joined row), an int64 written as
//                   strconv.FormatInt(v, 10), a float64 written as strconv.FormatFloat(v, 'f', prec, 64) (numformat_device.hpp),
//                   a slice [from, to) of a column's value in row i, Unix seconds written as RFC 3339 (timeparse_device.hpp),
//                   a float64 written with its shortest round-trip digits, FormatFloat(v, 'e' / 'f' / 'g', -1, 64) (shortfmt_device.hpp),
//                   a column's value in row i narrowed by a short program of span operations — TrimSpace, Trim*, TrimPrefix /
//                   TrimSuffix, one field of Split / SplitN, a slice of what is left (CPH_MAP_SPAN, span_device.hpp).
//                   Bytes are copied verbatim; nothing is escaped.
//
// The pipeline of the gather and of the two-pass CSV writer (materialize.hip): k_map_lens (bytes per row: offsets only, the
// literals' total, digit counts by compares) -> exclusive scan, whose nrows + 1 entries ARE the result column's offsets ->
// k_map_copy (a tile's rows assembled in the LDS stage 8 value bytes at a time, streamed out with 16-byte stores; a tile
// beyond the stage writes its rows to global memory itself).  Two passes, no look-back and no waiting between workgroups.
// The literals are packed into one small device block that every row reads 8 bytes at a time.
// Both kernels come in four piece sets (map_device.hpp: pieces_set), and a template launches the smallest that holds its
// pieces: the base pair carries no SLICE code (strpred_device.hpp: slice_span) and no float code; the slice pair
// (k_map_lens_sl / k_map_copy_sl) adds SLICE; the float pair (k_map_lens_f64 / k_map_copy_f64) adds SLICE, FLOAT64 and TIME,
// the pieces whose values can be refused (beyond the formatter's range; a local year outside 0000..9999).  Its length pass
// also finds the lowest refused row, which comes back in the same copy as the scan's total.  The shortest pair (k_map_lens_g64 /
// k_map_copy_g64) adds FLOAT64_SHORTEST (shortfmt_device.hpp) to all of those: the digit generator's registers stay out of the
// float pair, which compiles to what it was.  Both passes run the digit generator; nothing is cached between them.
// A SPAN piece is a boolean beside the piece set (SP): k_map_lens_sp / k_map_copy_sp carry SPAN over the slice set, so a template
// of spans, slices, columns, literals and ints pays no formatter's registers, and k_map_*_spg over the shortest set, for SPAN
// beside any other piece; both report as k_map_*_sp.  Their plan (MapPlanSp) carries the operations, at most 16 of 24 bytes,
// behind MapPlan; every launch without a SPAN piece takes MapPlan and the instantiation it took before.  For a SPAN piece the
// length pass reads value bytes (the span has to be found), and the copy pass finds the span again: nothing is cached between
// them either.  One lane runs one row's program: correct for any value length, tuned for CSV-sized values.
// Where things live: this file has the plan (a kernel argument), the two kernels' row loops and the entry point's own
// arguments.  map_device.hpp has what a row does in either pass; map_plan.hpp has the piece rules, the plan's pieces and
// literals, the scan with the refused-row report, the result column and the launch by piece set.  map_switch.hip shares both.
#include <new>
#include <type_traits>

#include "map_plan.hpp"

namespace cph {

struct MapPlan {
    const uint8_t* lits;
    int32_t npieces;
    uint32_t col_mask;     // bit c: some piece reads column c
    uint64_t fixed;        // bytes of the literals together
    MapPiece p[CPH_MAP_MAX_PIECES];
};
// the plan of a template with SPAN pieces: their operations ride behind it, and only the _sp kernels take them
struct MapPlanSp : MapPlan {
    SpanOp ops[CPH_SPAN_MAX_TOTAL];
};
template <bool SP>
using MapPlanOf = std::conditional_t<SP, MapPlanSp, MapPlan>;
__device__ __forceinline__ const SpanOp* plan_ops(const MapPlan&) { return nullptr; }
__device__ __forceinline__ const SpanOp* plan_ops(const MapPlanSp& plan) { return plan.ops; }

// lens[i] = bytes of value i.  PK >= kPiecesFloat (the plan has a FLOAT64 or TIME piece): lens[n + 1], preset to UINT64_MAX, = the lowest
// row with a value the formatter refuses.
template <int NC, int PK = kPiecesBase, bool SP = false>
__global__ __launch_bounds__(kMatThreads) void k_map_lens(ColsArg cols, ColIds ids, MapPlanOf<SP> plan, uint64_t n, uint64_t* __restrict__ lens) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    uint64_t* const refused = lens + n + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        uint64_t total = plan.fixed;
        RecordFields<NC> f;
        if constexpr (NC > 0) f.load(cols, ids, i, 0);   // offsets only
        for (int k = 0; k < plan.npieces; k++) total += map_piece_bytes<NC, PK, SP>(cols, ids, plan.p[k], f, i, refused, plan.lits, plan_ops(plan));
        lens[i] = total;
    }
}
// the piece sets under names CPH_CSV_DISPATCH can take
template <int NC>
constexpr auto k_map_lens_f64 = k_map_lens<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_map_lens_sl = k_map_lens<NC, kPiecesSlice>;
template <int NC>
constexpr auto k_map_lens_g64 = k_map_lens<NC, kPiecesShortest>;
template <int NC>
constexpr auto k_map_lens_sp = k_map_lens<NC, kPiecesSlice, true>;
template <int NC>
constexpr auto k_map_lens_spg = k_map_lens<NC, kPiecesShortest, true>;

// value i at out + offs[i]
template <int NC, int PK = kPiecesBase, bool SP = false>
__global__ __launch_bounds__(kMatThreads) void k_map_copy(ColsArg cols, ColIds ids, MapPlanOf<SP> plan, uint64_t n, const uint64_t* __restrict__ offs,
                                                         uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    for (uint64_t t0 = (uint64_t)blockIdx.x * kMatThreads; t0 < n; t0 += (uint64_t)gridDim.x * kMatThreads) {
        const uint64_t tend = t0 + kMatThreads < n ? t0 + kMatThreads : n;
        const uint64_t obase = offs[t0];
        const uint64_t span = offs[tend] - obase;
        const bool staged = span + 48 <= (uint64_t)kMatStage;   // uniform
        if (staged) {   // the words are OR-ed in: the stage starts out zero
            stage_clear(stage, span);
            __syncthreads();
        }
        const uint64_t i = t0 + threadIdx.x;
        // threads past the tile's end load its last record (never written): the loads of a record stay unbranched
        RecordFields<NC> f;
        if constexpr (NC > 0) f.load(cols, ids, i < tend ? i : tend - 1, plan.col_mask);
        if (i < tend) {
            if (staged) {
                WordSink s(reinterpret_cast<uint32_t*>(smem), (uint32_t)((offs[i] - obase) + (obase & 15)));
                map_put_record<NC, PK, SP>(s, cols, ids, plan.lits, plan.p, 0, plan.npieces, f, i, plan_ops(plan));
                s.finish();
            } else {
                GlobalSink s{out + offs[i]};
                map_put_record<NC, PK, SP>(s, cols, ids, plan.lits, plan.p, 0, plan.npieces, f, i, plan_ops(plan));
            }
        }
        if (staged) {
            lds_atomics_barrier();
            flush_stage(stage, out, obase, span);
            __syncthreads();
        }
    }
}
template <int NC>
constexpr auto k_map_copy_f64 = k_map_copy<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_map_copy_sl = k_map_copy<NC, kPiecesSlice>;
template <int NC>
constexpr auto k_map_copy_g64 = k_map_copy<NC, kPiecesShortest>;
template <int NC>
constexpr auto k_map_copy_sp = k_map_copy<NC, kPiecesSlice, true>;
template <int NC>
constexpr auto k_map_copy_spg = k_map_copy<NC, kPiecesShortest, true>;

}  // namespace cph

using namespace cph;

extern "C" {

CPH_API int32_t cph_map_format(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                               const cph_map_piece* pieces, int32_t npieces, int32_t out_mem, cph_colbuf** out) {
    if (!ctx) return CPH_ERR_INVALID;
    if (!out) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: out must not be NULL"});
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!pieces) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: pieces must not be NULL"});
    if (npieces < 1 || npieces > CPH_MAP_MAX_PIECES) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: 1..16 pieces"});
    if (ncols < 0 || ncols > CPH_MAX_KEY_COLS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: 0..16 columns"});
    if (ncols && !cols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: cols must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    const uint64_t n = nrows;
    const std::string who = "cph_map_format: ";
    uint64_t lit_bytes = 0;
    bool has_shortest = false, has_float = false, has_slice = false, has_span = false;
    int span_ops = 0;
    {
        Status s = check_map_pieces(pieces, npieces, ncols, n, [&](int) { return who; }, &lit_bytes, &has_shortest, &has_float, &has_slice, &has_span,
                                    &span_ops);
        if (s.ok()) s = check_row_sources(cols, sel, ncols, 0, n, true);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_colbuf_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    auto run = [&]() -> Status {
        if (n == 0) return deliver_map_column(ctx, r, 0, 0, out_mem);
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, nullptr, ncols, 0, n, &staged, &arg, &ids));
        MapPlanSp plan{};   // a launch without SPAN pieces takes its MapPlan part
        MapPlanBuild build;
        build.ops = plan.ops;
        plan.npieces = npieces;
        CPH_TRY(append_map_pieces(ctx, pieces, npieces, n, arg, ids, &build, plan.p, &staged, &plan.fixed));
        plan.col_mask = build.col_mask;
        DevBuf litbuf;
        CPH_TRY(upload_map_literals(ctx, build.lits, &litbuf));
        plan.lits = litbuf.as<uint8_t>();
        CPH_TRY(r->d_offs.alloc(&ctx->pool, (n + (has_float ? 2 : 1)) * sizeof(uint64_t)));   // a float plan: + the refused row
        uint64_t* offs = r->d_offs.as<uint64_t>();
        if (has_float) CPH_HIP_TRY(hipMemsetAsync(offs + n + 1, 0xFF, sizeof(uint64_t), ctx->stream));
        const int pk = pieces_set(has_shortest, has_float, has_slice);
        CPH_MAP_DISPATCH(ctx, k_map_lens, pk, has_span, 0, ncols, n, 0, arg, ids, plan, n, offs);
        uint64_t total = 0;
        CPH_TRY(scan_with_refusal(ctx, offs, n, has_float,
                                  [&](uint64_t, const cph_map_piece** ps, int32_t* nps, std::string* prefix) {
                                      *ps = pieces, *nps = npieces, *prefix = who;
                                      return Status{};
                                  },
                                  &total));
        CPH_TRY(r->d_data.alloc(&ctx->pool, total + 16));
        if (total) {
            CPH_MAP_DISPATCH(ctx, k_map_copy, pk, has_span, 2.0 * (double)total + (8.0 + build.in_bytes) * (double)n, ncols, n, kMatStage, arg, ids, plan, n, offs,
                             r->d_data.as<uint8_t>());
        }
        return deliver_map_column(ctx, r, n, total, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

}  // extern "C"
