// map_switch.hip — Map (csvplus.go:290-296) with an if / else if / else inside the closure, as data: one computed string
// column whose value in row i is the template of the FIRST case whose predicate holds for row i, otherwise a default template
// (csvplus_test.go:283-288: `if row["name"] == "Amelia" { row["name"] = "Julia" }`).
//
//   cph_map_switch   conditions: cph_filter_rows programs; values: cph_map_format templates; both over the same columns.
//
// Pipeline: k_pred_eval once per case (filter.hip: pred_eval_bitmap; a predicate's strings are read once, one bit per row
// stays) -> k_switch_lens (rows on lanes; a wave's 64 rows are ONE bitmap word per case, loaded through a wave-uniform
// address; alternative = the first case with the lane's bit set, written as one byte per row; bytes of that alternative's
// value) -> exclusive scan = the result's offsets -> k_switch_copy (k_map_copy's tiles: 256 records assembled in the LDS
// stage, 16-byte stores; the alternative comes from the byte, a row runs only its alternative's pieces).  Lanes of a wave
// may take different alternatives: every lane walks its own run [first[a], first[a + 1]) of the one flat piece array, so the
// k-th pieces of two alternatives run together where they are of one kind and one after the other where they are not; the
// stage sink ORs words into LDS, so no lane depends on another's progress and rows are not sorted by alternative.
// The kernels come in map_format.hip's four piece sets, chosen over the pieces of all alternatives together, and in its two
// SPAN instantiations (k_switch_*_sp / k_switch_*_spg) where any alternative holds a SPAN piece; the operations of all
// alternatives together, at most 16, ride behind the plan (SwitchPlanSp).
// Where things live: this file has what Switch adds to map_format.hip — the bitmaps, the byte per row, the plan with one run
// of pieces per alternative, and the alternative in the messages.  What a row does in either pass is map_device.hpp's; the
// piece rules, the plan's pieces and literals, the scan with the refused-row report, the result column and the launch by
// piece set are map_plan.hpp's.
#include <new>
#include <type_traits>

#include "map_plan.hpp"

namespace cph {

constexpr int kSwitchAlts = CPH_MAP_MAX_CASES + 1;   // the cases and `otherwise`

struct SwitchPlan {   // travels in the kernel arguments (~1 KB beside ColsArg and ColIds: 2.3 KB of the 4 KB block)
    const uint8_t* lits;
    const uint64_t* bits[CPH_MAP_MAX_CASES];   // case c: word w bit b = its predicate holds for row 64 w + b
    int32_t ncases;
    uint32_t col_mask;                         // bit c: some piece of some alternative reads column c
    int32_t first[kSwitchAlts + 1];            // alternative a: pieces [first[a], first[a + 1]) of p
    uint64_t fixed[kSwitchAlts];               // ... and the bytes of its literals together
    MapPiece p[CPH_MAP_SWITCH_MAX_PIECES];
};
// the plan of a switch with SPAN pieces: their operations (of all alternatives together) ride behind it, +384 bytes
struct SwitchPlanSp : SwitchPlan {
    SpanOp ops[CPH_SPAN_MAX_TOTAL];
};
template <bool SP>
using SwitchPlanOf = std::conditional_t<SP, SwitchPlanSp, SwitchPlan>;
__device__ __forceinline__ const SpanOp* plan_ops(const SwitchPlan&) { return nullptr; }
__device__ __forceinline__ const SpanOp* plan_ops(const SwitchPlanSp& plan) { return plan.ops; }

// which[i] = the alternative of row i, lens[i] = bytes of its value.  PK >= kPiecesFloat: lens[n + 1], preset to UINT64_MAX, = the lowest row
// whose OWN alternative holds a value the float formatter refuses.
template <int NC, int PK = kPiecesBase, bool SP = false>
__global__ __launch_bounds__(kMatThreads) void k_switch_lens(ColsArg cols, ColIds ids, SwitchPlanOf<SP> plan, uint64_t n, uint8_t* __restrict__ which,
                                                            uint64_t* __restrict__ lens) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;   // a multiple of 64: a wave's rows share their bitmap words
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        const uint32_t word = __builtin_amdgcn_readfirstlane((uint32_t)(i >> 6));   // n <= 2^32 - 1
        int a = plan.ncases;
        for (int c = plan.ncases - 1; c >= 0; c--)
            if ((plan.bits[c][word] >> lane) & 1ull) a = c;
        which[i] = (uint8_t)a;
        RecordFields<NC> f;
        if constexpr (NC > 0) f.load(cols, ids, i, 0);   // offsets only
        // the lane's own run of pieces: the k-th pieces of two alternatives that are of one kind run together
        uint64_t total = plan.fixed[a];
        for (int k = plan.first[a]; k < plan.first[a + 1]; k++) total += map_piece_bytes<NC, PK, SP>(cols, ids, plan.p[k], f, i, lens + n + 1, plan.lits, plan_ops(plan));
        lens[i] = total;
    }
}
template <int NC>
constexpr auto k_switch_lens_f64 = k_switch_lens<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_switch_lens_sl = k_switch_lens<NC, kPiecesSlice>;
template <int NC>
constexpr auto k_switch_lens_g64 = k_switch_lens<NC, kPiecesShortest>;
template <int NC>
constexpr auto k_switch_lens_sp = k_switch_lens<NC, kPiecesSlice, true>;
template <int NC>
constexpr auto k_switch_lens_spg = k_switch_lens<NC, kPiecesShortest, true>;

// row i's own run of pieces [first[a], first[a + 1]): the bounds and the piece index differ from lane to lane
template <int NC, int PK, bool SP, class Sink>
__device__ __forceinline__ void switch_put_record(Sink& s, const ColsArg& cols, const ColIds& ids, const SwitchPlanOf<SP>& plan, int a,
                                                  const RecordFields<NC>& f, uint64_t i) {
    map_put_record<NC, PK, SP>(s, cols, ids, plan.lits, plan.p, plan.first[a], plan.first[a + 1], f, i, plan_ops(plan));
}

// value i at out + offs[i]
template <int NC, int PK = kPiecesBase, bool SP = false>
__global__ __launch_bounds__(kMatThreads) void k_switch_copy(ColsArg cols, ColIds ids, SwitchPlanOf<SP> plan, uint64_t n, const uint8_t* __restrict__ which,
                                                            const uint64_t* __restrict__ offs, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    for (uint64_t t0 = (uint64_t)blockIdx.x * kMatThreads; t0 < n; t0 += (uint64_t)gridDim.x * kMatThreads) {
        const uint64_t tend = t0 + kMatThreads < n ? t0 + kMatThreads : n;
        const uint64_t obase = offs[t0];
        const uint64_t span = offs[tend] - obase;
        if (span == 0) continue;   // uniform: every row of the tile picked an empty value
        const bool staged = span + 48 <= (uint64_t)kMatStage;   // uniform
        if (staged) {   // the words are OR-ed in: the stage starts out zero
            stage_clear(stage, span);
            __syncthreads();
        }
        const uint64_t i = t0 + threadIdx.x;
        // threads past the tile's end load its last record (never written): the loads of a record stay unbranched, over the
        // union of the columns any alternative reads
        RecordFields<NC> f;
        if constexpr (NC > 0) f.load(cols, ids, i < tend ? i : tend - 1, plan.col_mask);
        if (i < tend) {
            const int a = which[i];
            if (staged) {
                WordSink s(reinterpret_cast<uint32_t*>(smem), (uint32_t)((offs[i] - obase) + (obase & 15)));
                switch_put_record<NC, PK, SP>(s, cols, ids, plan, a, f, i);
                s.finish();
            } else {
                GlobalSink s{out + offs[i]};
                switch_put_record<NC, PK, SP>(s, cols, ids, plan, a, f, i);
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
constexpr auto k_switch_copy_f64 = k_switch_copy<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_switch_copy_sl = k_switch_copy<NC, kPiecesSlice>;
template <int NC>
constexpr auto k_switch_copy_g64 = k_switch_copy<NC, kPiecesShortest>;
template <int NC>
constexpr auto k_switch_copy_sp = k_switch_copy<NC, kPiecesSlice, true>;
template <int NC>
constexpr auto k_switch_copy_spg = k_switch_copy<NC, kPiecesShortest, true>;

}  // namespace cph

using namespace cph;

extern "C" {

CPH_API int32_t cph_map_switch(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                               const cph_map_case* cases, int32_t ncases, const cph_map_piece* otherwise, int32_t notherwise,
                               int32_t out_mem, cph_colbuf** out, uint8_t* which) {
    if (!ctx) return CPH_ERR_INVALID;
    if (!out) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: out must not be NULL"});
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!cases) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: cases must not be NULL"});
    if (!otherwise) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: otherwise must not be NULL"});
    if (ncases < 1 || ncases > CPH_MAP_MAX_CASES) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: 1..8 cases"});
    if (notherwise < 1 || notherwise > CPH_MAP_MAX_PIECES) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: otherwise has 1..16 pieces"});
    if (ncols < 0 || ncols > CPH_MAX_KEY_COLS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: 0..16 columns"});
    if (ncols && !cols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: cols must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: bad out_mem"});
    int total_pieces = notherwise;
    for (int c = 0; c < ncases; c++) {
        const std::string who = "cph_map_switch: case " + std::to_string(c);
        if (!cases[c].prog) return fail_with(ctx, {CPH_ERR_INVALID, who + ": prog must not be NULL"});
        if (!cases[c].pieces) return fail_with(ctx, {CPH_ERR_INVALID, who + ": pieces must not be NULL"});
        if (cases[c].npieces < 1 || cases[c].npieces > CPH_MAP_MAX_PIECES) return fail_with(ctx, {CPH_ERR_INVALID, who + ": 1..16 pieces"});
        total_pieces += cases[c].npieces;
    }
    if (total_pieces > CPH_MAP_SWITCH_MAX_PIECES)
        return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_switch: " + std::to_string(total_pieces) + " pieces in all alternatives together, more than 32"});
    const uint64_t n = nrows;
    if (n > 0xFFFFFFFFull) return fail_with(ctx, {CPH_ERR_TOO_MANY_ROWS, "cph_map_switch: more than 2^32-1 rows in one call"});
    // alternative a: its pieces, and its name in front of a message
    auto alt_pieces = [&](int a) { return a < ncases ? cases[a].pieces : otherwise; };
    auto alt_npieces = [&](int a) { return a < ncases ? cases[a].npieces : notherwise; };
    auto alt_name = [&](int a) { return "cph_map_switch: " + (a < ncases ? "case " + std::to_string(a) : std::string("otherwise")) + ", "; };
    uint64_t lit_bytes = 0;
    bool has_shortest = false, has_float = false, has_slice = false, has_span = false;
    int span_ops = 0;   // of all alternatives together
    for (int a = 0; a <= ncases; a++) {
        if (a < ncases) {
            Status s = check_pred_program(cases[a].prog, cases[a].nops, ncols);
            if (!s.ok()) return fail_with(ctx, {s.code, "cph_map_switch: case " + std::to_string(a) + ": " + s.msg});
        }
        Status s = check_map_pieces(alt_pieces(a), alt_npieces(a), ncols, n, [&](int k) { return alt_name(a) + "piece " + std::to_string(k) + ": "; },
                                    &lit_bytes, &has_shortest, &has_float, &has_slice, &has_span, &span_ops);
        if (!s.ok()) return fail_with(ctx, s);
    }
    {
        Status s = check_row_sources(cols, sel, ncols, 0, n, true);
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
        // one bitmap per case; a float column several cases compare is converted once
        std::vector<PredFloatCol> fcols;
        PredBitmap maps[CPH_MAP_MAX_CASES];
        SwitchPlanSp plan{};   // a launch without SPAN pieces takes its SwitchPlan part
        plan.ncases = ncases;
        for (int c = 0; c < ncases; c++) {
            CPH_TRY(pred_eval_bitmap(ctx, arg, ids, cases[c].prog, cases[c].nops, 0, n, &fcols, &maps[c]));
            plan.bits[c] = maps[c].rows.words();
        }
        // the alternatives' pieces in one flat array, their literals in one block
        MapPlanBuild build;
        build.ops = plan.ops;
        for (int a = 0; a <= ncases; a++) {
            CPH_TRY(append_map_pieces(ctx, alt_pieces(a), alt_npieces(a), n, arg, ids, &build, plan.p + plan.first[a], &staged, &plan.fixed[a]));
            plan.first[a + 1] = plan.first[a] + alt_npieces(a);
        }
        plan.col_mask = build.col_mask;
        DevBuf litbuf;
        CPH_TRY(upload_map_literals(ctx, build.lits, &litbuf));
        plan.lits = litbuf.as<uint8_t>();
        DevBuf whichbuf;
        CPH_TRY(whichbuf.alloc(&ctx->pool, n));
        uint8_t* which_dev = whichbuf.as<uint8_t>();
        CPH_TRY(r->d_offs.alloc(&ctx->pool, (n + (has_float ? 2 : 1)) * sizeof(uint64_t)));   // a float plan: + the refused row
        uint64_t* offs = r->d_offs.as<uint64_t>();
        if (has_float) CPH_HIP_TRY(hipMemsetAsync(offs + n + 1, 0xFF, sizeof(uint64_t), ctx->stream));
        const int pk = pieces_set(has_shortest, has_float, has_slice);
        // besides the value bytes, both passes read or write the alternative's byte
        CPH_MAP_DISPATCH(ctx, k_switch_lens, pk, has_span, (8.0 + 1.0 + (double)ncases / 8.0 + build.in_bytes) * (double)n, ncols, n, 0, arg, ids, plan, n, which_dev,
                         offs);
        uint64_t total = 0;
        CPH_TRY(scan_with_refusal(ctx, offs, n, has_float,
                                  [&](uint64_t row, const cph_map_piece** ps, int32_t* nps, std::string* prefix) -> Status {
                                      uint8_t a = 0;   // the refused row's own alternative
                                      CPH_HIP_TRY(hipMemcpy(&a, which_dev + row, 1, hipMemcpyDeviceToHost));
                                      *ps = alt_pieces(a), *nps = alt_npieces(a), *prefix = alt_name(a);
                                      return {};
                                  },
                                  &total));
        CPH_TRY(r->d_data.alloc(&ctx->pool, total + 16));
        if (total) {
            CPH_MAP_DISPATCH(ctx, k_switch_copy, pk, has_span, 2.0 * (double)total + (8.0 + 1.0 + build.in_bytes) * (double)n, ncols, n, kMatStage, arg, ids, plan, n,
                             which_dev, offs, r->d_data.as<uint8_t>());
        }
        if (which) CPH_HIP_TRY(hipMemcpyAsync(which, which_dev, n, hipMemcpyDeviceToHost, ctx->stream));
        return deliver_map_column(ctx, r, n, total, out_mem);   // the bitmaps go back to the pool behind its wait, too
    };
    return finish_call(ctx, r, run(), out);
}

}  // extern "C"
