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
// A plan with a FLOAT64 or TIME piece runs float instantiations of both kernels, as map_format.hip does, and one with a SLICE piece
// but no FLOAT64 piece the slice instantiations (k_switch_lens_sl / k_switch_copy_sl).
#include <new>
#include <string>

#include "map_device.hpp"

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

// which[i] = the alternative of row i, lens[i] = bytes of its value.  PK == kPiecesFloat: lens[n + 1], preset to UINT64_MAX, = the lowest row
// whose OWN alternative holds a value the float formatter refuses.
template <int NC, int PK = kPiecesBase>
__global__ __launch_bounds__(kMatThreads) void k_switch_lens(ColsArg cols, ColIds ids, SwitchPlan plan, uint64_t n, uint8_t* __restrict__ which,
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
        for (int k = plan.first[a]; k < plan.first[a + 1]; k++) {
            const MapPiece& p = plan.p[k];
            if (p.kind == CPH_MAP_INT64) {
                total += int_chars(p.ints[i]);
            } else if (PK == kPiecesFloat && p.kind == CPH_MAP_FLOAT64) {
                const FixedParts r = fixed_split(p.floats[i], p.col);
                total += fixed_chars(r, p.col);
                if (r.kind == FIXED_RANGE) atomicMin(reinterpret_cast<unsigned long long*>(lens + n + 1), (unsigned long long)i);
            } else if (PK == kPiecesFloat && p.kind == CPH_MAP_TIME) {   // the length needs no look at the value; the refusal does
                total += rfc3339_chars(p.col);
                if (!rfc3339_in_range(p.ints[i], p.col)) atomicMin(reinterpret_cast<unsigned long long*>(lens + n + 1), (unsigned long long)i);
            } else if (p.kind == CPH_MAP_COLUMN || (PK >= kPiecesSlice && p.kind == CPH_MAP_SLICE)) {
                total += map_field_bytes<NC, PK>(cols, ids, p, f, i);
            }
        }
        lens[i] = total;
    }
}
template <int NC>
constexpr auto k_switch_lens_f64 = k_switch_lens<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_switch_lens_sl = k_switch_lens<NC, kPiecesSlice>;

// row i's own run of pieces [first[a], first[a + 1]): the bounds and the piece index differ from lane to lane
template <int NC, int PK, class Sink>
__device__ __forceinline__ void switch_put_record(Sink& s, const ColsArg& cols, const ColIds& ids, const SwitchPlan& plan, int a,
                                                  const RecordFields<NC>& f, uint64_t i) {
    map_put_record<NC, PK>(s, cols, ids, plan.lits, plan.p, plan.first[a], plan.first[a + 1], f, i);
}

// value i at out + offs[i]
template <int NC, int PK = kPiecesBase>
__global__ __launch_bounds__(kMatThreads) void k_switch_copy(ColsArg cols, ColIds ids, SwitchPlan plan, uint64_t n, const uint8_t* __restrict__ which,
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
                switch_put_record<NC, PK>(s, cols, ids, plan, a, f, i);
                s.finish();
            } else {
                GlobalSink s{out + offs[i]};
                switch_put_record<NC, PK>(s, cols, ids, plan, a, f, i);
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

}  // namespace cph

using namespace cph;

namespace {

std::string alt_name(int a, int ncases) { return a < ncases ? "case " + std::to_string(a) : std::string("otherwise"); }

// the rules of cph_map_format for the pieces of one alternative
Status check_pieces(const cph_map_piece* pieces, int32_t npieces, int32_t ncols, uint64_t n, const std::string& who, uint64_t* lit_bytes,
                    bool* has_float, bool* has_slice) {
    for (int k = 0; k < npieces; k++) {
        const cph_map_piece& p = pieces[k];
        const std::string at = "cph_map_switch: " + who + ", piece " + std::to_string(k) + ": ";
        switch (p.kind) {
            case CPH_MAP_LITERAL:
                if (!p.value.data && p.value.len) return {CPH_ERR_INVALID, at + "a literal with bytes but no data pointer"};
                *lit_bytes += p.value.len;
                if (p.value.len > 0xFFFFFFFFull || *lit_bytes > 0xFFFFFFFFull) return {CPH_ERR_INVALID, at + "literals beyond 4 GiB"};
                break;
            case CPH_MAP_COLUMN:
                if (p.arg < 0 || p.arg >= ncols) return {CPH_ERR_INVALID, at + "a COLUMN piece outside 0..ncols-1"};
                break;
            case CPH_MAP_INT64:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, at + "bad memory space of an INT64 piece"};
                if (!p.ints && n) return {CPH_ERR_INVALID, at + "an INT64 piece without values"};
                break;
            case CPH_MAP_FLOAT64:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, at + "bad memory space of a FLOAT64 piece"};
                if (!p.floats && n) return {CPH_ERR_INVALID, at + "a FLOAT64 piece without values"};
                if (p.prec < 0 || p.prec > kFixedMaxPrec) return {CPH_ERR_INVALID, at + "prec of a FLOAT64 piece outside 0..22"};
                *has_float = true;
                break;
            case CPH_MAP_TIME:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, at + "bad memory space of a TIME piece"};
                if (!p.ints && n) return {CPH_ERR_INVALID, at + "a TIME piece without values"};
                if (p.prec < -kTimeMaxZone || p.prec > kTimeMaxZone)
                    return {CPH_ERR_INVALID, at + "prec of a TIME piece (the zone in minutes east of UTC) outside -1439..1439"};
                *has_float = true;   // the instantiations that report a refused value
                break;
            case CPH_MAP_SLICE:
                if (p.arg < 0 || p.arg >= ncols) return {CPH_ERR_INVALID, at + "a SLICE piece's column outside 0..ncols-1"};
                if (!p.value.data || p.value.len != sizeof(cph_map_slice))
                    return {CPH_ERR_INVALID, at + "a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer"};
                *has_slice = true;
                break;
            default:
                return {CPH_ERR_INVALID, at + "unknown piece kind (1..4, 8, 10)"};
        }
    }
    return {};
}

}  // namespace

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
    uint64_t lit_bytes = 0;
    bool has_float = false, has_slice = false;
    for (int a = 0; a <= ncases; a++) {
        if (a < ncases) {
            Status s = check_pred_program(cases[a].prog, cases[a].nops, ncols);
            if (!s.ok()) return fail_with(ctx, {s.code, "cph_map_switch: case " + std::to_string(a) + ": " + s.msg});
        }
        Status s = check_pieces(a < ncases ? cases[a].pieces : otherwise, a < ncases ? cases[a].npieces : notherwise, ncols, n,
                                alt_name(a, ncases), &lit_bytes, &has_float, &has_slice);
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
        r->pub.col.offset_bits = 64;
        r->pub.col.mem = out_mem;
        r->pub.col.fixed_width = 0;
        if (n == 0) {
            CPH_TRY(r->d_offs.alloc(&ctx->pool, sizeof(uint64_t)));
            CPH_HIP_TRY(hipMemsetAsync(r->d_offs.get(), 0, sizeof(uint64_t), ctx->stream));
            CPH_TRY(r->d_data.alloc(&ctx->pool, 16));
            r->pub.nbytes = 0;
            r->pub.col.nrows = 0;
            const ResultPart parts[2] = {{&r->d_offs, sizeof(uint64_t), &r->pub.col.offsets}, {&r->d_data, 0, &r->pub.col.data}};
            return deliver(ctx, &r->own, parts, 2, out_mem);
        }
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, nullptr, ncols, 0, n, &staged, &arg, &ids));
        // one bitmap per case; a float column several cases compare is converted once
        std::vector<PredFloatCol> fcols;
        PredBitmap maps[CPH_MAP_MAX_CASES];
        SwitchPlan plan{};
        plan.ncases = ncases;
        for (int c = 0; c < ncases; c++) {
            CPH_TRY(pred_eval_bitmap(ctx, arg, ids, cases[c].prog, cases[c].nops, 0, n, &fcols, &maps[c]));
            plan.bits[c] = maps[c].bitmap.as<uint64_t>();
        }
        // the alternatives' pieces in one flat array, their literals in one block
        std::string lits;
        double in_bytes = 0;   // what the copy pass reads per row besides the value bytes and the alternative
        uint32_t slice_cols = 0;
        int np = 0;
        for (int a = 0; a <= ncases; a++) {
            const cph_map_piece* pieces = a < ncases ? cases[a].pieces : otherwise;
            const int npieces = a < ncases ? cases[a].npieces : notherwise;
            plan.first[a] = np;
            const size_t lit0 = lits.size();
            for (int k = 0; k < npieces; k++) {
                const cph_map_piece& p = pieces[k];
                MapPiece& d = plan.p[np++];
                d.kind = p.kind;
                if (p.kind == CPH_MAP_LITERAL) {
                    d.off = (uint32_t)lits.size();
                    d.len = (uint32_t)p.value.len;
                    if (d.len) lits.append(reinterpret_cast<const char*>(p.value.data), d.len);
                } else if (p.kind == CPH_MAP_COLUMN) {
                    d.col = p.arg;
                    if (!((plan.col_mask >> p.arg) & 1u)) {
                        in_bytes += arg.c[p.arg].fixed_width ? 0.0 : (double)(arg.c[p.arg].offset_bits / 8);
                        if (ids.ids[p.arg].ptr) in_bytes += (double)(ids.ids[p.arg].bits / 8);
                    }
                    plan.col_mask |= 1u << p.arg;
                } else if (p.kind == CPH_MAP_SLICE) {   // not in col_mask: a slice loads its own first chunk
                    cph_map_slice sl;
                    memcpy(&sl, p.value.data, sizeof sl);
                    d.col = p.arg;
                    d.from = sl.from;
                    d.to = sl.to;
                    if (!((slice_cols >> p.arg) & 1u) && !((plan.col_mask >> p.arg) & 1u)) {
                        in_bytes += arg.c[p.arg].fixed_width ? 0.0 : (double)(arg.c[p.arg].offset_bits / 8);
                        if (ids.ids[p.arg].ptr) in_bytes += (double)(ids.ids[p.arg].bits / 8);
                    }
                    slice_cols |= 1u << p.arg;
                } else {   // INT64 / FLOAT64 / TIME: 8 bytes per row
                    const void* vals = p.kind == CPH_MAP_FLOAT64 ? static_cast<const void*>(p.floats) : static_cast<const void*>(p.ints);
                    in_bytes += 8.0;
                    if (p.arg == CPH_MEM_HOST) {   // staged like the row ids of a host column
                        staged.emplace_back();
                        CPH_TRY(staged.back().alloc(&ctx->pool, n * sizeof(int64_t)));
                        CPH_HIP_TRY(hipMemcpyAsync(staged.back().get(), vals, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
                        vals = staged.back().get();
                    }
                    if (p.kind == CPH_MAP_INT64) {
                        d.ints = static_cast<const int64_t*>(vals);
                    } else if (p.kind == CPH_MAP_TIME) {
                        d.ints = static_cast<const int64_t*>(vals);
                        d.col = p.prec;
                    } else {
                        d.floats = static_cast<const double*>(vals);
                        d.col = p.prec;
                    }
                }
            }
            plan.fixed[a] = lits.size() - lit0;
        }
        plan.first[ncases + 1] = np;
        DevBuf litbuf;
        CPH_TRY(litbuf.alloc(&ctx->pool, lits.size() + 16));
        if (!lits.empty()) {
            void* slot = nullptr;
            CPH_TRY(pinned_upload(ctx, lits.size(), &slot));
            memcpy(slot, lits.data(), lits.size());
            CPH_HIP_TRY(hipMemcpyAsync(litbuf.get(), slot, lits.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        plan.lits = litbuf.as<uint8_t>();
        DevBuf whichbuf;
        CPH_TRY(whichbuf.alloc(&ctx->pool, n));
        uint8_t* which_dev = whichbuf.as<uint8_t>();
        CPH_TRY(r->d_offs.alloc(&ctx->pool, (n + (has_float ? 2 : 1)) * sizeof(uint64_t)));   // a float plan: + the refused row
        uint64_t* offs = r->d_offs.as<uint64_t>();
        if (has_float) CPH_HIP_TRY(hipMemsetAsync(offs + n + 1, 0xFF, sizeof(uint64_t), ctx->stream));
        {
            ProfScope ps(ctx, has_slice && !has_float ? "k_switch_lens_sl" : "k_switch_lens", (8.0 + 1.0 + (double)ncases / 8.0 + in_bytes) * (double)n);
            if (has_float) {
                CPH_CSV_DISPATCH(k_switch_lens_f64, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, which_dev, offs);
            } else if (has_slice) {
                CPH_CSV_DISPATCH(k_switch_lens_sl, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, which_dev, offs);
            } else {
                CPH_CSV_DISPATCH(k_switch_lens, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, which_dev, offs);
            }
        }
        CPH_HIP_TRY(hipGetLastError());
        uint64_t total = 0;
        if (has_float) {   // the total and the refused row in one copy: the call's one host wait
            CPH_TRY(exclusive_scan_u64(ctx, offs, n, offs + n));
            struct { uint64_t total, bad; } tail;
            CPH_TRY(read_device_value(ctx, reinterpret_cast<const decltype(tail)*>(offs + n), &tail));
            if (tail.bad != UINT64_MAX) {
                uint8_t a = 0;
                CPH_HIP_TRY(hipMemcpy(&a, which_dev + tail.bad, 1, hipMemcpyDeviceToHost));
                const cph_map_piece* pieces = a < ncases ? cases[a].pieces : otherwise;
                const int npieces = a < ncases ? cases[a].npieces : notherwise;
                int piece = 0;   // the first FLOAT64 or TIME piece of that row's alternative with such a value
                for (int k = 0; k < npieces; k++) {
                    if (pieces[k].kind == CPH_MAP_TIME) {
                        int64_t t = 0;
                        if (pieces[k].arg == CPH_MEM_HOST) t = pieces[k].ints[tail.bad];
                        else CPH_HIP_TRY(hipMemcpy(&t, pieces[k].ints + tail.bad, sizeof t, hipMemcpyDeviceToHost));
                        if (!rfc3339_in_range(t, pieces[k].prec))
                            return Status{CPH_ERR_INVALID, "cph_map_switch: " + alt_name(a, ncases) + ", TIME piece " + std::to_string(k) + ", row " +
                                                               std::to_string(tail.bad) + ": the local year of " + std::to_string(t) + " is outside 0000..9999"};
                        continue;
                    }
                    if (pieces[k].kind != CPH_MAP_FLOAT64) continue;
                    double v = 0;
                    if (pieces[k].arg == CPH_MEM_HOST) v = pieces[k].floats[tail.bad];
                    else CPH_HIP_TRY(hipMemcpy(&v, pieces[k].floats + tail.bad, sizeof v, hipMemcpyDeviceToHost));
                    if (fixed_split(v, 0).kind == FIXED_RANGE) {
                        piece = k;
                        break;
                    }
                }
                return Status{CPH_ERR_INVALID, "cph_map_switch: " + alt_name(a, ncases) + ", FLOAT64 piece " + std::to_string(piece) + ", row " +
                                                   std::to_string(tail.bad) + ": a finite value of 2^128 or more is not formatted"};
            }
            total = tail.total;
        } else {
            CPH_TRY(scan_lengths(ctx, offs, n, &total));
        }
        CPH_TRY(r->d_data.alloc(&ctx->pool, total + 16));
        if (total) {
            ProfScope ps(ctx, has_slice && !has_float ? "k_switch_copy_sl" : "k_switch_copy", 2.0 * (double)total + (8.0 + 1.0 + in_bytes) * (double)n);
            if (has_float) {
                CPH_CSV_DISPATCH(k_switch_copy_f64, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, which_dev, offs,
                                 r->d_data.as<uint8_t>());
            } else if (has_slice) {
                CPH_CSV_DISPATCH(k_switch_copy_sl, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, which_dev, offs,
                                 r->d_data.as<uint8_t>());
            } else {
                CPH_CSV_DISPATCH(k_switch_copy, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, which_dev, offs,
                                 r->d_data.as<uint8_t>());
            }
            CPH_HIP_TRY(hipGetLastError());
        }
        if (which) CPH_HIP_TRY(hipMemcpyAsync(which, which_dev, n, hipMemcpyDeviceToHost, ctx->stream));
        // the kernels read the bitmaps, the literal block and the staged arrays: they go back to the pool behind deliver's wait
        r->pub.nbytes = total;
        r->pub.col.nrows = n;
        const ResultPart parts[2] = {{&r->d_offs, (size_t)(n + 1) * sizeof(uint64_t), &r->pub.col.offsets},
                                     {&r->d_data, (size_t)total, &r->pub.col.data}};
        return deliver(ctx, &r->own, parts, 2, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

}  // extern "C"
