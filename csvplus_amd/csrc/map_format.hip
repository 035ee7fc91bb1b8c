// map_format.hip — Map (csvplus.go:290-296) with a ROW TEMPLATE instead of a closure: one computed string column.
//
//   cph_map_format  value i of the new column = the template's pieces in order: literal bytes, the value of a column in
//                   row i (read through that column's row ids, as the writers read a joined row), an int64 written as
//                   strconv.FormatInt(v, 10), a float64 written as strconv.FormatFloat(v, 'f', prec, 64) (numformat_device.hpp),
//                   a slice [from, to) of a column's value in row i.
//                   Bytes are copied verbatim; nothing is escaped.
//
// The pipeline of the gather and of the two-pass CSV writer (materialize.hip): k_map_lens (bytes per row: offsets only, the
// literals' total, digit counts by compares) -> exclusive scan, whose nrows + 1 entries ARE the result column's offsets ->
// k_map_copy (a tile's rows assembled in the LDS stage 8 value bytes at a time, streamed out with 16-byte stores; a tile
// beyond the stage writes its rows to global memory itself).  Two passes, no look-back and no waiting between workgroups.
// The literals are packed into one small device block that every row reads 8 bytes at a time.
// A template with a FLOAT64 piece runs its own instantiations of both kernels (k_map_lens_f64 / k_map_copy_f64): the others
// carry no float code.  The length pass of those also finds the lowest row whose value is beyond the formatter's range; the
// row number comes back in the same copy as the scan's total.
// A template with a TIME piece (Unix seconds written as RFC 3339, timeparse_device.hpp) runs the float pair as well: its values can be
// refused too (a local year outside 0000..9999), and the lowest refused row travels the same way.
// A template with a SLICE piece (bytes [from, to) of a column's value, strpred_device.hpp: slice_span) and no FLOAT64 piece runs
// a third pair (k_map_lens_sl / k_map_copy_sl); with both it runs the float pair, which carries the slice code too.  The length
// pass takes a slice from the value's span alone; the copy pass puts (begin + from', len') through a COLUMN piece's chunk loop.
// The digit counts, the integer writer and the loop over a run of pieces are shared with map_switch.hip (map_device.hpp).
#include <new>
#include <string>

#include "map_device.hpp"

namespace cph {

struct MapPlan {
    const uint8_t* lits;
    int32_t npieces;
    uint32_t col_mask;     // bit c: some piece reads column c
    uint64_t fixed;        // bytes of the literals together
    MapPiece p[CPH_MAP_MAX_PIECES];
};

// lens[i] = bytes of value i.  PK == kPiecesFloat (the plan has a FLOAT64 piece): lens[n + 1], preset to UINT64_MAX, = the lowest row with a
// value the formatter refuses.
template <int NC, int PK = kPiecesBase>
__global__ __launch_bounds__(kMatThreads) void k_map_lens(ColsArg cols, ColIds ids, MapPlan plan, uint64_t n, uint64_t* __restrict__ lens) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        uint64_t total = plan.fixed;
        RecordFields<NC> f;
        if constexpr (NC > 0) f.load(cols, ids, i, 0);   // offsets only
        for (int k = 0; k < plan.npieces; k++) {
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
// the float instantiations under names CPH_CSV_DISPATCH can take
template <int NC>
constexpr auto k_map_lens_f64 = k_map_lens<NC, kPiecesFloat>;
template <int NC>
constexpr auto k_map_lens_sl = k_map_lens<NC, kPiecesSlice>;

// value i at out + offs[i]
template <int NC, int PK = kPiecesBase>
__global__ __launch_bounds__(kMatThreads) void k_map_copy(ColsArg cols, ColIds ids, MapPlan plan, uint64_t n, const uint64_t* __restrict__ offs,
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
                map_put_record<NC, PK>(s, cols, ids, plan.lits, plan.p, 0, plan.npieces, f, i);
                s.finish();
            } else {
                GlobalSink s{out + offs[i]};
                map_put_record<NC, PK>(s, cols, ids, plan.lits, plan.p, 0, plan.npieces, f, i);
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
    uint64_t lit_bytes = 0;
    bool has_float = false, has_slice = false;
    for (int k = 0; k < npieces; k++) {
        const cph_map_piece& p = pieces[k];
        switch (p.kind) {
            case CPH_MAP_LITERAL:
                if (!p.value.data && p.value.len) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a literal with bytes but no data pointer"});
                lit_bytes += p.value.len;
                if (p.value.len > 0xFFFFFFFFull || lit_bytes > 0xFFFFFFFFull) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: literals beyond 4 GiB"});
                break;
            case CPH_MAP_COLUMN:
                if (p.arg < 0 || p.arg >= ncols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a COLUMN piece outside 0..ncols-1"});
                break;
            case CPH_MAP_INT64:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: bad memory space of an INT64 piece"});
                if (!p.ints && n) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: an INT64 piece without values"});
                break;
            case CPH_MAP_FLOAT64:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: bad memory space of a FLOAT64 piece"});
                if (!p.floats && n) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a FLOAT64 piece without values"});
                if (p.prec < 0 || p.prec > kFixedMaxPrec) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: prec of a FLOAT64 piece outside 0..22"});
                has_float = true;
                break;
            case CPH_MAP_TIME:
                if (p.arg != CPH_MEM_HOST && p.arg != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: bad memory space of a TIME piece"});
                if (!p.ints && n) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a TIME piece without values"});
                if (p.prec < -kTimeMaxZone || p.prec > kTimeMaxZone)
                    return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: prec of a TIME piece (the zone in minutes east of UTC) outside -1439..1439"});
                has_float = true;   // the instantiations that report a refused value
                break;
            case CPH_MAP_SLICE:
                if (p.arg < 0 || p.arg >= ncols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a SLICE piece's column outside 0..ncols-1"});
                if (!p.value.data || p.value.len != sizeof(cph_map_slice))
                    return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer"});
                has_slice = true;
                break;
            default:
                return fail_with(ctx, {CPH_ERR_INVALID, "cph_map_format: unknown piece kind (1..4, 8, 10)"});
        }
    }
    {
        Status s = check_row_sources(cols, sel, ncols, 0, n, true);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_colbuf_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    auto run = [&]() -> Status {
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, nullptr, ncols, 0, n, &staged, &arg, &ids));
        CPH_TRY(r->d_offs.alloc(&ctx->pool, (n + (has_float ? 2 : 1)) * sizeof(uint64_t)));   // a float plan: + the refused row
        uint64_t* offs = r->d_offs.as<uint64_t>();
        uint64_t total = 0;
        if (n) {
            MapPlan plan{};
            plan.npieces = npieces;
            std::string lits;
            double in_bytes = 0;   // what the copy pass reads per row besides the value bytes
            uint32_t slice_cols = 0;
            for (int k = 0; k < npieces; k++) {
                const cph_map_piece& p = pieces[k];
                MapPiece& d = plan.p[k];
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
            plan.fixed = lits.size();
            DevBuf litbuf;
            CPH_TRY(litbuf.alloc(&ctx->pool, lits.size() + 16));
            if (!lits.empty()) {
                void* slot = nullptr;
                CPH_TRY(pinned_upload(ctx, lits.size(), &slot));
                memcpy(slot, lits.data(), lits.size());
                CPH_HIP_TRY(hipMemcpyAsync(litbuf.get(), slot, lits.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            plan.lits = litbuf.as<uint8_t>();
            if (has_float) {
                CPH_HIP_TRY(hipMemsetAsync(offs + n + 1, 0xFF, sizeof(uint64_t), ctx->stream));
                ProfScope ps(ctx, "k_map_lens", 0);
                CPH_CSV_DISPATCH(k_map_lens_f64, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, offs);
            } else if (has_slice) {
                ProfScope ps(ctx, "k_map_lens_sl", 0);
                CPH_CSV_DISPATCH(k_map_lens_sl, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, offs);
            } else {
                ProfScope ps(ctx, "k_map_lens", 0);
                CPH_CSV_DISPATCH(k_map_lens, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, plan, n, offs);
            }
            CPH_HIP_TRY(hipGetLastError());
            if (has_float) {   // the total and the refused row in one copy: the call's one host wait
                CPH_TRY(exclusive_scan_u64(ctx, offs, n, offs + n));
                struct { uint64_t total, bad; } tail;
                CPH_TRY(read_device_value(ctx, reinterpret_cast<const decltype(tail)*>(offs + n), &tail));
                if (tail.bad != UINT64_MAX) {
                    int piece = 0;   // the first FLOAT64 or TIME piece with such a value in that row
                    for (int k = 0; k < npieces; k++) {
                        if (pieces[k].kind == CPH_MAP_TIME) {
                            int64_t t = 0;
                            if (pieces[k].arg == CPH_MEM_HOST) t = pieces[k].ints[tail.bad];
                            else CPH_HIP_TRY(hipMemcpy(&t, pieces[k].ints + tail.bad, sizeof t, hipMemcpyDeviceToHost));
                            if (!rfc3339_in_range(t, pieces[k].prec))
                                return Status{CPH_ERR_INVALID, "cph_map_format: TIME piece " + std::to_string(k) + ", row " + std::to_string(tail.bad) +
                                                                   ": the local year of " + std::to_string(t) + " is outside 0000..9999"};
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
                    return Status{CPH_ERR_INVALID, "cph_map_format: FLOAT64 piece " + std::to_string(piece) + ", row " + std::to_string(tail.bad) +
                                                       ": a finite value of 2^128 or more is not formatted"};
                }
                total = tail.total;
            } else {
                CPH_TRY(scan_lengths(ctx, offs, n, &total));
            }
            CPH_TRY(r->d_data.alloc(&ctx->pool, total + 16));
            if (total) {
                ProfScope ps(ctx, has_slice && !has_float ? "k_map_copy_sl" : "k_map_copy", 2.0 * (double)total + (8.0 + in_bytes) * (double)n);
                if (has_float) {
                    CPH_CSV_DISPATCH(k_map_copy_f64, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, offs, r->d_data.as<uint8_t>());
                } else if (has_slice) {
                    CPH_CSV_DISPATCH(k_map_copy_sl, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, offs, r->d_data.as<uint8_t>());
                } else {
                    CPH_CSV_DISPATCH(k_map_copy, ncols, dim3(grid_rows(n)), kMatStage, ctx->stream, arg, ids, plan, n, offs, r->d_data.as<uint8_t>());
                }
                CPH_HIP_TRY(hipGetLastError());
            }
            // the kernels read the literal block and the staged arrays: they go back to the pool behind deliver's wait
            r->pub.nbytes = total;
            r->pub.col.nrows = n;
            r->pub.col.offset_bits = 64;
            r->pub.col.mem = out_mem;
            r->pub.col.fixed_width = 0;
            const ResultPart parts[2] = {{&r->d_offs, (size_t)(n + 1) * sizeof(uint64_t), &r->pub.col.offsets},
                                         {&r->d_data, (size_t)total, &r->pub.col.data}};
            return deliver(ctx, &r->own, parts, 2, out_mem);
        }
        CPH_HIP_TRY(hipMemsetAsync(offs, 0, sizeof(uint64_t), ctx->stream));
        CPH_TRY(r->d_data.alloc(&ctx->pool, 16));
        r->pub.nbytes = 0;
        r->pub.col.nrows = 0;
        r->pub.col.offset_bits = 64;
        r->pub.col.mem = out_mem;
        r->pub.col.fixed_width = 0;
        const ResultPart parts[2] = {{&r->d_offs, sizeof(uint64_t), &r->pub.col.offsets}, {&r->d_data, 0, &r->pub.col.data}};
        return deliver(ctx, &r->own, parts, 2, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

}  // extern "C"
