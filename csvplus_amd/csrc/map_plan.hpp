// map_plan.hpp — the host side the two Map entry points share (map_format.hip: one template; map_switch.hip: one per
// alternative): the rules for a template's pieces, the pieces as the kernels see them (map_device.hpp: MapPiece) with their
// literal block and staged number arrays, the scan with the refused-row report, the result column, and the choice among a
// kernel's piece sets.  Host only; the kernels and their plans (kernel arguments) stay with each entry point.
#pragma once

#include <string>

#include "map_device.hpp"

namespace cph {

// The rules for the operations of one SPAN piece (include/csvplus_hip.h: cph_span_op).  fail(words) = the Status with the
// piece's prefix in front; the operations' literal bytes count into *lit_bytes, their number into *span_ops (the call's).
template <class Fail>
Status check_span_piece(const cph_map_piece& p, int32_t ncols, Fail fail, uint64_t* lit_bytes, int* span_ops) {
    if (p.arg < 0 || p.arg >= ncols) return fail("a SPAN piece's column outside 0..ncols-1");
    if (!p.value.data || p.value.len % sizeof(cph_span_op))
        return fail("a SPAN piece's value is a whole number of cph_span_op (40 bytes each) behind a non-NULL pointer");
    const uint64_t nops = p.value.len / sizeof(cph_span_op);
    if (nops < 1 || nops > CPH_SPAN_MAX_OPS) return fail("a SPAN piece holds 1..4 operations");
    *span_ops += (int)nops;
    if (*span_ops > CPH_SPAN_MAX_TOTAL) return fail("more than 16 SPAN operations in the pieces of one call together");
    for (uint64_t q = 0; q < nops; q++) {
        cph_span_op op;
        memcpy(&op, p.value.data + q * sizeof op, sizeof op);
        auto bad = [&](const char* name, const char* words) { return fail((std::string("SPAN operation ") + std::to_string(q) + " (" + name + "): " + words).c_str()); };
        const char* name = op.op == CPH_SPAN_TRIM_SPACE    ? "TRIM_SPACE"
                           : op.op == CPH_SPAN_TRIM_CUTSET ? "TRIM_CUTSET"
                           : op.op == CPH_SPAN_TRIM_PREFIX ? "TRIM_PREFIX"
                           : op.op == CPH_SPAN_TRIM_SUFFIX ? "TRIM_SUFFIX"
                           : op.op == CPH_SPAN_FIELD       ? "FIELD"
                           : op.op == CPH_SPAN_SLICE       ? "SLICE"
                                                           : nullptr;
        if (!name) return bad(std::to_string(op.op).c_str(), "unknown span op (1..6)");
        const bool trim = op.op == CPH_SPAN_TRIM_SPACE || op.op == CPH_SPAN_TRIM_CUTSET;
        if (trim && (op.mode < CPH_SPAN_LEFT || op.mode > CPH_SPAN_BOTH)) return bad(name, "unknown mode: 1 (left), 2 (right) or 3 (both)");
        if (op.op == CPH_SPAN_FIELD && (op.mode == 0 || op.mode < -1)) return bad(name, "the limit (mode) is -1 or at least 1");
        if (!trim && op.op != CPH_SPAN_FIELD && op.mode != 0) return bad(name, "unknown mode: 0 for this op");
        if (op.op == CPH_SPAN_TRIM_SPACE || op.op == CPH_SPAN_SLICE) continue;   // no literal
        if (!op.lit.data && op.lit.len) return bad(name, "a literal with bytes but no data pointer");
        if (op.op == CPH_SPAN_TRIM_CUTSET) {
            if (op.lit.len > CPH_SPAN_MAX_CUTSET) return bad(name, "a cutset of more than 32 bytes");
            for (uint64_t c = 0; c < op.lit.len; c++)
                if (op.lit.data[c] >= 0x80) return bad(name, "a cutset byte of 0x80 or above (only an ASCII cutset trims bytewise as Go trims runes)");
            continue;   // travels as a bitmap
        }
        if (op.op == CPH_SPAN_FIELD && op.lit.len == 0) return bad(name, "an empty separator");
        if (op.lit.len > CPH_SPAN_MAX_LITERAL) return bad(name, op.op == CPH_SPAN_FIELD ? "a separator of more than 255 bytes" : "a literal of more than 255 bytes");
        *lit_bytes += op.lit.len;
        if (*lit_bytes > 0xFFFFFFFFull) return bad(name, "literals beyond 4 GiB");
    }
    return {};
}

// The rules for the pieces of one template.  prefix(k) = the text in front of a rule's words for piece k.  Adds the literals'
// bytes to *lit_bytes (all templates of a call together stay below 4 GiB) and notes which piece set the call needs, whether
// it holds a SPAN piece, and in *span_ops the operations of the call's SPAN pieces together.
template <class Prefix>
Status check_map_pieces(const cph_map_piece* pieces, int32_t npieces, int32_t ncols, uint64_t n, Prefix prefix, uint64_t* lit_bytes,
                        bool* has_shortest, bool* has_float, bool* has_slice, bool* has_span, int* span_ops) {
    for (int k = 0; k < npieces; k++) {
        const cph_map_piece& p = pieces[k];
        auto fail = [&](const char* words) { return Status{CPH_ERR_INVALID, prefix(k) + words}; };
        const bool mem_ok = p.arg == CPH_MEM_HOST || p.arg == CPH_MEM_DEVICE;
        switch (p.kind) {
            case CPH_MAP_LITERAL:
                if (!p.value.data && p.value.len) return fail("a literal with bytes but no data pointer");
                *lit_bytes += p.value.len;
                if (p.value.len > 0xFFFFFFFFull || *lit_bytes > 0xFFFFFFFFull) return fail("literals beyond 4 GiB");
                break;
            case CPH_MAP_COLUMN:
                if (p.arg < 0 || p.arg >= ncols) return fail("a COLUMN piece outside 0..ncols-1");
                break;
            case CPH_MAP_INT64:
                if (!mem_ok) return fail("bad memory space of an INT64 piece");
                if (!p.ints && n) return fail("an INT64 piece without values");
                break;
            case CPH_MAP_FLOAT64:
                if (!mem_ok) return fail("bad memory space of a FLOAT64 piece");
                if (!p.floats && n) return fail("a FLOAT64 piece without values");
                if (p.prec < 0 || p.prec > kFixedMaxPrec) return fail("prec of a FLOAT64 piece outside 0..22");
                *has_float = true;
                break;
            case CPH_MAP_FLOAT64_SHORTEST:
                if (!mem_ok) return fail("bad memory space of a FLOAT64_SHORTEST piece");
                if (!p.floats && n) return fail("a FLOAT64_SHORTEST piece without values");
                if (!short_fmt_ok(p.prec)) return fail("prec of a FLOAT64_SHORTEST piece (the format byte) is none of 'e' 'E' 'f' 'g' 'G'");
                *has_shortest = true;
                break;
            case CPH_MAP_TIME:
                if (!mem_ok) return fail("bad memory space of a TIME piece");
                if (!p.ints && n) return fail("a TIME piece without values");
                if (p.prec < -kTimeMaxZone || p.prec > kTimeMaxZone)
                    return fail("prec of a TIME piece (the zone in minutes east of UTC) outside -1439..1439");
                *has_float = true;   // the instantiations that report a refused value
                break;
            case CPH_MAP_SLICE:
                if (p.arg < 0 || p.arg >= ncols) return fail("a SLICE piece's column outside 0..ncols-1");
                if (!p.value.data || p.value.len != sizeof(cph_map_slice))
                    return fail("a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer");
                *has_slice = true;
                break;
            case CPH_MAP_SPAN:
                CPH_TRY(check_span_piece(p, ncols, fail, lit_bytes, span_ops));
                *has_span = true;
                break;
            default:
                return fail("unknown piece kind (1..4, 8, 10)");   // the words are pinned by the message tests; 12 is a kind too
        }
    }
    return {};
}

// What the templates of one call accumulate while their pieces are appended.
struct MapPlanBuild {
    std::string lits;          // the literals of all templates, in piece order: one device block
    uint32_t col_mask = 0;     // bit c: some COLUMN piece reads column c (the copy pass preloads those)
    uint32_t slice_cols = 0;   // bit c: some SLICE or SPAN piece reads column c
    SpanOp* ops = nullptr;     // the plan's CPH_SPAN_MAX_TOTAL operations, for the SPAN pieces
    int nops = 0;              // ... and how many are taken
    double in_bytes = 0;       // what the copy pass reads per row besides the value bytes
};

// Appends one template's (checked) pieces to dst[0 .. npieces) as the kernels see them; a host array of numbers is staged into
// `staged`, like the row ids of a host column.  *lit_bytes = the bytes of this template's literals together.
inline Status append_map_pieces(cph_ctx* ctx, const cph_map_piece* pieces, int32_t npieces, uint64_t n, const ColsArg& arg, const ColIds& ids,
                                MapPlanBuild* b, MapPiece* dst, std::vector<DevBuf>* staged, uint64_t* lit_bytes) {
    uint64_t fixed = 0;   // what the LITERAL pieces give every row (a SPAN operation's literal lies in the block too, and gives nothing)
    auto offsets_and_ids = [&](int c) {   // what reading column c's spans costs per row
        return (arg.c[c].fixed_width ? 0.0 : (double)(arg.c[c].offset_bits / 8)) + (ids.ids[c].ptr ? (double)(ids.ids[c].bits / 8) : 0.0);
    };
    for (int k = 0; k < npieces; k++) {
        const cph_map_piece& p = pieces[k];
        MapPiece& d = dst[k];
        d.kind = p.kind;
        if (p.kind == CPH_MAP_LITERAL) {
            d.off = (uint32_t)b->lits.size();
            d.len = (uint32_t)p.value.len;
            if (d.len) b->lits.append(reinterpret_cast<const char*>(p.value.data), d.len);
            fixed += d.len;
        } else if (p.kind == CPH_MAP_COLUMN) {
            d.col = p.arg;
            if (!((b->col_mask >> p.arg) & 1u)) b->in_bytes += offsets_and_ids(p.arg);
            b->col_mask |= 1u << p.arg;
        } else if (p.kind == CPH_MAP_SLICE) {   // not in col_mask: a slice loads its own first chunk
            cph_map_slice sl;
            memcpy(&sl, p.value.data, sizeof sl);
            d.col = p.arg;
            d.from = sl.from;
            d.to = sl.to;
            if (!(((b->slice_cols | b->col_mask) >> p.arg) & 1u)) b->in_bytes += offsets_and_ids(p.arg);
            b->slice_cols |= 1u << p.arg;
        } else if (p.kind == CPH_MAP_SPAN) {   // its operations behind the plan's, their literals behind the block's; not in col_mask
            d.col = p.arg;
            d.off = (uint32_t)b->nops;
            d.len = (uint32_t)(p.value.len / sizeof(cph_span_op));
            for (uint32_t q = 0; q < d.len; q++) {
                cph_span_op op;
                memcpy(&op, p.value.data + q * sizeof op, sizeof op);
                SpanOp& o = b->ops[b->nops++];
                o = SpanOp{};
                o.op = op.op, o.mode = op.mode, o.a = op.a;
                if (op.op == CPH_SPAN_SLICE) {
                    o.b = op.b;
                } else if (op.op == CPH_SPAN_TRIM_CUTSET) {   // the set as a 128-bit bitmap
                    uint64_t set[2] = {0, 0};
                    for (uint64_t c = 0; c < op.lit.len; c++) set[op.lit.data[c] >> 6] |= 1ull << (op.lit.data[c] & 63);
                    o.a = (int64_t)set[0], o.b = (int64_t)set[1];
                } else if (op.op != CPH_SPAN_TRIM_SPACE) {
                    o.lit_off = (uint32_t)b->lits.size();
                    o.lit_len = (uint32_t)op.lit.len;
                    if (o.lit_len) b->lits.append(reinterpret_cast<const char*>(op.lit.data), o.lit_len);
                }
            }
            if (!(((b->slice_cols | b->col_mask) >> p.arg) & 1u)) b->in_bytes += offsets_and_ids(p.arg);
            b->slice_cols |= 1u << p.arg;
        } else {   // INT64 / FLOAT64 / FLOAT64_SHORTEST / TIME: 8 bytes per row
            const bool is_float = p.kind == CPH_MAP_FLOAT64 || p.kind == CPH_MAP_FLOAT64_SHORTEST;
            const void* vals = is_float ? static_cast<const void*>(p.floats) : static_cast<const void*>(p.ints);
            b->in_bytes += 8.0;
            staged->emplace_back();
            CPH_TRY(device_array(ctx, vals, p.arg, n * sizeof(int64_t), &staged->back(), &vals));
            if (is_float) d.floats = static_cast<const double*>(vals);
            else d.ints = static_cast<const int64_t*>(vals);
            if (p.kind != CPH_MAP_INT64) d.col = p.prec;   // FLOAT64: prec; TIME: the zone; FLOAT64_SHORTEST: the format byte
        }
    }
    *lit_bytes = fixed;
    return {};
}

// The literal block on the device (16 bytes of slack: the kernels read it 8 bytes at a time).
inline Status upload_map_literals(cph_ctx* ctx, const std::string& lits, DevBuf* litbuf) {
    return upload_block(ctx, lits.data(), lits.size(), litbuf, 16);
}

// The row's value of an INT64 / FLOAT64 / TIME piece, from whichever memory space holds it.
template <class T>
Status read_piece_value(const cph_map_piece& p, const T* vals, uint64_t row, T* v) {
    if (p.arg == CPH_MEM_HOST) *v = vals[row];
    else CPH_HIP_TRY(hipMemcpy(v, vals + row, sizeof *v, hipMemcpyDeviceToHost));
    return {};
}

// lens[n] -> offs[n + 1] in place, *total = offs[n].  A float plan's length pass left the lowest refused row in offs[n + 1]
// (UINT64_MAX: none); the total and that row come back in one copy, the call's one host wait.  For a refused row,
// pick(row, &pieces, &npieces, &prefix) names the template the row ran and the text in front of the report.
template <class Pick>
Status scan_with_refusal(cph_ctx* ctx, uint64_t* offs, uint64_t n, bool has_float, Pick pick, uint64_t* total) {
    if (!has_float) return scan_lengths(ctx, offs, n, total);
    CPH_TRY(exclusive_scan_u64(ctx, offs, n, offs + n));
    struct { uint64_t total, bad; } tail;
    CPH_TRY(read_device_value(ctx, reinterpret_cast<const decltype(tail)*>(offs + n), &tail));
    *total = tail.total;
    if (tail.bad == UINT64_MAX) return {};
    const cph_map_piece* pieces = nullptr;
    int32_t npieces = 0;
    std::string prefix;
    CPH_TRY(pick(tail.bad, &pieces, &npieces, &prefix));
    int piece = 0;   // the first FLOAT64 or TIME piece with such a value in that row
    for (int k = 0; k < npieces; k++) {
        if (pieces[k].kind == CPH_MAP_TIME) {
            int64_t t = 0;
            CPH_TRY(read_piece_value(pieces[k], pieces[k].ints, tail.bad, &t));
            if (!rfc3339_in_range(t, pieces[k].prec))
                return Status{CPH_ERR_INVALID, prefix + "TIME piece " + std::to_string(k) + ", row " + std::to_string(tail.bad) + ": the local year of " +
                                                   std::to_string(t) + " is outside 0000..9999"};
        } else if (pieces[k].kind == CPH_MAP_FLOAT64) {
            double v = 0;
            CPH_TRY(read_piece_value(pieces[k], pieces[k].floats, tail.bad, &v));
            if (fixed_split(v, 0).kind == FIXED_RANGE) {
                piece = k;
                break;
            }
        }
    }
    return Status{CPH_ERR_INVALID, prefix + "FLOAT64 piece " + std::to_string(piece) + ", row " + std::to_string(tail.bad) +
                                       ": a finite value of 2^128 or more is not formatted"};
}

// Hands out the result column: n values of `total` bytes behind 64-bit offsets in r->d_offs and r->d_data.  n == 0: the empty
// column is made here.  Whatever else the kernels read goes back to the pool behind deliver's wait.
inline Status deliver_map_column(cph_ctx* ctx, cph_colbuf_impl* r, uint64_t n, uint64_t total, int32_t out_mem) {
    if (n == 0) {
        CPH_TRY(r->d_offs.alloc(&ctx->pool, sizeof(uint64_t)));
        CPH_HIP_TRY(hipMemsetAsync(r->d_offs.get(), 0, sizeof(uint64_t), ctx->stream));
        CPH_TRY(r->d_data.alloc(&ctx->pool, 16));
    }
    r->pub.nbytes = total;
    r->pub.col.nrows = n;
    r->pub.col.offset_bits = 64;
    r->pub.col.mem = out_mem;
    r->pub.col.fixed_width = 0;
    const ResultPart parts[2] = {{&r->d_offs, (size_t)(n + 1) * sizeof(uint64_t), &r->pub.col.offsets}, {&r->d_data, (size_t)total, &r->pub.col.data}};
    return deliver(ctx, &r->own, parts, 2, out_mem);
}

// Launches KERNEL, KERNEL_sl, KERNEL_f64 or KERNEL_g64 for the piece set PK (map_device.hpp: pieces_set) over NROWS rows of NCOLS columns,
// inside a function that returns Status.  The slice kernels have a profile name of their own; the float and shortest
// ones report under the base name.  SP (the plan holds a SPAN piece): KERNEL_sp for a set up to kPiecesSlice, KERNEL_spg
// (every piece kind) above it, both under the profile name KERNEL_sp; without SP the launches are what they were.
#define CPH_MAP_DISPATCH(CTX, KERNEL, PK, SP, BYTES, NCOLS, NROWS, SMEM, ...)                                              \
    do {                                                                                                                   \
        {                                                                                                                  \
            ProfScope ps_(CTX, (SP) ? #KERNEL "_sp" : (PK) == kPiecesSlice ? #KERNEL "_sl" : #KERNEL, BYTES);              \
            if ((SP) && span_pieces_set(PK) == kPiecesShortest) {                                                          \
                CPH_CSV_DISPATCH(KERNEL##_spg, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);           \
            } else if (SP) {                                                                                               \
                CPH_CSV_DISPATCH(KERNEL##_sp, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);            \
            } else if ((PK) == kPiecesShortest) {                                                                                 \
                CPH_CSV_DISPATCH(KERNEL##_g64, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);           \
            } else if ((PK) == kPiecesFloat) {                                                                             \
                CPH_CSV_DISPATCH(KERNEL##_f64, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);           \
            } else if ((PK) == kPiecesSlice) {                                                                             \
                CPH_CSV_DISPATCH(KERNEL##_sl, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);            \
            } else {                                                                                                       \
                CPH_CSV_DISPATCH(KERNEL, NCOLS, dim3(grid_rows(NROWS)), SMEM, (CTX)->stream, __VA_ARGS__);                 \
            }                                                                                                              \
        }                                                                                                                  \
        CPH_HIP_TRY(hipGetLastError());                                                                                    \
    } while (0)

}  // namespace cph
