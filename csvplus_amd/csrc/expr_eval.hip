// expr_eval.hip — numeric expressions per row: the reference's `price * float64(qty)` (csvplus_test.go:516-571, :1391-1421)
// as a typed postfix program over string columns, number arrays and literals, with Go's arithmetic rules
// (include/csvplus_hip.h: cph_num_eval).
//
//   k_expr_eval   the geometry of k_num_parse (numparse.hip): rows on lanes, row = tile + 64 k + lane, 2048-row tiles,
//                 8 rows per lane and tile of which 4 are in flight.  The program is wave-uniform and lives in the kernel
//                 arguments; every lane interprets it over its 4 rows with a stack held in registers (the stack slot is
//                 uniform, so a slot is picked with compares against constants and nothing is indexed dynamically).  A
//                 string leaf is converted on the fly with numparse_device.hpp — span through the row ids, the value's first
//                 16 bytes with two branch-free loads, the SWAR conversion — with its 4 rows' loads issued together; a
//                 number leaf is a coalesced 8-byte load.  Values and status bytes leave as coalesced stores.  A wave that
//                 saw an error adds its count and sends ONE 64-bit atomicMin (the report of num_report.hpp, tag = the op); a
//                 wave that deferred float rows adds their count.
//   The kernel is instantiated for stacks of 2, 4 and 8 values (the host knows the program's depth): the reference's own
//   shape, COL_FLT COL_INT TO_FLT MUL, needs 2.
//
//   k_expr_cmp    a condition over two expressions (CPH_PRED_EXPR_*, a term of cph_filter_rows and cph_map_switch: filter.hip calls
//                 expr_cmp_bitmap): the same interpreter and geometry over a program that leaves TWO values of one type, lhs in slot
//                 0 and rhs in slot 1.  Behind the last op the two are compared (int64 signed, float64 IEEE) under the relation's
//                 outcome mask, and the wave's ballot of `live && status == OK && holds` IS the bitmap word of its 64 rows: the tile
//                 leaves through tile_store_words (tile_bitmap.hpp) as a complete TileBitmap, 1 bit per row instead of 9 bytes.  It
//                 takes first_row, and three index spaces meet in it: a COL leaf reads source_row(rid, first_row + i); a caller's
//                 array belongs to POSITIONS of the selection, so the host hands the kernel its entry first_row as entry 0; a
//                 converted leaf of the plain route is entry i because convert_rows(first_row, n) made it.  Errors are not reported:
//                 a failing row is false.  Deferred rows are counted per lane and summed once per tile (the kernel is short of
//                 SGPRs); a program without a COL_FLT leaf gets no counter and its call no host wait.
//                 The op loop is k_expr_eval's, as a COPY (expr_run_phase): shared as one inline body it moved k_expr_eval<2/4/8>
//                 from 133 / 149 / 181 to 137 / 153 / 193 VGPRs, so k_expr_eval keeps its own text.  Change both together.
//
// The float rows the device defers (numparse.hip) make the call take the plain route: every string leaf goes through
// convert_rows — host finishing included — into a temporary array with its status bytes, and the same kernel runs with
// every leaf as a number array.  Both routes run the same conversion and the same arithmetic code: the bits agree.
//
// This file must never contract a*b+c into a fused multiply-add (Go on amd64 never fuses): the pragma below and the
// Makefile's -ffp-contract=off for this file both say so.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "num_report.hpp"
#include "numparse_device.hpp"
#include "tile_bitmap.hpp"

#pragma clang fp contract(off)

namespace cph {

constexpr int kExprRows  = 8;                           // rows per lane and tile
constexpr int kExprPhase = 4;                           // ... of which this many are in flight at once
constexpr int kExprTile  = kMatThreads * kExprRows;     // 2048 rows

struct ExprOp {          // one op as the kernel sees it
    int32_t op, arg;     // CPH_EXPR_*; COL_*: the column
    uint64_t a;          // LIT_*: the value's bits; NUM_*: the array (on the device)
    const uint8_t* st;   // NUM_*: CPH_NUM_* per row (a converted string leaf), or null (a caller's array: no errors)
};
struct ExprPlan {
    int32_t nops, pad_;
    ExprOp ops[CPH_EXPR_MAX_OPS];
};
struct ExprCounters {    // preset by the host in front of k_expr_eval (ErrReport)
    ErrWord err;         // first
    unsigned long long ndeferred;
};

template <int D>
__device__ __forceinline__ uint64_t stack_get(const uint64_t (&s)[D][kExprPhase], int slot, int k) {
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < D; j++)
        if (j == slot) v = s[j][k];
    return v;
}
template <int D>
__device__ __forceinline__ void stack_set(uint64_t (&s)[D][kExprPhase], int slot, int k, uint64_t v) {
#pragma unroll
    for (int j = 0; j < D; j++)
        if (j == slot) s[j][k] = v;
}

__device__ __forceinline__ double as_f64(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ uint64_t f64_bits(double v) { return (uint64_t)__double_as_longlong(v); }

// a OP b on int64 with Go's rules; returns CPH_NUM_OK or CPH_NUM_ERR_DIV_ZERO
__device__ __forceinline__ uint32_t int_binary(int32_t op, uint64_t a, uint64_t b, uint64_t* out) {
    switch (op) {
        case CPH_EXPR_ADD: *out = a + b; return CPH_NUM_OK;
        case CPH_EXPR_SUB: *out = a - b; return CPH_NUM_OK;
        case CPH_EXPR_MUL: *out = a * b; return CPH_NUM_OK;
        default: break;
    }
    *out = 0;
    if (b == 0) return CPH_NUM_ERR_DIV_ZERO;
    if (b == ~0ull) {   // a / -1 wraps (INT64_MIN stays), a % -1 is 0: the hardware-free form of Go's rule
        if (op == CPH_EXPR_DIV) *out = 0ull - a;
        return CPH_NUM_OK;
    }
    const int64_t x = (int64_t)a, y = (int64_t)b;
    *out = (uint64_t)(op == CPH_EXPR_DIV ? x / y : x % y);   // C++ and Go agree: toward zero, the dividend's sign
    return CPH_NUM_OK;
}

// one correctly rounded IEEE operation (the file is compiled without contraction)
__device__ __forceinline__ double flt_binary(int32_t op, double a, double b) {
    switch (op) {
        case CPH_EXPR_ADD: return a + b;
        case CPH_EXPR_SUB: return a - b;
        case CPH_EXPR_MUL: return a * b;
        default: return a / b;
    }
}

template <int D>
__global__ __launch_bounds__(kMatThreads) void k_expr_eval(ColsArg cols, ColIds ids, ExprPlan plan, uint64_t n, uint64_t* __restrict__ values,
                                                          uint8_t* __restrict__ status, ExprCounters* cnt) {
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = (n + kExprTile - 1) / kExprTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kExprTile;
        WaveErr we;          // wave-uniform: the wave's errors in this tile
        uint32_t ndef = 0;   // wave-uniform
#pragma unroll 1
        for (int ph = 0; ph < kExprRows / kExprPhase; ph++) {
            uint64_t row[kExprPhase];       // rows past the end look at the last row; their result is dropped
            bool live[kExprPhase];
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t i = t0 + (uint64_t)((wave * kExprRows + ph * kExprPhase + k) * 64 + lane);
                live[k] = i < n;
                row[k] = live[k] ? i : n - 1;
            }
            uint64_t stk[D][kExprPhase];
            uint32_t rst[kExprPhase], rop[kExprPhase];   // the row's status and the op that set it
            bool deferred[kExprPhase];
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                rst[k] = CPH_NUM_OK, rop[k] = 0, deferred[k] = false;
#pragma unroll
                for (int j = 0; j < D; j++) stk[j][k] = 0;
            }
            int sp = 0;   // uniform
            for (int q = 0; q < plan.nops; q++) {
                const int32_t op = plan.ops[q].op;
                uint64_t r[kExprPhase];
                uint32_t e[kExprPhase];
                int slot = sp;   // where the result goes
                if (op == CPH_EXPR_COL_INT || op == CPH_EXPR_COL_FLT) {
                    const DevCol& col = cols.c[plan.ops[q].arg];
                    const RowIds& rid = ids.ids[plan.ops[q].arg];
                    uint64_t b[kExprPhase], l[kExprPhase], c0[kExprPhase], c1[kExprPhase];
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) value_span(col, source_row(rid, row[k]), &b[k], &l[k]);
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) load_head16(col, b[k], l[k], &c0[k], &c1[k]);
                    if (op == CPH_EXPR_COL_FLT) {
#pragma unroll
                        for (int k = 0; k < kExprPhase; k++) {
                            double v;
                            e[k] = parse_float64(col, b[k], l[k], c0[k], c1[k], &v);
                            r[k] = f64_bits(v);
                            if (e[k] == kNumDeferred) deferred[k] = true, e[k] = CPH_NUM_OK;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < kExprPhase; k++) {
                            int64_t v;
                            e[k] = parse_int64(col, b[k], l[k], c0[k], c1[k], &v);
                            r[k] = (uint64_t)v;
                        }
                    }
                    sp++;
                } else if (op == CPH_EXPR_NUM_INT || op == CPH_EXPR_NUM_FLT) {
                    const uint64_t* vals = reinterpret_cast<const uint64_t*>((uintptr_t)plan.ops[q].a);
                    const uint8_t* st = plan.ops[q].st;
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) {
                        r[k] = vals[row[k]];
                        e[k] = st ? (uint32_t)st[row[k]] : (uint32_t)CPH_NUM_OK;
                    }
                    sp++;
                } else if (op == CPH_EXPR_LIT_INT || op == CPH_EXPR_LIT_FLT) {
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) r[k] = plan.ops[q].a, e[k] = CPH_NUM_OK;
                    sp++;
                } else if (op == CPH_EXPR_TO_FLT || op == CPH_EXPR_TO_INT || op == CPH_EXPR_NEG) {
                    slot = sp - 1;
                    const bool flt = plan.ops[q].arg != 0;   // NEG: the host wrote the operand's type here
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) {
                        const uint64_t x = stack_get<D>(stk, slot, k);
                        e[k] = CPH_NUM_OK;
                        if (op == CPH_EXPR_TO_FLT) {
                            r[k] = f64_bits((double)(int64_t)x);
                        } else if (op == CPH_EXPR_TO_INT) {
                            const double v = as_f64(x);
                            const bool fits = v >= -9223372036854775808.0 && v < 9223372036854775808.0;   // false for a NaN
                            r[k] = fits ? (uint64_t)(int64_t)v : 0ull;
                            if (!fits) e[k] = CPH_NUM_ERR_CONVERT;
                        } else {
                            r[k] = flt ? x ^ 0x8000000000000000ull : 0ull - x;
                        }
                    }
                } else {   // ADD SUB MUL DIV MOD: arg = 1 for float64 operands
                    slot = sp - 2;
                    const bool flt = plan.ops[q].arg != 0;
#pragma unroll
                    for (int k = 0; k < kExprPhase; k++) {
                        const uint64_t x = stack_get<D>(stk, slot, k), y = stack_get<D>(stk, slot + 1, k);
                        if (flt) {
                            r[k] = f64_bits(flt_binary(op, as_f64(x), as_f64(y)));
                            e[k] = CPH_NUM_OK;
                        } else {
                            e[k] = int_binary(op, x, y, &r[k]);
                        }
                    }
                    sp--;
                }
#pragma unroll
                for (int k = 0; k < kExprPhase; k++) {
                    stack_set<D>(stk, slot, k, r[k]);
                    if (e[k] != CPH_NUM_OK && rst[k] == CPH_NUM_OK) rst[k] = e[k], rop[k] = (uint32_t)q;   // the first failing op decides
                }
            }
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t g0 = t0 + (uint64_t)((wave * kExprRows + ph * kExprPhase + k) * 64);
                if (live[k]) {
                    values[g0 + lane] = rst[k] == CPH_NUM_OK ? stk[0][k] : 0ull;
                    status[g0 + lane] = (uint8_t)rst[k];
                }
                we.note_ballot(__ballot(live[k] && rst[k] != CPH_NUM_OK), g0, err_tag_kind(rop[k], rst[k]));
                ndef += (uint32_t)__popcll(__ballot(live[k] && deferred[k]));
            }
        }
        we.flush(&cnt->err);
        if (lane == 0 && ndef) atomicAdd(&cnt->ndeferred, (unsigned long long)ndef);
    }
}

// The program over the 4 rows of one phase, for k_expr_cmp: k_expr_eval's op loop with two row indices.  It is a COPY: with the loop
// shared as one inline body k_expr_eval<2/4/8> grew by 4, 4 and 12 VGPRs (profiles/expr_conditions.txt), so that kernel keeps its
// own text and stays the kernel it was.  Change both together.  crow[k] = the row's position in the selection (a COL leaf reads
// source_row(rid, crow[k])), arow[k] = its entry in the number arrays.  Leaves the values in stk (slot 0, and slot 1
// of a two-value program), the row's status and the op that set it in rst / rop, and the rows with a deferred float leaf.
template <int D>
__device__ __forceinline__ void expr_run_phase(const ColsArg& cols, const ColIds& ids, const ExprPlan& plan, const uint64_t (&crow)[kExprPhase],
                                               const uint64_t (&arow)[kExprPhase], uint64_t (&stk)[D][kExprPhase], uint32_t (&rst)[kExprPhase],
                                               uint32_t (&rop)[kExprPhase], bool (&deferred)[kExprPhase]) {
#pragma unroll
    for (int k = 0; k < kExprPhase; k++) {
        rst[k] = CPH_NUM_OK, rop[k] = 0, deferred[k] = false;
#pragma unroll
        for (int j = 0; j < D; j++) stk[j][k] = 0;
    }
    int sp = 0;   // uniform
    for (int q = 0; q < plan.nops; q++) {
        const int32_t op = plan.ops[q].op;
        uint64_t r[kExprPhase];
        uint32_t e[kExprPhase];
        int slot = sp;   // where the result goes
        if (op == CPH_EXPR_COL_INT || op == CPH_EXPR_COL_FLT) {
            const DevCol& col = cols.c[plan.ops[q].arg];
            const RowIds& rid = ids.ids[plan.ops[q].arg];
            uint64_t b[kExprPhase], l[kExprPhase], c0[kExprPhase], c1[kExprPhase];
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) value_span(col, source_row(rid, crow[k]), &b[k], &l[k]);
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) load_head16(col, b[k], l[k], &c0[k], &c1[k]);
            if (op == CPH_EXPR_COL_FLT) {
#pragma unroll
                for (int k = 0; k < kExprPhase; k++) {
                    double v;
                    e[k] = parse_float64(col, b[k], l[k], c0[k], c1[k], &v);
                    r[k] = f64_bits(v);
                    if (e[k] == kNumDeferred) deferred[k] = true, e[k] = CPH_NUM_OK;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kExprPhase; k++) {
                    int64_t v;
                    e[k] = parse_int64(col, b[k], l[k], c0[k], c1[k], &v);
                    r[k] = (uint64_t)v;
                }
            }
            sp++;
        } else if (op == CPH_EXPR_NUM_INT || op == CPH_EXPR_NUM_FLT) {
            const uint64_t* vals = reinterpret_cast<const uint64_t*>((uintptr_t)plan.ops[q].a);
            const uint8_t* st = plan.ops[q].st;
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                r[k] = vals[arow[k]];
                e[k] = st ? (uint32_t)st[arow[k]] : (uint32_t)CPH_NUM_OK;
            }
            sp++;
        } else if (op == CPH_EXPR_LIT_INT || op == CPH_EXPR_LIT_FLT) {
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) r[k] = plan.ops[q].a, e[k] = CPH_NUM_OK;
            sp++;
        } else if (op == CPH_EXPR_TO_FLT || op == CPH_EXPR_TO_INT || op == CPH_EXPR_NEG) {
            slot = sp - 1;
            const bool flt = plan.ops[q].arg != 0;   // NEG: the host wrote the operand's type here
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t x = stack_get<D>(stk, slot, k);
                e[k] = CPH_NUM_OK;
                if (op == CPH_EXPR_TO_FLT) {
                    r[k] = f64_bits((double)(int64_t)x);
                } else if (op == CPH_EXPR_TO_INT) {
                    const double v = as_f64(x);
                    const bool fits = v >= -9223372036854775808.0 && v < 9223372036854775808.0;   // false for a NaN
                    r[k] = fits ? (uint64_t)(int64_t)v : 0ull;
                    if (!fits) e[k] = CPH_NUM_ERR_CONVERT;
                } else {
                    r[k] = flt ? x ^ 0x8000000000000000ull : 0ull - x;
                }
            }
        } else {   // ADD SUB MUL DIV MOD: arg = 1 for float64 operands
            slot = sp - 2;
            const bool flt = plan.ops[q].arg != 0;
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t x = stack_get<D>(stk, slot, k), y = stack_get<D>(stk, slot + 1, k);
                if (flt) {
                    r[k] = f64_bits(flt_binary(op, as_f64(x), as_f64(y)));
                    e[k] = CPH_NUM_OK;
                } else {
                    e[k] = int_binary(op, x, y, &r[k]);
                }
            }
            sp--;
        }
#pragma unroll
        for (int k = 0; k < kExprPhase; k++) {
            stack_set<D>(stk, slot, k, r[k]);
            if (e[k] != CPH_NUM_OK && rst[k] == CPH_NUM_OK) rst[k] = e[k], rop[k] = (uint32_t)q;   // the first failing op decides
        }
    }
}

// Two values per row compared: one bit per row in the layout of tile_bitmap.hpp (an expression tile IS a bitmap tile: a wave's 8
// phases-times-rows are its 8 words).  rel_flt: the kCmp* outcomes under which the relation holds | kCmpIsFloat for float64 values.
// Row i of the call is position first_row + i of the selection for a COL leaf and entry i of every number array (the host has
// moved a caller's array to its entry first_row; a converted leaf starts at the call's first row anyway).  A row with a failing op
// is false under every relation.  ndeferred may be null (a program without a COL_FLT leaf).
constexpr uint32_t kCmpIsFloat = 16;   // rel_flt: beside the kCmp* outcomes under which the relation holds
static_assert(kExprTile == kTileRows && kExprRows == kTileWaveWords, "k_expr_cmp: an expression tile is a bitmap tile");
template <int D>
__global__ __launch_bounds__(kMatThreads) void k_expr_cmp(ColsArg cols, ColIds ids, ExprPlan plan, uint64_t first_row, uint64_t n, uint32_t rel_flt,
                                                         uint64_t* __restrict__ bitmap, uint32_t* __restrict__ counts,
                                                         unsigned long long* ndeferred) {
    static_assert(D >= 2, "two values are left");
    __shared__ uint64_t s_words[kTileWords];
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = tile_count(n);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kExprTile;
        uint64_t myword = 0;   // lane w < 8: word w of this wave
        uint32_t ndef = 0;     // per lane: its rows with a deferred leaf (summed once per tile: the kernel is short of SGPRs, not VGPRs)
#pragma unroll 1
        for (int ph = 0; ph < kExprRows / kExprPhase; ph++) {
            uint64_t crow[kExprPhase], arow[kExprPhase];   // rows past the end look at the last row; their bit is 0
            bool live[kExprPhase];
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t i = t0 + (uint64_t)((wave * kExprRows + ph * kExprPhase + k) * 64 + lane);
                live[k] = i < n;
                arow[k] = live[k] ? i : n - 1;
                crow[k] = first_row + arow[k];
            }
            uint64_t stk[D][kExprPhase];
            uint32_t rst[kExprPhase], rop[kExprPhase];
            bool deferred[kExprPhase];
            expr_run_phase<D>(cols, ids, plan, crow, arow, stk, rst, rop, deferred);
#pragma unroll
            for (int k = 0; k < kExprPhase; k++) {
                const uint64_t x = stk[0][k], y = stk[1][k];
                uint32_t cls;
                if (rel_flt & kCmpIsFloat) {
                    const double a = as_f64(x), b = as_f64(y);
                    cls = a < b ? kCmpLess : a == b ? kCmpEqual : a > b ? kCmpGreater : kCmpUnordered;
                } else {
                    cls = (int64_t)x < (int64_t)y ? kCmpLess : x == y ? kCmpEqual : kCmpGreater;
                }
                const uint64_t word = __ballot(live[k] && rst[k] == CPH_NUM_OK && (rel_flt & cls) != 0);
                if (lane == ph * kExprPhase + k) myword = word;
                ndef += (uint32_t)(live[k] && deferred[k]);
            }
        }
        if (lane < kTileWaveWords) s_words[wave * kTileWaveWords + lane] = myword;
        tile_store_words(s_words, tile, bitmap, counts);
        if (ndeferred) {
            const uint32_t total = wave_sum(ndef);
            if (lane == 0 && total) atomicAdd(ndeferred, (unsigned long long)total);
        }
    }
}

namespace {


bool is_leaf(int32_t op) { return op >= CPH_EXPR_COL_INT && op <= CPH_EXPR_LIT_FLT; }

// Go's typing, checked before anything is launched.  kinds[q] = the type op q pushes (CPH_NUM_*), *depth = the deepest stack.
// who: what the messages begin with; want: the values the program must leave (cph_num_eval: 1; an expression term: 2, of one type)
Status check_program(const cph_expr_op* prog, int32_t nops, int32_t ncols, int32_t nnums, int32_t* kinds, int32_t* depth, int32_t* result,
                     const std::string& who = "cph_num_eval: ", int want = 1) {
    int32_t stack[CPH_EXPR_MAX_STACK];
    int sp = 0;
    *depth = 0;
    for (int q = 0; q < nops; q++) {
        const int32_t op = prog[q].op;
        const std::string where = who + "op " + std::to_string(q) + ": ";
        int32_t push = 0;
        switch (op) {
            case CPH_EXPR_COL_INT:
            case CPH_EXPR_COL_FLT:
                if (prog[q].arg < 0 || prog[q].arg >= ncols) return {CPH_ERR_INVALID, where + "a column outside 0..ncols-1"};
                push = op == CPH_EXPR_COL_INT ? CPH_NUM_INT64 : CPH_NUM_FLOAT64;
                break;
            case CPH_EXPR_NUM_INT:
            case CPH_EXPR_NUM_FLT:
                if (prog[q].arg < 0 || prog[q].arg >= nnums) return {CPH_ERR_INVALID, where + "a number array outside 0..nnums-1"};
                push = op == CPH_EXPR_NUM_INT ? CPH_NUM_INT64 : CPH_NUM_FLOAT64;
                break;
            case CPH_EXPR_LIT_INT: push = CPH_NUM_INT64; break;
            case CPH_EXPR_LIT_FLT: push = CPH_NUM_FLOAT64; break;
            case CPH_EXPR_TO_FLT:
            case CPH_EXPR_TO_INT:
            case CPH_EXPR_NEG:
                if (sp < 1) return {CPH_ERR_INVALID, where + "no operand on the stack"};
                if (op == CPH_EXPR_TO_FLT && stack[sp - 1] != CPH_NUM_INT64) return {CPH_ERR_INVALID, where + "TO_FLT takes an int64"};
                if (op == CPH_EXPR_TO_INT && stack[sp - 1] != CPH_NUM_FLOAT64) return {CPH_ERR_INVALID, where + "TO_INT takes a float64"};
                push = op == CPH_EXPR_TO_FLT ? CPH_NUM_FLOAT64 : op == CPH_EXPR_TO_INT ? CPH_NUM_INT64 : stack[sp - 1];
                sp -= 1;
                break;
            case CPH_EXPR_ADD:
            case CPH_EXPR_SUB:
            case CPH_EXPR_MUL:
            case CPH_EXPR_DIV:
            case CPH_EXPR_MOD:
                if (sp < 2) return {CPH_ERR_INVALID, where + "a binary op needs two operands on the stack"};
                if (stack[sp - 1] != stack[sp - 2])
                    return {CPH_ERR_INVALID, where + "mismatched operand types (int64 and float64): there are no implicit conversions"};
                if (op == CPH_EXPR_MOD && stack[sp - 1] != CPH_NUM_INT64) return {CPH_ERR_INVALID, where + "MOD takes int64 operands"};
                push = stack[sp - 1];
                sp -= 2;
                break;
            default:
                return {CPH_ERR_INVALID, where + "unknown op (1..6, 8..15)"};
        }
        if (sp >= CPH_EXPR_MAX_STACK) return {CPH_ERR_INVALID, where + "a stack deeper than CPH_EXPR_MAX_STACK"};
        stack[sp++] = push;
        kinds[q] = push;
        if (sp > *depth) *depth = sp;
    }
    if (sp != want) return {CPH_ERR_INVALID, who + "the program leaves " + std::to_string(sp) + " values, not exactly " + (want == 1 ? "one" : "two")};
    if (want == 2 && stack[0] != stack[1])
        return {CPH_ERR_INVALID, who + "mismatched operand types (int64 and float64) on the two sides: there are no implicit conversions"};
    *result = stack[0];
    return {};
}

// The kernel's plan of a checked program: dnums[k] = number array k on the device.  *in_row: the byte model per row — per string leaf
// offsets (or nothing for a fixed width) + row ids + ~8 value bytes, 8 per array leaf.
void build_plan(const cph_expr_op* prog, int32_t nops, const int32_t* kinds, const void* const* dnums, const ColsArg& arg, const ColIds& ids,
                ExprPlan* plan, double* in_row, bool* has_col, bool* has_flt) {
    plan->nops = nops;
    uint32_t col_seen = 0;
    for (int q = 0; q < nops; q++) {
        ExprOp& d = plan->ops[q];
        d.op = prog[q].op;
        d.arg = 0;
        switch (prog[q].op) {
            case CPH_EXPR_COL_INT:
            case CPH_EXPR_COL_FLT: {
                d.arg = prog[q].arg;
                *has_col = true;
                if (d.op == CPH_EXPR_COL_FLT) *has_flt = true;
                const DevCol& c = arg.c[d.arg];
                if (!((col_seen >> d.arg) & 1u)) *in_row += c.fixed_width ? 0.0 : (double)(c.offset_bits / 8);
                if (!((col_seen >> d.arg) & 1u) && ids.ids[d.arg].ptr) *in_row += (double)(ids.ids[d.arg].bits / 8);
                col_seen |= 1u << d.arg;
                *in_row += c.fixed_width ? (double)c.fixed_width : 8.0;
                break;
            }
            case CPH_EXPR_NUM_INT:
            case CPH_EXPR_NUM_FLT:
                d.a = (uint64_t)(uintptr_t)dnums[prog[q].arg];
                *in_row += 8.0;
                break;
            case CPH_EXPR_LIT_INT:
            case CPH_EXPR_LIT_FLT:
                memcpy(&d.a, &prog[q].lit, 8);
                break;
            case CPH_EXPR_TO_FLT:
            case CPH_EXPR_TO_INT:
                break;
            default:   // NEG and the binary ops: the operands' type
                d.arg = kinds[q] == CPH_NUM_FLOAT64 ? 1 : 0;
                break;
        }
    }
}

// The plain route: every string leaf of the plan converted as cph_col_to_number converts it — rows [first_row, first_row + n), one
// array per column and type in converted[4 c + 2 f (+ 1: its status)] — and turned into a number leaf that carries its status bytes.
Status plan_over_arrays(cph_ctx* ctx, const ColsArg& arg, const ColIds& ids, uint64_t first_row, uint64_t n, ExprPlan* plan,
                        std::vector<DevBuf>* converted, double* row_bytes, uint64_t* host_rows) {
    bool have[CPH_MAX_KEY_COLS][2] = {};
    for (int q = 0; q < plan->nops; q++) {
        ExprOp& d = plan->ops[q];
        if (d.op != CPH_EXPR_COL_INT && d.op != CPH_EXPR_COL_FLT) {
            if (d.op == CPH_EXPR_NUM_INT || d.op == CPH_EXPR_NUM_FLT) *row_bytes += 8.0;
            continue;
        }
        const int c = d.arg, f = d.op == CPH_EXPR_COL_FLT ? 1 : 0;
        DevBuf& cv = (*converted)[(size_t)(4 * c + 2 * f)];
        DevBuf& cs = (*converted)[(size_t)(4 * c + 2 * f + 1)];
        if (!have[c][f]) {
            NumColStats st;
            CPH_TRY(convert_rows(ctx, arg.c[c], ids.ids[c], first_row, n, f ? CPH_NUM_FLOAT64 : CPH_NUM_INT64, &cv, &cs, &st));
            have[c][f] = true;
            *host_rows += st.host_rows;
        }
        d.op = f ? CPH_EXPR_NUM_FLT : CPH_EXPR_NUM_INT;
        d.arg = 0;
        d.a = (uint64_t)(uintptr_t)cv.get();
        d.st = cs.as<uint8_t>();
        *row_bytes += 9.0;
    }
    return {};
}

Status launch_eval(cph_ctx* ctx, const ColsArg& arg, const ColIds& ids, const ExprPlan& plan, int depth, uint64_t n, double bytes, DevBuf* values,
                   DevBuf* status, ErrFirst* err, ExprCounters* got) {
    ErrReport<ExprCounters> cnt;
    CPH_TRY(cnt.init(ctx));
    const dim3 grid(tile_grid((n + kExprTile - 1) / kExprTile));
    {
        ProfScope ps(ctx, "k_expr_eval", bytes);
        if (depth <= 2)
            hipLaunchKernelGGL(k_expr_eval<2>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, n, values->as<uint64_t>(),
                               status->as<uint8_t>(), cnt.counters());
        else if (depth <= 4)
            hipLaunchKernelGGL(k_expr_eval<4>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, n, values->as<uint64_t>(),
                               status->as<uint8_t>(), cnt.counters());
        else
            hipLaunchKernelGGL(k_expr_eval<CPH_EXPR_MAX_STACK>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, n,
                               values->as<uint64_t>(), status->as<uint8_t>(), cnt.counters());
    }
    CPH_HIP_TRY(hipGetLastError());
    return cnt.read(ctx, err, got);   // the call's host wait
}

const char* const kTermWho = "cph_filter_rows: expression term: ";

}  // namespace

// ---- an expression term of cph_filter_rows / cph_map_switch (CPH_PRED_EXPR_*): filter.hip calls these two ----------------------

Status check_pred_expr(const cph_strval& value, int32_t ncols) {
    const std::string who = kTermWho;
    if (!value.data || value.len != sizeof(cph_pred_expr))
        return {CPH_ERR_INVALID, who + "value is exactly one cph_pred_expr (" + std::to_string(sizeof(cph_pred_expr)) + " bytes) behind a non-NULL pointer"};
    cph_pred_expr e;
    memcpy(&e, value.data, sizeof e);
    if (!e.prog) return {CPH_ERR_INVALID, who + "prog must not be NULL"};
    if (e.nops < 2 || e.nops > CPH_EXPR_MAX_OPS) return {CPH_ERR_INVALID, who + "2..CPH_EXPR_MAX_OPS (32) ops for both sides together"};
    if (e.nnums < 0 || e.nnums > CPH_EXPR_MAX_NUMS) return {CPH_ERR_INVALID, who + "0..CPH_EXPR_MAX_NUMS (8) number arrays"};
    if (e.nnums && !e.nums) return {CPH_ERR_INVALID, who + "nums must not be NULL"};
    for (int k = 0; k < e.nnums; k++)
        if (e.nums[k].mem != CPH_MEM_HOST && e.nums[k].mem != CPH_MEM_DEVICE)
            return {CPH_ERR_INVALID, who + "bad memory space of number array " + std::to_string(k)};
    int32_t kinds[CPH_EXPR_MAX_OPS], depth = 0, result = 0;
    return check_program(e.prog, e.nops, ncols, e.nnums, kinds, &depth, &result, who, 2);
}

Status expr_cmp_bitmap(cph_ctx* ctx, const ColsArg& arg, const ColIds& ids, const cph_strval& value, uint32_t rel, uint64_t first_row, uint64_t n,
                       TileBitmap* out, std::vector<DevBuf>* hold) {
    cph_pred_expr e;
    memcpy(&e, value.data, sizeof e);
    int32_t kinds[CPH_EXPR_MAX_OPS], depth = 0, result = 0;
    CPH_TRY(check_program(e.prog, e.nops, CPH_MAX_KEY_COLS, e.nnums, kinds, &depth, &result, kTermWho, 2));
    // a caller's array: entry p belongs to position p of the selection, so entry first_row is the call's row 0 (a host array
    // travels from there on)
    const void* dnums[CPH_EXPR_MAX_NUMS] = {};
    for (int k = 0; k < e.nnums; k++) {
        bool used = false;
        for (int q = 0; q < e.nops; q++) used = used || ((e.prog[q].op == CPH_EXPR_NUM_INT || e.prog[q].op == CPH_EXPR_NUM_FLT) && e.prog[q].arg == k);
        if (!used) continue;
        if (!e.nums[k].ptr) return {CPH_ERR_INVALID, std::string(kTermWho) + "number array " + std::to_string(k) + " without values"};
        hold->emplace_back();
        CPH_TRY(device_array(ctx, static_cast<const void*>(static_cast<const uint8_t*>(e.nums[k].ptr) + first_row * 8), e.nums[k].mem, (size_t)n * 8,
                             &hold->back(), &dnums[k]));
    }
    ExprPlan plan{};
    double in_row = 0;
    bool has_col = false, has_flt = false;
    build_plan(e.prog, e.nops, kinds, dnums, arg, ids, &plan, &in_row, &has_col, &has_flt);
    CPH_TRY(out->alloc(ctx, n));
    const uint32_t rel_flt = rel | (result == CPH_NUM_FLOAT64 ? kCmpIsFloat : 0u);
    const double out_bytes = (double)n / 8.0 + 4.0 * (double)out->ntiles;
    auto launch = [&](double row_bytes, unsigned long long* ndeferred) -> Status {
        const dim3 grid(tile_grid(out->ntiles));
        ProfScope ps(ctx, "k_expr_cmp", row_bytes * (double)n + out_bytes);
        if (depth <= 2)
            hipLaunchKernelGGL(k_expr_cmp<2>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, first_row, n, rel_flt, out->words(), out->counts(),
                               ndeferred);
        else if (depth <= 4)
            hipLaunchKernelGGL(k_expr_cmp<4>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, first_row, n, rel_flt, out->words(), out->counts(),
                               ndeferred);
        else
            hipLaunchKernelGGL(k_expr_cmp<CPH_EXPR_MAX_STACK>, grid, dim3(kMatThreads), 0, ctx->stream, arg, ids, plan, first_row, n, rel_flt, out->words(),
                               out->counts(), ndeferred);
        return {};
    };
    if (!has_flt) {   // nothing can be deferred: no counter, no wait
        CPH_TRY(launch(in_row, nullptr));
        CPH_HIP_TRY(hipGetLastError());
        return {};
    }
    DevBuf cnt;
    CPH_TRY(upload_block(ctx, 0ull, &cnt));
    CPH_TRY(launch(in_row, cnt.as<unsigned long long>()));
    CPH_HIP_TRY(hipGetLastError());
    unsigned long long ndeferred = 0;
    CPH_TRY(read_device_value(ctx, cnt.as<unsigned long long>(), &ndeferred));   // the term's host wait
    if (!ndeferred) return {};
    // the plain route of cph_num_eval: every string leaf converted first (rows first_row .. of the selection -> entries 0 ..), the
    // same kernel over number arrays with status bytes
    const size_t base = hold->size();
    hold->resize(base + 2 * 2 * CPH_MAX_KEY_COLS);
    std::vector<DevBuf> converted(2 * 2 * CPH_MAX_KEY_COLS);
    double row2 = 0;
    uint64_t host_rows = 0;
    CPH_TRY(plan_over_arrays(ctx, arg, ids, first_row, n, &plan, &converted, &row2, &host_rows));
    for (size_t k = 0; k < converted.size(); k++) (*hold)[base + k] = std::move(converted[k]);   // the kernel reads them
    CPH_TRY(launch(row2, nullptr));
    CPH_HIP_TRY(hipGetLastError());
    return {};
}

}  // namespace cph

using namespace cph;

extern "C" {

CPH_API int32_t cph_num_eval(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                             const cph_expr_nums* nums, int32_t nnums, const cph_expr_op* prog, int32_t nops, int32_t out_mem,
                             cph_numcol** out, int32_t* first_error_op) {
    if (!ctx) return CPH_ERR_INVALID;
    if (!out) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: out must not be NULL"});
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (first_error_op) *first_error_op = -1;
    if (!prog) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: prog must not be NULL"});
    if (nops < 1 || nops > CPH_EXPR_MAX_OPS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: 1..CPH_EXPR_MAX_OPS (32) ops"});
    if (ncols < 0 || ncols > CPH_MAX_KEY_COLS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: 0..16 columns"});
    if (ncols && !cols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: cols must not be NULL"});
    if (nnums < 0 || nnums > CPH_EXPR_MAX_NUMS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: 0..CPH_EXPR_MAX_NUMS (8) number arrays"});
    if (nnums && !nums) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: nums must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: bad out_mem"});
    for (int k = 0; k < nnums; k++) {
        if (nums[k].mem != CPH_MEM_HOST && nums[k].mem != CPH_MEM_DEVICE)
            return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: bad memory space of number array " + std::to_string(k)});
        if (!nums[k].ptr && nrows) return fail_with(ctx, {CPH_ERR_INVALID, "cph_num_eval: number array " + std::to_string(k) + " without values"});
    }
    int32_t kinds[CPH_EXPR_MAX_OPS], depth = 0, result = 0;
    {
        Status s = check_program(prog, nops, ncols, nnums, kinds, &depth, &result);
        if (!s.ok()) return fail_with(ctx, s);
        s = check_row_sources(cols, sel, ncols, 0, nrows, true);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_numcol_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.nrows = nrows;
    r->pub.kind = result;
    r->pub.mem = out_mem;
    r->pub.first_error_row = UINT64_MAX;
    const uint64_t n = nrows;
    auto run = [&]() -> Status {
        if (n == 0) return {};
        std::vector<DevBuf> staged;
        std::vector<DevBuf> converted(2 * 2 * CPH_MAX_KEY_COLS);   // the plain route: values and status per (column, type)
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, nullptr, ncols, 0, n, &staged, &arg, &ids));
        const void* dnums[CPH_EXPR_MAX_NUMS] = {};
        for (int k = 0; k < nnums; k++) {
            dnums[k] = nums[k].ptr;
            bool used = false;
            for (int q = 0; q < nops; q++) used = used || ((prog[q].op == CPH_EXPR_NUM_INT || prog[q].op == CPH_EXPR_NUM_FLT) && prog[q].arg == k);
            if (!used) continue;
            staged.emplace_back();   // staged like the row ids of a host column
            CPH_TRY(device_array(ctx, nums[k].ptr, nums[k].mem, (size_t)n * 8, &staged.back(), &dnums[k]));
        }
        ExprPlan plan{};
        double in_row = 0;
        bool has_col = false, has_flt = false;
        build_plan(prog, nops, kinds, dnums, arg, ids, &plan, &in_row, &has_col, &has_flt);
        CPH_TRY(r->d_values.alloc(&ctx->pool, (size_t)n * 8));
        CPH_TRY(r->d_status.alloc(&ctx->pool, (size_t)n));
        ExprCounters got{};
        ErrFirst err;
        CPH_TRY(launch_eval(ctx, arg, ids, plan, depth, n, (in_row + 9.0) * (double)n, &r->d_values, &r->d_status, &err, &got));
        r->pub.host_rows = got.ndeferred;
        if (got.ndeferred && has_col) {
            // the plain route: every string leaf converted as cph_col_to_number converts it (one array per column and type),
            // then the same program over number arrays that carry their status bytes
            double row2 = 0;
            uint64_t host_rows = 0;   // "float_device": the values the leaves' conversions finished on the host
            CPH_TRY(plan_over_arrays(ctx, arg, ids, 0, n, &plan, &converted, &row2, &host_rows));
            CPH_TRY(launch_eval(ctx, arg, ids, plan, depth, n, (row2 + 9.0) * (double)n, &r->d_values, &r->d_status, &err, &got));
            if (ctx->float_device) r->pub.host_rows = host_rows;
        }
        r->pub.nerrors = err.nerrors;
        if (err.nerrors) {
            r->pub.first_error_row = err.row;
            r->pub.first_error_kind = err.kind;
            if (first_error_op) *first_error_op = err.tag;
        }
        // the kernels read the staged arrays: they go back to the pool behind deliver's wait
        const ResultPart parts[2] = {{&r->d_values, (size_t)n * 8, &r->pub.values}, {&r->d_status, (size_t)n, &r->pub.status}};
        return deliver(ctx, &r->own, parts, 2, out_mem);
    };
    const Status s = run();
    if (!s.ok() && first_error_op) *first_error_op = -1;
    return finish_call(ctx, r, s, out);
}

}  // extern "C"
