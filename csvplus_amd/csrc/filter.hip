// filter.hip — Filter / TakeWhile / DropWhile / Top / Drop with the reference's named predicates (csvplus.go:276-374,
// :1243-1293): the one stage that PRODUCES a list of row numbers from the data; every other stage consumes one.
//
//   cph_filter_rows   a postfix program of Like / Not / All / Any over the columns of a call -> an ascending row list
//   cph_rowsel_take   out[i] = sel.ids[list[i]] - sel.base: a Join's per-column row ids narrowed to the rows a Filter kept
//
// The predicate's strings are read ONCE:
//   k_pred_eval   rows on lanes (row = tile + 64 k + lane, 4 rows per lane in flight).  Every LIKE term over a real column
//                 (at most 32) becomes one bit of a per-row mask; the boolean program then runs over that mask on a bit
//                 stack — it is wave-uniform, only the data differs per lane.  __ballot is 64 bits wide on gfx950: a
//                 wave's ballot IS the bitmap word of its 64 rows.  The tile's words and count leave through the tile
//                 store of tile_bitmap.hpp, which describes the layout.
//   exclusive scan of the tile counts (TileBitmap::scan); its total is the result size — the call's host wait.
//   k_pred_emit   the rank walker of tile_bitmap.hpp: out[rank - skip] = first_row + row for the ranks in
//                 [skip, skip + limit).  No atomics in either kernel of the WHERE mode.
// The two WHILE modes only need the first failing row: the same evaluation without the bitmap, one 64-bit atomicMin per
// wave that saw a failure (none when the value it read at the tile's start is already smaller; tiles behind that value
// are not read at all).  Their answer is a range: nothing is materialised.
//
// Numeric compare terms (CPH_PRED_INT_* / CPH_PRED_FLT_*) are term bits like a LIKE, so the boolean program does not know
// them apart:
//   int64    converted in k_pred_eval itself (numparse_device.hpp: parse_int64) from the same 16-byte head a LIKE would
//            compare; the device decides every integer, so nothing else is needed.
//   float64  the term's column is converted FIRST through the path of cph_col_to_number (numparse.hip: convert_rows, once
//            per column and call, deferred rows finished on the host and patched in) and k_pred_eval compares the
//            resulting doubles — so a WHERE or WHILE answer never depends on where a value was converted.
// A program without numeric terms launches the NUM = false instantiations: the kernels it always launched.
//
// String terms that look INSIDE a value (CPH_PRED_STR_* / HAS_PREFIX / HAS_SUFFIX / CONTAINS) are term bits too.  Their
// per-value routines live in strpred_device.hpp (host-compilable, tested on the CPU); here they read the value through
// load_value_chunk and the literal as a LIKE's literal is kept: lit8, or the literal block in LDS / global memory.  A program
// with such a term launches the STR = true instantiations; every other program launches exactly what it launched before.
//
// Time terms (CPH_PRED_TIME_*) take the route of the float terms: the column is converted first through convert_rows
// (CPH_NUM_TIME_UNIX, once per column and call) and k_pred_eval compares the int64 seconds with their status; the literal is RFC
// 3339 text the host converts with the same routine (timeparse_device.hpp).  A program with such a term launches the TIM = true
// instantiations (which carry the numeric code too); every other program launches exactly what it launched before.
//
// Two more term kinds, behind template flags of their own (BITS, COLS) so that the twelve instantiations above stay the kernels they
// are (profiles/expr_conditions.txt):
//   CPH_PRED_EXPR_*  two numeric expressions compared.  k_expr_cmp (expr_eval.hip) evaluates the term FIRST into a TileBitmap of its
//                    own, kept beside the converted float columns for the call; here the term is kTermBits: row i of the call is bit
//                    i & 63 of word i >> 6, one wave-uniform 8-byte load per 64 rows.  A WHERE (or Switch-case) program that consists
//                    of exactly one such op is answered with that bitmap: no k_pred_eval is launched.
//   CPH_PRED_COLS_*  two columns of the row compared as strings: str_compare with the second column's value (its own value_span and
//                    source_row: another layout, other row ids) in the literal's place, kTermColCmp.
// A program with either launches one of five further instantiations: the lean ones of a program without numeric and time terms, or
// the one that carries every term kind.
// The way from a cph_pred_op program to the bitmap (terms, literal block, float columns, the k_pred_eval<true, NUM> launch) is
// pred_eval_bitmap (cph_internal.hpp): the WHERE mode calls it, and so does cph_map_switch (map_switch.hip), once per case.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "numparse_device.hpp"
#include "strpred_device.hpp"
#include "tile_bitmap.hpp"
#include "timeparse_device.hpp"

namespace cph {

constexpr int kFiltRows  = kTileWaveWords;             // rows per lane and tile: one of each word of the lane's wave
constexpr int kFiltPhase = 4;                          // ... of which this many are in flight at once
static_assert(kMatThreads == kTileWaves * kWave, "one workgroup per tile");
constexpr int kLitLds    = 4096;                       // literal bytes kept in LDS; more than that stay in global memory

enum : uint32_t { kTermBytes = 0, kTermFix8 = 1, kTermInt = 2, kTermF64 = 3,     // low byte of PredTerm::kind
                  kTermStrCmp = 4, kTermPrefix = 5, kTermSuffix = 6, kTermContains = 7,    // STR instantiations only
                  kTermTime = 8,                                                            // TIM instantiations only
                  kTermBits = 9,                                                            // BITS instantiations only
                  kTermColCmp = 10 };                                                       // COLS instantiations only
// bits 8..11 of a numeric, kTermStrCmp or kTermColCmp term's kind: which outcomes of (value ? literal) make the relation hold (kCmp*,
// cph_internal.hpp)
constexpr uint8_t kTermNever = 0xFF;                   // a LIKE decided on the host: no such column, or a fixed width other than the literal's

// One LIKE over a real column.  A literal of at most 8 bytes is lit8 (zero padded); a longer one lies in the literal
// block at word lit_off, zero padded to whole 8-byte words.
struct PredTerm {
    uint64_t lit8;
    uint32_t lit_off, len;
    int32_t  col;
    uint32_t kind;   // kTermFix8: a fixed-width column of 8 bytes on an 8-byte aligned base — one aligned load and one compare
                     // kTermInt / kTermF64 / kTermTime: lit8 = the literal's bits (kTermTime: its Unix seconds), the relation in bits 8..11
                     // kTermStrCmp .. kTermContains: the literal as a LIKE's (lit8 / lit_off, len); kTermStrCmp: the relation in bits 8..11
                     // kTermBits: an expression term k_expr_cmp has evaluated: fval = the bitmap's words, row i of the call = word i >> 6, bit i & 63
                     // kTermColCmp: col REL the column lit_off (both >= 0), the relation in bits 8..11
    const double*  fval;   // kTermF64 / kTermTime: the converted column (kTermTime: int64 seconds), entry i = row first_row + i of the selection ...
    const uint8_t* fstat;  // ... and its CPH_NUM_* status bytes
};
struct PredProg {    // travels in the kernel arguments (~0.9 KB): a wave reads it with scalar loads
    PredTerm term[CPH_PRED_MAX_LIKE];
    uint8_t  op[CPH_PRED_MAX_OPS];
    uint8_t  arg[CPH_PRED_MAX_OPS];   // LIKE: its term (kTermNever: false); ALL / ANY: the operand count
    int32_t  nops, nterms;
    const uint64_t* lits;
    uint32_t lit_words, lits_in_lds;
};

// value bytes [0, len) == the literal; len is the literal's length too
__device__ __forceinline__ bool like_bytes(const DevCol& col, uint64_t begin, const PredTerm& t, const uint64_t* glits,
                                           const CPH_LDS uint64_t* slits, bool in_lds) {
    const uint64_t len = t.len;
    for (uint64_t j = 0; 8 * j < len; j++) {
        const uint64_t chunk = load_value_chunk(col.data, begin, len, (int)j);
        const uint64_t nb = len - 8 * j;
        const uint64_t valid = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
        const uint64_t lit = len <= 8 ? t.lit8 : in_lds ? slits[t.lit_off + j] : glits[t.lit_off + j];
        if ((chunk ^ lit) & valid) return false;
    }
    return true;
}

// the two functors of strpred_device.hpp over a column's value and a term's literal
struct ValueChunks {
    const uint8_t* data;
    uint64_t begin;
    __device__ __forceinline__ uint64_t operator()(uint64_t off, uint64_t len, int j) const { return load_value_chunk(data, begin + off, len, j); }
};
struct ValueWords {   // a second column's value in the literal's place (kTermColCmp): word j of its len bytes
    const uint8_t* data;
    uint64_t begin, len;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return load_value_chunk(data, begin, len, (int)j); }
};
struct LiteralWords {
    const PredTerm& t;
    const uint64_t* glits;
    const CPH_LDS uint64_t* slits;
    bool in_lds;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return t.len <= 8 ? t.lit8 : in_lds ? slits[t.lit_off + j] : glits[t.lit_off + j]; }
};

// one string term on one value (what: kTermStrCmp .. kTermContains, uniform; rel: kCmp* outcomes of a kTermStrCmp)
__device__ __forceinline__ bool str_term(uint32_t what, uint32_t rel, const DevCol& col, uint64_t begin, uint64_t vlen, const PredTerm& t,
                                         const uint64_t* glits, const CPH_LDS uint64_t* slits, bool in_lds) {
    const ValueChunks v{col.data, begin};
    const LiteralWords lit{t, glits, slits, in_lds};
    if (what == kTermStrCmp) {
        const int c = str_compare(v, vlen, lit, (uint64_t)t.len);
        return (rel & (c < 0 ? kCmpLess : c == 0 ? kCmpEqual : kCmpGreater)) != 0;
    }
    if (what == kTermPrefix) return str_has_prefix(v, vlen, lit, (uint64_t)t.len);
    if (what == kTermSuffix) return str_has_suffix(v, vlen, lit, (uint64_t)t.len);
    return str_contains(v, vlen, lit, (uint64_t)t.len);
}

// BITMAP: bit = the predicate holds for that row of the call, in the layout of tile_bitmap.hpp.
// else:   *first_fail = min(*first_fail, the first row where it does not hold); the host presets it to n.
// STR: the program has a term of strpred_device.hpp; NUM: a numeric one; TIM (with NUM): a time term; BITS: an expression term's
// bits; COLS (with STR): a column-against-column term.  The instantiations without BITS and COLS are the kernels they were.
template <bool BITMAP, bool NUM, bool STR = false, bool TIM = false, bool BITS = false, bool COLS = false>
__global__ __launch_bounds__(kMatThreads) void k_pred_eval(ColsArg cols, ColIds ids, PredProg prog, uint64_t first_row, uint64_t n,
                                                          uint64_t* __restrict__ bitmap, uint32_t* __restrict__ counts,
                                                          unsigned long long* first_fail) {
    __shared__ uint64_t s_lits[kLitLds / 8];
    __shared__ uint64_t s_words[kTileWords];
    const CPH_LDS uint64_t* slits = (const CPH_LDS uint64_t*)s_lits;
    const bool in_lds = prog.lits_in_lds != 0;
    if (in_lds) {
        for (uint32_t q = threadIdx.x; q < prog.lit_words; q += kMatThreads) s_lits[q] = prog.lits[q];
        __syncthreads();
    }
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = tile_count(n);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kTileRows;
        unsigned long long seen = 0;
        if constexpr (!BITMAP) {
            seen = __hip_atomic_load(first_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t0 >= seen) continue;   // an earlier row has failed already: nothing here can be the first
        }
        uint64_t myword = 0;
        unsigned long long fail = ~0ull;
#pragma unroll
        for (int ph = 0; ph < kFiltRows / kFiltPhase; ph++) {
            uint64_t pos[kFiltPhase];   // position in the selection (rows past the end look at the last row; their result is dropped)
            uint32_t mask[kFiltPhase];
#pragma unroll
            for (int k = 0; k < kFiltPhase; k++) {
                const uint64_t i = t0 + (uint64_t)((wave * kTileWaveWords + ph * kFiltPhase + k) * 64 + lane);
                pos[k] = first_row + (i < n ? i : n - 1);
                mask[k] = 0;
            }
            for (int t = 0; t < prog.nterms; t++) {   // uniform
                const PredTerm& tm = prog.term[t];
                const DevCol& col = cols.c[tm.col];
                const RowIds& rid = ids.ids[tm.col];
                if (tm.kind == kTermFix8) {
                    uint64_t v[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) v[k] = reinterpret_cast<const uint64_t*>(col.data)[source_row(rid, pos[k])];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) mask[k] |= (uint32_t)(v[k] == tm.lit8) << t;
                } else if (NUM && (tm.kind & 0xFFu) == kTermInt) {
                    const uint32_t rel = tm.kind >> 8;
                    const int64_t lit = (int64_t)tm.lit8;
                    uint64_t b[kFiltPhase], l[kFiltPhase], c0[kFiltPhase], c1[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) value_span(col, source_row(rid, pos[k]), &b[k], &l[k]);
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) load_head16(col, b[k], l[k], &c0[k], &c1[k]);
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        int64_t v;
                        const uint32_t st = parse_int64(col, b[k], l[k], c0[k], c1[k], &v);
                        const uint32_t cls = v < lit ? kCmpLess : v == lit ? kCmpEqual : kCmpGreater;
                        mask[k] |= (uint32_t)(st == CPH_NUM_OK && (rel & cls) != 0) << t;   // a row that does not convert: false
                    }
                } else if (NUM && (tm.kind & 0xFFu) == kTermF64) {
                    const uint32_t rel = tm.kind >> 8;
                    const double lit = __longlong_as_double((long long)tm.lit8);
                    double v[kFiltPhase];
                    uint32_t st[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        v[k] = tm.fval[pos[k] - first_row];
                        st[k] = tm.fstat[pos[k] - first_row];
                    }
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        const uint32_t cls = v[k] < lit ? kCmpLess : v[k] == lit ? kCmpEqual : v[k] > lit ? kCmpGreater : kCmpUnordered;
                        mask[k] |= (uint32_t)(st[k] == CPH_NUM_OK && (rel & cls) != 0) << t;
                    }
                } else if (TIM && (tm.kind & 0xFFu) == kTermTime) {
                    const uint32_t rel = tm.kind >> 8;
                    const int64_t lit = (int64_t)tm.lit8;
                    const int64_t* tval = reinterpret_cast<const int64_t*>(tm.fval);
                    int64_t v[kFiltPhase];
                    uint32_t st[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        v[k] = tval[pos[k] - first_row];
                        st[k] = tm.fstat[pos[k] - first_row];
                    }
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        const uint32_t cls = v[k] < lit ? kCmpLess : v[k] == lit ? kCmpEqual : kCmpGreater;
                        mask[k] |= (uint32_t)(st[k] == CPH_NUM_OK && (rel & cls) != 0) << t;   // a row that does not convert: false
                    }
                } else if (BITS && (tm.kind & 0xFFu) == kTermBits) {
                    const uint64_t* words = reinterpret_cast<const uint64_t*>(tm.fval);
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {   // wave-uniform: one 8-byte load per 64 rows (a tile's 32 words are all written)
                        const uint64_t w = words[tile * kTileWords + (uint64_t)(wave * kTileWaveWords + ph * kFiltPhase + k)];
                        mask[k] |= (uint32_t)((w >> lane) & 1ull) << t;
                    }
                } else if (COLS && (tm.kind & 0xFFu) == kTermColCmp) {
                    const uint32_t rel = tm.kind >> 8;
                    const DevCol& colb = cols.c[tm.lit_off];
                    const RowIds& ridb = ids.ids[tm.lit_off];
                    uint64_t b[kFiltPhase], l[kFiltPhase], b2[kFiltPhase], l2[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        value_span(col, source_row(rid, pos[k]), &b[k], &l[k]);
                        value_span(colb, source_row(ridb, pos[k]), &b2[k], &l2[k]);
                    }
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        const int c = str_compare(ValueChunks{col.data, b[k]}, l[k], ValueWords{colb.data, b2[k], l2[k]}, l2[k]);
                        mask[k] |= (uint32_t)((rel & (c < 0 ? kCmpLess : c == 0 ? kCmpEqual : kCmpGreater)) != 0) << t;
                    }
                } else if (STR && (tm.kind & 0xFFu) >= kTermStrCmp) {
                    const uint32_t what = tm.kind & 0xFFu, rel = tm.kind >> 8;   // uniform: the wave diverges on the values' lengths alone
                    uint64_t b[kFiltPhase], l[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) value_span(col, source_row(rid, pos[k]), &b[k], &l[k]);
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++)
                        mask[k] |= (uint32_t)str_term(what, rel, col, b[k], l[k], tm, prog.lits, slits, in_lds) << t;
                } else {
                    uint64_t b[kFiltPhase], l[kFiltPhase];
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) value_span(col, source_row(rid, pos[k]), &b[k], &l[k]);
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++)
                        mask[k] |= (uint32_t)(l[k] == tm.len && like_bytes(col, b[k], tm, prog.lits, slits, in_lds)) << t;
                }
            }
            // the program over the term bits: a stack of at most 32 booleans, bit 0 = its top
            uint64_t st[kFiltPhase];
#pragma unroll
            for (int k = 0; k < kFiltPhase; k++) st[k] = 0;
            for (int q = 0; q < prog.nops; q++) {     // uniform
                const uint32_t op = prog.op[q], a = prog.arg[q];
                if (op == CPH_PRED_LIKE) {
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) st[k] = (st[k] << 1) | (a == kTermNever ? 0u : (mask[k] >> a) & 1u);
                } else if (op == CPH_PRED_NOT) {
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) st[k] ^= 1ull;
                } else {
                    const uint64_t m = (1ull << a) - 1;   // a <= 32
#pragma unroll
                    for (int k = 0; k < kFiltPhase; k++) {
                        const uint64_t r = op == CPH_PRED_ALL ? (uint64_t)((st[k] & m) == m) : (uint64_t)((st[k] & m) != 0);
                        st[k] = ((st[k] >> a) << 1) | r;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kFiltPhase; k++) {
                const int w = ph * kFiltPhase + k;
                const uint64_t i = t0 + (uint64_t)((wave * kTileWaveWords + w) * 64 + lane);
                const bool holds = (st[k] & 1ull) != 0;
                if constexpr (BITMAP) {
                    const uint64_t word = __ballot(i < n && holds);
                    if (lane == w) myword = word;
                } else {
                    const uint64_t bad = __ballot(i < n && !holds);
                    const unsigned long long at = t0 + (uint64_t)((wave * kTileWaveWords + w) * 64) + (uint64_t)__builtin_ctzll(bad | (1ull << 63));
                    if (bad && at < fail) fail = at;
                }
            }
        }
        if constexpr (BITMAP) {
            if (lane < kTileWaveWords) s_words[wave * kTileWaveWords + lane] = myword;
            tile_store_words(s_words, tile, bitmap, counts);
        } else {
            if (lane == 0 && fail < seen) atomicMin(first_fail, fail);
        }
    }
}

// offs[tile] = kept rows in front of the tile (offs[ntiles] = all of them); rank r of the filter's result goes to
// out[r - skip] for skip <= r < end
template <class T>
__global__ __launch_bounds__(kMatThreads) void k_pred_emit(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs,
                                                          uint64_t ntiles, uint64_t first_row, uint64_t skip, uint64_t end,
                                                          T* __restrict__ out) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t o0 = offs[tile], o1 = offs[tile + 1];
        if (o0 == o1 || o1 <= skip || o0 >= end) continue;   // uniform
        tile_for_each_set(bitmap, tile, o0, [&](uint64_t rank, int r) {
            if (rank >= skip && rank < end) out[rank - skip] = (T)(first_row + tile * kTileRows + (uint64_t)r);
        });
    }
}

// out[i] = sel[list[i]] - sel.base, as wide as sel (list.ptr == NULL: list[i] = list.base + i, see the caller)
__global__ __launch_bounds__(kMatThreads) void k_rowsel_take(RowIds sel, RowIds list, uint64_t list_first, uint64_t n, void* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t li = list.ptr ? source_row(list, i) : list_first + i;
        const uint64_t v = source_row(sel, li);
        if (sel.bits == 32) reinterpret_cast<uint32_t*>(out)[i] = (uint32_t)v;
        else reinterpret_cast<uint64_t*>(out)[i] = v;
    }
}

}  // namespace cph

using namespace cph;

// the library-owned row list behind cph_rowlist
struct cph_rowlist_impl {
    cph_rowlist pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_ids;
};

namespace {

// r->pub.ids / mem from the device array `dev` of n row numbers (the call's last synchronisation)
Status deliver_ids(cph_ctx* ctx, cph_rowlist_impl* r, DevBuf&& dev, uint64_t n, int32_t bits, int32_t out_mem) {
    r->pub.nrows = n;
    r->pub.first = 0;
    r->pub.bits = bits;
    r->pub.mem = out_mem;
    r->d_ids = std::move(dev);
    const ResultPart part{&r->d_ids, (size_t)n * (size_t)(bits / 8), &r->pub.ids};
    return deliver(ctx, &r->own, &part, 1, out_mem);
}

void set_range(cph_rowlist_impl* r, uint64_t first, uint64_t n, int32_t bits, int32_t out_mem) {
    r->pub.nrows = n;
    r->pub.first = first;
    r->pub.ids = nullptr;
    r->pub.bits = bits;
    r->pub.mem = out_mem;
}

// the functor of timeparse_device.hpp over a literal in host memory
struct HostTimeChunks {
    const uint8_t* p;
    uint64_t len;
    uint64_t operator()(int j) const {
        uint64_t w = 0;
        const uint64_t at = 8ull * (uint64_t)j;
        if (at < len) memcpy(&w, p + at, (size_t)(len - at < 8 ? len - at : 8));
        return w;
    }
};

// a time term's literal -> its Unix seconds, with the routine the device runs; a literal with a fraction is refused
Status time_literal(const cph_strval& value, int64_t* secs) {
    const HostTimeChunks v{value.data, value.len};
    const std::string text(reinterpret_cast<const char*>(value.data ? value.data : (const uint8_t*)""), (size_t)(value.len < 64 ? value.len : 64));
    if (value.len > 35) return {CPH_ERR_INVALID, "cph_filter_rows: a time term's literal is no RFC 3339 timestamp: \"" + text + "...\""};
    const uint32_t st = parse_rfc3339(value.len, v(0), v(1), v(2), v(3), v, false, secs);
    if (st != CPH_NUM_OK)
        return {CPH_ERR_INVALID, "cph_filter_rows: a time term's literal \"" + text + "\" does not convert (" +
                                     (st == CPH_NUM_ERR_SYNTAX ? "invalid syntax" : st == CPH_NUM_ERR_RANGE ? "a field out of range" : "not decided by this library") + ")"};
    if (value.len > 20 && value.data[19] == '.')
        return {CPH_ERR_INVALID, "cph_filter_rows: a time term's literal \"" + text + "\" has a fraction: the term compares whole seconds"};
    return {};
}

// the program's shape: every rule of the header's comment that does not need the columns
Status check_program(const cph_pred_op* prog, int32_t nops, int32_t ncols) {
    if (nops < 1 || nops > CPH_PRED_MAX_OPS) return {CPH_ERR_INVALID, "cph_filter_rows: a program has 1..64 ops"};
    int depth = 0, likes = 0;
    for (int q = 0; q < nops; q++) {
        const cph_pred_op& o = prog[q];
        switch (o.op) {
            case CPH_PRED_STR_LT: case CPH_PRED_STR_LE: case CPH_PRED_STR_EQ: case CPH_PRED_STR_NE: case CPH_PRED_STR_GE: case CPH_PRED_STR_GT:
            case CPH_PRED_HAS_PREFIX: case CPH_PRED_HAS_SUFFIX: case CPH_PRED_CONTAINS:
                if (o.arg < -1 || o.arg >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: string term column outside -1..ncols-1"};
                if (!o.value.data && o.value.len) return {CPH_ERR_INVALID, "cph_filter_rows: a string term's literal with bytes but no data pointer"};
                if (o.value.len > 0xFFFFFFFFull) return {CPH_ERR_INVALID, "cph_filter_rows: a string term's literal beyond 4 GiB"};
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE, numeric and string terms"};
                depth++;
                break;
            case CPH_PRED_LIKE:
                if (o.arg < -1 || o.arg >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: LIKE column outside -1..ncols-1"};
                if (!o.value.data && o.value.len) return {CPH_ERR_INVALID, "cph_filter_rows: a LIKE value with bytes but no data pointer"};
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE and numeric terms"};
                depth++;
                break;
            case CPH_PRED_INT_LT: case CPH_PRED_INT_LE: case CPH_PRED_INT_EQ: case CPH_PRED_INT_NE: case CPH_PRED_INT_GE: case CPH_PRED_INT_GT:
            case CPH_PRED_FLT_LT: case CPH_PRED_FLT_LE: case CPH_PRED_FLT_EQ: case CPH_PRED_FLT_NE: case CPH_PRED_FLT_GE: case CPH_PRED_FLT_GT:
                if (o.arg < -1 || o.arg >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: numeric compare column outside -1..ncols-1"};
                if (!o.value.data || o.value.len != 8)
                    return {CPH_ERR_INVALID, "cph_filter_rows: a numeric literal is exactly 8 bytes (an int64_t or a double) behind a non-NULL pointer"};
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE and numeric terms"};
                depth++;
                break;
            case CPH_PRED_TIME_LT: case CPH_PRED_TIME_LE: case CPH_PRED_TIME_EQ: case CPH_PRED_TIME_NE: case CPH_PRED_TIME_GE: case CPH_PRED_TIME_GT: {
                if (o.arg < -1 || o.arg >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: time term column outside -1..ncols-1"};
                if (!o.value.data && o.value.len) return {CPH_ERR_INVALID, "cph_filter_rows: a time term's literal with bytes but no data pointer"};
                int64_t secs = 0;
                Status s = time_literal(o.value, &secs);
                if (!s.ok()) return s;
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE, numeric, string and time terms"};
                depth++;
                break;
            }
            case CPH_PRED_EXPR_LT: case CPH_PRED_EXPR_LE: case CPH_PRED_EXPR_EQ: case CPH_PRED_EXPR_NE: case CPH_PRED_EXPR_GE: case CPH_PRED_EXPR_GT: {
                if (o.arg != 0 && o.arg != -1) return {CPH_ERR_INVALID, "cph_filter_rows: expression term: arg is 0, or -1 for a column the rows lack"};
                if (o.arg == 0) {   // arg == -1: the value is ignored
                    Status s = check_pred_expr(o.value, ncols);
                    if (!s.ok()) return s;
                }
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE, numeric, string, time, expression and column terms"};
                depth++;
                break;
            }
            case CPH_PRED_COLS_LT: case CPH_PRED_COLS_LE: case CPH_PRED_COLS_EQ: case CPH_PRED_COLS_NE: case CPH_PRED_COLS_GE: case CPH_PRED_COLS_GT: {
                if (o.arg < -1 || o.arg >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: column-against-column term: column outside -1..ncols-1"};
                if (!o.value.data || o.value.len != 4)
                    return {CPH_ERR_INVALID, "cph_filter_rows: column-against-column term: value is exactly 4 bytes (the int32_t second column) behind a non-NULL pointer"};
                int32_t b = 0;
                memcpy(&b, o.value.data, 4);
                if (b < -1 || b >= ncols) return {CPH_ERR_INVALID, "cph_filter_rows: column-against-column term: second column outside -1..ncols-1"};
                if (++likes > CPH_PRED_MAX_LIKE) return {CPH_ERR_INVALID, "cph_filter_rows: more than 32 LIKE, numeric, string, time, expression and column terms"};
                depth++;
                break;
            }
            case CPH_PRED_NOT:
                if (depth < 1) return {CPH_ERR_INVALID, "cph_filter_rows: stack underflow (NOT on an empty stack)"};
                break;
            case CPH_PRED_ALL:
            case CPH_PRED_ANY:
                if (o.arg < 0 || o.arg > depth) return {CPH_ERR_INVALID, "cph_filter_rows: stack underflow (ALL / ANY pops more than there is)"};
                depth += 1 - o.arg;
                break;
            default:
                return {CPH_ERR_INVALID, "cph_filter_rows: unknown op (1..4, 16..21, 24..29, 32..37, 40..42, 48..53, 56..61, 72..77)"};
        }
        if (depth > CPH_PRED_MAX_STACK) return {CPH_ERR_INVALID, "cph_filter_rows: stack deeper than 32"};
    }
    if (depth != 1) return {CPH_ERR_INVALID, "cph_filter_rows: the program must leave exactly one value"};
    return {};
}

bool is_int_cmp(int32_t op) { return op >= CPH_PRED_INT_LT && op <= CPH_PRED_INT_GT; }
bool is_flt_cmp(int32_t op) { return op >= CPH_PRED_FLT_LT && op <= CPH_PRED_FLT_GT; }
bool is_str_cmp(int32_t op) { return op >= CPH_PRED_STR_LT && op <= CPH_PRED_STR_GT; }
bool is_time_cmp(int32_t op) { return op >= CPH_PRED_TIME_LT && op <= CPH_PRED_TIME_GT; }
bool is_expr_cmp(int32_t op) { return op >= CPH_PRED_EXPR_LT && op <= CPH_PRED_EXPR_GT; }
bool is_cols_cmp(int32_t op) { return op >= CPH_PRED_COLS_LT && op <= CPH_PRED_COLS_GT; }
bool is_str_term(int32_t op) { return is_str_cmp(op) || (op >= CPH_PRED_HAS_PREFIX && op <= CPH_PRED_CONTAINS); }
// LT LE EQ NE GE GT -> the outcomes under which the relation holds (IEEE: unordered satisfies NE alone)
uint32_t rel_outcomes(int32_t rel) {
    static const uint32_t m[6] = {kCmpLess, kCmpLess | kCmpEqual, kCmpEqual, kCmpLess | kCmpGreater | kCmpUnordered, kCmpEqual | kCmpGreater, kCmpGreater};
    return m[rel];
}

struct BuiltProg {   // a program as k_pred_eval takes it
    PredProg pp{};
    DevBuf litbuf;          // the literals beyond 8 bytes; the kernels read it
    double col_bytes = 0;   // byte model: what the evaluation reads of the columns
    bool numeric = false;   // the NUM instantiations
    bool strings = false;   // the STR instantiations
    bool times = false;     // the TIM instantiations
    bool bits = false;      // the BITS instantiations: an expression term
    bool colcmp = false;    // the COLS instantiations: a column-against-column term
    size_t expr_term = 0;   // bits: the last expression term's entry of the call's PredFloatCol vector
};

// fcols: the float columns converted so far in this call (reused, appended to)
Status build_pred_prog(cph_ctx* ctx, const ColsArg& arg, const ColIds& ids, const cph_pred_op* prog, int32_t nops, uint64_t first_row, uint64_t n,
                       std::vector<PredFloatCol>* fcols, BuiltProg* bp) {
    PredProg& pp = bp->pp;
    // the program: LIKE terms over real columns get a bit each, the others are decided here
    std::vector<uint64_t> lits;
    uint32_t seen_cols = 0;
    for (int q = 0; q < nops; q++) {
        pp.op[q] = (uint8_t)prog[q].op;
        pp.arg[q] = (uint8_t)prog[q].arg;
        if (is_time_cmp(prog[q].op)) {   // a term bit too: the column converted first, as for a float term
            const int c = prog[q].arg;
            pp.op[q] = (uint8_t)CPH_PRED_LIKE;
            if (c < 0) {
                pp.arg[q] = kTermNever;
                continue;
            }
            bp->numeric = bp->times = true;
            PredTerm& t = pp.term[pp.nterms];
            pp.arg[q] = (uint8_t)pp.nterms++;
            t.col = c;
            int64_t secs = 0;
            CPH_TRY(time_literal(prog[q].value, &secs));
            t.lit8 = (uint64_t)secs;
            t.kind = kTermTime | (rel_outcomes(prog[q].op - CPH_PRED_TIME_LT) << 8);
            size_t f = 0;
            while (f < fcols->size() && ((*fcols)[f].col != c || (*fcols)[f].kind != CPH_NUM_TIME_UNIX)) f++;
            if (f == fcols->size()) {
                fcols->emplace_back();
                (*fcols)[f].col = c;
                (*fcols)[f].kind = CPH_NUM_TIME_UNIX;
                NumColStats st;
                CPH_TRY(convert_rows(ctx, arg.c[c], ids.ids[c], first_row, n, CPH_NUM_TIME_UNIX, &(*fcols)[f].values, &(*fcols)[f].status, &st));
                bp->col_bytes += 9.0 * (double)n;   // the converted column read back (its conversion is timed on its own)
            }
            t.fval = (*fcols)[f].values.as<double>();
            t.fstat = (*fcols)[f].status.as<uint8_t>();
            continue;
        }
        if (is_expr_cmp(prog[q].op)) {   // a term bit k_expr_cmp evaluates first: a bitmap of its own, kept beside the float columns
            pp.op[q] = (uint8_t)CPH_PRED_LIKE;
            if (prog[q].arg < 0) {
                pp.arg[q] = kTermNever;
                continue;
            }
            bp->bits = true;
            fcols->emplace_back();
            PredFloatCol& e = fcols->back();
            e.col = -1, e.kind = 0;
            CPH_TRY(expr_cmp_bitmap(ctx, arg, ids, prog[q].value, rel_outcomes(prog[q].op - CPH_PRED_EXPR_LT), first_row, n, &e.bits, &e.hold));
            bp->expr_term = fcols->size() - 1;
            PredTerm& t = pp.term[pp.nterms];
            pp.arg[q] = (uint8_t)pp.nterms++;
            t.col = 0;
            t.kind = kTermBits;
            t.fval = reinterpret_cast<const double*>(e.bits.words());
            bp->col_bytes += (double)n / 8.0;
            continue;
        }
        if (is_cols_cmp(prog[q].op)) {
            int32_t c2 = 0;
            memcpy(&c2, prog[q].value.data, 4);
            const int c = prog[q].arg;
            pp.op[q] = (uint8_t)CPH_PRED_LIKE;
            if (c < 0 || c2 < 0) {
                pp.arg[q] = kTermNever;
                continue;
            }
            bp->strings = bp->colcmp = true;
            PredTerm& t = pp.term[pp.nterms];
            pp.arg[q] = (uint8_t)pp.nterms++;
            t.col = c;
            t.lit_off = (uint32_t)c2;
            t.kind = kTermColCmp | (rel_outcomes(prog[q].op - CPH_PRED_COLS_LT) << 8);
            for (const int k : {c, (int)c2}) {   // byte model: offsets (or nothing) + ~8 value bytes, once per column
                if ((seen_cols >> k) & 1u) continue;
                seen_cols |= 1u << k;
                bp->col_bytes += arg.c[k].fixed_width ? (double)arg.c[k].fixed_width * (double)n : ((double)(arg.c[k].offset_bits / 8) + 8.0) * (double)n;
                if (ids.ids[k].ptr) bp->col_bytes += (double)(ids.ids[k].bits / 8) * (double)n;
            }
            continue;
        }
        if (is_int_cmp(prog[q].op) || is_flt_cmp(prog[q].op)) {   // a term bit like a LIKE: the kernel's program sees a LIKE
            const int c = prog[q].arg;
            pp.op[q] = (uint8_t)CPH_PRED_LIKE;
            if (c < 0) {
                pp.arg[q] = kTermNever;
                continue;
            }
            bp->numeric = true;
            const bool flt = is_flt_cmp(prog[q].op);
            PredTerm& t = pp.term[pp.nterms];
            pp.arg[q] = (uint8_t)pp.nterms++;
            t.col = c;
            memcpy(&t.lit8, prog[q].value.data, 8);
            t.kind = (flt ? kTermF64 : kTermInt) | (rel_outcomes(prog[q].op - (flt ? CPH_PRED_FLT_LT : CPH_PRED_INT_LT)) << 8);
            if (flt) {
                size_t f = 0;
                while (f < fcols->size() && ((*fcols)[f].col != c || (*fcols)[f].kind != CPH_NUM_FLOAT64)) f++;
                if (f == fcols->size()) {
                    fcols->emplace_back();
                    (*fcols)[f].col = c;
                    NumColStats st;
                    CPH_TRY(convert_rows(ctx, arg.c[c], ids.ids[c], first_row, n, CPH_NUM_FLOAT64, &(*fcols)[f].values, &(*fcols)[f].status, &st));
                    bp->col_bytes += 9.0 * (double)n;   // the converted column read back (its conversion is timed on its own)
                }
                t.fval = (*fcols)[f].values.as<double>();
                t.fstat = (*fcols)[f].status.as<uint8_t>();
            } else if (!((seen_cols >> c) & 1u)) {   // offsets (or nothing) + the value's head, once per column
                seen_cols |= 1u << c;
                bp->col_bytes += arg.c[c].fixed_width ? (double)arg.c[c].fixed_width * (double)n
                                                  : ((double)(arg.c[c].offset_bits / 8) + 8.0) * (double)n;
                if (ids.ids[c].ptr) bp->col_bytes += (double)(ids.ids[c].bits / 8) * (double)n;
            }
            continue;
        }
        const bool str = is_str_term(prog[q].op);
        if (prog[q].op != CPH_PRED_LIKE && !str) continue;
        const int c = prog[q].arg;
        const uint64_t len = prog[q].value.len;
        pp.op[q] = (uint8_t)CPH_PRED_LIKE;   // a string term: a term bit like a LIKE
        if (c < 0 || len > 0xFFFFFFFFull || (!str && arg.c[c].fixed_width && arg.c[c].fixed_width != len)) {
            pp.arg[q] = kTermNever;
            continue;
        }
        PredTerm& t = pp.term[pp.nterms];
        pp.arg[q] = (uint8_t)pp.nterms++;
        t.col = c;
        t.len = (uint32_t)len;
        if (str) {
            bp->strings = true;
            t.kind = is_str_cmp(prog[q].op)               ? kTermStrCmp | (rel_outcomes(prog[q].op - CPH_PRED_STR_LT) << 8)
                     : prog[q].op == CPH_PRED_HAS_PREFIX ? kTermPrefix
                     : prog[q].op == CPH_PRED_HAS_SUFFIX ? kTermSuffix
                                                         : kTermContains;
        } else {
            t.kind = arg.c[c].fixed_width == 8 && ((uintptr_t)arg.c[c].data & 7u) == 0 ? kTermFix8 : kTermBytes;
        }
        if (len <= 8) {
            if (len) memcpy(&t.lit8, prog[q].value.data, (size_t)len);
        } else {
            t.lit_off = (uint32_t)lits.size();
            lits.resize(lits.size() + (size_t)((len + 7) / 8), 0);
            memcpy(lits.data() + t.lit_off, prog[q].value.data, (size_t)len);
        }
        if (!((seen_cols >> c) & 1u)) {   // byte model: a column's offsets and bytes count once
            seen_cols |= 1u << c;
            bp->col_bytes += arg.c[c].fixed_width ? (double)arg.c[c].fixed_width * (double)n
                                              : ((double)(arg.c[c].offset_bits / 8) + (double)len) * (double)n;
            if (ids.ids[c].ptr) bp->col_bytes += (double)(ids.ids[c].bits / 8) * (double)n;
        }
    }
    pp.nops = nops;
    if (!lits.empty()) {
        if (lits.size() > 0xFFFFFFFFull / 8) return {CPH_ERR_INVALID, "cph_filter_rows: literals beyond 4 GiB"};
        const size_t lb = lits.size() * sizeof(uint64_t);
        CPH_TRY(upload_block(ctx, lits.data(), lb, &bp->litbuf));
        pp.lits = bp->litbuf.as<uint64_t>();
        pp.lit_words = (uint32_t)lits.size();
        pp.lits_in_lds = lb <= (size_t)kLitLds;
    }
    return {};
}

// the instantiation a program needs: NUM / STR only where it has such a term
template <bool BITMAP>
void launch_pred_eval(cph_ctx* ctx, const BuiltProg& bp, const ColsArg& arg, const ColIds& ids, uint64_t first_row, uint64_t n, uint64_t ntiles,
                      uint64_t* bitmap, uint32_t* counts, unsigned long long* first_fail) {
    const dim3 grid(tile_grid(ntiles)), block(kMatThreads);
    if (bp.bits || bp.colcmp) {   // the new terms: the lean kernel of a program without numeric and time terms, else the one with every kind
        const bool lean = !bp.numeric && !bp.times;
        if (!lean)
            hipLaunchKernelGGL((k_pred_eval<BITMAP, true, true, true, true, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
        else if (bp.colcmp && bp.bits)
            hipLaunchKernelGGL((k_pred_eval<BITMAP, false, true, false, true, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
        else if (bp.colcmp)
            hipLaunchKernelGGL((k_pred_eval<BITMAP, false, true, false, false, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
        else if (bp.strings)
            hipLaunchKernelGGL((k_pred_eval<BITMAP, false, true, false, true, false>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
        else
            hipLaunchKernelGGL((k_pred_eval<BITMAP, false, false, false, true, false>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    } else if (bp.times && bp.strings)
        hipLaunchKernelGGL((k_pred_eval<BITMAP, true, true, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    else if (bp.times)
        hipLaunchKernelGGL((k_pred_eval<BITMAP, true, false, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    else if (bp.strings && bp.numeric)
        hipLaunchKernelGGL((k_pred_eval<BITMAP, true, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    else if (bp.strings)
        hipLaunchKernelGGL((k_pred_eval<BITMAP, false, true>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    else if (bp.numeric)
        hipLaunchKernelGGL((k_pred_eval<BITMAP, true, false>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
    else
        hipLaunchKernelGGL((k_pred_eval<BITMAP, false, false>), grid, block, 0, ctx->stream, arg, ids, bp.pp, first_row, n, bitmap, counts, first_fail);
}

}  // namespace

namespace cph {

Status check_pred_program(const cph_pred_op* prog, int32_t nops, int32_t ncols) { return check_program(prog, nops, ncols); }

Status pred_eval_bitmap(cph_ctx* ctx, const ColsArg& arg, const ColIds& ids, const cph_pred_op* prog, int32_t nops, uint64_t first_row,
                        uint64_t n, std::vector<PredFloatCol>* fcols, PredBitmap* out) {
    BuiltProg bp;
    CPH_TRY(build_pred_prog(ctx, arg, ids, prog, nops, first_row, n, fcols, &bp));
    TileBitmap& tb = out->rows;
    if (nops == 1 && bp.bits) {   // the program IS one expression term: k_expr_cmp's bitmap is the answer, no k_pred_eval
        PredFloatCol& e = (*fcols)[bp.expr_term];
        tb.bitmap = std::move(e.bits.bitmap);
        tb.tile_counts = std::move(e.bits.tile_counts);
        tb.ntiles = e.bits.ntiles;
        return {};
    }
    CPH_TRY(tb.alloc(ctx, n));
    {
        ProfScope ps(ctx, bp.strings ? "k_pred_eval_str" : "k_pred_eval", bp.col_bytes + (double)n / 8.0 + 4.0 * (double)tb.ntiles);
        launch_pred_eval<true>(ctx, bp, arg, ids, first_row, n, tb.ntiles, tb.words(), tb.counts(), nullptr);
    }
    CPH_HIP_TRY(hipGetLastError());
    out->lits = std::move(bp.litbuf);   // the kernel reads it: it lives as long as the bitmap
    return {};
}

}  // namespace cph

extern "C" {

CPH_API int32_t cph_filter_rows(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                                const cph_pred_op* prog, int32_t nops, const cph_filter_opts* opts, int32_t out_mem,
                                cph_rowlist** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!prog || !opts) return fail_with(ctx, {CPH_ERR_INVALID, "cph_filter_rows: prog and opts must not be NULL"});
    if (ncols < 0 || ncols > CPH_MAX_KEY_COLS) return fail_with(ctx, {CPH_ERR_INVALID, "cph_filter_rows: 0..16 columns"});
    if (ncols && !cols) return fail_with(ctx, {CPH_ERR_INVALID, "cph_filter_rows: cols must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    if (opts->mode != CPH_FILTER_WHERE && opts->mode != CPH_FILTER_TAKE_WHILE && opts->mode != CPH_FILTER_DROP_WHILE)
        return fail_with(ctx, {CPH_ERR_INVALID, "cph_filter_rows: unknown mode"});
    if (opts->out_bits != 32 && opts->out_bits != 64) return fail_with(ctx, {CPH_ERR_INVALID, "cph_filter_rows: out_bits must be 32 or 64"});
    {
        Status s = check_program(prog, nops, ncols);
        if (!s.ok()) return fail_with(ctx, s);
    }
    const uint64_t n = nrows, first_row = opts->first_row;
    if (first_row + n < n) return fail_with(ctx, {CPH_ERR_TOO_MANY_ROWS, "cph_filter_rows: first_row + nrows overflows"});
    if (n > 0xFFFFFFFFull) return fail_with(ctx, {CPH_ERR_TOO_MANY_ROWS, "cph_filter_rows: more than 2^32-1 rows in one call"});
    if (opts->out_bits == 32 && first_row + n > 0xFFFFFFFFull)
        return fail_with(ctx, {CPH_ERR_TOO_MANY_ROWS, "cph_filter_rows: first_row + nrows > 2^32-1 needs out_bits 64"});
    {
        Status s = check_row_sources(cols, sel, ncols, first_row, n, false);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_rowlist_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    const int32_t bits = opts->out_bits;
    auto run = [&]() -> Status {
        if (n == 0) {
            set_range(r, first_row, 0, bits, out_mem);
            return {};
        }
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, nullptr, ncols, first_row, n, &staged, &arg, &ids));
        std::vector<PredFloatCol> fcols;
        const uint64_t ntiles = tile_count(n);
        CPH_TRY(ensure_pinned_scratch(ctx, sizeof(uint64_t)));
        if (opts->mode != CPH_FILTER_WHERE) {
            BuiltProg bp;
            CPH_TRY(build_pred_prog(ctx, arg, ids, prog, nops, first_row, n, &fcols, &bp));
            DevBuf ff;   // rows in front of the first failing one; n: none fails
            CPH_TRY(upload_block(ctx, n, &ff));
            {
                ProfScope ps(ctx, bp.strings ? "k_pred_eval_str" : "k_pred_eval", bp.col_bytes);
                launch_pred_eval<false>(ctx, bp, arg, ids, first_row, n, ntiles, nullptr, nullptr, ff.as<unsigned long long>());
            }
            CPH_HIP_TRY(hipGetLastError());
            uint64_t stop = 0;   // rows in front of the first failing one
            CPH_TRY(read_device_value(ctx, ff.as<uint64_t>(), &stop));
            // TakeWhile: [0, stop); DropWhile: [stop, n) — then .Drop(skip).Top(limit)
            uint64_t lo = opts->mode == CPH_FILTER_TAKE_WHILE ? 0 : stop, hi = opts->mode == CPH_FILTER_TAKE_WHILE ? stop : n;
            lo = hi - lo > opts->skip ? lo + opts->skip : hi;
            if (hi - lo > opts->limit) hi = lo + opts->limit;
            set_range(r, first_row + lo, hi - lo, bits, out_mem);
            return {};
        }
        PredBitmap pb;
        CPH_TRY(pred_eval_bitmap(ctx, arg, ids, prog, nops, first_row, n, &fcols, &pb));
        const TileBitmap& tb = pb.rows;
        CPH_TRY(tb.scan(ctx));
        uint32_t total = 0;
        CPH_TRY(tb.read_total(ctx, &total));   // the call's host wait
        uint64_t kept = total > opts->skip ? total - opts->skip : 0;
        if (kept > opts->limit) kept = opts->limit;
        if (kept == 0) {
            set_range(r, first_row, 0, bits, out_mem);
            return {};
        }
        DevBuf outb;
        CPH_TRY(outb.alloc(&ctx->pool, kept * (size_t)(bits / 8)));
        {
            ProfScope ps(ctx, "k_pred_emit", (double)n / 8.0 + 4.0 * (double)ntiles + (double)kept * (double)(bits / 8));
            if (bits == 32)
                hipLaunchKernelGGL(k_pred_emit<uint32_t>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, tb.words(), tb.counts(), ntiles,
                                   first_row, opts->skip, opts->skip + kept, outb.as<uint32_t>());
            else
                hipLaunchKernelGGL(k_pred_emit<uint64_t>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, tb.words(), tb.counts(), ntiles,
                                   first_row, opts->skip, opts->skip + kept, outb.as<uint64_t>());
        }
        CPH_HIP_TRY(hipGetLastError());
        return deliver_ids(ctx, r, std::move(outb), kept, bits, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API int32_t cph_rowsel_take(cph_ctx* ctx, const cph_rowsel* sel, int32_t sel_mem, const cph_rowlist* list, int32_t out_mem,
                                cph_rowlist** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!list) return fail_with(ctx, {CPH_ERR_INVALID, "cph_rowsel_take: list must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    const bool ident = !sel || !sel->ids;
    if (!ident && sel_mem != CPH_MEM_HOST && sel_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad sel_mem"});
    if (!ident && sel->bits != 32 && sel->bits != 64) return fail_with(ctx, {CPH_ERR_INVALID, "row id bits must be 32 or 64"});
    if (list->ids && list->bits != 32 && list->bits != 64) return fail_with(ctx, {CPH_ERR_INVALID, "cph_rowsel_take: list bits must be 32 or 64"});
    if (list->ids && list->mem != CPH_MEM_HOST && list->mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_rowsel_take: bad list mem"});
    auto* r = new (std::nothrow) cph_rowlist_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    const uint64_t n = list->nrows;
    auto run = [&]() -> Status {
        if (n == 0 || (ident && !list->ids)) {   // nothing to gather: an empty list, or a range through the identity
            set_range(r, n ? list->first : 0, n, list->bits == 64 ? 64 : 32, out_mem);
            return {};
        }
        // the list on the device
        RowIds lst;
        DevBuf lbuf;
        const size_t lw = (size_t)(list->bits / 8);
        if (list->ids) {
            lst.bits = list->bits;
            CPH_TRY(device_array(ctx, list->ids, list->mem, n * lw, &lbuf, &lst.ptr));
        }
        if (ident) {   // a copy of the list in out_mem
            DevBuf copy;
            if (list->mem == CPH_MEM_HOST) {
                copy = std::move(lbuf);
            } else {
                CPH_TRY(copy.alloc(&ctx->pool, n * lw));
                CPH_HIP_TRY(hipMemcpyAsync(copy.get(), list->ids, n * lw, hipMemcpyDeviceToDevice, ctx->stream));
            }
            return deliver_ids(ctx, r, std::move(copy), n, list->bits, out_mem);
        }
        RowIds s;
        s.bits = sel->bits;
        s.base = sel->base;
        s.ptr = sel->ids;
        DevBuf sbuf;
        if (sel_mem == CPH_MEM_HOST) {   // entries 0 .. the list's last (= largest) row number travel to the device
            uint64_t last = 0;
            if (!list->ids) {
                last = list->first + n - 1;
            } else if (list->mem == CPH_MEM_HOST) {
                last = list->bits == 32 ? (uint64_t) static_cast<const uint32_t*>(list->ids)[n - 1] : static_cast<const uint64_t*>(list->ids)[n - 1];
            } else if (list->bits == 32) {
                uint32_t v = 0;
                CPH_TRY(read_device_value(ctx, static_cast<const uint32_t*>(list->ids) + (n - 1), &v));
                last = v;
            } else {
                CPH_TRY(read_device_value(ctx, static_cast<const uint64_t*>(list->ids) + (n - 1), &last));
            }
            CPH_TRY(device_array(ctx, sel->ids, sel_mem, (size_t)(last + 1) * (size_t)(sel->bits / 8), &sbuf, &s.ptr));
        }
        DevBuf outb;
        CPH_TRY(outb.alloc(&ctx->pool, n * (size_t)(sel->bits / 8)));
        {
            ProfScope ps(ctx, "k_rowsel_take", (double)n * (double)(lst.ptr ? lw : 0) + 2.0 * (double)n * (double)(sel->bits / 8));
            hipLaunchKernelGGL(k_rowsel_take, dim3(grid_rows(n)), dim3(kMatThreads), 0, ctx->stream, s, lst, list->first, n, outb.get());
        }
        CPH_HIP_TRY(hipGetLastError());
        return deliver_ids(ctx, r, std::move(outb), n, sel->bits, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API void cph_rowlist_release(cph_rowlist* pub) { release_result<cph_rowlist_impl>(pub); }

}  // extern "C"
