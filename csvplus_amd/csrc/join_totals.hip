// join_totals.hip — Totals over a Join: Count and Sum / Min / Max per BUILD ROW of one step of a chain (cph_chain_aggregate),
// the reduction the reference's TestSimpleUniqueJoin (`qtyMap[id] += qty`, csvplus_test.go:368-452) and TestTransformedSource
// (`custAmounts[cid] += amount`, csvplus_test.go:754-806) accumulate in a Go map over the joined stream.  The Join has already
// found the group: build_row[step][m] is a dense integer below the index's row count, so there is no codec, no key string and no
// second index here — the group table is addressed directly.
//
//   direct route   Count, int Sum, int Min / Max, float Min / Max: all order-independent, so 64-bit INTEGER atomics are exact and
//                  reproducible.  One pass per column over the joined rows (k_jt_direct: 4 bytes of build_row + 8 of value per
//                  row, every load coalesced: row = tile + k * 256 + thread).  Min / Max run on an order-preserving map of the
//                  value to uint64 (int: sign bit flipped; double: sign bit flipped for non-negative values, all bits for
//                  negative ones, which puts -0 below +0; a NaN becomes the extreme key of the op, so it wins) and are decoded
//                  by k_jt_decode, which also zeroes the groups no row matched.
//                  ngroups <= CPH_CHAIN_AGG_LDS_GROUPS: the table is kept per workgroup in LDS (32 KiB), accumulated with LDS
//                  atomics and flushed once, untouched groups skipped; above it the atomics go to global memory (device scope).
//                  In front of either a wave whose 64 rows all hit ONE group folds them with shuffles and issues one atomic
//                  (the 1-group and the sorted-stream case); never needed for correctness.
//   float Sum      bits must reproduce, so no floating-point atomics: (build_row, m) pairs sorted with the stable radix sort
//                  over bits(ngroups - 1) key bits, run starts marked on the sorted keys, aggregate.hip's segmented reduce +
//                  carry with the sorted m as gather permutation, each run's sum scattered to its group (k_jt_scatter).  Inside
//                  a group the rows are in ascending m (the sort is stable) and the association order is a function of the
//                  sorted positions alone.
//   sorted runs    above the LDS limit one 8-byte atomic per row is one memory request per lane: measured on an MI355X at 1e8 random
//                  rows, 4.2 ms per column into 1e5 or 1e7 groups (24 G atomics/s), against 2.1 ms for the sort plus 1.9 ms per
//                  column for the segmented reduce (profiles/join_totals.txt).  So once the rows are sorted anyway (a float Sum is
//                  asked for) or there are enough of them to be bound by throughput and not by launches (n >= kJtSortRows), EVERY
//                  column of such a table rides the sorted runs: Count = the run lengths, int Sum / Min / Max and float Min / Max
//                  by the same segmented reduce (aggregate.hip's agg_join: the same results as the direct route, bit for bit).
//                  Smaller calls keep the global atomics: two launches per column instead of a dozen.
//   k_jt_errors    a non-zero status byte is DATA: counted, and the lowest (row, spec) kept (the report of num_report.hpp, tag = the spec).
// Every launch goes on the ctx stream, scratch comes from the ctx pool; the call waits once for the error words and the
// out-of-range flag, then hands the arrays over.
#include <algorithm>
#include <cstring>
#include <new>

#include "num_report.hpp"
#include "runs_device.hpp"

namespace cph {

constexpr int kJtThreads = 256;
constexpr int kJtRows = 4;                          // rows per lane and tile, strided by the workgroup: coalesced 4 / 8-byte loads
constexpr int kJtTile = kJtThreads * kJtRows;       // 1024: tests/test_join_totals.py calls it T
constexpr int kJtLdsGroups = CPH_CHAIN_AGG_LDS_GROUPS;
constexpr uint64_t kJtSortRows = 1ull << 20;        // joined rows from which a table above the LDS limit is reduced over sorted runs
enum { kJtAdd = 0, kJtMin = 1, kJtMax = 2 };
enum { kJtOne = 0, kJtRaw = 1, kJtIntKey = 2, kJtFltKey = 3 };   // what a row contributes: 1 | its 8 bytes | an ordered key of them

constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr uint64_t kGoNaN = 0x7FF8000000000001ull;

struct JtFlags {     // what the call waits for once (ErrReport)
    ErrWord err;     // first
    uint32_t bad;    // a build_row outside the index
    uint32_t pad_;
};

template <int OP>
__host__ __device__ constexpr uint64_t jt_identity() { return OP == kJtMin ? ~0ull : 0ull; }

template <int OP, int ENC>
__device__ __forceinline__ uint64_t jt_encode(uint64_t bits) {
    if constexpr (ENC == kJtOne) return 1ull;
    else if constexpr (ENC == kJtRaw) return bits;
    else if constexpr (ENC == kJtIntKey) return bits ^ kSign;
    else {
        if ((bits & ~kSign) > 0x7FF0000000000000ull) return OP == kJtMin ? 0ull : ~0ull;   // NaN: the op's winning key
        return (bits & kSign) ? ~bits : bits | kSign;
    }
}
template <int OP>
__device__ __forceinline__ uint64_t jt_join(uint64_t a, uint64_t b) {
    if constexpr (OP == kJtAdd) return a + b;
    else if constexpr (OP == kJtMin) return a < b ? a : b;
    else return a > b ? a : b;
}
template <int OP>
__device__ __forceinline__ void jt_atomic(uint64_t* p, uint64_t v) {   // LDS or global (device scope); no return value used
    unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
    if constexpr (OP == kJtAdd) (void)atomicAdd(q, (unsigned long long)v);
    else if constexpr (OP == kJtMin) (void)atomicMin(q, (unsigned long long)v);
    else (void)atomicMax(q, (unsigned long long)v);
}

__global__ __launch_bounds__(kJtThreads) void k_jt_fill(uint64_t* __restrict__ p, uint64_t n, uint64_t v) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kJtThreads + threadIdx.x; i < n; i += stride) p[i] = v;
}

// table[g] (pre-filled with the op's identity) joined with the contribution of every row m < n with rows[m] == g.  A row whose
// group is not below ngroups is left out and raises *bad (the chain does not belong to this index).
template <int OP, int ENC, bool LDS>
__global__ __launch_bounds__(kJtThreads) void k_jt_direct(const uint32_t* __restrict__ rows, const uint64_t* __restrict__ vals, uint64_t n,
                                                         uint32_t ngroups, uint64_t* __restrict__ table, uint32_t* __restrict__ bad) {
    __shared__ uint64_t s_tab[LDS ? kJtLdsGroups : 1];
    constexpr uint64_t ident = jt_identity<OP>();
    if constexpr (LDS) {
        for (uint32_t g = threadIdx.x; g < ngroups; g += kJtThreads) s_tab[g] = ident;   // ngroups <= kJtLdsGroups (host)
        __syncthreads();
    }
    uint64_t* tab = LDS ? s_tab : table;
    const uint64_t ntiles = (n + kJtTile - 1) / kJtTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * kJtTile + threadIdx.x;
        uint32_t g[kJtRows];
        uint64_t v[kJtRows];
        bool live[kJtRows];
#pragma unroll
        for (int k = 0; k < kJtRows; k++) {
            const uint64_t m = base + (uint64_t)k * kJtThreads;
            live[k] = m < n;
            g[k] = live[k] ? rows[m] : 0u;
            v[k] = ident;
            if constexpr (ENC != kJtOne) {
                if (live[k]) v[k] = jt_encode<OP, ENC>(vals[m]);
            } else if (live[k]) v[k] = 1ull;
        }
#pragma unroll
        for (int k = 0; k < kJtRows; k++) {
            if (live[k] && g[k] >= ngroups) {
                live[k] = false;
                *bad = 1u;
            }
            const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g[k]);
            if (__all(live[k] && g[k] == g0)) {   // wave-uniform: the whole wave hits one group -> one atomic
                uint64_t x = v[k];
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) x = jt_join<OP>(x, (uint64_t)__shfl_xor((unsigned long long)x, d, kWave));
                if (lane_id() == 0) jt_atomic<OP>(tab + g0, x);
            } else if (live[k]) {
                jt_atomic<OP>(tab + g[k], v[k]);
            }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < ngroups; i += kJtThreads) {
            const uint64_t x = s_tab[i];
            if (x != ident) jt_atomic<OP>(table + i, x);   // a group this workgroup never touched (or touched without effect) is skipped
        }
    }
}

// Min / Max keys back to the 8 bytes of the value; 0 / +0.0 for a group without rows.
template <bool FLT, int OP>
__global__ __launch_bounds__(kJtThreads) void k_jt_decode(uint64_t* __restrict__ table, const uint64_t* __restrict__ count, uint64_t ngroups) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    for (uint64_t g = (uint64_t)blockIdx.x * kJtThreads + threadIdx.x; g < ngroups; g += stride) {
        const uint64_t key = table[g];
        uint64_t out;
        if (count[g] == 0) out = 0;
        else if constexpr (!FLT) out = key ^ kSign;
        else if (key == (OP == kJtMin ? 0ull : ~0ull)) out = kGoNaN;
        else out = (key & kSign) ? key ^ kSign : ~key;
        table[g] = out;
    }
}

// The status bytes != 0 into *err: their number, and the lowest row, there the lowest spec (the specs run one after the other, all
// through this word), and its kind.
__global__ __launch_bounds__(kJtThreads) void k_jt_errors(const uint8_t* __restrict__ status, uint64_t n, uint32_t spec, ErrWord* __restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    const uint64_t rounds = (n + stride - 1) / stride;
    WaveErr we;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t m = r * stride + (uint64_t)blockIdx.x * kJtThreads + threadIdx.x;
        const uint32_t s = m < n ? status[m] : 0u;
        if (s) we.note_lane(m, spec, s);
    }
    we.reduce();
    we.flush(err);
}

// keys[m] = rows[m] clamped below ngroups (a row outside raises *bad): what the sort route sorts, so that its runs stay <= ngroups
__global__ __launch_bounds__(kJtThreads) void k_jt_keys(const uint32_t* __restrict__ rows, uint64_t n, uint32_t ngroups, uint32_t* __restrict__ keys,
                                                       uint32_t* __restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    for (uint64_t m = (uint64_t)blockIdx.x * kJtThreads + threadIdx.x; m < n; m += stride) {
        uint32_t g = rows[m];
        if (g >= ngroups) {
            g = ngroups - 1;
            *bad = 1u;
        }
        keys[m] = g;
    }
}

// values[key of run r] = sums[r] for the *nruns runs of the sorted keys; run_key[r] < ngroups (k_jt_keys)
__global__ __launch_bounds__(kJtThreads) void k_jt_scatter(const uint64_t* __restrict__ sums, const uint32_t* __restrict__ run_key,
                                                          const uint32_t* __restrict__ nruns, uint64_t max_runs, uint32_t ngroups,
                                                          uint64_t* __restrict__ values) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    uint64_t nr = *nruns;
    if (nr > max_runs) nr = max_runs;
    for (uint64_t r = (uint64_t)blockIdx.x * kJtThreads + threadIdx.x; r < nr; r += stride) {
        const uint32_t g = run_key[r];
        if (g < ngroups) values[g] = sums[r];
    }
}

// count[key of run r] = the run's length: the distance to the next run start (n behind the last run)
__global__ __launch_bounds__(kJtThreads) void k_jt_run_counts(const uint64_t* __restrict__ run_pos, const uint32_t* __restrict__ run_key,
                                                             const uint32_t* __restrict__ nruns, uint64_t max_runs, uint64_t n, uint32_t ngroups,
                                                             uint64_t* __restrict__ count) {
    const uint64_t stride = (uint64_t)gridDim.x * kJtThreads;
    uint64_t nr = *nruns;
    if (nr > max_runs) nr = max_runs;
    for (uint64_t r = (uint64_t)blockIdx.x * kJtThreads + threadIdx.x; r < nr; r += stride) {
        const uint32_t g = run_key[r];
        if (g < ngroups) count[g] = (r + 1 < nr ? run_pos[r + 1] : n) - run_pos[r];
    }
}

}  // namespace cph

using namespace cph;

struct cph_chain_aggregated_impl {
    cph_chain_aggregated pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_cnt, d_val[CPH_AGG_MAX_SPECS];
};

namespace {

unsigned jt_grid(uint64_t n) {
    const uint64_t ntiles = (n + kJtTile - 1) / kJtTile;
    return (unsigned)(ntiles < 2048 ? (ntiles ? ntiles : 1) : 2048);
}

template <int OP, int ENC>
void launch_direct(cph_ctx* ctx, const char* name, const uint32_t* rows, const uint64_t* vals, uint64_t n, uint32_t ngroups, uint64_t* table,
                   uint32_t* bad) {
    {
        ProfScope ps(ctx, "k_jt_fill", 8.0 * (double)ngroups);
        hipLaunchKernelGGL(k_jt_fill, dim3(grid_for_items(ngroups)), dim3(kJtThreads), 0, ctx->stream, table, (uint64_t)ngroups, jt_identity<OP>());
    }
    if (!n) return;
    ProfScope ps(ctx, name, (double)n * (ENC == kJtOne ? 4.0 : 12.0) + 8.0 * (double)ngroups);
    if (ngroups <= (uint32_t)kJtLdsGroups)
        hipLaunchKernelGGL((k_jt_direct<OP, ENC, true>), dim3(jt_grid(n)), dim3(kJtThreads), 0, ctx->stream, rows, vals, n, ngroups, table, bad);
    else
        hipLaunchKernelGGL((k_jt_direct<OP, ENC, false>), dim3(jt_grid(n)), dim3(kJtThreads), 0, ctx->stream, rows, vals, n, ngroups, table, bad);
}

template <bool FLT, int OP>
void launch_decode(cph_ctx* ctx, uint64_t* table, const uint64_t* count, uint64_t ngroups) {
    ProfScope ps(ctx, "k_jt_decode", 24.0 * (double)ngroups);
    hipLaunchKernelGGL((k_jt_decode<FLT, OP>), dim3(grid_for_items(ngroups)), dim3(kJtThreads), 0, ctx->stream, table, count, ngroups);
}

// one order-independent spec: fill, accumulate, decode
void run_direct_spec(cph_ctx* ctx, int32_t op, bool flt, const uint32_t* rows, const uint64_t* vals, uint64_t n, uint32_t ng, uint64_t* table,
                     const uint64_t* count, uint32_t* bad) {
    if (op == CPH_AGG_SUM) {   // int only: the caller sends float sums down the sort route
        launch_direct<kJtAdd, kJtRaw>(ctx, "k_jt_direct_sum", rows, vals, n, ng, table, bad);
    } else if (op == CPH_AGG_MIN) {
        if (flt) launch_direct<kJtMin, kJtFltKey>(ctx, "k_jt_direct_min", rows, vals, n, ng, table, bad);
        else launch_direct<kJtMin, kJtIntKey>(ctx, "k_jt_direct_min", rows, vals, n, ng, table, bad);
        if (flt) launch_decode<true, kJtMin>(ctx, table, count, ng);
        else launch_decode<false, kJtMin>(ctx, table, count, ng);
    } else {
        if (flt) launch_direct<kJtMax, kJtFltKey>(ctx, "k_jt_direct_max", rows, vals, n, ng, table, bad);
        else launch_direct<kJtMax, kJtIntKey>(ctx, "k_jt_direct_max", rows, vals, n, ng, table, bad);
        if (flt) launch_decode<true, kJtMax>(ctx, table, count, ng);
        else launch_decode<false, kJtMax>(ctx, table, count, ng);
    }
}

int bits_for(uint64_t max_value) {
    int b = 0;
    while (max_value) {
        b++;
        max_value >>= 1;
    }
    return b;
}

// what the float Sum specs of one call share: the joined rows sorted by group, the run starts, the key of every run
struct SortedRuns {
    DevBuf ka, kb, va, vb, run_pos, run_key, partials, sums;
    TileBitmap starts;                           // the run starts over the sorted keys
    uint32_t *keys = nullptr, *rows = nullptr;   // sorted group per position, joined row m per position
    uint64_t max_runs = 0;
};

Status sort_runs(cph_ctx* ctx, const uint32_t* build_rows, uint64_t n, uint32_t ng, uint32_t* bad, SortedRuns* sr) {
    CPH_TRY(sr->ka.alloc(&ctx->pool, n * sizeof(uint32_t)));
    CPH_TRY(sr->kb.alloc(&ctx->pool, n * sizeof(uint32_t)));
    CPH_TRY(sr->va.alloc(&ctx->pool, n * sizeof(uint32_t)));
    CPH_TRY(sr->vb.alloc(&ctx->pool, n * sizeof(uint32_t)));
    {
        ProfScope ps(ctx, "k_jt_keys", 8.0 * (double)n);
        hipLaunchKernelGGL(k_jt_keys, dim3(grid_for_items(n)), dim3(kJtThreads), 0, ctx->stream, build_rows, n, ng, sr->ka.as<uint32_t>(), bad);
    }
    CPH_HIP_TRY(hipGetLastError());
    int passes = 0;
    CPH_TRY(radix_sort_pairs<uint32_t>(ctx, sr->ka.as<uint32_t>(), sr->kb.as<uint32_t>(), sr->va.as<uint32_t>(), sr->vb.as<uint32_t>(), true, n,
                                       bits_for((uint64_t)ng - 1), &sr->keys, &sr->rows, &passes));
    sr->max_runs = std::min<uint64_t>(n, ng);
    CPH_TRY(sr->starts.alloc(ctx, n));
    agg_launch_heads(ctx, sr->keys, true, 1, n, 4.0, sr->starts.words(), sr->starts.counts());
    CPH_HIP_TRY(hipGetLastError());
    CPH_TRY(sr->starts.scan(ctx));
    // the keys are below ng and sorted, so there are at most min(n, ng) runs: no host trip for the count
    CPH_TRY(sr->run_pos.alloc(&ctx->pool, sr->max_runs * sizeof(uint64_t)));
    CPH_TRY(sr->run_key.alloc(&ctx->pool, sr->max_runs * sizeof(uint32_t)));
    agg_launch_emit(ctx, sr->starts.words(), sr->starts.counts(), sr->keys, n, sr->max_runs, sr->run_pos.as<uint64_t>(),
                    sr->run_key.as<uint32_t>());   // "perm" = the sorted keys: first_row[r] = the key of run r
    CPH_HIP_TRY(hipGetLastError());
    CPH_TRY(sr->partials.alloc(&ctx->pool, 2 * sr->starts.ntiles * sizeof(uint64_t)));
    CPH_TRY(sr->sums.alloc(&ctx->pool, sr->max_runs * sizeof(uint64_t)));
    return {};
}

Status check_args(const cph_chain* chain, int32_t step, const cph_index* ix, const cph_chain_agg_spec* specs, int32_t nspecs, int32_t out_mem) {
    if (!chain) return {CPH_ERR_INVALID, "cph_chain_aggregate: chain must not be NULL"};
    if (!ix) return {CPH_ERR_INVALID, "cph_chain_aggregate: index must not be NULL"};
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, "cph_chain_aggregate: bad out_mem"};
    if (chain->mem != CPH_MEM_HOST && chain->mem != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, "cph_chain_aggregate: bad chain->mem"};
    if (step < 0 || step >= chain->nsteps || step >= CPH_MAX_CHAIN)
        return {CPH_ERR_INVALID, "cph_chain_aggregate: step must be 0..chain->nsteps-1"};
    if (chain->nrows >= (1ull << 32)) return {CPH_ERR_INVALID, "cph_chain_aggregate: chain->nrows must be below 2^32"};
    if (chain->nrows && !chain->build_row[step]) return {CPH_ERR_INVALID, "cph_chain_aggregate: the chain has no build_row for this step"};
    if (!chain->positions && ix->table_rows != ix->nrows)
        return {CPH_ERR_INVALID, "cph_chain_aggregate: an index over a subset of its table needs a chain made with CPH_CHAIN_POSITIONS"};
    if (chain->nrows && !ix->nrows) return {CPH_ERR_INVALID, "cph_chain_aggregate: the index has fewer rows than the chain step's index"};
    if (nspecs < 0 || nspecs > CPH_AGG_MAX_SPECS) return {CPH_ERR_INVALID, "cph_chain_aggregate: nspecs must be 0..CPH_AGG_MAX_SPECS"};
    if (nspecs && !specs) return {CPH_ERR_INVALID, "cph_chain_aggregate: specs is NULL"};
    for (int32_t s = 0; s < nspecs; s++) {
        const cph_chain_agg_spec& sp = specs[s];
        if (sp.op != CPH_AGG_SUM && sp.op != CPH_AGG_MIN && sp.op != CPH_AGG_MAX)
            return {CPH_ERR_INVALID, "cph_chain_aggregate: unknown op (CPH_AGG_SUM, CPH_AGG_MIN or CPH_AGG_MAX)"};
        if (sp.kind != CPH_NUM_INT64 && sp.kind != CPH_NUM_FLOAT64)
            return {CPH_ERR_INVALID, "cph_chain_aggregate: kind must be CPH_NUM_INT64 or CPH_NUM_FLOAT64"};
        if (sp.numbers_mem != CPH_MEM_HOST && sp.numbers_mem != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, "cph_chain_aggregate: bad numbers_mem"};
        if (!sp.numbers) return {CPH_ERR_INVALID, "cph_chain_aggregate: numbers must not be NULL"};
    }
    return {};
}

}  // namespace

extern "C" {

CPH_API int32_t cph_chain_aggregate(cph_ctx* ctx, const cph_chain* chain, int32_t step, const cph_index* ix, const cph_chain_agg_spec* specs,
                                    int32_t nspecs, int32_t out_mem, cph_chain_aggregated** out) {
    if (!ctx || !out) return fail_with(ctx, {CPH_ERR_INVALID, "cph_chain_aggregate: ctx and out must not be NULL"});
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    {
        const Status s = check_args(chain, step, ix, specs, nspecs, out_mem);
        if (!s.ok()) return fail_with(ctx, s);
    }
    auto* r = new (std::nothrow) cph_chain_aggregated_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.mem = out_mem;
    r->pub.nspecs = nspecs;
    r->pub.positions = chain->positions;
    r->pub.first_error_row = UINT64_MAX;
    auto run = [&]() -> Status {
        const uint64_t n = chain->nrows;
        const uint64_t ng64 = ix->nrows;
        if (ng64 >= (1ull << 32)) return {CPH_ERR_INVALID, "cph_chain_aggregate: the index has 2^32 rows or more"};
        const uint32_t ng = (uint32_t)ng64;
        if (!ng) return {};   // no build rows, hence no joined rows: no groups, every array stays NULL
        // everything the kernels read, on the device
        DevBuf up_rows, up_vals[CPH_AGG_MAX_SPECS], up_status[CPH_AGG_MAX_SPECS];
        const uint32_t* rows = chain->build_row[step];
        const uint64_t* vals[CPH_AGG_MAX_SPECS] = {nullptr};
        const uint8_t* status[CPH_AGG_MAX_SPECS] = {nullptr};
        CPH_TRY(device_array(ctx, chain->build_row[step], chain->mem, (size_t)n, &up_rows, &rows));
        for (int32_t s = 0; s < nspecs; s++) {   // a spec's status bytes lie where its numbers lie
            const cph_chain_agg_spec& sp = specs[s];
            CPH_TRY(device_array(ctx, static_cast<const uint64_t*>(sp.numbers), sp.numbers_mem, (size_t)n, &up_vals[s], &vals[s]));
            CPH_TRY(device_array(ctx, sp.status, sp.numbers_mem, sp.status ? (size_t)n : 0, &up_status[s], &status[s]));
        }
        ErrReport<JtFlags> flags;
        CPH_TRY(flags.init(ctx));
        uint32_t* d_bad = &flags.counters()->bad;
        for (int32_t s = 0; s < nspecs && n; s++) {
            if (!status[s]) continue;
            ProfScope ps(ctx, "k_jt_errors", (double)n);
            hipLaunchKernelGGL(k_jt_errors, dim3(grid_for_items(n, 2048)), dim3(kJtThreads), 0, ctx->stream, status[s], n, (uint32_t)s, flags.word());
            CPH_HIP_TRY(hipGetLastError());
        }
        bool has_fsum = false;
        for (int32_t s = 0; s < nspecs; s++) has_fsum |= specs[s].kind == CPH_NUM_FLOAT64 && specs[s].op == CPH_AGG_SUM;
        const bool by_runs = n && ng > (uint32_t)kJtLdsGroups && (has_fsum || n >= kJtSortRows);   // see the head of the file
        SortedRuns sr;
        bool sorted = false;
        if (by_runs) {
            CPH_TRY(sort_runs(ctx, rows, n, ng, d_bad, &sr));
            sorted = true;
        }
        auto fill = [&](uint64_t* table, uint64_t v) -> Status {
            ProfScope ps(ctx, "k_jt_fill", 8.0 * (double)ng);
            hipLaunchKernelGGL(k_jt_fill, dim3(grid_for_items(ng)), dim3(kJtThreads), 0, ctx->stream, table, (uint64_t)ng, v);
            CPH_HIP_TRY(hipGetLastError());
            return {};
        };
        // one spec over the sorted runs: the segmented reduce with the sorted m as gather permutation, each run's value to its group
        auto reduce_runs = [&](int32_t op, bool flt, const uint64_t* v, uint64_t* table) -> Status {
            const AggReduceArgs a{sr.starts.words(), sr.starts.counts(), v, sr.rows, n, sr.starts.ntiles, sr.sums.as<uint64_t>(),
                                  sr.partials.as<uint64_t>(), sr.partials.as<uint64_t>() + sr.starts.ntiles};
            agg_launch_reduce(ctx, op, flt, true, a);
            CPH_HIP_TRY(hipGetLastError());
            ProfScope ps(ctx, "k_jt_scatter", 20.0 * (double)sr.max_runs);
            hipLaunchKernelGGL(k_jt_scatter, dim3(grid_for_items(sr.max_runs)), dim3(kJtThreads), 0, ctx->stream, sr.sums.as<uint64_t>(),
                               sr.run_key.as<uint32_t>(), sr.starts.total(), sr.max_runs, ng, table);
            CPH_HIP_TRY(hipGetLastError());
            return {};
        };
        // Count: every route's "is the group empty"
        CPH_TRY(r->d_cnt.alloc(&ctx->pool, (size_t)ng * sizeof(uint64_t)));
        uint64_t* count = r->d_cnt.as<uint64_t>();
        if (by_runs) {
            CPH_TRY(fill(count, 0ull));
            ProfScope ps(ctx, "k_jt_run_counts", 20.0 * (double)sr.max_runs);
            hipLaunchKernelGGL(k_jt_run_counts, dim3(grid_for_items(sr.max_runs)), dim3(kJtThreads), 0, ctx->stream, sr.run_pos.as<uint64_t>(),
                               sr.run_key.as<uint32_t>(), sr.starts.total(), sr.max_runs, n, ng, count);
        } else {
            launch_direct<kJtAdd, kJtOne>(ctx, "k_jt_direct_count", rows, nullptr, n, ng, count, d_bad);
        }
        CPH_HIP_TRY(hipGetLastError());
        for (int32_t s = 0; s < nspecs; s++) {
            CPH_TRY(r->d_val[s].alloc(&ctx->pool, (size_t)ng * sizeof(uint64_t)));
            uint64_t* table = r->d_val[s].as<uint64_t>();
            const bool flt = specs[s].kind == CPH_NUM_FLOAT64;
            const bool fsum = flt && specs[s].op == CPH_AGG_SUM;
            if (!by_runs && !fsum) {
                run_direct_spec(ctx, specs[s].op, flt, rows, vals[s], n, ng, table, count, d_bad);
                CPH_HIP_TRY(hipGetLastError());
                continue;
            }
            CPH_TRY(fill(table, 0ull));   // 0 / +0.0 for the groups without rows
            if (!n) continue;
            if (!sorted) {
                CPH_TRY(sort_runs(ctx, rows, n, ng, d_bad, &sr));
                sorted = true;
            }
            CPH_TRY(reduce_runs(specs[s].op, flt, vals[s], table));
        }
        // the call's host wait
        JtFlags got{};
        ErrFirst e;
        CPH_TRY(flags.read(ctx, &e, &got));
        if (got.bad)
            return {CPH_ERR_INVALID, "cph_chain_aggregate: a build_row of the chain is not below the index's row count (not the chain step's index?)"};
        if (e.nerrors) {   // data, not a failure: no arrays
            r->pub.nerrors = e.nerrors;
            r->pub.first_error_row = e.row;
            r->pub.first_error_spec = e.tag;
            r->pub.first_error_kind = e.kind;
            r->d_cnt.reset();
            for (int32_t s = 0; s < nspecs; s++) r->d_val[s].reset();
            return {};
        }
        r->pub.ngroups = ng;
        ResultPart parts[1 + CPH_AGG_MAX_SPECS];
        parts[0] = ResultPart{&r->d_cnt, (size_t)ng * sizeof(uint64_t), &r->pub.count};
        for (int32_t s = 0; s < nspecs; s++) parts[1 + s] = ResultPart{&r->d_val[s], (size_t)ng * sizeof(uint64_t), &r->pub.values[s]};
        return deliver(ctx, &r->own, parts, 1 + nspecs, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API void cph_chain_aggregated_release(cph_chain_aggregated* pub) { release_result<cph_chain_aggregated_impl>(pub); }

}  // extern "C"

namespace cph {
void warm_join_totals() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_jt_fill));
    (void)hipGetLastError();
}
}  // namespace cph
