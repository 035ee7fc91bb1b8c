// order.hip — OrderBy: the rows of a selection in the order of up to CPH_ORDER_MAX_KEYS typed keys (cph_order_rows), the
// statement being Go's slices.SortStableFunc over cmp.Compare per key (include/csvplus_hip.h).  Every key becomes an unsigned
// integer of the same order, and the stable LSD radix sort of the index build (radix_sort.hip) does the rest:
//
//   k_order_key_i64 / _f64   one pass per number key: value -> order_key64 (order_device.hpp) by selection position; the rows
//                            whose status byte is not OK are counted and the lowest (row, key) is kept (the report of
//                            num_report.hpp, tag = the key).
//   k_order_key_rank         a BYTES key: the index's run starts (k_agg_heads, aggregate.hip) and their scan give every sorted
//                            position the DENSE RANK of its run (the reverse lookup of tile_bitmap.hpp); key[perm[p]] = rank
//                            (ngroups - 1 - rank when descending):
//                            32 bits, of which the sort looks at bit_length(ngroups - 1).
//   sort                     least significant key first: k_order_gather reads the key through the current order, then
//                            radix_sort_pairs<uint64_t / uint32_t> over (key, row id).  The first sort of a call without
//                            candidates reads the key array itself (row ids = iota).
//
// Top-N select (limit given, skip + limit <= nrows / kSelectGate, option order_select): only rows whose FIRST key is at or
// below the key of ascending rank skip + limit - 1 can reach the result, whatever the later keys say.
//   k_order_select_hist      MSD radix select over key 0, 8 bits per pass: counts the digit of the rows that match the prefix
//                            chosen so far.  16 bytes per lane and load, LDS counters per wave, one flush per workgroup.
//   k_order_select_pick      one workgroup: scans the 256 counters, picks the bin that holds the wanted rank, leaves the longer
//                            prefix and the rank inside the bin in device memory for the next pass.  No host wait in between.
//   k_order_select_flag      bitmap of the rows with key 0 <= threshold (every tie at the threshold included) + counts per tile
//                            (tile_bitmap.hpp: the layout, the tile store)
//   k_order_select_emit      its rank walker: bitmap -> candidate row ids in input order (scan of the tile counts in between)
// The host reads the candidate count once (allocation and sort plan need it); the multi-key sort then runs over the candidates.
#include <algorithm>
#include <cstring>
#include <new>

#include "num_report.hpp"
#include "order_device.hpp"
#include "runs_device.hpp"

namespace cph {

// skip + limit <= nrows / kSelectGate takes the select route.  Measured (profiles/order_rows.txt, one int64 key): the select wins
// at every recorded k — by 4x at k = 10 and still by 1.3x (1e7 rows) / 1.9x (1e8 rows) at k = nrows / 4; at nrows / 2 the
// two routes are 5 % apart at 1e7 rows, so they cross just above it.  4 leaves room for what a call with more keys adds to
// the candidates' side (one gather per key), which was not recorded.
constexpr uint64_t kSelectGate = 4;

struct SelectState {              // device: what one select pass leaves for the next
    unsigned long long prefix;    // the threshold's digits chosen so far (lower bits 0)
    unsigned long long rank;      // wanted ascending rank among the rows that match the prefix
};

template <bool FLT>
__global__ __launch_bounds__(kMatThreads) void k_order_key_num(const uint64_t* __restrict__ values, const uint8_t* __restrict__ status, uint64_t n,
                                                              uint32_t descending, uint32_t key_index, uint64_t* __restrict__ out,
                                                              ErrWord* __restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    WaveErr we;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        out[i] = order_key64(values[i], FLT, descending != 0);
        if (status) {
            const uint32_t st = status[i];
            if (st != CPH_NUM_OK) we.note_lane(i, key_index, st);
        }
    }
    if (status) {   // uniform
        we.reduce();
        we.flush(err);
    }
}

// bitmap / offs: the index's run starts and their scan (agg_launch_heads; offs[ntiles] = the number of runs).  Row perm[p] gets
// the dense rank of p's run.  nout = rows of `out`: a perm value at or beyond it (a malformed index) is not written.
__global__ __launch_bounds__(kMatThreads) void k_order_key_rank(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs,
                                                               const uint32_t* __restrict__ perm, uint64_t n, uint64_t nout,
                                                               uint32_t descending, uint32_t* __restrict__ out) {
    __shared__ uint64_t s_word[kResWords];
    __shared__ uint32_t s_pre[kResWords];
    const uint64_t ntiles = tile_count(n);
    const uint32_t top = offs[ntiles] - 1u;   // ngroups - 1 (n >= 1 has a run)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        tile_load_words(bitmap, tile, s_word, s_pre);
        const uint32_t r0 = threadIdx.x * kResRows;
        const uint64_t base = tile * kResTile + r0;
        uint32_t starts, before;
        tile_lane_bits(s_word, s_pre, r0, &starts, &before);
        const uint32_t o0 = offs[tile];
#pragma unroll
        for (int k = 0; k < kResRows; k++) {
            const uint64_t pos = base + (uint64_t)k;
            if (pos < n) {
                // run starts at or in front of the row: at least one (position 0 starts a run)
                const uint32_t rank = o0 + before + (uint32_t)__popc(starts & ((2u << k) - 1u)) - 1u;
                const uint32_t row = perm[pos];
                if ((uint64_t)row < nout) out[row] = descending ? top - rank : rank;
            }
        }
        __syncthreads();
    }
}

template <class K>
__global__ __launch_bounds__(kMatThreads) void k_order_gather(const K* __restrict__ src, const uint32_t* __restrict__ ids, K* __restrict__ dst, uint64_t m) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < m; i += stride) dst[i] = src[ids[i]];
}

// ---- Top-N select ------------------------------------------------------------------------------------------------------------
template <class K> struct KeyVec;
template <> struct KeyVec<uint64_t> {
    static constexpr int N = 2;
    typedef ulonglong2 V;
    __device__ static __forceinline__ void unpack(const V& v, uint64_t* k) { k[0] = v.x; k[1] = v.y; }
};
template <> struct KeyVec<uint32_t> {
    static constexpr int N = 4;
    typedef uint4 V;
    __device__ static __forceinline__ void unpack(const V& v, uint32_t* k) { k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w; }
};

// hist[d] += rows whose key matches st->prefix above bit shift + 8 (every row when `top`) and has digit d at `shift`.
// `keys` is 16-byte aligned (a pool block).
template <class K>
__global__ __launch_bounds__(kMatThreads) void k_order_select_hist(const K* __restrict__ keys, uint64_t n, int shift, int top,
                                                                  const SelectState* __restrict__ st, uint32_t* __restrict__ hist) {
    constexpr int NV = KeyVec<K>::N;
    constexpr int kWaves = kMatThreads / kWave;
    __shared__ uint32_t s_hist[kWaves][256];
    for (int i = threadIdx.x; i < kWaves * 256; i += kMatThreads) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    const uint64_t prefix = top ? 0ull : st->prefix;
    const int up = top ? 0 : shift + 8;   // top: nothing above the digit is compared (and shift + 8 may be the key's width)
    const int w = wave_id();
    const uint64_t nvec = n / NV;
    const typename KeyVec<K>::V* vp = reinterpret_cast<const typename KeyVec<K>::V*>(keys);
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t v = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; v < nvec; v += stride) {
        K k[NV];
        KeyVec<K>::unpack(vp[v], k);
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const uint64_t key = (uint64_t)k[j];
            if (top || ((key ^ prefix) >> up) == 0) atomicAdd(&s_hist[w][(uint32_t)(key >> shift) & 0xFFu], 1u);
        }
    }
    if (blockIdx.x == 0) {   // the rows behind the last whole vector
        const uint64_t i = nvec * NV + threadIdx.x;
        if (threadIdx.x < NV && i < n) {
            const uint64_t key = (uint64_t)keys[i];
            if (top || ((key ^ prefix) >> up) == 0) atomicAdd(&s_hist[w][(uint32_t)(key >> shift) & 0xFFu], 1u);
        }
    }
    lds_atomics_barrier();
    uint32_t c = 0;
#pragma unroll
    for (int ww = 0; ww < kWaves; ww++) c += s_hist[ww][threadIdx.x];   // kMatThreads == 256 digits
    if (c) atomicAdd(&hist[threadIdx.x], c);
}
static_assert(kMatThreads == 256, "one thread per digit in k_order_select_hist / k_order_select_pick");

// One workgroup: the bin that holds the wanted rank.  Exactly one thread finds it (the counters sum to more than the rank).
__global__ __launch_bounds__(kMatThreads) void k_order_select_pick(const uint32_t* __restrict__ hist, int shift, SelectState* __restrict__ st) {
    __shared__ uint32_t s_tmp[kMatThreads / kWave + 1];
    const unsigned long long rank = st->rank, prefix = st->prefix;   // read by everyone in front of the barriers below
    const uint32_t c = hist[threadIdx.x];
    uint32_t total;
    const uint32_t excl = block_exclusive_sum<uint32_t, kMatThreads>(c, s_tmp, &total);
    if (c && rank >= (unsigned long long)excl && rank - (unsigned long long)excl < (unsigned long long)c) {
        st->prefix = prefix | ((unsigned long long)threadIdx.x << shift);
        st->rank = rank - (unsigned long long)excl;
    }
}

// bit = that row has key <= st->prefix (tile_bitmap.hpp)
template <class K>
__global__ __launch_bounds__(kMatThreads) void k_order_select_flag(const K* __restrict__ keys, uint64_t n, const SelectState* __restrict__ st,
                                                                  uint64_t* __restrict__ bitmap, uint32_t* __restrict__ counts) {
    constexpr int NV = KeyVec<K>::N;
    __shared__ uint64_t s_word[kResWords];
    uint8_t* s_byte = reinterpret_cast<uint8_t*>(s_word);   // kResRows == 8: one byte per lane
    const uint64_t ntiles = tile_count(n);
    const uint64_t thr = st->prefix;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * kResTile + (uint64_t)threadIdx.x * kResRows;
        uint32_t flags = 0;
        if (base + kResRows <= n) {   // base is a multiple of 8 keys: 16-byte aligned
            const typename KeyVec<K>::V* vp = reinterpret_cast<const typename KeyVec<K>::V*>(keys + base);
#pragma unroll
            for (int v = 0; v < kResRows / NV; v++) {
                K k[NV];
                KeyVec<K>::unpack(vp[v], k);
#pragma unroll
                for (int j = 0; j < NV; j++) flags |= ((uint64_t)k[j] <= thr ? 1u : 0u) << (v * NV + j);
            }
        } else {
            for (int j = 0; j < kResRows; j++)
                if (base + (uint64_t)j < n) flags |= ((uint64_t)keys[base + (uint64_t)j] <= thr ? 1u : 0u) << j;
        }
        s_byte[threadIdx.x] = (uint8_t)flags;
        tile_store_words(s_word, tile, bitmap, counts);
    }
}

// offs[tile] = set bits in front of the tile; cand[rank] = the row of the rank-th set bit: the candidates in input order
__global__ __launch_bounds__(kMatThreads) void k_order_select_emit(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs, uint64_t ntiles,
                                                                  uint64_t ncand, uint32_t* __restrict__ cand) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t o0 = offs[tile], o1 = offs[tile + 1];
        if (o0 == o1) continue;   // uniform
        tile_for_each_set(bitmap, tile, o0, [&](uint64_t rank, int r) {
            if (rank < ncand) cand[rank] = (uint32_t)(tile * kResTile + (uint64_t)r);
        });
    }
}

}  // namespace cph

using namespace cph;

// the library-owned result behind cph_ordered
struct cph_ordered_impl {
    cph_ordered pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_ids;
};

namespace {

struct DevKey {           // one key on the device, by selection position
    DevBuf buf;           // uint64_t[n] (numbers) or uint32_t[n] (rank of a BYTES key)
    bool wide = true;     // 64-bit
    int bits = 64;        // key bits the sort looks at
};

int bit_length(uint64_t v) {
    int b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

Status check_keys(const cph_order_key* keys, int32_t nkeys, uint64_t nrows) {
    if (!keys) return {CPH_ERR_INVALID, "cph_order_rows: keys is NULL"};
    if (nkeys < 1 || nkeys > CPH_ORDER_MAX_KEYS) return {CPH_ERR_INVALID, "cph_order_rows: nkeys must be 1..CPH_ORDER_MAX_KEYS"};
    for (int32_t k = 0; k < nkeys; k++) {
        const cph_order_key& key = keys[k];
        if (key.kind == CPH_NUM_INT64 || key.kind == CPH_NUM_FLOAT64) {
            if (key.values_mem != CPH_MEM_HOST && key.values_mem != CPH_MEM_DEVICE) return {CPH_ERR_INVALID, "cph_order_rows: bad values_mem"};
            if (!key.values && nrows) return {CPH_ERR_INVALID, "cph_order_rows: a number key needs values"};
        } else if (key.kind == CPH_ORDER_BYTES) {
            if (!key.index) return {CPH_ERR_INVALID, "cph_order_rows: a CPH_ORDER_BYTES key needs an index"};
            if (key.index->nrows != nrows || key.index->table_rows != nrows)
                return {CPH_ERR_INVALID, "cph_order_rows: the index of a CPH_ORDER_BYTES key has another row count than the rows being ordered"};
        } else {
            return {CPH_ERR_INVALID, "cph_order_rows: kind must be CPH_NUM_INT64, CPH_NUM_FLOAT64 or CPH_ORDER_BYTES"};
        }
    }
    return {};
}

// A number key: values (and status) made device resident, mapped into dk->buf.
Status key_pass_number(cph_ctx* ctx, const cph_order_key& key, int32_t k, uint64_t n, DevKey* dk, ErrWord* d_err) {
    DevBuf up_values, up_status;
    const uint64_t* values = nullptr;
    const uint8_t* status = nullptr;   // lies where the values lie
    CPH_TRY(device_array(ctx, static_cast<const uint64_t*>(key.values), key.values_mem, (size_t)n, &up_values, &values));
    CPH_TRY(device_array(ctx, key.status, key.values_mem, key.status ? (size_t)n : 0, &up_status, &status));
    CPH_TRY(dk->buf.alloc(&ctx->pool, (size_t)n * 8));
    dk->wide = true;
    dk->bits = 64;
    const bool flt = key.kind == CPH_NUM_FLOAT64;
    // byte model: 8 B in, 8 B out (+ 1 B of status) per row
    ProfScope ps(ctx, flt ? "k_order_key_f64" : "k_order_key_i64", (double)n * (16.0 + (status ? 1.0 : 0.0)));
    if (flt)
        hipLaunchKernelGGL(k_order_key_num<true>, dim3(grid_for_items(n)), dim3(kMatThreads), 0, ctx->stream, values, status, n,
                           (uint32_t)(key.descending != 0), (uint32_t)k, dk->buf.as<uint64_t>(), d_err);
    else
        hipLaunchKernelGGL(k_order_key_num<false>, dim3(grid_for_items(n)), dim3(kMatThreads), 0, ctx->stream, values, status, n,
                           (uint32_t)(key.descending != 0), (uint32_t)k, dk->buf.as<uint64_t>(), d_err);
    CPH_HIP_TRY(hipGetLastError());
    return {};   // the uploads go back to the pool: reuse is stream-ordered
}

// A BYTES key: the dense rank of every row's run in the index.  One host read (the number of runs: the sort's bits).
Status key_pass_bytes(cph_ctx* ctx, const cph_order_key& key, uint64_t n, DevKey* dk) {
    const cph_index* ix = key.index;
    TileBitmap tb;
    CPH_TRY(tb.alloc(ctx, n));
    const uint64_t ntiles = tb.ntiles;
    agg_launch_heads(ctx, ix->sorted_codes.get(), ix->codec.key32, ix->total_words(), n, (double)index_code_bytes(ix), tb.words(), tb.counts());
    CPH_HIP_TRY(hipGetLastError());
    CPH_TRY(tb.scan(ctx));
    CPH_TRY(dk->buf.alloc(&ctx->pool, (size_t)n * 4));
    CPH_HIP_TRY(hipMemsetAsync(dk->buf.get(), 0, (size_t)n * 4, ctx->stream));   // a malformed perm leaves no row without a key
    {
        // byte model: 1 bit of bitmap, 4 B of perm, a 4-byte scattered store per row
        ProfScope ps(ctx, "k_order_key_rank", (double)n * (8.0 + 1.0 / 8.0) + 4.0 * (double)ntiles);
        hipLaunchKernelGGL(k_order_key_rank, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, tb.words(), tb.counts(), ix->perm.as<uint32_t>(), n,
                           n, (uint32_t)(key.descending != 0), dk->buf.as<uint32_t>());
    }
    CPH_HIP_TRY(hipGetLastError());
    uint32_t ng = 0;
    CPH_TRY(tb.read_total(ctx, &ng));
    if (ng == 0 || (uint64_t)ng > n) return {CPH_ERR_HIP, "cph_order_rows: the run count of an index is out of range"};
    dk->wide = false;
    dk->bits = bit_length((uint64_t)ng - 1);
    return {};
}

template <class K>
Status launch_gather(cph_ctx* ctx, const K* src, const uint32_t* ids, K* dst, uint64_t m) {
    // byte model: 4 B of ids, a sector-granular read of the key, sizeof(K) out per row
    ProfScope ps(ctx, sizeof(K) == 8 ? "k_order_gather_u64" : "k_order_gather_u32", (double)m * (4.0 + 2.0 * sizeof(K)));
    hipLaunchKernelGGL(k_order_gather<K>, dim3(grid_for_items(m)), dim3(kMatThreads), 0, ctx->stream, src, ids, dst, m);
    CPH_HIP_TRY(hipGetLastError());
    return {};
}

// The stable multi-key sort of m rows: cand (their row ids in input order, consumed as a sort buffer) or, when null, rows
// 0..m-1 = all rows.  *order = the row ids in output order (inside va / vb, which the caller keeps alive).
Status sort_rows(cph_ctx* ctx, DevKey* keys, int32_t nkeys, uint64_t m, DevBuf* va, DevBuf* vb, bool have_cand, const uint32_t** order_out) {
    DevBuf ka, kb;
    uint32_t* order = have_cand ? va->as<uint32_t>() : nullptr;
    for (int32_t j = nkeys - 1; j >= 0; j--) {
        DevKey& dk = keys[j];
        if (dk.bits <= 0) continue;   // one run: every row ties
        if (!kb) CPH_TRY(kb.alloc(&ctx->pool, (size_t)m * 8));
        void* kin = dk.buf.get();     // without an order yet the key array IS the key of row i (it is not needed again: the
                                      // select, the only other reader of key 0, runs in front of the sort)
        if (order) {
            if (!ka) CPH_TRY(ka.alloc(&ctx->pool, (size_t)m * 8));
            if (dk.wide) CPH_TRY(launch_gather<uint64_t>(ctx, dk.buf.as<uint64_t>(), order, ka.as<uint64_t>(), m));
            else CPH_TRY(launch_gather<uint32_t>(ctx, dk.buf.as<uint32_t>(), order, ka.as<uint32_t>(), m));
            kin = ka.get();
        }
        uint32_t* vin = order ? order : va->as<uint32_t>();
        uint32_t* vother = vin == va->as<uint32_t>() ? vb->as<uint32_t>() : va->as<uint32_t>();
        uint32_t* vout = nullptr;
        int passes = 0;
        if (dk.wide) {
            uint64_t* kout = nullptr;
            CPH_TRY(radix_sort_pairs<uint64_t>(ctx, static_cast<uint64_t*>(kin), kb.as<uint64_t>(), vin, vother, order == nullptr, m, dk.bits, &kout, &vout, &passes));
        } else {
            uint32_t* kout = nullptr;
            CPH_TRY(radix_sort_pairs<uint32_t>(ctx, static_cast<uint32_t*>(kin), kb.as<uint32_t>(), vin, vother, order == nullptr, m, dk.bits, &kout, &vout, &passes));
        }
        order = vout;
    }
    if (!order) {   // no key decided anything: input order
        CPH_TRY(fill_iota_u32(ctx, va->as<uint32_t>(), m));
        order = va->as<uint32_t>();
    }
    *order_out = order;
    return {};   // ka / kb go back to the pool: reuse is stream-ordered
}

// The candidates of the first key: every row at or below the key of ascending rank want - 1, in input order.
template <class K>
Status select_candidates(cph_ctx* ctx, const DevKey& dk, uint64_t n, uint64_t want, DevBuf* cand, uint64_t* ncand) {
    const K* keys = dk.buf.as<K>();
    const int npass = (dk.bits + 7) / 8;   // >= 1: the caller skips a key of 0 bits
    DevBuf state, hist;
    CPH_TRY(upload_block(ctx, SelectState{0ull, (unsigned long long)(want - 1)}, &state));
    CPH_TRY(hist.alloc(&ctx->pool, (size_t)npass * 256 * sizeof(uint32_t)));
    CPH_HIP_TRY(hipMemsetAsync(hist.get(), 0, (size_t)npass * 256 * sizeof(uint32_t), ctx->stream));
    constexpr int NV = sizeof(K) == 8 ? 2 : 4;
    for (int p = 0; p < npass; p++) {
        const int shift = 8 * (npass - 1 - p);
        {
            ProfScope ps(ctx, sizeof(K) == 8 ? "k_order_select_hist_u64" : "k_order_select_hist_u32", (double)n * sizeof(K));   // one read of the key array
            hipLaunchKernelGGL(k_order_select_hist<K>, dim3(grid_for_items(n / NV + 1, 2048)), dim3(kMatThreads), 0, ctx->stream, keys, n, shift, p == 0 ? 1 : 0,
                               state.as<SelectState>(), hist.as<uint32_t>() + (size_t)p * 256);
        }
        CPH_HIP_TRY(hipGetLastError());
        ProfScope ps(ctx, "k_order_select_pick", 1024.0 + 2.0 * sizeof(SelectState));
        hipLaunchKernelGGL(k_order_select_pick, dim3(1), dim3(kMatThreads), 0, ctx->stream, hist.as<uint32_t>() + (size_t)p * 256, shift, state.as<SelectState>());
        CPH_HIP_TRY(hipGetLastError());
    }
    TileBitmap tb;
    CPH_TRY(tb.alloc(ctx, n));
    const uint64_t ntiles = tb.ntiles;
    {
        ProfScope ps(ctx, sizeof(K) == 8 ? "k_order_select_flag_u64" : "k_order_select_flag_u32", (double)n * (sizeof(K) + 1.0 / 8.0) + 4.0 * (double)ntiles);
        hipLaunchKernelGGL(k_order_select_flag<K>, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, keys, n, state.as<SelectState>(), tb.words(),
                           tb.counts());
    }
    CPH_HIP_TRY(hipGetLastError());
    CPH_TRY(tb.scan(ctx));
    uint32_t total = 0;
    CPH_TRY(tb.read_total(ctx, &total));   // the route's one host wait
    if ((uint64_t)total < want || (uint64_t)total > n) return {CPH_ERR_HIP, "cph_order_rows: the candidate count is out of range"};
    CPH_TRY(cand->alloc(&ctx->pool, (size_t)total * sizeof(uint32_t)));
    {
        ProfScope ps(ctx, "k_order_select_emit", (double)n / 8.0 + 8.0 * (double)ntiles + 4.0 * (double)total);
        hipLaunchKernelGGL(k_order_select_emit, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, tb.words(), tb.counts(), ntiles, (uint64_t)total,
                           cand->as<uint32_t>());
    }
    CPH_HIP_TRY(hipGetLastError());
    *ncand = total;
    return {};
}

}  // namespace

extern "C" {

CPH_API int32_t cph_order_rows(cph_ctx* ctx, const cph_order_key* keys, int32_t nkeys, uint64_t nrows, uint64_t skip, uint64_t limit,
                               int32_t out_mem, cph_ordered** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "cph_order_rows: bad out_mem"});
    {
        const Status s = check_keys(keys, nkeys, nrows);
        if (!s.ok()) return fail_with(ctx, s);
    }
    if (nrows > 0xFFFFFFFFull) return fail_with(ctx, {CPH_ERR_TOO_MANY_ROWS, "cph_order_rows: more than 2^32-1 rows"});
    auto* r = new (std::nothrow) cph_ordered_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.mem = out_mem;
    r->pub.first_error_row = UINT64_MAX;
    auto run = [&]() -> Status {
        const uint64_t n = nrows;
        if (!n) return {};
        // ---- key pass ----
        DevKey dkeys[CPH_ORDER_MAX_KEYS];
        ErrReport<> err;
        bool any_status = false;
        for (int32_t k = 0; k < nkeys; k++) any_status = any_status || (keys[k].kind != CPH_ORDER_BYTES && keys[k].status);
        if (any_status) CPH_TRY(err.init(ctx));
        for (int32_t k = 0; k < nkeys; k++) {
            if (keys[k].kind == CPH_ORDER_BYTES) CPH_TRY(key_pass_bytes(ctx, keys[k], n, &dkeys[k]));
            else CPH_TRY(key_pass_number(ctx, keys[k], k, n, &dkeys[k], err.word()));
        }
        if (any_status) {
            ErrFirst e;
            CPH_TRY(err.read(ctx, &e));
            if (e.nerrors) {   // data, not a failure: no ids
                r->pub.nerrors = e.nerrors;
                r->pub.first_error_row = e.row;
                r->pub.first_error_key = e.tag;
                r->pub.first_error_kind = e.kind;
                return {};
            }
        }
        // ---- order[skip : skip + limit] ----
        const uint64_t end = skip >= n ? n : (limit > n - skip ? n : skip + limit);
        const uint64_t first = skip >= n ? n : skip;
        const uint64_t count = end - first;
        if (!count) return {};
        DevBuf va, vb;
        uint64_t m = n;
        bool have_cand = false;
        if (ctx->order_select && limit != UINT64_MAX && (end <= n / kSelectGate || ctx->order_select == 2) && dkeys[0].bits > 0) {
            if (dkeys[0].wide) CPH_TRY(select_candidates<uint64_t>(ctx, dkeys[0], n, end, &va, &m));
            else CPH_TRY(select_candidates<uint32_t>(ctx, dkeys[0], n, end, &va, &m));
            have_cand = true;
            r->pub.select_used = 1;
        } else {
            CPH_TRY(va.alloc(&ctx->pool, (size_t)m * sizeof(uint32_t)));
        }
        CPH_TRY(vb.alloc(&ctx->pool, (size_t)m * sizeof(uint32_t)));
        r->pub.candidates = m;
        const uint32_t* order = nullptr;
        CPH_TRY(sort_rows(ctx, dkeys, nkeys, m, &va, &vb, have_cand, &order));
        CPH_TRY(r->d_ids.alloc(&ctx->pool, (size_t)count * sizeof(uint32_t)));
        CPH_HIP_TRY(hipMemcpyAsync(r->d_ids.get(), order + first, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        r->pub.nrows = count;
        const ResultPart part{&r->d_ids, (size_t)count * sizeof(uint32_t), &r->pub.ids};
        return deliver(ctx, &r->own, &part, 1, out_mem);   // waits for the stream: the keys and sort buffers may go after it
    };
    return finish_call(ctx, r, run(), out);
}

CPH_API void cph_ordered_release(cph_ordered* pub) { release_result<cph_ordered_impl>(pub); }

}  // extern "C"

// Loads this translation unit's code object now (cph_ctx_create) instead of inside the first timed call.
namespace cph {
void warm_order() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_order_select_pick));
    (void)hipGetLastError();
}
}  // namespace cph
