// resolve.hip — Index.ResolveDuplicates (csvplus.go:643-653) with a NAMED rule: the choice per group, dedup's compaction
// (csvplus.go:810-867) and the new index on the device.  The callback route (cph_index_dup_groups + a host loop +
// cph_index_select) stays for arbitrary closures; the rules people write — first, last, newest / largest by a column, drop
// every ambiguous key — are data here, as Like / IntCmp are for Filter.
//
//   cph_index_resolve   sorted codes (+ an order column of the build table) -> the surviving sorted positions, the group
//                       statistics, the first conversion error inside a group, and (optionally) the compacted index
//
//   convert_rows      MIN / MAX by int64 / float64: the order column read through perm, so values[p] / status[p] lie in SORTED
//                     order and the reduce pass reads them coalesced (numparse.hip; deferred floats finished on the host).
//                     CPH_ORDER_BYTES compares the strings in place through perm.
//   k_resolve_tile    one pass over the sorted codes, kResRows CONSECUTIVE rows per lane: equal-to-previous / equal-to-next
//                     flags; a segmented arg-best scan (serial in the lane, 64-lane shuffles, LDS across the 4 waves); the
//                     winners of runs closed inside the tile go into the tile's keep bitmap (LDS), rows outside groups too;
//                     ONE partial for the tile's open head run and one for its open tail run; group / error counters.
//   k_resolve_carry   (MIN / MAX) one wave per tile whose head run CLOSES there: walks back over the tail partials of the
//                     tiles in front, 64 at a time, to the tile where the run started (a run may span every tile), and sets
//                     the winner's bit.
//   k_resolve_finish  one lane: the reference's tail rule (it needs the GLOBAL group count) and perm[first error].
//   exclusive scan of the tile counts (TileBitmap::scan), then
//   k_resolve_emit    the rank walker of tile_bitmap.hpp: positions[rank].
//   index_select_device (index_ops.hip) gathers perm and the codes: the device half of cph_index_select.
// The group count, the rows in groups, the error fields and the number of survivors come back in ONE small read.
#include <algorithm>
#include <cstring>
#include <new>

#include "num_report.hpp"
#include "runs_device.hpp"

namespace cph {

// kResRows / kResTile / kResWords / kResWaves and equal_flags: runs_device.hpp; the keep bitmap's layout: tile_bitmap.hpp
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

enum : int { kOrdNone = 0, kOrdKey = 1, kOrdBytes = 2 };   // how k_resolve_tile orders the rows of a group

// A candidate for a run's chosen row.  kOrdKey: `key` = the order value mapped so that the LARGER key wins under MIN and MAX
// alike (order_key); kOrdBytes: the strings decide.  pos == kNoPos: no candidate (the identity of pick()).
struct Best {
    uint64_t key;
    uint32_t pos;
};
struct ResCounters {   // preset by the host in front of k_resolve_tile (ErrReport)
    ErrWord err;           // first; its row = the sorted position, tag = 0
    unsigned long long ngroups, group_rows;
    unsigned long long first_error_row;   // k_resolve_finish: perm[that position], ~0: none
    uint32_t last_single;   // the final sorted row is not inside a group
    uint32_t total;         // surviving rows (copied in behind the scan)
};
struct TilePartial {
    Best head, tail;        // best of the run that reaches the tile from the left / leaves it to the right, over this tile's rows
    uint32_t head_closes;   // 1: that head run ends inside this tile
    uint32_t tail_state;    // 0: the last row ends its run; 1: it goes on into the next tile; 2: and it came in from the left (one run spans the tile)
};
struct OrderArg {
    const uint64_t* values;   // kOrdKey: int64 / double bits per SORTED position
    const uint8_t* status;    //          and their CPH_NUM_* status bytes
    const uint32_t* perm;     // kOrdBytes: row of `col` per sorted position
    DevCol col;
    int32_t is_float, is_min;
};

// strings.Compare over two values of one column: unsigned bytewise, a proper prefix is smaller
__device__ __forceinline__ int compare_values(const DevCol& col, uint64_t ra, uint64_t rb) {
    uint64_t ba, la, bb, lb;
    value_span(col, ra, &ba, &la);
    value_span(col, rb, &bb, &lb);
    const uint64_t m = la < lb ? la : lb;
    for (uint64_t j = 0; 8 * j < m; j++) {
        const uint64_t nb = m - 8 * j;
        const uint64_t valid = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
        const uint64_t x = load_value_chunk(col.data, ba, m, (int)j) & valid, y = load_value_chunk(col.data, bb, m, (int)j) & valid;
        if (x != y) {   // little endian: the first differing byte is the lowest one
            const int sh = __builtin_ctzll(x ^ y) & ~7;
            return ((x >> sh) & 0xFFull) < ((y >> sh) & 0xFFull) ? -1 : 1;
        }
    }
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// int64: order preserving into uint64.  double: -0 = +0, NaN -> 0 (below every number under MIN and MAX), numbers > 0.
__device__ __forceinline__ uint64_t order_key(uint64_t bits, uint32_t status, const OrderArg& o) {
    if (status != CPH_NUM_OK) return 0;   // an error row inside a group voids the call
    uint64_t f;
    if (o.is_float) {
        if ((bits & 0x7FFFFFFFFFFFFFFFull) == 0) bits = 0;
        if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0;
        f = (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
    } else {
        f = bits ^ 0x8000000000000000ull;
    }
    return o.is_min ? ~f : f;
}

// the better of two candidates; ties go to the lower position (a total order: pick is commutative and associative)
template <int ORD>
__device__ __forceinline__ Best pick(const Best a, const Best b, const OrderArg& o) {
    bool a_wins;
    if constexpr (ORD == kOrdBytes) {
        a_wins = true;
        if (a.pos != kNoPos && b.pos != kNoPos && a.pos != b.pos) {
            const int c = compare_values(o.col, o.perm[a.pos], o.perm[b.pos]);
            a_wins = c == 0 ? a.pos < b.pos : (o.is_min ? c < 0 : c > 0);
        }
    } else {
        a_wins = a.key != b.key ? a.key > b.key : a.pos < b.pos;
    }
    a_wins = b.pos == kNoPos || (a.pos != kNoPos && a_wins);
    Best r;   // by field: selecting whole structs goes through scratch memory
    r.key = a_wins ? a.key : b.key;
    r.pos = a_wins ? a.pos : b.pos;
    return r;
}

// one element of the segmented scan: the best since the last run start at or before this point, and whether there was one
struct Seg {
    Best b;
    uint32_t start;
};
template <int ORD>
__device__ __forceinline__ Seg seg_join(const Seg left, const Seg right, const OrderArg& o) {
    Seg r;
    const Best p = pick<ORD>(left.b, right.b, o);
    r.b.key = right.start ? right.b.key : p.key;
    r.b.pos = right.start ? right.b.pos : p.pos;
    r.start = left.start | right.start;
    return r;
}
__device__ __forceinline__ Seg seg_shfl_up(const Seg& s, int d) {
    Seg r;
    r.b.key = __shfl_up(s.b.key, d, kWave);
    r.b.pos = __shfl_up(s.b.pos, d, kWave);
    r.start = __shfl_up(s.start, d, kWave);
    return r;
}

// bit = that sorted position survives (tile_bitmap.hpp; the winners of runs that span tiles are added by k_resolve_carry),
// part[tile] = the tile's open runs (ORD != kOrdNone).
// n >= 1; ORD == kOrdNone: rule is FIRST / LAST / DROP and nothing is scanned.
template <bool KEY32, int ORD>
__global__ __launch_bounds__(kMatThreads) void k_resolve_tile(const void* __restrict__ codes, uint64_t n, int nwords, int32_t rule, OrderArg ord,
                                                             uint64_t* __restrict__ bitmap, uint32_t* __restrict__ counts,
                                                             TilePartial* __restrict__ part, ResCounters* cnt) {
    __shared__ uint32_t s_keep[kResTile / 32];
    __shared__ uint32_t s_cnt[3];
    __shared__ Seg s_wave[kResWaves];
    __shared__ TilePartial s_part;
    const int lane = lane_id(), wave = wave_id();
    const uint64_t ntiles = tile_count(n);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kResTile;
        const uint64_t tend = t0 + kResTile < n ? t0 + kResTile : n;   // one past the tile's last row
        if (threadIdx.x < kResTile / 32) s_keep[threadIdx.x] = 0;
        if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            s_part.head = Best{0, kNoPos};
            s_part.tail = Best{0, kNoPos};
            s_part.head_closes = 0;
            s_part.tail_state = 0;
        }
        __syncthreads();
        const uint32_t r0 = threadIdx.x * kResRows;   // the lane's first row inside the tile
        const uint64_t base = t0 + r0;
        const uint32_t e = base < n ? equal_flags<KEY32>(codes, n, nwords, base) : 0u;
        // tile_live_rows(base, tend) spelled out: this kernel's register count moves with the shared function (profiles/tile_bitmap_refactor.txt)
        const uint32_t live = base >= tend ? 0u : (tend - base >= (uint64_t)kResRows ? (1u << kResRows) - 1 : (1u << (uint32_t)(tend - base)) - 1);
        const uint32_t eq_prev = e & live, eq_next = (e >> 1) & live;
        const uint32_t single = live & ~eq_prev & ~eq_next;
        const uint32_t gstart = live & ~eq_prev & eq_next;     // first row of a run of >= 2
        const uint32_t gend = live & eq_prev & ~eq_next;       // its last row
        uint32_t keep = single;
        if (rule == CPH_RESOLVE_FIRST) keep |= gstart;
        if (rule == CPH_RESOLVE_LAST) keep |= gend;
        uint32_t ngroups = (uint32_t)__popc(gstart), grows = (uint32_t)__popc(eq_prev | eq_next), nerr = 0;
        unsigned long long first_err = ~0ull;

        if constexpr (ORD != kOrdNone) {
            // the lane's own rows: loc[k] = best since the last run start inside the lane (or since its first row)
            uint64_t loc_key[kResRows];
            uint32_t loc_pos[kResRows];
            Best cur{0, kNoPos};
            uint32_t started = 0;   // bit k: a run starts at one of the lane's rows 0..k
#pragma unroll
            for (int k = 0; k < kResRows; k++) {
                const bool on = (live >> k) & 1u;
                Best self{0, kNoPos};
                if (on) {
                    self.pos = (uint32_t)(base + (uint64_t)k);
                    if constexpr (ORD == kOrdKey) {
                        const uint32_t st = ord.status[base + (uint64_t)k];
                        self.key = order_key(ord.values[base + (uint64_t)k], st, ord);
                        if (st != CPH_NUM_OK && (((eq_prev | eq_next) >> k) & 1u)) {
                            nerr++;
                            const unsigned long long key = err_pack(base + (uint64_t)k, 0u, st);
                            if (key < first_err) first_err = key;
                        }
                    }
                }
                const bool starts = on && !((eq_prev >> k) & 1u);
                if (starts) cur = self;
                else if (on) cur = pick<ORD>(cur, self, ord);
                if (starts) started |= 1u << k;
                if (k > 0) started |= ((started >> (k - 1)) & 1u) << k;
                loc_key[k] = cur.key;
                loc_pos[k] = cur.pos;
            }
            // across the lanes of the wave, then across the waves: incl = everything up to and including this lane
            Seg mine{cur, started >> (kResRows - 1)};
            Seg incl = mine;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const Seg up = seg_shfl_up(incl, d);
                if (lane >= d) incl = seg_join<ORD>(up, incl, ord);
            }
            if (lane == kWave - 1) s_wave[wave] = incl;
            Seg excl = seg_shfl_up(incl, 1);
            if (lane == 0) excl = Seg{Best{0, kNoPos}, 0u};
            __syncthreads();
            Seg front{Best{0, kNoPos}, 0u};   // the waves in front of this one
            for (int w = 0; w < wave; w++) front = seg_join<ORD>(front, s_wave[w], ord);
            excl = seg_join<ORD>(front, excl, ord);
#pragma unroll
            for (int k = 0; k < kResRows; k++) {
                if (!((live >> k) & 1u)) continue;
                const bool own = (started >> k) & 1u;                 // the row's run started inside this lane
                const bool in_tile = own || excl.start != 0;           // ... inside this tile
                const bool is_end = (gend >> k) & 1u;
                const bool is_last = base + (uint64_t)k + 1 == tend;
                if (!is_end && !(is_last && ((eq_next >> k) & 1u))) continue;
                const Best mine_k{loc_key[k], loc_pos[k]};
                const Best s = own ? mine_k : pick<ORD>(excl.b, mine_k, ord);
                if (is_end) {
                    if (in_tile) {
                        const uint32_t r = s.pos - (uint32_t)t0;       // the winner of a run closed inside the tile
                        if (r < (uint32_t)kResTile) atomicOr(&s_keep[r >> 5], 1u << (r & 31));
                    } else {
                        s_part.head = s;
                        s_part.head_closes = 1;
                    }
                } else {   // the tile's last row, its run goes on
                    s_part.tail = s;
                    s_part.tail_state = in_tile ? 1u : 2u;
                }
            }
        }
        // keep bits of the lane's own rows, counters
        if (keep) {
            const uint32_t w = r0 >> 5, sh = r0 & 31;   // 8 rows never straddle a 32-bit word
            atomicOr(&s_keep[w], keep << sh);
        }
        ngroups = wave_sum(ngroups);
        grows = wave_sum(grows);
        nerr = wave_sum(nerr);
        first_err = wave_min(first_err);
        if (lane == 0) {
            if (ngroups) atomicAdd(&s_cnt[0], ngroups);
            if (grows) atomicAdd(&s_cnt[1], grows);
            if (nerr) {
                atomicAdd(&s_cnt[2], nerr);
                atomicMin(&cnt->err.first, first_err);
            }
        }
        if (base + kResRows >= n && base < n) cnt->last_single = (single >> (uint32_t)(n - 1 - base)) & 1u;   // the lane of row n-1
        lds_atomics_barrier();
        if (wave == 0) {
            const uint32_t lo = s_keep[2 * (lane & (kResWords - 1))], hi = s_keep[2 * (lane & (kResWords - 1)) + 1];
            const uint64_t word = lane < kResWords ? ((uint64_t)lo | ((uint64_t)hi << 32)) : 0;
            if (lane < kResWords) bitmap[tile * kResWords + lane] = word;
            const uint32_t c = wave_sum((uint32_t)__popcll(word));
            if (lane == 0) {
                counts[tile] = c;
                if (s_cnt[0]) atomicAdd(&cnt->ngroups, (unsigned long long)s_cnt[0]);
                if (s_cnt[1]) atomicAdd(&cnt->group_rows, (unsigned long long)s_cnt[1]);
                if (s_cnt[2]) atomicAdd(&cnt->err.nerrors, (unsigned long long)s_cnt[2]);
                if constexpr (ORD != kOrdNone) part[tile] = s_part;
            }
        }
        __syncthreads();
    }
}

// One wave per tile whose head run closes there: the run's winner over all the tiles it spans gets its bit.
template <int ORD>
__global__ __launch_bounds__(kMatThreads) void k_resolve_carry(const TilePartial* __restrict__ part, uint64_t ntiles, OrderArg ord,
                                                              unsigned long long* __restrict__ bitmap, uint32_t* __restrict__ counts) {
    const int lane = lane_id();
    const uint64_t nwaves = (uint64_t)gridDim.x * kResWaves;
    for (uint64_t t = (uint64_t)blockIdx.x * kResWaves + (uint64_t)wave_id(); t < ntiles; t += nwaves) {
        if (t == 0 || !part[t].head_closes) continue;   // uniform
        Best cur = part[t].head;
        for (uint64_t j = t;;) {   // tiles j-1, j-2, ... j-64 on the lanes
            const bool valid = (uint64_t)lane < j;
            const uint64_t q = valid ? j - 1 - (uint64_t)lane : 0;
            const uint32_t st = valid ? part[q].tail_state : 0u;
            const uint64_t stop = __ballot(!valid || st != 2u);   // the first tile that the run does not span: it started there
            const int first = stop ? __builtin_ctzll(stop) : kWave;
            Best cand{0, kNoPos};
            if (valid && st != 0u && lane <= first) cand = part[q].tail;
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) {
                Best o;
                o.key = __shfl_xor(cand.key, d, kWave);
                o.pos = __shfl_xor(cand.pos, d, kWave);
                cand = pick<ORD>(cand, o, ord);
            }
            cur = pick<ORD>(cur, cand, ord);
            if (stop || j <= (uint64_t)kWave) break;
            j -= kWave;
        }
        if (lane == 0 && cur.pos != kNoPos) {
            const unsigned long long bit = 1ull << (cur.pos & 63u);   // counts and bitmap stay in step: the emit pass ranks by both
            if (!(atomicOr(&bitmap[cur.pos >> 6], bit) & bit)) atomicAdd(&counts[cur.pos / kResTile], 1u);
        }
    }
}

// The tail rule (csvplus.go:851-859: once a group was resolved, the final row survives only inside the last group) and the
// table row of the first conversion error.  One lane.
__global__ void k_resolve_finish(ResCounters* cnt, const uint32_t* __restrict__ perm, uint64_t n, int32_t keep_last_row,
                                 unsigned long long* __restrict__ bitmap, uint32_t* __restrict__ counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!keep_last_row && cnt->ngroups > 0 && cnt->last_single) {
        const uint64_t p = n - 1;
        const unsigned long long bit = 1ull << (p & 63u);
        if (atomicAnd(&bitmap[p >> 6], ~bit) & bit) atomicSub(&counts[p / kResTile], 1u);
    }
    cnt->first_error_row = cnt->err.first == kErrNone ? ~0ull : (unsigned long long)perm[err_row(cnt->err.first)];
}

// offs[tile] = survivors in front of the tile; out[rank] = the sorted position
__global__ __launch_bounds__(kMatThreads) void k_resolve_emit(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ offs,
                                                             uint64_t ntiles, uint64_t* __restrict__ out) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t o0 = offs[tile], o1 = offs[tile + 1];
        if (o0 == o1) continue;   // uniform
        tile_for_each_set(bitmap, tile, o0, [&](uint64_t rank, int r) { out[rank] = tile * kResTile + (uint64_t)r; });
    }
}

}  // namespace cph

using namespace cph;

// the library-owned result behind cph_resolved
struct cph_resolved_impl {
    cph_resolved pub;   // first
    cph::ResultOwner own;
    cph::DevBuf d_pos;
};

namespace {

template <int ORD>
void launch_tile(cph_ctx* ctx, const cph_index* ix, int32_t rule, const OrderArg& ord, uint64_t ntiles, uint64_t* bitmap, uint32_t* counts,
                 TilePartial* part, ResCounters* cnt) {
    if (ix->codec.key32)
        hipLaunchKernelGGL((k_resolve_tile<true, ORD>), dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, ix->sorted_codes.get(),
                           ix->nrows, ix->total_words(), rule, ord, bitmap, counts, part, cnt);
    else
        hipLaunchKernelGGL((k_resolve_tile<false, ORD>), dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, ix->sorted_codes.get(),
                           ix->nrows, ix->total_words(), rule, ord, bitmap, counts, part, cnt);
}

}  // namespace

extern "C" {

CPH_API int32_t cph_index_resolve(cph_ctx* ctx, const cph_index* ix, const cph_resolve_opts* opts, const cph_strcol* order_col,
                                  int32_t out_mem, cph_index** out_index, cph_resolved** out) {
    if (!ctx || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (out_index) *out_index = nullptr;
    if (!ix || !opts) return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_resolve: index and opts must not be NULL"});
    if (opts->rule < CPH_RESOLVE_FIRST || opts->rule > CPH_RESOLVE_MAX) return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_resolve: unknown rule"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    const bool ordered = opts->rule == CPH_RESOLVE_MIN || opts->rule == CPH_RESOLVE_MAX;
    if (ordered) {
        if (opts->order_kind != CPH_NUM_INT64 && opts->order_kind != CPH_NUM_FLOAT64 && opts->order_kind != CPH_ORDER_BYTES)
            return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_resolve: order_kind must be CPH_NUM_INT64, CPH_NUM_FLOAT64 or CPH_ORDER_BYTES"});
        if (!order_col) return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_resolve: MIN / MAX need an order column"});
        Status s = validate_cols(order_col, 1);
        if (!s.ok()) return fail_with(ctx, s);
        if (order_col->nrows < ix->table_rows)
            return fail_with(ctx, {CPH_ERR_INVALID, "cph_index_resolve: the order column has fewer rows than the index's build table"});
    }
    auto* r = new (std::nothrow) cph_resolved_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    r->pub.mem = out_mem;
    r->pub.first_error_position = r->pub.first_error_row = UINT64_MAX;
    cph_index* nx = nullptr;
    auto run = [&]() -> Status {
        const uint64_t n = ix->nrows;
        uint64_t kept = 0;
        if (n) {
            const double cb = (double)index_code_bytes(ix);
            std::vector<DevBuf> staged;
            DevBuf values, status;
            OrderArg ord{};
            ord.is_min = opts->rule == CPH_RESOLVE_MIN;
            int mode = kOrdNone;
            double order_bytes = 0;
            if (ordered) {
                CPH_TRY(stage_cols(ctx, order_col, 1, &staged, &ord.col));
                ord.perm = ix->perm.as<uint32_t>();
                if (opts->order_kind == CPH_ORDER_BYTES) {
                    mode = kOrdBytes;
                    order_bytes = 4.0 + (ord.col.fixed_width ? (double)ord.col.fixed_width : (double)(ord.col.offset_bits / 8) + 8.0);
                } else {
                    mode = kOrdKey;
                    ord.is_float = opts->order_kind == CPH_NUM_FLOAT64;
                    RowIds ids;
                    ids.ptr = ix->perm.get();
                    ids.bits = 32;
                    NumColStats st;
                    CPH_TRY(convert_rows(ctx, ord.col, ids, 0, n, opts->order_kind, &values, &status, &st));
                    r->pub.host_rows = st.host_rows;
                    ord.values = values.as<uint64_t>();
                    ord.status = status.as<uint8_t>();
                    order_bytes = 9.0;
                }
            }
            TileBitmap tb;
            CPH_TRY(tb.alloc(ctx, n));
            const uint64_t ntiles = tb.ntiles;
            DevBuf part;
            ErrReport<ResCounters> cnt;
            if (mode != kOrdNone) CPH_TRY(part.alloc(&ctx->pool, ntiles * sizeof(TilePartial)));
            CPH_TRY(cnt.init(ctx));   // first_error_row is k_resolve_finish's to write
            {
                // byte model: the codes and the order values (or perm + offsets + ~8 string bytes) in, bitmap, counts and partials out
                ProfScope ps(ctx, "k_resolve_tile", (double)n * (cb + order_bytes + 1.0 / 8.0) + (double)ntiles * (4.0 + (mode != kOrdNone ? (double)sizeof(TilePartial) : 0.0)));
                if (mode == kOrdNone) launch_tile<kOrdNone>(ctx, ix, opts->rule, ord, ntiles, tb.words(), tb.counts(), nullptr, cnt.counters());
                else if (mode == kOrdKey) launch_tile<kOrdKey>(ctx, ix, opts->rule, ord, ntiles, tb.words(), tb.counts(), part.as<TilePartial>(), cnt.counters());
                else launch_tile<kOrdBytes>(ctx, ix, opts->rule, ord, ntiles, tb.words(), tb.counts(), part.as<TilePartial>(), cnt.counters());
            }
            CPH_HIP_TRY(hipGetLastError());
            if (mode != kOrdNone && ntiles > 1) {
                ProfScope ps(ctx, "k_resolve_carry", (double)ntiles * (double)sizeof(TilePartial));
                const unsigned grid = (unsigned)std::min<uint64_t>((ntiles + kResWaves - 1) / kResWaves, 4096);
                if (mode == kOrdKey)
                    hipLaunchKernelGGL(k_resolve_carry<kOrdKey>, dim3(grid), dim3(kMatThreads), 0, ctx->stream, part.as<TilePartial>(), ntiles, ord,
                                       tb.bitmap.as<unsigned long long>(), tb.counts());
                else
                    hipLaunchKernelGGL(k_resolve_carry<kOrdBytes>, dim3(grid), dim3(kMatThreads), 0, ctx->stream, part.as<TilePartial>(), ntiles, ord,
                                       tb.bitmap.as<unsigned long long>(), tb.counts());
                CPH_HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(k_resolve_finish, dim3(1), dim3(kWave), 0, ctx->stream, cnt.counters(), ix->perm.as<uint32_t>(), n,
                               opts->keep_last_row, tb.bitmap.as<unsigned long long>(), tb.counts());
            CPH_HIP_TRY(hipGetLastError());
            CPH_TRY(tb.scan(ctx));
            CPH_HIP_TRY(hipMemcpyAsync(&cnt.counters()->total, tb.total(), sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            ResCounters got{};
            ErrFirst e;
            CPH_TRY(cnt.read(ctx, &e, &got));   // the call's host wait
            r->pub.ngroups = got.ngroups;
            r->pub.group_rows = got.group_rows;
            r->pub.nerrors = e.nerrors;
            if (e.nerrors) {   // data, not a failure: no positions, no index
                r->pub.first_error_position = e.row;
                r->pub.first_error_row = got.first_error_row;
                r->pub.first_error_kind = e.kind;
                return {};
            }
            kept = got.total;
            if (kept) {
                CPH_TRY(r->d_pos.alloc(&ctx->pool, kept * sizeof(uint64_t)));
                ProfScope ps(ctx, "k_resolve_emit", (double)n / 8.0 + 4.0 * (double)ntiles + 8.0 * (double)kept);
                hipLaunchKernelGGL(k_resolve_emit, dim3(tile_grid(ntiles)), dim3(kMatThreads), 0, ctx->stream, tb.words(), tb.counts(), ntiles,
                                   r->d_pos.as<uint64_t>());
                CPH_HIP_TRY(hipGetLastError());
            }
        }
        r->pub.nrows = kept;
        if (out_index) {
            nx = new (std::nothrow) cph_index();
            if (!nx) return {CPH_ERR_NOMEM, "out of host memory"};
            CPH_TRY(index_select_device(ctx, ix, r->d_pos.as<uint64_t>(), kept, nx));
        }
        const ResultPart part{&r->d_pos, (size_t)kept * sizeof(uint64_t), &r->pub.positions};
        return deliver(ctx, &r->own, &part, 1, out_mem);
    };
    const Status s = run();
    if (!s.ok()) {
        (void)hipStreamSynchronize(ctx->stream);
        delete nx;
    } else if (out_index) {
        *out_index = nx;
    }
    return finish_call(ctx, r, s, out);
}

CPH_API void cph_resolved_release(cph_resolved* pub) { release_result<cph_resolved_impl>(pub); }

}  // extern "C"

// Loads this translation unit's code object now (cph_ctx_create) instead of inside the first timed call.
namespace cph {
void warm_resolve() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_resolve_emit));
    (void)hipGetLastError();
}
}  // namespace cph
