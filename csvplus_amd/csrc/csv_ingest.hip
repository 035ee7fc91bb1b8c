// csv_ingest.hip — the step BEFORE the path: CSV bytes -> SoA string columns
// without per-row maps.  Replaces the parse loop of Reader.Iterate (csvplus.go:1080-1146:
// csv.NewReader + per-line map construction :1117-1131); the header logic (makeHeader :1149-1206)
// stays on the host, which passes the field INDICES of the wanted columns.
//
// Semantics = Go's encoding/csv Reader as csvplus configures it (Comma, Comment, TrimLeadingSpace,
// FieldsPerRecord; LazyQuotes through cph_csv_parse_lazy, below): "\r\n" line ends become "\n" (also inside quoted
// fields), empty lines and comment lines between records are skipped, `""` is a literal quote, a
// quote inside an unquoted field is ErrBareQuote, anything but Comma / end of line after a closing
// quote (or EOF inside quotes) is ErrQuote, field counts follow FieldsPerRecord.  The FIRST error in
// record order is reported with its record index; the records before it are returned, as the
// reference delivers them before failing.
//
// Parallel structure (text resident in HBM, 16-byte aligned):
//   1. k_csv_tile_stats: per 16 KiB tile the number of quotes and of newlines at even / odd quote parity
//      (SWAR byte masks, ballot prefix parity) -> scans over tiles give the parity at every tile start and the
//      number of record separators before it
//   2. k_csv_separators: positions of the newlines outside quotes, in text order
//   3. k_csv_classify: blank and comment lines; when none was dropped inside the text, record r IS segment r
//      (no compaction), otherwise k_csv_compact
//   4. k_csv_fields: 256 records per workgroup, their text staged in LDS together with delimiter / quote
//      bitmasks; a record without quotes is split with bit scans, any other runs Go readRecord's state
//      machine; field count, first error, lengths of the wanted fields
//   5. per column: exclusive scan of the lengths -> offsets; k_csv_copy_fields parses again and assembles
//      each column's bytes of the tile in LDS, then streams them out
// A bare quote flips the parity of everything after it, but everything BEFORE the first error is
// segmented correctly, and only the first error (smallest record index) is reported.
//
// LazyQuotes (cph_csv_parse_lazy; Reader.LazyQuotes, csvplus.go:982-987): a quote inside an unquoted field is a byte, a quote
// inside a quoted field that is followed by neither a quote, Comma nor the line end is a byte, the end of the text inside
// quotes ends the field; ErrFieldCount is the only error left.  Parity says nothing about such a text, so passes 1 and 2 are
// replaced by a scan of the seven-state byte automaton of csv_lazy_device.hpp (the tile geometry stays: 16 KiB tiles, 16-byte
// chunks, j-major text order):
//   1L. k_csv_lazy_tile_maps     every chunk's state map (16 bytes walked with two v_perm_b32 each), composed over the wave with
//                                shuffles, over the tile's 4 waves x 4 rounds through LDS: one packed map per tile
//   1M. k_csv_lazy_tile_entry    exclusive compose-scan over the tile maps, RS in front of the text: every tile's entry STATE.
//                                One workgroup takes kLazyScanStep tiles per step and carries a single state to the next step
//                                (plain stream order, no look-back between workgroups: nothing here needs a resident grid).
//                                4 bytes per 16 KiB of text: 0.03 % of the bytes the passes beside it read.
//   2L. k_csv_lazy_marks         the same walk again with the entry state known: a 16-bit mask per chunk of the newlines that end
//                                a record, and their number per tile (-> the existing exclusive_scan_u64)
//   2M. k_csv_lazy_separators    reads the masks only (1/8 of the text, 16 bytes = 8 chunks per thread) and writes the positions
// Choices.  (a) The second text pass RECOMPUTES the automaton instead of reading per-chunk maps saved by the first: a saved map
// is 4-8 bytes per 16 bytes of text, written once and read once — 0.5 byte of traffic per byte of text to save about 250 VALU
// instructions per chunk, on passes that run at a small fraction of the HBM roof either way; the bytes would also have to be
// kept for a text of any size.  What IS saved is the result of the second walk, 2 bytes per chunk, so that positions are written
// without a third walk (their place needs the scan of the counts, which needs the walk).  (b) Four launches + the count scan, as
// the strict side has two + two scans.  (c) Per byte: a select chain picks the class map, two v_perm_b32 apply it to all seven
// start states at once — no per-state registers, no branches, no run-length shortcut for plain bytes (it would diverge within
// the wave; left as the follow-up if the walk's VALU time matters).  TrimLeadingSpace and the comment character each add a
// class test per byte: the walk is instantiated four ways and a uniform branch picks one.
// Behind the separators everything is shared with the strict side: k_csv_classify (a segment starts in RS, so its first byte
// still decides "comment line"; a comment's quotes were kept from meaning anything by the CM state, so the strict side's
// "comment line containing a quote" refusal does not apply), k_csv_compact, RecIndex, and the record-parallel kernels in their
// LAZY instantiation of csv_parse_record.  A text without any quote reads the same under both rules: k_csv_fast is tried first.
// One detected limit: the automaton trims ASCII spaces only (the multi-byte spaces of unicode.IsSpace would need eight more
// states); the per-record parser trims them all and reports a field whose trimmed-off prefix held a multi-byte space and
// whose next byte is a quote — Go reads it as quoted, the automaton read it as unquoted.  Everything in front of the
// earliest such field is segmented correctly and the field's first bytes lie inside its own record's segment, so the
// earliest occurrence is always seen: the call fails with CPH_ERR_INVALID.
#include <cstdlib>
#include <new>

#include "lds_stage.hpp"
#include "csv_lazy_device.hpp"   // (behind the HIP runtime's __forceinline__)

namespace cph {

constexpr int kCsvThreads = 256;
constexpr int kCsvWaves = kCsvThreads / kWave;
constexpr int kCsvChunks = 4;                                  // 16-byte chunks per thread per tile
constexpr int kCsvTile = kCsvThreads * 16 * kCsvChunks;       // 16 KiB per workgroup (tests/test_gpu_csv_strict_edges.py: TILE)
constexpr int kCsvStageMax = 32 * 1024;                       // LDS bytes for one 256-record tile (in, and out): the host picks
constexpr int kCsvStageMin = 8 * 1024;                        // the smallest power of two that holds 1.5x an average tile
                                                              // (tests/test_gpu_csv_strict_edges.py: STAGE_MIN, STAGE_MAX)

struct CsvOpts {
    uint8_t comma, comment;   // comment 0 = none
    int32_t trim;
};
struct CsvCols {
    int32_t ncols;
    int32_t index[kMaxKeyCols];
};

// ---- byte classification, 16 bytes at a time ---------------------------------------------------------------
// bit i of the result = (byte i of w == byte of pat)
__device__ __forceinline__ uint32_t eq_mask4(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every zero byte of x
    return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}
struct ChunkMasks {
    uint32_t quote, newline;   // 16-bit masks
};
// chunk at byte offset pos (multiple of 16) of the 16-byte aligned text d[0,size); bytes past size read as 0
__device__ __forceinline__ ChunkMasks chunk_masks(const uint8_t* __restrict__ d, uint64_t size, uint64_t pos) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (pos + 16 <= size) {
        const uint4 v = *reinterpret_cast<const uint4*>(d + pos);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        for (uint64_t k = pos; k < size; k++) w[(k - pos) >> 2] |= (uint32_t)d[k] << (8 * ((k - pos) & 3));
    }
    ChunkMasks m{0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        m.quote |= eq_mask4(w[i], 0x22222222u) << (4 * i);
        m.newline |= eq_mask4(w[i], 0x0A0A0A0Au) << (4 * i);
    }
    return m;
}
// bit i = parity of the bits [0, i] of a 16-bit mask
__device__ __forceinline__ uint32_t prefix_parity16(uint32_t q) {
    q ^= q << 1;
    q ^= q << 2;
    q ^= q << 4;
    q ^= q << 8;
    return q & 0xFFFFu;
}

// One tile = kCsvChunks rounds of 256 coalesced 16-byte chunks; chunk (j, thread t) covers the bytes at
// tile_base + (j*256 + t)*16, so text order is j-major.  Computes for every chunk of this thread the mask of
// newlines at EVEN quote parity, the parity counted from the tile start (start_par = parity at the tile start).
// s_par: kCsvChunks * kCsvWaves words of LDS.  Contains one __syncthreads.
struct TileScan {
    uint32_t even[kCsvChunks];   // newlines outside quotes (given start_par), per chunk
    uint32_t odd[kCsvChunks];    // newlines inside quotes
    uint32_t quotes;             // quotes in this thread's chunks
};
__device__ __forceinline__ TileScan scan_tile(const uint8_t* __restrict__ d, uint64_t size, uint64_t tile_base, uint32_t start_par,
                                              uint32_t* s_par) {
    ChunkMasks m[kCsvChunks];
    uint32_t lane_par[kCsvChunks];
    TileScan r;
    r.quotes = 0;
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        m[j] = chunk_masks(d, size, tile_base + ((uint64_t)j * kCsvThreads + threadIdx.x) * 16);
        const uint32_t nq = (uint32_t)__popc(m[j].quote);
        r.quotes += nq;
        const unsigned long long b = __ballot(nq & 1u);
        lane_par[j] = (uint32_t)__popcll(b & lanemask_lt()) & 1u;
        if (lane_id() == 0) s_par[j * kCsvWaves + wave_id()] = (uint32_t)__popcll(b) & 1u;
    }
    __syncthreads();
    uint32_t run = start_par & 1u;
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        uint32_t mine = 0;
#pragma unroll
        for (int w = 0; w < kCsvWaves; w++) {
            if (w == wave_id()) mine = run;
            run ^= s_par[j * kCsvWaves + w];
        }
        const uint32_t par = mine ^ lane_par[j];                       // parity at the first byte of this chunk
        uint32_t inq = prefix_parity16(m[j].quote);                    // relative to the chunk start
        if (par) inq ^= 0xFFFFu;
        r.even[j] = m[j].newline & ~inq;
        r.odd[j] = m[j].newline & inq;
    }
    return r;
}

// ---- 1. per tile: quotes, newlines at even / odd parity relative to the tile start ---------------------------
__global__ __launch_bounds__(kCsvThreads) void k_csv_tile_stats(const uint8_t* __restrict__ d, uint64_t size,
                                                               uint32_t* __restrict__ tile_quotes, uint32_t* __restrict__ tile_even,
                                                               uint32_t* __restrict__ tile_odd) {
    __shared__ uint32_t s_par[kCsvChunks * kCsvWaves];
    __shared__ uint32_t s_red[3 * kCsvWaves];
    const uint64_t t = blockIdx.x;
    const TileScan r = scan_tile(d, size, t * kCsvTile, 0, s_par);
    uint32_t ev = 0, od = 0;
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        ev += (uint32_t)__popc(r.even[j]);
        od += (uint32_t)__popc(r.odd[j]);
    }
    const uint32_t q = wave_sum(r.quotes);
    ev = wave_sum(ev);
    od = wave_sum(od);
    if (lane_id() == 0) {
        s_red[wave_id()] = q;
        s_red[kCsvWaves + wave_id()] = ev;
        s_red[2 * kCsvWaves + wave_id()] = od;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0;
        for (int w = 0; w < kCsvWaves; w++) s += s_red[threadIdx.x * kCsvWaves + w];
        (threadIdx.x == 0 ? tile_quotes : threadIdx.x == 1 ? tile_even : tile_odd)[t] = s;
    }
}

// quotes_before = exclusive scan of tile_quotes.  counts[t] = separators of tile t.
__global__ void k_csv_pick_counts(const uint32_t* __restrict__ quotes_before, const uint32_t* __restrict__ tile_even,
                                  const uint32_t* __restrict__ tile_odd, uint64_t* __restrict__ counts, uint64_t ntiles) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) counts[t] = (quotes_before[t] & 1u) ? tile_odd[t] : tile_even[t];
}

// ---- 2. positions of the record separators ('\n' outside quotes), in text order ----------------------------------
__global__ __launch_bounds__(kCsvThreads) void k_csv_separators(const uint8_t* __restrict__ d, uint64_t size,
                                                               const uint32_t* __restrict__ quotes_before,
                                                               const uint64_t* __restrict__ sep_base, uint64_t* __restrict__ seps) {
    __shared__ uint32_t s_par[kCsvChunks * kCsvWaves];
    __shared__ uint32_t s_cnt[kCsvChunks * kCsvWaves];
    const uint64_t t = blockIdx.x;
    const uint64_t tile_base = t * kCsvTile;
    const TileScan r = scan_tile(d, size, tile_base, quotes_before[t], s_par);
    uint32_t incl[kCsvChunks], cnt[kCsvChunks];
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        cnt[j] = (uint32_t)__popc(r.even[j]);
        incl[j] = wave_inclusive_sum(cnt[j]);
        if (lane_id() == kWave - 1) s_cnt[j * kCsvWaves + wave_id()] = incl[j];
    }
    __syncthreads();
    uint64_t run = sep_base[t];
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        uint64_t mine = 0;
#pragma unroll
        for (int w = 0; w < kCsvWaves; w++) {
            if (w == wave_id()) mine = run;
            run += s_cnt[j * kCsvWaves + w];
        }
        uint64_t o = mine + incl[j] - cnt[j];
        const uint64_t pos = tile_base + ((uint64_t)j * kCsvThreads + threadIdx.x) * 16;
        uint32_t mk = r.even[j];
        while (mk) {
            const int b = __ffs(mk) - 1;
            mk &= mk - 1;
            seps[o++] = pos + b;
        }
    }
}

// ---- 1L / 1M / 2L / 2M: the separator passes under LazyQuotes (the automaton: csv_lazy_device.hpp) --------------------
constexpr int kLazyScanThreads = 1024;
constexpr int kLazyScanStep = kLazyScanThreads;   // tiles per step of k_csv_lazy_tile_entry: one per thread (16 MiB of text)
constexpr int kLazyMarkChunks = 8;                // k_csv_lazy_separators: masks per thread = one 16-byte load
constexpr int kLazySepTiles = kCsvThreads * kLazyMarkChunks * 16 / kCsvTile;   // text tiles per workgroup there
static_assert(kLazySepTiles * kCsvTile == kCsvThreads * kLazyMarkChunks * 16, "a separator workgroup covers whole tiles");

__device__ __forceinline__ LzMap lz_shfl_up(const LzMap& v, int d) {
    return LzMap{(uint32_t)__shfl_up(v.lo, d, kWave), (uint32_t)__shfl_up(v.hi, d, kWave)};
}
// lane l gets the composition of the maps of lanes 0 .. l, in lane order
__device__ __forceinline__ LzMap lz_wave_inclusive(LzMap v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const LzMap o = lz_shfl_up(v, d);
        if (lane_id() >= d) v = lz_compose(o, v);
    }
    return v;
}
__device__ __forceinline__ LzMap lz_wave_exclusive(const LzMap& incl) {
    const LzMap ex = lz_shfl_up(incl, 1);
    return lane_id() == 0 ? lz_identity() : ex;
}

// This thread's kCsvChunks chunks of the tile (w[j] = the 16 bytes at tile_base + (j*256 + t)*16, zeros past the text's end: a zero
// byte is no newline, and the map of the text's last tile is never applied), each chunk's map scanned over its wave (incl[j]) and
// every (round, wave) stretch's map in s_map[j * kCsvWaves + wave].  Ends with a __syncthreads.
template <bool TRIM, bool CMT>
__device__ __forceinline__ void lazy_scan_tile(const uint8_t* __restrict__ d, uint64_t size, uint64_t tile_base, const LzTable& tb,
                                               uint32_t (&w)[kCsvChunks][4], LzMap (&incl)[kCsvChunks], LzMap* s_map) {
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        const uint64_t pos = tile_base + ((uint64_t)j * kCsvThreads + threadIdx.x) * 16;
        w[j][0] = w[j][1] = w[j][2] = w[j][3] = 0;
        if (pos + 16 <= size) {
            const uint4 v = *reinterpret_cast<const uint4*>(d + pos);
            w[j][0] = v.x; w[j][1] = v.y; w[j][2] = v.z; w[j][3] = v.w;
        } else {
            for (uint64_t k = pos; k < size; k++) w[j][(k - pos) >> 2] |= (uint32_t)d[k] << (8 * ((k - pos) & 3));
        }
        incl[j] = lz_wave_inclusive(lz_walk16<TRIM, CMT, false>(w[j], tb, lz_identity(), nullptr));
        if (lane_id() == kWave - 1) s_map[j * kCsvWaves + wave_id()] = incl[j];
    }
    __syncthreads();
}

template <bool TRIM, bool CMT>
__device__ __forceinline__ void lazy_tile_map(const uint8_t* __restrict__ d, uint64_t size, const LzTable& tb, uint32_t* __restrict__ tile_map,
                                              LzMap* s_map) {
    uint32_t w[kCsvChunks][4];
    LzMap incl[kCsvChunks];
    lazy_scan_tile<TRIM, CMT>(d, size, (uint64_t)blockIdx.x * kCsvTile, tb, w, incl, s_map);
    if (threadIdx.x == 0) {
        LzMap run = lz_identity();
#pragma unroll
        for (int k = 0; k < kCsvChunks * kCsvWaves; k++) run = lz_compose(run, s_map[k]);
        tile_map[blockIdx.x] = lz_pack(run);
    }
}
__global__ __launch_bounds__(kCsvThreads) void k_csv_lazy_tile_maps(const uint8_t* __restrict__ d, uint64_t size, LzTable tb,
                                                                   uint32_t* __restrict__ tile_map) {
    __shared__ LzMap s_map[kCsvChunks * kCsvWaves];
    if (tb.trim) {   // (uniform)
        if (tb.comment < 0x100u) lazy_tile_map<true, true>(d, size, tb, tile_map, s_map);
        else lazy_tile_map<true, false>(d, size, tb, tile_map, s_map);
    } else {
        if (tb.comment < 0x100u) lazy_tile_map<false, true>(d, size, tb, tile_map, s_map);
        else lazy_tile_map<false, false>(d, size, tb, tile_map, s_map);
    }
}

// tile_map[t] (packed map of tile t) -> the state in front of tile t, RS in front of tile 0.  ONE workgroup.
__global__ __launch_bounds__(kLazyScanThreads) void k_csv_lazy_tile_entry(uint32_t* __restrict__ tile_map, uint64_t ntiles) {
    constexpr int kW = kLazyScanThreads / kWave;
    __shared__ LzMap s_w[kW];
    uint32_t carry = kLzRS;
    const uint32_t id = lz_pack(lz_identity());
    uint32_t nxt = threadIdx.x < ntiles ? tile_map[threadIdx.x] : id;
    for (uint64_t base = 0; base < ntiles; base += kLazyScanStep) {
        const uint64_t t = base + threadIdx.x;
        const LzMap m = lz_unpack(nxt);
        nxt = t + kLazyScanStep < ntiles ? tile_map[t + kLazyScanStep] : id;   // in flight while this step is scanned
        const LzMap incl = lz_wave_inclusive(m);
        if (lane_id() == kWave - 1) s_w[wave_id()] = incl;
        const LzMap ex = lz_wave_exclusive(incl);
        __syncthreads();
        LzMap pre = lz_identity(), tot = lz_identity();
#pragma unroll
        for (int w = 0; w < kW; w++) {
            if (w == wave_id()) pre = tot;
            tot = lz_compose(tot, s_w[w]);
        }
        if (t < ntiles) tile_map[t] = lz_apply(lz_compose(pre, ex), carry);
        carry = lz_apply(tot, carry);
        __syncthreads();   // s_w is rewritten by the next step
    }
}

template <bool TRIM, bool CMT>
__device__ __forceinline__ void lazy_tile_marks(const uint8_t* __restrict__ d, uint64_t size, const LzTable& tb, uint32_t entry,
                                                uint16_t* __restrict__ marks, uint64_t* __restrict__ counts, LzMap* s_map, uint32_t* s_cnt) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    uint32_t w[kCsvChunks][4];
    LzMap incl[kCsvChunks];
    const uint64_t t = blockIdx.x;
    lazy_scan_tile<TRIM, CMT>(d, size, t * kCsvTile, tb, w, incl, s_map);
    LzMap run = lz_constant(entry);   // every byte = the one true state, from here on
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < kCsvChunks; j++) {
        LzMap mine = run;
#pragma unroll
        for (int wv = 0; wv < kCsvWaves; wv++) {
            if (wv == wave_id()) mine = run;
            run = lz_compose(run, s_map[j * kCsvWaves + wv]);
        }
        uint32_t mk = 0;
        lz_walk16<TRIM, CMT, true>(w[j], tb, lz_compose(mine, lz_wave_exclusive(incl[j])), &mk);
        total += (uint32_t)__popc(mk);
        // eight lanes' masks = one 16-byte store
        const uint32_t v = mk | ((uint32_t)__shfl_down(mk, 1, kWave) << 16);
        u32x4 q;
        q.x = v;
        q.y = (uint32_t)__shfl_down(v, 2, kWave);
        q.z = (uint32_t)__shfl_down(v, 4, kWave);
        q.w = (uint32_t)__shfl_down(v, 6, kWave);
        if ((threadIdx.x & 7u) == 0) *reinterpret_cast<u32x4*>(marks + t * (kCsvTile / 16) + (uint64_t)j * kCsvThreads + threadIdx.x) = q;
    }
    total = wave_sum(total);
    if (lane_id() == 0) s_cnt[wave_id()] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (int wv = 0; wv < kCsvWaves; wv++) s += s_cnt[wv];
        counts[t] = s;
    }
}
// marks: one 16-bit mask per 16-byte chunk of every tile (ntiles * 1024 of them, 16-byte aligned); counts[t] = separators of tile t
__global__ __launch_bounds__(kCsvThreads) void k_csv_lazy_marks(const uint8_t* __restrict__ d, uint64_t size, LzTable tb,
                                                               const uint32_t* __restrict__ tile_entry, uint16_t* __restrict__ marks,
                                                               uint64_t* __restrict__ counts) {
    __shared__ LzMap s_map[kCsvChunks * kCsvWaves];
    __shared__ uint32_t s_cnt[kCsvWaves];
    const uint32_t entry = tile_entry[blockIdx.x];
    if (tb.trim) {   // (uniform)
        if (tb.comment < 0x100u) lazy_tile_marks<true, true>(d, size, tb, entry, marks, counts, s_map, s_cnt);
        else lazy_tile_marks<true, false>(d, size, tb, entry, marks, counts, s_map, s_cnt);
    } else {
        if (tb.comment < 0x100u) lazy_tile_marks<false, true>(d, size, tb, entry, marks, counts, s_map, s_cnt);
        else lazy_tile_marks<false, false>(d, size, tb, entry, marks, counts, s_map, s_cnt);
    }
}

// positions of the separators, in text order, from the masks alone.  Workgroup b: the chunks of the tiles [b * kLazySepTiles, ...),
// eight consecutive chunks per thread; sep_base = exclusive scan of k_csv_lazy_marks' counts.
__global__ __launch_bounds__(kCsvThreads) void k_csv_lazy_separators(const uint16_t* __restrict__ marks, uint64_t nchunks,
                                                                    const uint64_t* __restrict__ sep_base, uint64_t* __restrict__ seps) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t s_scan[kCsvWaves + 1];
    const uint64_t c0 = ((uint64_t)blockIdx.x * kCsvThreads + threadIdx.x) * kLazyMarkChunks;
    u32x4 q = {0, 0, 0, 0};
    if (c0 < nchunks) q = *reinterpret_cast<const u32x4*>(marks + c0);   // (nchunks is a multiple of kLazyMarkChunks)
    const uint32_t m[4] = {q.x, q.y, q.z, q.w};
    const uint32_t cnt = (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
    uint32_t total;
    const uint32_t ex = block_exclusive_sum<uint32_t, kCsvThreads>(cnt, s_scan, &total);
    if (!cnt) return;
    uint64_t o = sep_base[(uint64_t)blockIdx.x * kLazySepTiles] + ex;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t mk = m[k];   // two chunks: bit b = byte b of the 32 bytes at chunk c0 + 2k
        while (mk) {
            const int b = __ffs(mk) - 1;
            mk &= mk - 1;
            seps[o++] = (c0 + 2 * (uint64_t)k) * 16 + (uint64_t)b;
        }
    }
}

// ---- 3. classify segments ---------------------------------------------------------------------------------
// segment s = bytes [s ? seps[s-1]+1 : 0, seps[s]) (the separator itself excluded; seps[nseg-1] may be `size`).
// keep[s] = 1 for a record, 0 for an empty or comment line.  rec range written for kept segments later.
__device__ __forceinline__ void segment_range(const uint8_t* d, const uint64_t* seps, uint64_t s, uint64_t* b, uint64_t* e) {
    *b = s ? seps[s - 1] + 1 : 0;
    uint64_t end = seps[s];
    if (end > *b && d[end - 1] == '\r') end--;   // "\r\n" -> "\n"; a final "\r" at EOF is dropped too
    *e = end;
}

// stats[0] += kept segments; stats[1] = 1 if a segment other than the last one was dropped; stats[2] = 1 if unsupported
__global__ void k_csv_classify(const uint8_t* __restrict__ d, const uint64_t* __restrict__ seps, uint64_t nseg, CsvOpts o,
                               uint32_t* __restrict__ keep, unsigned long long* __restrict__ stats) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t kept = 0;
    bool dropped_inner = false;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        uint64_t b, e;
        segment_range(d, seps, s, &b, &e);
        uint32_t k = 1;
        if (e == b) k = 0;
        else if (o.comment && d[b] == o.comment) {
            k = 0;
            // a comment is skipped WITHOUT interpreting its quotes; the parity model cannot do that
            for (uint64_t i = b; i < e; i++)
                if (d[i] == '"') atomicExch(&stats[2], 1ull);
        }
        keep[s] = k;
        kept += k;
        dropped_inner |= !k && s + 1 < nseg;
    }
    if (__any(dropped_inner) && lane_id() == 0) atomicExch(&stats[1], 1ull);
    __shared__ uint32_t s_kept[4];
    kept = wave_sum(kept);
    if (lane_id() == 0) s_kept[wave_id()] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
        if (total) atomicAdd(&stats[0], (unsigned long long)total);
    }
}

// rec_e keeps the RAW end (a trailing '\r' is stripped by the parser, which reads it from LDS)
__global__ void k_csv_compact(const uint64_t* __restrict__ seps, uint64_t nseg, const uint32_t* __restrict__ keep_scan,
                              const uint32_t* __restrict__ keep_flag, uint64_t* __restrict__ rec_b, uint64_t* __restrict__ rec_e) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        if (!keep_flag[s]) continue;
        rec_b[keep_scan[s]] = s ? seps[s - 1] + 1 : 0;
        rec_e[keep_scan[s]] = seps[s];
    }
}

// Where record r lies in the text: [b, e) with e the RAW end (the separator position, or the text size).
// Identity mode (seps != NULL): no segment was dropped except possibly the last, so record r IS segment r.
struct RecIndex {
    const uint64_t* seps;
    const uint64_t* rec_b;
    const uint64_t* rec_e;
    __device__ __forceinline__ void get(uint64_t r, uint64_t* b, uint64_t* e) const {
        if (seps) {
            *b = r ? seps[r - 1] + 1 : 0;
            *e = seps[r];
        } else {
            *b = rec_b[r];
            *e = rec_e[r];
        }
    }
};

// ---- 4. the sequential field parser (one record) ---------------------------------------------------------------
// Text sources: global memory, or the tile's bytes staged in LDS (addressed by their global offset).
struct GlobalSrc {
    const uint8_t* d;
    __device__ __forceinline__ uint8_t operator[](uint64_t p) const { return d[p]; }
};
struct LdsSrc {
    const CPH_LDS uint8_t* s;   // holds the text from global offset `base` on
    uint64_t base;
    __device__ __forceinline__ uint8_t operator[](uint64_t p) const { return s[p - base]; }
};

template <class Src>
__device__ __forceinline__ bool rune_is_space_at(const Src& d, uint64_t p, uint64_t e, int* len) {
    const uint32_t b0 = d[p], b1 = p + 1 < e ? d[p + 1] : 0, b2 = p + 2 < e ? d[p + 2] : 0;
    *len = b0 < 0x80 ? 1 : (b0 < 0xE0 ? 2 : 3);
    if (b0 < 0x80) return b0 == ' ' || (b0 >= 9 && b0 <= 13);
    if (b0 == 0xC2 && p + 1 < e) return b1 == 0x85 || b1 == 0xA0;
    if (p + 2 >= e) return false;
    if (b0 == 0xE1) return b1 == 0x9A && b2 == 0x80;
    if (b0 == 0xE2) {
        if (b1 == 0x80) return (b2 >= 0x80 && b2 <= 0x8A) || b2 == 0xA8 || b2 == 0xA9 || b2 == 0xAF;
        return b1 == 0x81 && b2 == 0x9F;
    }
    return b0 == 0xE3 && b1 == 0x80 && b2 == 0x80;
}

enum { kCsvOk = 0, kCsvBareQuote = CPH_CSV_ERR_BARE_QUOTE, kCsvQuote = CPH_CSV_ERR_QUOTE,
       kCsvFieldCount = CPH_CSV_ERR_FIELD_COUNT,
       kCsvLazySpace = 8 };   // LAZY + TrimLeadingSpace: a multi-byte space in front of an opening quote (its error key's kind bits are 0: it
                              // outranks a field count error of the same record, whose field count means nothing)

// Sink: begin(field) ... put(byte)* ... end(field) for every COMPLETE field.  Returns the number of fields;
// *err = kind of the first problem (the field it happens in is never end()ed).
// LAZY (Reader.LazyQuotes): a quote in an unquoted field is a byte; in a quoted field a quote that is followed by neither a quote,
// Comma nor the record's end is a byte, and the record's end closes the field.  No ErrBareQuote, no ErrQuote.
template <bool LAZY = false, class Src, class Sink>
__device__ __forceinline__ int csv_parse_record(const Src& d, uint64_t b, uint64_t e, const CsvOpts& o, Sink& s, int* err) {
    uint64_t p = b;
    int field = 0;
    *err = kCsvOk;
    for (;;) {
        if (o.trim) {
            int l;
            bool wide = false;
            while (p < e && rune_is_space_at(d, p, e, &l)) { p += l; wide |= l > 1; }
            if (p > e) p = e;
            // the separator scan trims ASCII spaces only and took this field for an unquoted one (csv_lazy_device.hpp)
            if (LAZY && wide && p < e && d[p] == '"') { *err = kCsvLazySpace; return field + 1; }
        }
        if (p >= e || d[p] != '"') {   // unquoted field
            uint64_t i = p;
            bool bare = false;
            while (i < e) {
                const uint8_t c = d[i];
                if (c == o.comma) break;
                bare |= c == '"';
                i++;
            }
            if (!LAZY && bare) { *err = kCsvBareQuote; return field + 1; }
            s.begin(field);
            if (s.wanted())
                for (uint64_t k = p; k < i; k++) s.put(d[k]);
            else
                s.skip(i - p);
            s.end(field);
            field++;
            if (i < e) { p = i + 1; continue; }
            return field;
        }
        p++;   // quoted field
        s.begin(field);
        for (;;) {
            while (p < e) {
                const uint8_t c = d[p];
                if (c == '"') break;
                if (c == '\r' && p + 1 < e && d[p + 1] == '\n') { p++; continue; }   // "\r\n" -> "\n" inside quotes
                s.put(c);
                p++;
            }
            if (p >= e) {   // no closing quote before the record ends
                if (LAZY) { s.end(field); return field + 1; }
                *err = kCsvQuote;
                return field + 1;
            }
            p++;
            if (p < e && d[p] == '"') { s.put('"'); p++; continue; }
            if (p < e && d[p] == o.comma) { p++; s.end(field); field++; break; }
            if (p == e) { s.end(field); return field + 1; }
            if (LAZY) { s.put('"'); continue; }   // a literal quote; the byte behind it is content of the same field
            *err = kCsvQuote;
            return field + 1;
        }
    }
}

// length of every wanted field -> lens[c][r] (no per-thread arrays: the store happens when the field ends)
template <class OT>
struct LenSink {
    const CsvCols* cols;
    OT* lens;            // column c, this record: lens[c * stride]
    uint64_t stride;
    uint64_t flen;
    CPH_LDS uint32_t* mine;   // this thread's copy of its lengths: mine[c * kCsvThreads] (the tile total reads it back from LDS, not from global memory)
    __device__ __forceinline__ void begin(int) { flen = 0; }
    __device__ __forceinline__ bool wanted() const { return false; }
    __device__ __forceinline__ void skip(uint64_t n) { flen += n; }
    __device__ __forceinline__ void put(uint8_t) { flen++; }
    __device__ __forceinline__ void end(int field) {
        for (int c = 0; c < cols->ncols; c++)
            if (cols->index[c] == field) {
                lens[(uint64_t)c * stride] = (OT)flen;
                mine[c * kCsvThreads] = (uint32_t)flen;
            }
    }
};

// bytes of every wanted field -> its column.  DestFn(c) = where column c's value of this record starts.
template <class Ptr, class DestFn>
struct CopySink {
    const CsvCols* cols;
    DestFn dest;
    Ptr cur;
    uint32_t want;      // columns that take the current field
    uint64_t k;         // bytes of the current field so far
    __device__ __forceinline__ void begin(int field) {
        want = 0;
        k = 0;
        for (int c = 0; c < cols->ncols; c++)
            if (cols->index[c] == field) want |= 1u << c;
        if (want) cur = dest(__ffs(want) - 1);
    }
    __device__ __forceinline__ bool wanted() const { return want != 0; }
    __device__ __forceinline__ void skip(uint64_t) {}
    __device__ __forceinline__ void put(uint8_t b) {
        if (!want) return;
        cur[k] = b;
        uint32_t more = want & (want - 1);   // the same field requested by several columns: rare
        while (more) {
            dest(__ffs(more) - 1)[k] = b;
            more &= more - 1;
        }
        k++;
    }
    __device__ __forceinline__ void end(int) {}
};

// one 16-bit mask per staged 16-byte chunk (+ slack for 64-bit reads)
__host__ __device__ constexpr int csv_mask_halves(int stage) { return stage / 16 + 8; }

// Stages the text [gb, ge) (gb multiple of 16) into LDS with coalesced 16-byte loads, and with it one bit per
// byte for "is the delimiter" / "is a quote": bit j of the 64-bit word w of a mask = byte gb + 64*w + j.
__device__ __forceinline__ void stage_text(const uint8_t* __restrict__ d, uint64_t size, uint64_t gb, uint64_t ge, uint8_t comma,
                                           CPH_LDS uint8_t* stage, CPH_LDS uint16_t* comma_mask, CPH_LDS uint16_t* quote_mask) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t cpat = 0x01010101u * comma;
    for (uint64_t off = (uint64_t)threadIdx.x * 16; gb + off < ge; off += (uint64_t)kCsvThreads * 16) {
        u32x4 v = {0, 0, 0, 0};
        if (gb + off + 16 <= size) {
            v = *reinterpret_cast<const u32x4*>(d + gb + off);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint64_t q = gb + off; q < size; q++) w[(q - gb - off) >> 2] |= (uint32_t)d[q] << (8 * ((q - gb - off) & 3));
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *(CPH_LDS u32x4*)(stage + off) = v;
        comma_mask[off >> 4] = (uint16_t)(eq_mask4(v.x, cpat) | eq_mask4(v.y, cpat) << 4 | eq_mask4(v.z, cpat) << 8 | eq_mask4(v.w, cpat) << 12);
        quote_mask[off >> 4] = (uint16_t)(eq_mask4(v.x, 0x22222222u) | eq_mask4(v.y, 0x22222222u) << 4 | eq_mask4(v.z, 0x22222222u) << 8 |
                                          eq_mask4(v.w, 0x22222222u) << 12);
    }
}

// first set bit at a position in [p, e) of a staged mask (positions relative to the stage start), or e
__device__ __forceinline__ uint32_t next_set(const CPH_LDS uint64_t* mask, uint32_t p, uint32_t e) {
    uint32_t w = p >> 6;
    uint64_t m = mask[w] & (~0ull << (p & 63));
    while (m == 0) {
        w++;
        if (w * 64 >= e) return e;
        m = mask[w];
    }
    const uint32_t pos = w * 64 + (uint32_t)__ffsll((long long)m) - 1;
    return pos < e ? pos : e;
}

// A record without any quote (and no TrimLeadingSpace): its fields are the runs between delimiters.
template <class Sink>
__device__ __forceinline__ int csv_split_plain(const LdsSrc& src, const CPH_LDS uint64_t* comma_mask, uint64_t b, uint64_t e, Sink& s) {
    uint32_t p = (uint32_t)(b - src.base);
    const uint32_t end = (uint32_t)(e - src.base);
    int field = 0;
    for (;;) {
        const uint32_t c = p < end ? next_set(comma_mask, p, end) : end;
        s.begin(field);
        if (s.wanted())
            for (uint32_t k = p; k < c; k++) s.put(src.s[k]);
        else
            s.skip(c - p);
        s.end(field);
        field++;
        if (c >= end) return field;
        p = c + 1;
    }
}

// One tile = 256 consecutive records, one per thread.  Every thread first loads its own record bounds (one
// global latency for the whole tile: the tile's text range is thread 0's begin .. the last thread's end).
// Tiles are aligned so that the first RETURNED record (index `pad`-shifted: record r sits at linear slot r + pad, pad < 256)
// starts a tile: the copy pass walks the same tiles, and tile_tot[c * ntile + T] = the bytes of column c in tile T is all it
// needs of a scan — the offsets of a tile's records are a workgroup-local prefix sum on top of the tile's base (round 5:
// the per-record scans over every column, 1.2 of the parse's 4.9 ms, are gone).
template <class OT, bool LAZY = false>
__global__ __launch_bounds__(kCsvThreads) void k_csv_fields(const uint8_t* __restrict__ d, uint64_t size, RecIndex ri, uint64_t nrec,
                                                           CsvOpts o, CsvCols cols, OT* __restrict__ lens /* column c at lens + c * lens_stride */,
                                                           uint64_t lens_stride, uint32_t* __restrict__ nfields,
                                                           unsigned long long* __restrict__ err_key, int stage_bytes, uint32_t pad,
                                                           uint64_t ntile, uint64_t* __restrict__ tile_tot) {
    // dynamic LDS: text stage (stage_bytes + 16) | delimiter mask | quote mask | this tile's lengths [ncols][256]
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_tot[kMaxKeyCols][kCsvWaves];
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    CPH_LDS uint16_t* s_cm = (CPH_LDS uint16_t*)(stage + stage_bytes + 16);
    CPH_LDS uint16_t* s_qm = s_cm + csv_mask_halves(stage_bytes);
    CPH_LDS uint32_t* s_len = (CPH_LDS uint32_t*)(s_qm + csv_mask_halves(stage_bytes));
    // a tile's record bounds are loaded one tile AHEAD (while the tile before it is staged and parsed): the chain of dependent
    // global round trips per tile is bounds -> text -> stores, and the workgroups wait on it, not on bandwidth
    auto bounds = [&](uint64_t T, uint64_t* b, uint64_t* e) -> bool {
        const uint64_t lin = T * kCsvThreads + threadIdx.x;
        const bool h = T < ntile && lin >= pad && lin - pad < nrec;
        *b = *e = 0;
        if (h) ri.get(lin - pad, b, e);
        return h;
    };
    uint64_t nb, ne;
    bool nhas = bounds(blockIdx.x, &nb, &ne);
    for (uint64_t T = blockIdx.x; T < ntile; T += gridDim.x) {
        const bool has = nhas;
        uint64_t b = nb, e = ne;
        const uint64_t r = T * kCsvThreads + threadIdx.x - pad;
        const uint64_t rfirst = T * kCsvThreads >= pad ? T * kCsvThreads - pad : 0;
        const uint64_t rlast = ((T + 1) * kCsvThreads - pad < nrec ? (T + 1) * kCsvThreads - pad : nrec) - 1;
        if (has) {
            if (r == rfirst) s_range[0] = b & ~15ull;
            if (r == rlast) s_range[1] = e;
        }
        __syncthreads();
        nhas = bounds(T + gridDim.x, &nb, &ne);   // in flight while this tile is staged and parsed
        const uint64_t gb = s_range[0], ge = s_range[1];
        const bool staged = ge - gb <= (uint64_t)stage_bytes;
        if (staged) stage_text(d, size, gb, ge, o.comma, stage, s_cm, s_qm);
        for (int c = 0; c < cols.ncols; c++) s_len[c * kCsvThreads + threadIdx.x] = 0;   // (a record with fewer fields: the value is "")
        __syncthreads();
        if (has) {
            LenSink<OT> s{&cols, lens + r, lens_stride, 0, s_len + threadIdx.x};
            int err = 0, nf;
            if (staged) {
                const LdsSrc src{stage, gb};
                if (e > b && src[e - 1] == '\r') e--;
                if (!o.trim && next_set((const CPH_LDS uint64_t*)s_qm, (uint32_t)(b - gb), (uint32_t)(e - gb)) == (uint32_t)(e - gb))
                    nf = csv_split_plain(src, (const CPH_LDS uint64_t*)s_cm, b, e, s);
                else
                    nf = csv_parse_record<LAZY>(src, b, e, o, s, &err);
            } else {
                const GlobalSrc src{d};
                if (e > b && src[e - 1] == '\r') e--;
                nf = csv_parse_record<LAZY>(src, b, e, o, s, &err);
            }
            nfields[r] = (uint32_t)nf;
            for (int c = 0; c < cols.ncols; c++)   // a record with fewer fields: the value is ""
                if (cols.index[c] >= nf || err) {
                    lens[(uint64_t)c * lens_stride + r] = 0;
                    s_len[c * kCsvThreads + threadIdx.x] = 0;
                }
            if (err) atomicMin(err_key, ((unsigned long long)r << 3) | (unsigned long long)(err & 7));
        }
        if (tile_tot) {   // uniform
            for (int c = 0; c < cols.ncols; c++) {   // (a thread reads back its own LDS words: no barrier needed in front)
                const uint32_t v = wave_sum(has ? s_len[c * kCsvThreads + threadIdx.x] : 0u);
                if (lane_id() == 0) s_tot[c][wave_id()] = v;
            }
            __syncthreads();
            if ((int)threadIdx.x < cols.ncols) {
                uint64_t tsum = 0;
                for (int w = 0; w < kCsvWaves; w++) tsum += s_tot[threadIdx.x][w];
                tile_tot[(uint64_t)threadIdx.x * ntile + T] = tsum;
            }
        }
        __syncthreads();   // s_range / s_tot / s_len are rewritten by the next tile
    }
}

__global__ void k_csv_check_counts(const uint32_t* __restrict__ nfields, uint64_t nrec, int32_t fields_per_record,
                                   unsigned long long* __restrict__ err_key) {
    const uint32_t expected = fields_per_record > 0 ? (uint32_t)fields_per_record : nfields[0];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += stride)
        if (nfields[r] != expected) atomicMin(err_key, ((unsigned long long)r << 3) | (unsigned long long)kCsvFieldCount);
}

// Where this record's value of column c goes in global memory: the tile's base (64-bit) + the record's offset inside the tile
// (modular difference of the 32-bit offsets the tile keeps in LDS).
struct GlobalDest {
    uint8_t* const* out_data;
    const uint64_t* obase;               // [ncols] (LDS)
    const CPH_LDS uint32_t* off32;       // as in LdsDest
    uint32_t i;
    __device__ __forceinline__ uint8_t* operator()(int c) const {
        const CPH_LDS uint32_t* oc = off32 + c * (kCsvThreads + 1);
        return out_data[c] + obase[c] + (uint64_t)(oc[i] - oc[0]);
    }
};
struct LdsDest {
    CPH_LDS uint8_t* stage;
    const CPH_LDS uint32_t* colstart;    // start of column c's region (already shifted by obase & 15)
    const CPH_LDS uint32_t* off32;       // low 32 bits of offs[c][r0 + i] at [c * (kCsvThreads + 1) + i]
    uint32_t i;                          // this thread's record within the tile
    __device__ __forceinline__ CPH_LDS uint8_t* operator()(int c) const {
        const CPH_LDS uint32_t* oc = off32 + c * (kCsvThreads + 1);
        return stage + colstart[c] + (oc[i] - oc[0]);   // modular difference: a tile's span is far below 4 GiB
    }
};

// dynamic LDS: text stage | output stage | delimiter mask | quote mask | off32[ncols][257]
// offs (in / out): column c's entries start at offs + c * stride; entry r holds the LENGTH of output record r's value on entry
// (k_csv_fields) and its OFFSET on exit (entry nout: the column's size).  tile_scan = exclusive scan of k_csv_fields' tile totals
// over the concatenation [ncols][ntile] (+ the grand total): column c's bytes in front of output tile t are
// tile_scan[c * ntile + T0 + t] - tile_scan[c * ntile + T0].
template <class OT, bool LAZY = false>
__global__ __launch_bounds__(kCsvThreads) void k_csv_copy_fields(const uint8_t* __restrict__ d, uint64_t size, RecIndex ri, uint64_t first,
                                                                uint64_t nout, CsvOpts o, CsvCols cols, OT* __restrict__ offs,
                                                                uint64_t stride, uint8_t* const* __restrict__ out_data, int stage_bytes,
                                                                const uint64_t* __restrict__ tile_scan, uint64_t ntile, uint64_t T0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_colstart[kMaxKeyCols];
    __shared__ uint64_t s_obase[kMaxKeyCols];
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_scan[kCsvWaves + 1];
    const uint32_t kOutCap = (uint32_t)stage_bytes + 32 * kMaxKeyCols;   // tests/test_gpu_csv_strict_edges.py: out_cap(), copy_fits()
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    CPH_LDS uint8_t* ostage = stage + (stage_bytes + 16);
    CPH_LDS uint16_t* cmask = (CPH_LDS uint16_t*)(ostage + kOutCap);
    CPH_LDS uint16_t* qmask = cmask + csv_mask_halves(stage_bytes);
    CPH_LDS uint32_t* off32 = (CPH_LDS uint32_t*)(qmask + csv_mask_halves(stage_bytes));
    // record bounds, lengths and tile bases are loaded one tile AHEAD (k_csv_fields does the same): they are in flight while the
    // tile before is staged, parsed and flushed
    constexpr int kPre = 4;   // (tests/test_gpu_csv_strict_edges.py: K_PRE) columns whose lengths and bases are prefetched (registers); any further column is loaded in its tile
    uint32_t nlen[kPre];
    uint64_t nbase[kPre], nb = 0, ne = 0;
    auto prefetch = [&](uint64_t r0) {
        const uint64_t r = r0 + threadIdx.x;
        const bool h = r < nout;
        nb = ne = 0;
        if (h) ri.get(first + r, &nb, &ne);
#pragma unroll
        for (int c = 0; c < kPre; c++) {   // independent loads: one latency for all columns
            nlen[c] = (c < cols.ncols && h) ? (uint32_t)offs[(uint64_t)c * stride + r] : 0u;
            nbase[c] = (c < cols.ncols && r0 < nout) ? tile_scan[(uint64_t)c * ntile + T0 + r0 / kCsvThreads] - tile_scan[(uint64_t)c * ntile + T0] : 0ull;
        }
    };
    prefetch((uint64_t)blockIdx.x * kCsvThreads);
    for (uint64_t r0 = (uint64_t)blockIdx.x * kCsvThreads; r0 < nout; r0 += (uint64_t)gridDim.x * kCsvThreads) {
        const uint64_t rend = r0 + kCsvThreads < nout ? r0 + kCsvThreads : nout;
        const uint32_t nt = (uint32_t)(rend - r0);
        const uint64_t r = r0 + threadIdx.x;
        uint64_t b = nb, e = ne;
        if (r < rend) {
            if (threadIdx.x == 0) s_range[0] = b & ~15ull;
            if (r == rend - 1) s_range[1] = e;
        }
        {
            // lengths -> offsets: a workgroup-local exclusive sum per column on top of the tile's base; the offsets go back to
            // where the lengths were (and stay in LDS, low 32 bits, for the destinations below)
            uint32_t len[kPre];
            uint64_t tbase[kPre];
#pragma unroll
            for (int c = 0; c < kPre; c++) { len[c] = nlen[c]; tbase[c] = nbase[c]; }
            prefetch(r0 + (uint64_t)gridDim.x * kCsvThreads);
            for (int c = 0; c < cols.ncols; c++) {
                uint32_t mylen = 0;
                uint64_t base = 0;
                if (c < kPre) {
#pragma unroll
                    for (int q = 0; q < kPre; q++)
                        if (q == c) { mylen = len[q]; base = tbase[q]; }
                } else {
                    mylen = r < rend ? (uint32_t)offs[(uint64_t)c * stride + r] : 0u;
                    base = tile_scan[(uint64_t)c * ntile + T0 + r0 / kCsvThreads] - tile_scan[(uint64_t)c * ntile + T0];
                }
                uint32_t total;
                const uint32_t ex = block_exclusive_sum<uint32_t, kCsvThreads>(mylen, s_scan, &total);
                if (r < rend) {
                    off32[c * (kCsvThreads + 1) + threadIdx.x] = (uint32_t)base + ex;
                    offs[(uint64_t)c * stride + r] = (OT)(base + ex);
                }
                if (threadIdx.x == 0) {
                    off32[c * (kCsvThreads + 1) + nt] = (uint32_t)base + total;
                    s_obase[c] = base;
                    if (rend == nout) offs[(uint64_t)c * stride + nout] = (OT)(base + total);
                }
            }
        }
        __syncthreads();
        const uint64_t gb = s_range[0], ge = s_range[1];
        uint32_t pos = 0;
        bool fits = ge - gb <= (uint64_t)stage_bytes;
        for (int c = 0; c < cols.ncols && fits; c++) {
            const uint32_t span = off32[c * (kCsvThreads + 1) + nt] - off32[c * (kCsvThreads + 1)];
            if (threadIdx.x == 0) s_colstart[c] = pos + (uint32_t)(s_obase[c] & 15);
            if (span > kOutCap || pos + ((span + 31) & ~15u) > kOutCap) fits = false;
            pos += (span + 31) & ~15u;
        }
        if (fits) stage_text(d, size, gb, ge, o.comma, stage, cmask, qmask);
        __syncthreads();
        if (r < rend) {
            int err;
            if (fits) {
                const LdsSrc src{stage, gb};
                if (e > b && src[e - 1] == '\r') e--;
                CopySink<CPH_LDS uint8_t*, LdsDest> s{
                    &cols, LdsDest{ostage, (const CPH_LDS uint32_t*)s_colstart, off32, (uint32_t)threadIdx.x}, nullptr, 0, 0};
                if (!o.trim && next_set((const CPH_LDS uint64_t*)qmask, (uint32_t)(b - gb), (uint32_t)(e - gb)) == (uint32_t)(e - gb))
                    csv_split_plain(src, (const CPH_LDS uint64_t*)cmask, b, e, s);
                else
                    csv_parse_record<LAZY>(src, b, e, o, s, &err);
            } else {
                const GlobalSrc src{d};
                if (e > b && src[e - 1] == '\r') e--;
                CopySink<uint8_t*, GlobalDest> s{&cols, GlobalDest{out_data, s_obase, off32, (uint32_t)threadIdx.x}, nullptr, 0, 0};
                csv_parse_record<LAZY>(src, b, e, o, s, &err);
            }
        }
        __syncthreads();
        if (fits)
            for (int c = 0; c < cols.ncols; c++) {
                const uint32_t span = off32[c * (kCsvThreads + 1) + nt] - off32[c * (kCsvThreads + 1)];
                flush_stage(ostage + (s_colstart[c] - (uint32_t)(s_obase[c] & 15)), out_data[c], s_obase[c], span);
            }
        __syncthreads();
    }
}

// ================================================================================================================
// (round 6) The fast path: BYTE-parallel passes over TEXT tiles.
//
// k_csv_fields / k_csv_copy_fields above are record-parallel: one thread walks one record byte by byte through LDS, twice
// (lengths, then bytes) — 0.85 + 1.28 ms per 0.89 GB, 0.036 of the HBM roof, waiting on LDS byte work.  When the text holds NO quote
// at all (k_csv_tile_stats counts them), TrimLeadingSpace is off and no line in the middle is blank or a comment, every byte's
// role follows from two bit masks (delimiter, newline) and three workgroup scans:
//   record of a byte       = newlines before it                                  (sum scan)
//   field index of a byte  = delimiters since the last newline                   (segmented sum scan)
//   start of its field     = position behind the last delimiter / newline       (max scan)
// A tile OWNS the records that begin behind a newline inside its 16 KiB (tile 0 also owns record 0) and reads up to 4 KiB
// past its end to finish the last one.  Each thread looks at 64 bytes = two 64-bit masks, walks the ~10 terminators in them
// and knows for each the record, the field index and the field's extent:
//   k_csv_fast_count   bytes of every wanted column per tile (+ the field counts' minimum / maximum, and anything the fast
//                      path cannot do — a blank or comment line, a record beyond the staged window — raises *slow: the
//                      classic kernels then parse the text; the first error, if any, is theirs to report)
//   (one scan over the tiles' totals of all columns)
//   k_csv_fast_copy    the same walk with the tile's base known: offsets per record, field bytes gathered per column in LDS
//                      and streamed out.
// Neither k_csv_separators (0.22 ms, 8 bytes per record written) nor k_csv_classify (0.29 ms) runs: the text is read three times
// (tile statistics, count, copy), never walked byte by byte.
// ================================================================================================================
constexpr int kFtThreads = 320;
constexpr int kFtWaves = kFtThreads / kWave;
constexpr int kFtStage = kFtThreads * 64;   // 20 KiB staged per 16 KiB tile: a record may run 4 KiB past its tile (tests/test_gpu_csv_strict_edges.py: FT_STAGE)
constexpr int kFtOwn = kCsvTile / 64;       // the chunks (threads) of the tile's own 16 KiB
constexpr int kFtMaxCols = 8;
static_assert(kFtStage > kCsvTile && kFtStage % 64 == 0, "a tile's stage must reach past its end");
struct FtCols {
    int32_t ncols;
    int32_t index[kFtMaxCols];
};
// device words the two kernels share with the host
struct FtFlags {
    uint32_t slow;         // something the fast path cannot do
    uint32_t min_nf;       // fields per record, over all records
    uint32_t max_nf;
    uint32_t last_empty;   // nothing (or a lone '\r') behind the text's last newline: that line is no record
};

struct FtScan {   // what a thread's 64 bytes contribute, and the operator that chains them
    uint32_t nsep;   // newlines
    uint32_t cc;     // delimiters behind the last newline (all of them when there is none)
    uint32_t hs;     // has a newline
};
__device__ __forceinline__ FtScan ft_combine(const FtScan& a, const FtScan& b) {   // a in front of b
    FtScan r;
    r.nsep = a.nsep + b.nsep;
    r.cc = b.hs ? b.cc : a.cc + b.cc;
    r.hs = a.hs | b.hs;
    return r;
}
__device__ __forceinline__ FtScan ft_shfl_up(const FtScan& v, int d) {
    FtScan r;
    r.nsep = __shfl_up(v.nsep, d, kWave);
    r.cc = __shfl_up(v.cc, d, kWave);
    r.hs = __shfl_up(v.hs, d, kWave);
    return r;
}
// Exclusive scan over the workgroup's threads.  *own = the newlines of the tile's own 16 KiB (threads 0 .. kFtOwn - 1), *all = those of
// the whole staged window.  s_w: kFtWaves + 1 entries.  Two barriers.
__device__ __forceinline__ FtScan ft_block_exclusive(FtScan v, FtScan* s_w, uint32_t* own, uint32_t* all) {
    FtScan incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const FtScan o = ft_shfl_up(incl, d);
        if (lane_id() >= d) incl = ft_combine(o, incl);
    }
    if (lane_id() == kWave - 1) s_w[wave_id()] = incl;
    FtScan ex = ft_shfl_up(incl, 1);
    if (lane_id() == 0) ex = FtScan{0, 0, 0};
    __syncthreads();
    FtScan pre{0, 0, 0};
    uint32_t o = 0, a = 0;
#pragma unroll
    for (int w = 0; w < kFtWaves; w++) {
        if (w < wave_id()) pre = ft_combine(pre, s_w[w]);
        if (w < kFtOwn / kWave) o += s_w[w].nsep;
        a += s_w[w].nsep;
    }
    __syncthreads();
    *own = o;
    *all = a;
    return ft_combine(pre, ex);
}

// 0x80 in every byte of w that equals the pattern's byte
__device__ __forceinline__ uint32_t eq_hi4(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// Stages [tile_start, tile_start + kFtStage) (zeros past the text's end) and one bit per byte for delimiter / newline / '\r'; the
// text's end counts as a newline (it terminates the last record).  Returns whether this thread saw a quote.
__device__ __forceinline__ bool ft_stage(const uint8_t* __restrict__ d, uint64_t size, uint64_t tile_start, uint8_t comma, CPH_LDS uint8_t* stage,
                                         CPH_LDS uint16_t* cmask, CPH_LDS uint16_t* nmask, CPH_LDS uint16_t* rmask) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t cpat = 0x01010101u * comma;
    uint32_t quote = 0;
#pragma unroll
    for (int i = 0; i < kFtStage / (kFtThreads * 16); i++) {
        const uint32_t off = ((uint32_t)i * kFtThreads + threadIdx.x) * 16u;
        const uint64_t g = tile_start + off;
        u32x4 v = {0, 0, 0, 0};
        if (g + 16 <= size) {
            v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(d + g));
        } else if (g < size) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint64_t q = g; q < size; q++) w[(q - g) >> 2] |= (uint32_t)d[q] << (8 * ((q - g) & 3));
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *(CPH_LDS u32x4*)(stage + off) = v;
        quote |= eq_hi4(v.x, 0x22222222u) | eq_hi4(v.y, 0x22222222u) | eq_hi4(v.z, 0x22222222u) | eq_hi4(v.w, 0x22222222u);
        cmask[off >> 4] = (uint16_t)(eq_mask4(v.x, cpat) | eq_mask4(v.y, cpat) << 4 | eq_mask4(v.z, cpat) << 8 | eq_mask4(v.w, cpat) << 12);
        uint32_t nl = eq_mask4(v.x, 0x0A0A0A0Au) | eq_mask4(v.y, 0x0A0A0A0Au) << 4 | eq_mask4(v.z, 0x0A0A0A0Au) << 8 | eq_mask4(v.w, 0x0A0A0A0Au) << 12;
        if (size >= g && size - g < 16u) nl |= 1u << (uint32_t)(size - g);
        nmask[off >> 4] = (uint16_t)nl;
        rmask[off >> 4] = (uint16_t)(eq_mask4(v.x, 0x0D0D0D0Du) | eq_mask4(v.y, 0x0D0D0D0Du) << 4 | eq_mask4(v.z, 0x0D0D0D0Du) << 8 |
                                     eq_mask4(v.w, 0x0D0D0D0Du) << 12);
    }
    return quote != 0;
}

// inclusive XOR scan over the 64 positions, restarting where `cont` is clear (cont bit i: position i continues position i - 1)
__device__ __forceinline__ uint64_t ft_seg_xor(uint64_t v, uint64_t p) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        v ^= (v << s) & p;
        p &= (p << s) | ((1ull << s) - 1ull);
    }
    return v;
}
// the positions up to and including the k-th (k >= 1) set bit of m; all of them when m has fewer
__device__ __forceinline__ uint64_t ft_through_kth(uint64_t m, uint32_t k) {
    while (k > 1 && m) { m &= m - 1; k--; }
    return m ? (((m & (0ull - m)) << 1) - 1ull) : ~0ull;
}

// A tile OWNS the records that begin behind a newline of its own 16 KiB (tile 0: also record 0): in the staged window these are the
// bytes whose LOCAL record number (newlines in front of them, from the window's start) lies in [t ? 1 : 0, own]; record `own` ends at
// the window's newline number own + 1 — when the window holds it.
//   COUNT: tile_tot[c][t] = bytes of wanted column c; tile_tot[ncols][t] = newlines of the tile's own 16 KiB; flags.
//   COPY:  tile_tot holds the exclusive scan over the concatenation of these arrays.
// MAXC: 4 or 8 — the wanted columns the instantiation has registers for (per column: a 64-bit byte mask, position, span, base)
template <bool COPY, int MAXC>
__global__ __launch_bounds__(kFtThreads) void k_csv_fast(const uint8_t* __restrict__ d, uint64_t size, uint64_t ntiles, CsvOpts o, FtCols cols,
                                                        uint64_t first, uint64_t nrec /* COPY only */, uint64_t* __restrict__ tile_tot,
                                                        FtFlags* __restrict__ flags, uint32_t* __restrict__ offs /* column c at offs + c * stride */,
                                                        uint64_t stride, uint8_t* const* __restrict__ out_data, int dbg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ FtScan s_w[kFtWaves + 1];
    __shared__ uint32_t s_col[MAXC][kFtWaves + 1];
    __shared__ uint32_t s_sel[16];
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    CPH_LDS uint16_t* cmask = (CPH_LDS uint16_t*)(stage + kFtStage + 16);
    CPH_LDS uint16_t* nmask = cmask + kFtStage / 16 + 8;
    CPH_LDS uint16_t* rmask = nmask + kFtStage / 16 + 8;
    CPH_LDS uint8_t* ostage = (CPH_LDS uint8_t*)(rmask + kFtStage / 16 + 8);
    const uint64_t t = blockIdx.x;
    const uint64_t tile_start = t * kCsvTile;
    const uint32_t base = threadIdx.x * 64u;
    const bool quote = ft_stage(d, size, tile_start, o.comma, stage, cmask, nmask, rmask);
    if (threadIdx.x < 4) nmask[kFtStage / 16 + threadIdx.x] = 0;   // (the word behind the last chunk's: read as "the next chunk")
    if (COPY) {
        if (threadIdx.x < 16) {   // v_perm_b32 selectors: the bytes of a word that a 4-bit mask keeps, moved to its low end (0x0C = a zero byte)
            uint32_t sel = 0x0C0C0C0Cu, k = 0;
            for (uint32_t b = 0; b < 4; b++)
                if ((threadIdx.x >> b) & 1u) {
                    sel = (sel & ~(0xFFu << (8 * k))) | (b << (8 * k));
                    k++;
                }
            s_sel[threadIdx.x] = sel;
        }
        const u32x4 z = {0, 0, 0, 0};
        for (uint32_t i = threadIdx.x; i < (uint32_t)(kFtStage + 64) / 16; i += kFtThreads) ((CPH_LDS u32x4*)ostage)[i] = z;
    } else if (__ballot(quote) && lane_id() == 0) {
        atomicOr(&flags->slow, 1u);   // a quote: quoted fields are the classic kernels' business
    }
    __syncthreads();
    if (dbg & 1) return;
    const uint64_t cm = ((const CPH_LDS uint64_t*)cmask)[threadIdx.x], nm = ((const CPH_LDS uint64_t*)nmask)[threadIdx.x];
    const uint64_t rm = ((const CPH_LDS uint64_t*)rmask)[threadIdx.x];
    const uint64_t next_nl = ((const CPH_LDS uint64_t*)nmask)[threadIdx.x + 1] & 1ull;   // is the byte behind this chunk a newline
    FtScan mine;
    mine.nsep = (uint32_t)__popcll(nm);
    mine.hs = nm ? 1u : 0u;
    mine.cc = (uint32_t)__popcll(nm ? cm & ~((2ull << (63 - __clzll((long long)nm))) - 1ull) : cm);
    uint32_t own, all;
    const FtScan ex = ft_block_exclusive(mine, s_w, &own, &all);
    if (size - tile_start < (uint64_t)kCsvTile) own--;   // the text's end terminates a record, it does not begin one
    const uint32_t lo_rec = t ? 1u : 0u;
    const bool any = own >= lo_rec;          // (tile 0 always owns record 0)
    const bool slow = any && all < own + 1u;   // the last owned record's end is not in the window
    if (!COPY && slow && threadIdx.x == 0) atomicOr(&flags->slow, 1u);
    if (!any || slow) {
        if (!COPY && threadIdx.x <= (uint32_t)cols.ncols) tile_tot[(uint64_t)threadIdx.x * ntiles + t] = threadIdx.x == (uint32_t)cols.ncols && !slow ? own : 0;
        return;
    }
    // the bytes of owned records: local record number in [lo_rec, own]
    uint64_t vm = ~0ull;
    if (ex.nsep < lo_rec) vm = nm ? ~ft_through_kth(nm, 1) : 0ull;                       // behind the window's first newline
    if (ex.nsep > own) vm = 0;
    else if (ex.nsep + mine.nsep > own) vm &= ft_through_kth(nm, own - ex.nsep + 1u);   // through the newline that ends record `own`
    // a '\r' right in front of a record's terminating newline (or of the text's end) is not data: "\r\n" -> "\n" (segment_range)
    const uint64_t cr_strip = rm & ((nm >> 1) | (next_nl << 63));
    const uint64_t data = vm & ~(cm | nm) & ~cr_strip;
    const uint64_t nmv = nm & vm;   // the newlines that end owned records

    // ---- which of this thread's 64 bytes belong to which wanted column ----
    // The field index of a byte = the delimiters between the last newline and it, as FOUR BIT PLANES over the 64 positions: plane 0 is a
    // segmented prefix parity of the delimiter mask (segments restart behind newlines), plane b + 1 the same over the positions where
    // plane b carries.  No loop over the chunk's ~11 terminators, no divergence (the first version walked them: 1200 instructions
    // per chunk).  Positions in front of the chunk's first newline continue a record of the chunk before: their index starts at ex.cc.
    // A record with a 16th delimiter inside one chunk's reach aliases: *slow.
    uint64_t wm[MAXC] = {};
    bool bad = false;
    const uint64_t cont = ~(nm << 1);   // position i continues the record of position i - 1
    uint64_t e[4] = {0, 0, 0, 0};       // bit b of the number of delimiters in front of every position, since its record began (or the chunk)
    const bool wave_owns = __ballot(vm != 0) != 0;   // (the waves behind the last owned record's end — most of the overhang — have nothing to do)
    if (wave_owns) {
        uint64_t carry = cm;            // positions whose delimiter increments bit b
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint64_t incl = (dbg & 2) ? carry : ft_seg_xor(carry, cont);
            e[b] = (incl << 1) & cont;
            carry &= e[b];
        }
        if (carry & vm) bad = true;     // a 16th delimiter in one record
    }
    const uint64_t open = nm ? (((nm & (0ull - nm)) << 1) - 1ull) : ~0ull;   // up to and including the chunk's first newline
    // the record of the chunk's first byte.  COUNT does not know the records in front of its tile: only tile 0 can hold header records
    // (skip_records) — the kernel raises *slow otherwise
    const uint64_t rs = COPY ? tile_tot[(uint64_t)cols.ncols * ntiles + t] - tile_tot[(uint64_t)cols.ncols * ntiles] + ex.nsep
                             : (t ? first + ex.nsep : (uint64_t)ex.nsep);
    uint64_t keep = data;
    if (rs < first) keep = data & ~ft_through_kth(nm, (uint32_t)(first - rs));   // header records end inside or behind this chunk
    if (!COPY && t == 0 && threadIdx.x == 0 && first > (uint64_t)own + 1u) atomicOr(&flags->slow, 1u);
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        if (c >= cols.ncols || !wave_owns) continue;
        const uint32_t k = (uint32_t)cols.index[c];
        uint64_t m_closed = k < 16u ? ~open : 0ull, m_open = (k >= ex.cc && k - ex.cc < 16u) ? open : 0ull;
        const uint32_t ko = k - ex.cc;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            m_closed &= (k >> b) & 1u ? e[b] : ~e[b];
            m_open &= (ko >> b) & 1u ? e[b] : ~e[b];
        }
        wm[c] = (m_closed | m_open) & keep;
    }
    uint32_t colbytes[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) colbytes[c] = (uint32_t)__popcll(wm[c]);
    if (!COPY) {
        uint32_t nf_min = 0xFFFFFFFFu, nf_max = 0;
        if (!(dbg & 4) && wave_owns) {
            // empty lines (Go's Reader skips them; the classic path does): a newline right behind a newline or the text's first byte, also
            // with a '\r' in between
            const uint64_t pN = threadIdx.x ? ((const CPH_LDS uint64_t*)nmask)[threadIdx.x - 1] : 0ull;
            const uint64_t pR = threadIdx.x ? ((const CPH_LDS uint64_t*)rmask)[threadIdx.x - 1] : 0ull;
            const uint64_t st = (t == 0 && threadIdx.x == 0) ? 1ull : 0ull;
            const uint64_t PN = (nm << 1) | (pN >> 63) | st;          // position i begins a line
            const uint64_t PNm1 = (PN << 1) | ((pN >> 62) & 1ull);      // position i - 1 begins a line
            const uint64_t Rm1 = (rm << 1) | (pR >> 63);                // position i - 1 is a '\r'
            const uint64_t blank = nmv & (PN | (Rm1 & PNm1));
            const uint64_t eofpos = size - tile_start;
            const uint64_t eofbit = (eofpos >= base && eofpos < (uint64_t)base + 64u) ? 1ull << (eofpos - base) : 0ull;
            if (blank & ~eofbit) bad = true;
            if (blank & eofbit) flags->last_empty = 1u;
            // fields per record, at every newline that ends one
            uint64_t nls = nmv & ~blank;
            while (nls) {
                const uint32_t bit = (uint32_t)__ffsll((long long)nls) - 1u;
                nls &= nls - 1;
                uint32_t cntf = (uint32_t)((e[0] >> bit) & 1ull) | (uint32_t)((e[1] >> bit) & 1ull) << 1 | (uint32_t)((e[2] >> bit) & 1ull) << 2 |
                                (uint32_t)((e[3] >> bit) & 1ull) << 3;
                if ((open >> bit) & 1ull) cntf += ex.cc;
                nf_min = cntf + 1 < nf_min ? cntf + 1 : nf_min;
                nf_max = cntf + 1 > nf_max ? cntf + 1 : nf_max;
            }
            if (o.comment) {   // a record whose first byte is the comment character (Go's Reader skips the line): the classic path
                uint64_t starts = PN & vm;
                while (starts) {
                    const uint32_t bit = (uint32_t)__ffsll((long long)starts) - 1u;
                    starts &= starts - 1;
                    if (stage[base + bit] == o.comment) bad = true;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < MAXC; c++) {
            const uint32_t v = wave_sum(colbytes[c]);
            if (lane_id() == 0) s_col[c][wave_id()] = v;
        }
        nf_min = wave_min(nf_min);
        nf_max = wave_max(nf_max);
        if (lane_id() == 0) {
            if (nf_min != 0xFFFFFFFFu && nf_min < __hip_atomic_load(&flags->min_nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&flags->min_nf, nf_min);
            if (nf_max > __hip_atomic_load(&flags->max_nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&flags->max_nf, nf_max);
        }
        if (__ballot(bad) && lane_id() == 0) atomicOr(&flags->slow, 1u);
        __syncthreads();
        if (threadIdx.x < (uint32_t)cols.ncols) {
            uint64_t tsum = 0;
            for (int w = 0; w < kFtWaves; w++) tsum += s_col[threadIdx.x][w];
            tile_tot[(uint64_t)threadIdx.x * ntiles + t] = tsum;
        } else if (threadIdx.x == (uint32_t)cols.ncols) {
            tile_tot[(uint64_t)threadIdx.x * ntiles + t] = own;
        }
        return;
    }
    // ---- COPY: where this thread's bytes of every column go inside the tile ----
    uint32_t pos[MAXC];       // bytes of column c in this tile in front of this thread's chunk
    uint64_t obase[MAXC];     // the tile's first byte of column c in the column's data
    uint32_t span[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        const uint32_t incl = wave_inclusive_sum(colbytes[c]);
        if (lane_id() == kWave - 1) s_col[c][wave_id()] = incl;
        pos[c] = incl - colbytes[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kFtWaves; w++) {
            pre += w < wave_id() ? s_col[c][w] : 0u;
            tot += s_col[c][w];
        }
        pos[c] += pre;
        span[c] = tot;
        obase[c] = c < cols.ncols ? tile_tot[(uint64_t)c * ntiles + t] - tile_tot[(uint64_t)c * ntiles] : 0ull;
    }
    // offsets: record r + 1's value of column c begins behind the bytes of column c in front of record r's terminating newline
    // (entry nout: the column's size); the first owned record's offsets: the tile in front wrote the same values behind ITS last record
    {
        const uint64_t r_first = tile_tot[(uint64_t)cols.ncols * ntiles + t] - tile_tot[(uint64_t)cols.ncols * ntiles] + lo_rec;
        if (threadIdx.x == 0 && r_first >= first && r_first <= nrec) {
#pragma unroll
            for (int c = 0; c < MAXC; c++)
                if (c < cols.ncols) offs[(uint64_t)c * stride + (r_first - first)] = (uint32_t)obase[c];
        }
    }
    if (!(dbg & 4)) {
        uint64_t nls = nmv;
        uint64_t r = rs + (uint32_t)__popcll(nm & (nmv ? ((nmv & (0ull - nmv)) - 1ull) : 0ull));   // (+ the chunk's newlines in front of the owned ones)
        while (nls) {
            const uint32_t bit = (uint32_t)__ffsll((long long)nls) - 1u;
            nls &= nls - 1;
            if (r + 1 >= first && r + 1 <= nrec) {
                const uint64_t below = (1ull << bit) - 1ull;
#pragma unroll
                for (int c = 0; c < MAXC; c++)
                    if (c < cols.ncols) offs[(uint64_t)c * stride + (r + 1 - first)] = (uint32_t)(obase[c] + pos[c] + (uint32_t)__popcll(wm[c] & below));
            }
            r++;
        }
    }
    // ---- the chunk's wanted bytes, compacted word by word (v_perm_b32) and OR-ed into the zeroed output stage, one column at a time
    // (the same field may be wanted as several columns: the output can be larger than the text), then streamed out ----
    uint32_t w32[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u32x4 v = ((const CPH_LDS u32x4*)(stage + base))[i];
        w32[4 * i] = v.x; w32[4 * i + 1] = v.y; w32[4 * i + 2] = v.z; w32[4 * i + 3] = v.w;
    }
    // (a plain pointer into the dynamic LDS block: atomicOr has no overload for address-space pointers; the compiler still emits ds_or_b32)
    uint32_t* ost32 = reinterpret_cast<uint32_t*>(smem + ((size_t)kFtStage + 16 + 3 * (size_t)(kFtStage / 16 + 8) * sizeof(uint16_t)));
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        if (c >= cols.ncols) break;   // uniform
        const uint32_t phase = (uint32_t)(obase[c] & 15);   // the stage is phase-aligned with the column's place in global memory (flush_stage)
        if (c > 0) {   // (zeroed before the kernel's first barrier for column 0)
            __syncthreads();
            const u32x4 z = {0, 0, 0, 0};
            for (uint32_t i = threadIdx.x; i < (span[c] + 47u) / 16u; i += kFtThreads) ((CPH_LDS u32x4*)ostage)[i] = z;
            __syncthreads();
        }
        if (wm[c] && !(dbg & 8)) {
            const uint32_t a0 = phase + pos[c];
            uint32_t fill = a0 & 3u, w = a0 >> 2;
            uint64_t acc = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t m4 = (uint32_t)(wm[c] >> (4 * i)) & 0xFu;
                const uint32_t cw = __builtin_amdgcn_perm(0u, w32[i], s_sel[m4]);
                acc |= (uint64_t)cw << (8u * fill);
                fill += (uint32_t)__popc(m4);
                if (fill >= 4u) {
                    atomicOr(&ost32[w], (uint32_t)acc);
                    w++;
                    acc >>= 32;
                    fill -= 4u;
                }
            }
            if (fill) atomicOr(&ost32[w], (uint32_t)acc);
        }
        lds_atomics_barrier();
        flush_stage(ostage, out_data[c], obase[c], span[c]);
    }
}

__global__ void k_csv_set_u64(uint64_t* p, uint64_t v) { *p = v; }

}  // namespace cph

using namespace cph;

struct cph_csv_table_impl {
    cph_csv_table pub;   // first
    ResultOwner own;
    DevBuf d_data[CPH_MAX_KEY_COLS], d_offs;
};

// The fast path's host side: count pass, one scan, copy pass — tried FIRST (it needs neither the quote parity nor the separator
// positions of the classic passes).  *done stays false when the text needs the classic kernels (a quote, a blank or comment line, a
// record beyond the staged window, field counts that differ, 16 fields or more): nothing has been published then.
static Status csv_fast_path(cph_ctx* ctx, cph_csv_table_impl* t, const uint8_t* d, uint64_t size, const CsvOpts& o, const int32_t* col_index,
                            int32_t ncols, const cph_csv_options* opt, uint64_t lead, bool* done, uint64_t* nrec_out, uint64_t* first_out,
                            uint64_t* nout_out, uint64_t* stride_out, uint8_t** offs_all_out, std::vector<uint64_t>* totals) {
    const uint64_t ntiles = (size + kCsvTile - 1) / kCsvTile;
    if (ntiles > 0x7FFFFFFFull) return {};
    for (int c = 0; c < ncols; c++)
        if (col_index[c] > 0xFFFF) return {};
    FtCols fc{};
    fc.ncols = ncols;
    for (int c = 0; c < ncols; c++) fc.index[c] = col_index[c];
    DevBuf flags, ttot;
    const uint64_t narr = (uint64_t)ncols + 1;   // bytes per wanted column, newlines: per tile
    CPH_TRY(upload_block(ctx, FtFlags{0u, 0xFFFFFFFFu, 0u, 0u}, &flags));
    CPH_TRY(ttot.alloc(&ctx->pool, (narr * ntiles + 1) * sizeof(uint64_t)));
    const size_t lds_count = (size_t)kFtStage + 16 + 3 * (size_t)(kFtStage / 16 + 8) * sizeof(uint16_t) + 16;
    const size_t lds_copy = lds_count + (size_t)kFtStage + 64;
    const uint64_t first_req = opt->skip_records;
    {
        const void* fn = ncols <= 4 ? reinterpret_cast<const void*>(&k_csv_fast<false, 4>) : reinterpret_cast<const void*>(&k_csv_fast<false, 8>);
        CPH_TRY(kernel_setup(ctx, fn, kFtThreads, lds_count, nullptr));
        ProfScope ps(ctx, "k_csv_fast_count", (double)size);
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kFtThreads), lds_count, ctx->stream, d, size, ntiles, o, fc, first_req, 0ull,
                           ttot.as<uint64_t>(), flags.as<FtFlags>(), (uint32_t*)nullptr, 0ull, (uint8_t* const*)nullptr, ctx->chain_debug >> 16); };
        if (ncols <= 4) go(&k_csv_fast<false, 4>);
        else go(&k_csv_fast<false, 8>);
        CPH_HIP_TRY(hipGetLastError());
    }
    CPH_TRY(exclusive_scan_u64(ctx, ttot.as<uint64_t>(), narr * ntiles, ttot.as<uint64_t>() + narr * ntiles));
    // one wait: the flags + where every array's tiles begin in the scan (an array's total = the difference to the next one's start)
    CPH_TRY(ensure_pinned_scratch(ctx, sizeof(FtFlags) + ((size_t)narr + 1) * sizeof(uint64_t)));
    uint8_t* h = static_cast<uint8_t*>(ctx->pinned_scratch);
    CPH_HIP_TRY(hipMemcpyAsync(h, flags.get(), sizeof(FtFlags), hipMemcpyDeviceToHost, ctx->stream));
    for (uint64_t c = 0; c <= narr; c++)
        CPH_HIP_TRY(hipMemcpyAsync(h + sizeof(FtFlags) + (size_t)c * sizeof(uint64_t), ttot.as<uint64_t>() + c * ntiles, sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, ctx->stream));
    CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const FtFlags fl = *reinterpret_cast<const FtFlags*>(h);
    const uint64_t* bounds = reinterpret_cast<const uint64_t*>(h + sizeof(FtFlags));
    if (fl.slow) return {};
    const uint64_t nsep = bounds[narr] - bounds[narr - 1];
    const uint64_t nrec = nsep + (fl.last_empty ? 0 : 1);
    if (nrec == 0 || nrec > 0xFFFFFFFFull) return {};
    if (opt->fields_per_record >= 0) {   // 0: every record as many fields as the first one (csv.Reader.FieldsPerRecord)
        if (fl.min_nf != fl.max_nf) return {};   // the classic path finds WHICH record is the first wrong one
        if (opt->fields_per_record > 0 && (uint32_t)opt->fields_per_record != fl.min_nf) return {};
    }
    const uint64_t first = std::min<uint64_t>(first_req, nrec);
    const uint64_t nout = nrec - first;
    if (nout == 0) return {};
    const uint64_t stride = (nrec + 1 + lead + 3) & ~3ull;
    CPH_TRY(t->d_offs.alloc(&ctx->pool, (size_t)ncols * stride * sizeof(uint32_t) + 64));
    uint8_t* offs_all = t->d_offs.as<uint8_t>() + lead * sizeof(uint32_t);
    for (int c = 0; c < ncols; c++) {
        (*totals)[(size_t)c] = bounds[c + 1] - bounds[c];
        if ((*totals)[(size_t)c] > 0xFFFFFFFFull) return {CPH_ERR_INVALID, "a column beyond 4 GiB with 32-bit offsets"};   // (cannot happen: text < 4 GiB)
        CPH_TRY(t->d_data[c].alloc(&ctx->pool, (*totals)[(size_t)c] + 16));
    }
    DevBuf ptrs;
    CPH_TRY(ptrs.alloc(&ctx->pool, (size_t)ncols * sizeof(uint8_t*)));
    void* slot = nullptr;
    CPH_TRY(pinned_upload(ctx, (size_t)ncols * sizeof(uint8_t*), &slot));
    for (int c = 0; c < ncols; c++) static_cast<uint8_t**>(slot)[c] = t->d_data[c].as<uint8_t>();
    CPH_HIP_TRY(hipMemcpyAsync(ptrs.get(), slot, (size_t)ncols * sizeof(uint8_t*), hipMemcpyHostToDevice, ctx->stream));
    {
        double out_bytes = 0;
        for (int c = 0; c < ncols; c++) out_bytes += (double)(*totals)[(size_t)c];
        const void* fn = ncols <= 4 ? reinterpret_cast<const void*>(&k_csv_fast<true, 4>) : reinterpret_cast<const void*>(&k_csv_fast<true, 8>);
        CPH_TRY(kernel_setup(ctx, fn, kFtThreads, lds_copy, nullptr));
        ProfScope ps(ctx, "k_csv_fast_copy", (double)size + out_bytes + (double)nout * 4.0 * ncols);
        // offs: entry r - first of column c at offs + c * stride
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kFtThreads), lds_copy, ctx->stream, d, size, ntiles, o, fc, first, nrec,
                           ttot.as<uint64_t>(), flags.as<FtFlags>(), reinterpret_cast<uint32_t*>(offs_all) + first, stride, ptrs.as<uint8_t*>(),
                           ctx->chain_debug >> 16); };
        if (ncols <= 4) go(&k_csv_fast<true, 4>);
        else go(&k_csv_fast<true, 8>);
        CPH_HIP_TRY(hipGetLastError());
    }
    *done = true;
    *nrec_out = nrec;
    *first_out = first;
    *nout_out = nout;
    *stride_out = stride;
    *offs_all_out = offs_all;
    return {};
}

// The separator stage under LazyQuotes: the state scan (passes 1L-2M of the header comment) in place of the parity passes.
// cnt: ntiles + 1 words, on return the exclusive scan of the tiles' separator counts (+ their total, also in *nsep); seps is
// allocated here (nsep + 1 entries: the caller appends the text's end).
static Status csv_lazy_separators(cph_ctx* ctx, const uint8_t* d, uint64_t size, const CsvOpts& o, uint64_t ntiles, DevBuf* cnt, DevBuf* seps,
                                  uint64_t* nsep) {
    const LzTable tb = lz_table(o.comma, o.comment, o.trim != 0);
    const uint64_t nchunks = ntiles * (kCsvTile / 16);
    DevBuf tmap, marks;
    CPH_TRY(tmap.alloc(&ctx->pool, ntiles * sizeof(uint32_t)));
    CPH_TRY(marks.alloc(&ctx->pool, nchunks * sizeof(uint16_t)));
    {
        ProfScope ps(ctx, "k_csv_lazy_tile_maps", (double)size);
        hipLaunchKernelGGL(k_csv_lazy_tile_maps, dim3((unsigned)ntiles), dim3(kCsvThreads), 0, ctx->stream, d, size, tb, tmap.as<uint32_t>());
    }
    {
        ProfScope ps(ctx, "k_csv_lazy_tile_entry", 8.0 * (double)ntiles);
        hipLaunchKernelGGL(k_csv_lazy_tile_entry, dim3(1), dim3(kLazyScanThreads), 0, ctx->stream, tmap.as<uint32_t>(), ntiles);
    }
    {
        ProfScope ps(ctx, "k_csv_lazy_marks", (double)size + 2.0 * (double)nchunks);
        hipLaunchKernelGGL(k_csv_lazy_marks, dim3((unsigned)ntiles), dim3(kCsvThreads), 0, ctx->stream, d, size, tb, tmap.as<uint32_t>(),
                           marks.as<uint16_t>(), cnt->as<uint64_t>());
    }
    CPH_HIP_TRY(hipGetLastError());
    CPH_TRY(exclusive_scan_u64(ctx, cnt->as<uint64_t>(), ntiles, cnt->as<uint64_t>() + ntiles));
    CPH_TRY(read_device_value(ctx, cnt->as<uint64_t>() + ntiles, nsep));
    if (*nsep + 1 > 0xFFFFFFFFull) return {CPH_ERR_TOO_MANY_ROWS, "more than 2^32-1 lines"};
    CPH_TRY(seps->alloc(&ctx->pool, (*nsep + 1) * sizeof(uint64_t)));
    {
        ProfScope ps(ctx, "k_csv_lazy_separators", 2.0 * (double)nchunks + 8.0 * (double)*nsep);
        hipLaunchKernelGGL(k_csv_lazy_separators, dim3((unsigned)((ntiles + kLazySepTiles - 1) / kLazySepTiles)), dim3(kCsvThreads), 0, ctx->stream,
                           marks.as<uint16_t>(), nchunks, cnt->as<uint64_t>(), seps->as<uint64_t>());
    }
    CPH_HIP_TRY(hipGetLastError());
    return {};
}

// cph_csv_parse (lazy = false) and cph_csv_parse_lazy (lazy = true)
static int32_t csv_parse_any(cph_ctx* ctx, const uint8_t* data, uint64_t size, int32_t mem, const cph_csv_options* opt,
                             const int32_t* col_index, int32_t ncols, int32_t out_mem, cph_csv_table** out, const bool lazy) {
    if (!ctx || !out || !opt || !col_index || ncols < 1 || ncols > CPH_MAX_KEY_COLS || (size && !data)) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if ((mem != CPH_MEM_HOST && mem != CPH_MEM_DEVICE) || (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE))
        return fail_with(ctx, {CPH_ERR_INVALID, "bad memory space"});
    if (!lazy && opt->lazy_quotes) return fail_with(ctx, {CPH_ERR_INVALID, "LazyQuotes is not supported by the GPU parser"});
    if (lazy && opt->lazy_quotes != 1) return fail_with(ctx, {CPH_ERR_INVALID, "cph_csv_parse_lazy takes lazy_quotes = 1"});
    if (opt->comma == '"' || opt->comma == '\n' || opt->comma == '\r' || opt->comma == 0 || opt->comma >= 0x80 ||
        opt->comment >= 0x80 || (opt->comment && opt->comment == opt->comma))
        return fail_with(ctx, {CPH_ERR_INVALID, "unsupported delimiter / comment character"});
    for (int c = 0; c < ncols; c++)
        if (col_index[c] < 0) return fail_with(ctx, {CPH_ERR_INVALID, "negative field index"});
    auto* t = new (std::nothrow) cph_csv_table_impl();
    if (!t) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    t->own.ctx = ctx;
    auto run = [&]() -> Status {
        CsvOpts o{opt->comma, opt->comment, opt->trim_leading_space ? 1 : 0};
        CsvCols cc{};
        cc.ncols = ncols;
        for (int c = 0; c < ncols; c++) cc.index[c] = col_index[c];
        // bytes on the device, 16-byte aligned
        DevBuf staged;
        const uint8_t* d = data;
        if (size && (mem == CPH_MEM_HOST || ((uintptr_t)data & 15))) {
            CPH_TRY(staged.alloc(&ctx->pool, size + 16));
            CPH_HIP_TRY(hipMemcpyAsync(staged.get(), data, size, mem == CPH_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                       ctx->stream));
            d = staged.as<uint8_t>();
        }
        uint64_t nrec = 0;
        DevBuf rec_b, rec_e, nfields, errk, seps_keep;
        RecIndex ri{nullptr, nullptr, nullptr};
        uint64_t first = 0, nout = 0;
        t->pub.error_kind = 0;
        t->pub.error_record = 0;
        // Offsets are 32-bit whenever the text is smaller than 4 GiB (no column can then be larger).
        const char* force64 = getenv("CPH_CSV_OFFSETS64");   // test hook for the >= 4 GiB code path
        const bool off32 = size < (1ull << 32) && !(force64 && force64[0] == '1');
        const size_t osz = off32 ? sizeof(uint32_t) : sizeof(uint64_t);
        // column c's entries start `lead` elements into its stride so that the first RETURNED record (index
        // skip_records) lands on a 16-byte boundary: the offset scans then move 16-byte vectors
        const uint64_t lead = (4 - (opt->skip_records & 3)) & 3;
        uint64_t stride = 0;
        uint8_t* offs_all = nullptr;
        std::vector<uint64_t> totals((size_t)ncols, 0);
        bool fast_done = false;
        // ---- the fast path (k_csv_fast): no TrimLeadingSpace, at most kFtMaxCols columns, 32-bit offsets; the kernels themselves find what
        // else sends a text to the classic passes below ----
        if (size && ctx->csv_fast && !o.trim && ncols <= kFtMaxCols && off32)
            CPH_TRY(csv_fast_path(ctx, t, d, size, o, col_index, ncols, opt, lead, &fast_done, &nrec, &first, &nout, &stride, &offs_all, &totals));
        if (size && !fast_done) {
            const uint64_t ntiles = (size + kCsvTile - 1) / kCsvTile;
            if (ntiles > 0x7FFFFFFFull) return {CPH_ERR_INVALID, "text too large"};
            DevBuf tq, tev, tod, cnt, seps;
            CPH_TRY(cnt.alloc(&ctx->pool, (ntiles + 1) * sizeof(uint64_t)));
            uint64_t nsep = 0;
            if (lazy) {
                CPH_TRY(csv_lazy_separators(ctx, d, size, o, ntiles, &cnt, &seps, &nsep));
            } else {
            CPH_TRY(tq.alloc(&ctx->pool, ntiles * sizeof(uint32_t)));
            CPH_TRY(tev.alloc(&ctx->pool, ntiles * sizeof(uint32_t)));
            CPH_TRY(tod.alloc(&ctx->pool, ntiles * sizeof(uint32_t)));
            {
                ProfScope ps(ctx, "k_csv_tile_stats", (double)size);
                hipLaunchKernelGGL(k_csv_tile_stats, dim3((unsigned)ntiles), dim3(kCsvThreads), 0, ctx->stream, d, size,
                                   tq.as<uint32_t>(), tev.as<uint32_t>(), tod.as<uint32_t>());
            }
            CPH_TRY(exclusive_scan_u32(ctx, tq.as<uint32_t>(), ntiles));   // mod 2^32 keeps the parity
            hipLaunchKernelGGL(k_csv_pick_counts, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, ctx->stream, tq.as<uint32_t>(),
                               tev.as<uint32_t>(), tod.as<uint32_t>(), cnt.as<uint64_t>(), ntiles);
            CPH_TRY(exclusive_scan_u64(ctx, cnt.as<uint64_t>(), ntiles, cnt.as<uint64_t>() + ntiles));
            CPH_TRY(read_device_value(ctx, cnt.as<uint64_t>() + ntiles, &nsep));
            if (nsep + 1 > 0xFFFFFFFFull) return {CPH_ERR_TOO_MANY_ROWS, "more than 2^32-1 lines"};
            CPH_TRY(seps.alloc(&ctx->pool, (nsep + 1) * sizeof(uint64_t)));
            {
                ProfScope ps(ctx, "k_csv_separators", (double)size + 8.0 * (double)nsep);
                hipLaunchKernelGGL(k_csv_separators, dim3((unsigned)ntiles), dim3(kCsvThreads), 0, ctx->stream, d, size,
                                   tq.as<uint32_t>(), cnt.as<uint64_t>(), seps.as<uint64_t>());
            }
            }   // (!lazy)
            const uint64_t nseg = nsep + 1;   // the bytes after the last separator (possibly none) form the last segment
            {
            hipLaunchKernelGGL(k_csv_set_u64, dim3(1), dim3(1), 0, ctx->stream, seps.as<uint64_t>() + nsep, size);
            // classify; compact only when a line in the middle of the text was dropped (blank / comment)
            DevBuf keep_flag, stats;
            CPH_TRY(keep_flag.alloc(&ctx->pool, nseg * sizeof(uint32_t)));
            CPH_TRY(stats.alloc(&ctx->pool, 3 * sizeof(unsigned long long)));
            CPH_HIP_TRY(hipMemsetAsync(stats.get(), 0, 3 * sizeof(unsigned long long), ctx->stream));
            {
                ProfScope ps(ctx, "k_csv_classify", 13.0 * (double)nseg);
                hipLaunchKernelGGL(k_csv_classify, dim3(std::min(grid_for_items(nseg), 2048u)), dim3(256), 0, ctx->stream, d, seps.as<uint64_t>(), nseg, o,
                                   keep_flag.as<uint32_t>(), stats.as<unsigned long long>());
            }
            CPH_TRY(ensure_pinned_scratch(ctx, 3 * sizeof(unsigned long long)));
            CPH_HIP_TRY(hipMemcpyAsync(ctx->pinned_scratch, stats.get(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
            const unsigned long long* hs = static_cast<const unsigned long long*>(ctx->pinned_scratch);
            nrec = hs[0];
            const bool dropped_inner = hs[1] != 0;
            if (hs[2] && !lazy) return {CPH_ERR_INVALID, "comment line containing a quote: not supported by the GPU parser"};
            if (nrec > 0xFFFFFFFFull) return {CPH_ERR_TOO_MANY_ROWS, "more than 2^32-1 records"};
            if (!dropped_inner) {
                ri.seps = seps.as<uint64_t>();   // record r is segment r
                seps_keep = std::move(seps);
            } else {
                DevBuf keep;
                CPH_TRY(keep.alloc(&ctx->pool, nseg * sizeof(uint32_t)));
                CPH_HIP_TRY(hipMemcpyAsync(keep.get(), keep_flag.get(), nseg * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
                CPH_TRY(exclusive_scan_u32(ctx, keep.as<uint32_t>(), nseg));
                CPH_TRY(rec_b.alloc(&ctx->pool, (nrec + 1) * sizeof(uint64_t)));
                CPH_TRY(rec_e.alloc(&ctx->pool, (nrec + 1) * sizeof(uint64_t)));
                ProfScope ps(ctx, "k_csv_compact", 32.0 * (double)nseg);
                hipLaunchKernelGGL(k_csv_compact, dim3(grid_for_items(nseg)), dim3(256), 0, ctx->stream, seps.as<uint64_t>(), nseg,
                                   keep.as<uint32_t>(), keep_flag.as<uint32_t>(), rec_b.as<uint64_t>(), rec_e.as<uint64_t>());
                ri.rec_b = rec_b.as<uint64_t>();
                ri.rec_e = rec_e.as<uint64_t>();
            }
            CPH_HIP_TRY(hipGetLastError());
            }   // (!fast_done)
        }
        auto col_offs = [&](int c) { return offs_all + ((uint64_t)c * stride + first) * osz; };
        if (!fast_done) {
        // fields: lengths (written where the offsets will be), counts, first error.
        stride = (nrec + 1 + lead + 3) & ~3ull;
        CPH_TRY(t->d_offs.alloc(&ctx->pool, (size_t)ncols * stride * osz + 64));
        offs_all = t->d_offs.as<uint8_t>() + lead * osz;
        uint64_t good = nrec;   // records before the first error
        // LDS stage of the record-parallel kernels: the smallest power of two holding 1.5x an average 256-record tile
        // (small stages leave room for more workgroups per CU; tiles that do not fit are parsed from global memory)
        int stage_bytes = kCsvStageMin;
        if (nrec)
            while (stage_bytes < kCsvStageMax && (double)stage_bytes < 1.5 * 256.0 * (double)size / (double)nrec) stage_bytes *= 2;   // tests/test_gpu_csv_strict_edges.py: stage_bytes()
        // tiles of 256 records, aligned so that the first returned record starts one (k_csv_fields); their per-column byte totals
        const uint64_t skip_eff = std::min<uint64_t>(opt->skip_records, nrec);
        const uint32_t pad = (uint32_t)((kCsvThreads - skip_eff % kCsvThreads) % kCsvThreads);   // tests/test_gpu_csv_strict_edges.py: pad_of()
        const uint64_t ntile = (nrec + pad + kCsvThreads - 1) / kCsvThreads;
        const uint64_t T0 = (skip_eff + pad) / kCsvThreads;
        DevBuf tile_tot;
        if (nrec) {
            CPH_TRY(tile_tot.alloc(&ctx->pool, ((size_t)ncols * ntile + 1) * sizeof(uint64_t)));
            CPH_TRY(nfields.alloc(&ctx->pool, nrec * sizeof(uint32_t)));
            CPH_TRY(errk.alloc(&ctx->pool, sizeof(unsigned long long)));
            CPH_HIP_TRY(hipMemsetAsync(errk.get(), 0xFF, sizeof(unsigned long long), ctx->stream));
            {
                ProfScope ps(ctx, "k_csv_fields", (double)size + (double)nrec * (12.0 + (double)osz * ncols));
                const size_t fsmem = (size_t)stage_bytes + 16 + 2 * (size_t)csv_mask_halves(stage_bytes) * sizeof(uint16_t) +
                                     (size_t)ncols * kCsvThreads * sizeof(uint32_t);
                auto go = [&](auto kernel, auto* lens) {
                    hipLaunchKernelGGL(kernel, dim3(grid_for_items(nrec)), dim3(kCsvThreads), fsmem, ctx->stream, d, size, ri, nrec, o, cc, lens, stride,
                                       nfields.as<uint32_t>(), errk.as<unsigned long long>(), stage_bytes, pad, ntile, tile_tot.as<uint64_t>());
                };
                if (off32 && !lazy) go(&k_csv_fields<uint32_t>, reinterpret_cast<uint32_t*>(offs_all));
                else if (!lazy) go(&k_csv_fields<uint64_t>, reinterpret_cast<uint64_t*>(offs_all));
                else if (off32) go(&k_csv_fields<uint32_t, true>, reinterpret_cast<uint32_t*>(offs_all));
                else go(&k_csv_fields<uint64_t, true>, reinterpret_cast<uint64_t*>(offs_all));
            }
            if (opt->fields_per_record >= 0)
                hipLaunchKernelGGL(k_csv_check_counts, dim3(grid_for_items(nrec)), dim3(256), 0, ctx->stream, nfields.as<uint32_t>(),
                                   nrec, opt->fields_per_record, errk.as<unsigned long long>());
            CPH_HIP_TRY(hipGetLastError());
            unsigned long long key = 0;
            CPH_TRY(read_device_value(ctx, errk.as<unsigned long long>(), &key));
            if (key != ~0ull) {
                if ((key & 7) == 0)   // kCsvLazySpace
                    return {CPH_ERR_INVALID, "LazyQuotes with TrimLeadingSpace: a non-ASCII Unicode space in front of an opening quote is not "
                                             "supported by the GPU parser"};
                t->pub.error_kind = (int32_t)(key & 7);
                t->pub.error_record = key >> 3;
                good = key >> 3;
            }
        }
        first = std::min<uint64_t>(opt->skip_records, good);
        nout = good - first;
        // offsets (in place, over the records that are returned) + copy
        t->pub.nrecords = nout;
        t->pub.ncols = ncols;
        // ONE scan over the tiles' totals of all columns (the concatenation [ncols][ntile]; the copy pass takes differences):
        // the per-record offsets are formed by the copy pass itself.  totals[c] = the bytes of the tiles that hold returned
        // records — the column's size, or a few values more when the text ends in an error inside the last tile (the
        // column's offsets end at the true size either way: entry nout is written by the copy pass)
        const uint64_t ntile_out = (nout + kCsvThreads - 1) / kCsvThreads;
        if (!nout) {
            for (int c = 0; c < ncols; c++) CPH_HIP_TRY(hipMemsetAsync(col_offs(c), 0, osz, ctx->stream));
        } else {
            CPH_TRY(exclusive_scan_u64(ctx, tile_tot.as<uint64_t>(), (uint64_t)ncols * ntile, tile_tot.as<uint64_t>() + (uint64_t)ncols * ntile));
            CPH_TRY(ensure_pinned_scratch(ctx, 2 * (size_t)ncols * sizeof(uint64_t)));
            uint64_t* hs = static_cast<uint64_t*>(ctx->pinned_scratch);
            for (int c = 0; c < ncols; c++) {
                const uint64_t* sc = tile_tot.as<uint64_t>() + (uint64_t)c * ntile + T0;
                CPH_HIP_TRY(hipMemcpyAsync(hs + 2 * c, sc, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
                CPH_HIP_TRY(hipMemcpyAsync(hs + 2 * c + 1, sc + ntile_out, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
            }
            CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (int c = 0; c < ncols; c++) totals[(size_t)c] = hs[2 * c + 1] - hs[2 * c];
            if (off32)
                for (int c = 0; c < ncols; c++)
                    if (totals[(size_t)c] > 0xFFFFFFFFull) return {CPH_ERR_INVALID, "a column beyond 4 GiB with 32-bit offsets"};   // (cannot happen: text < 4 GiB)
        }
        for (int c = 0; c < ncols; c++) CPH_TRY(t->d_data[c].alloc(&ctx->pool, totals[(size_t)c] + 16));
        if (nout) {
            DevBuf ptrs;
            CPH_TRY(ptrs.alloc(&ctx->pool, (size_t)ncols * sizeof(uint8_t*)));
            void* slot = nullptr;
            CPH_TRY(pinned_upload(ctx, (size_t)ncols * sizeof(uint8_t*), &slot));
            for (int c = 0; c < ncols; c++) static_cast<uint8_t**>(slot)[c] = t->d_data[c].as<uint8_t>();
            CPH_HIP_TRY(hipMemcpyAsync(ptrs.get(), slot, (size_t)ncols * sizeof(uint8_t*), hipMemcpyHostToDevice, ctx->stream));
            double out_bytes = 0;
            for (int c = 0; c < ncols; c++) out_bytes += (double)totals[(size_t)c];
            ProfScope ps(ctx, "k_csv_copy_fields", (double)size + out_bytes + (double)nout * (8.0 + (double)osz * ncols));
            const size_t smem = (size_t)(stage_bytes + 16) + (size_t)(stage_bytes + 32 * kMaxKeyCols) +
                                2 * (size_t)csv_mask_halves(stage_bytes) * sizeof(uint16_t) + (size_t)ncols * (kCsvThreads + 1) * sizeof(uint32_t);
            Status st{};
            auto go = [&](auto kernel, auto* offs) {
                if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
                    st = {CPH_ERR_HIP, "hipFuncSetAttribute failed (k_csv_copy_fields)"};
                    return;
                }
                hipLaunchKernelGGL(kernel, dim3(grid_for_items(nout)), dim3(kCsvThreads), smem, ctx->stream, d, size, ri, first, nout, o, cc, offs + first,
                                   stride, ptrs.as<uint8_t*>(), stage_bytes, tile_tot.as<uint64_t>(), ntile, T0);
            };
            if (off32 && !lazy) go(&k_csv_copy_fields<uint32_t>, reinterpret_cast<uint32_t*>(offs_all));
            else if (!lazy) go(&k_csv_copy_fields<uint64_t>, reinterpret_cast<uint64_t*>(offs_all));
            else if (off32) go(&k_csv_copy_fields<uint32_t, true>, reinterpret_cast<uint32_t*>(offs_all));
            else go(&k_csv_copy_fields<uint64_t, true>, reinterpret_cast<uint64_t*>(offs_all));
            CPH_TRY(st);
            CPH_HIP_TRY(hipGetLastError());
        }
        }   // (!fast_done)
        t->pub.nrecords = nout;
        t->pub.ncols = ncols;
        // publish: every column's offsets (all inside d_offs) in front of every column's bytes
        ResultPart parts[2 * CPH_MAX_KEY_COLS];
        for (int c = 0; c < ncols; c++) {
            cph_strcol& sc = t->pub.cols[c];
            sc.nrows = nout;
            sc.offset_bits = off32 ? 32 : 64;
            sc.mem = out_mem;
            sc.fixed_width = 0;
            parts[c] = {&t->d_offs, (size_t)(nout + 1) * osz, &sc.offsets, col_offs(c)};
            parts[ncols + c] = {&t->d_data[c], (size_t)totals[(size_t)c], &sc.data};
        }
        return deliver(ctx, &t->own, parts, 2 * ncols, out_mem);
    };
    return finish_call(ctx, t, run(), out);
}

extern "C" {

CPH_API int32_t cph_csv_parse(cph_ctx* ctx, const uint8_t* data, uint64_t size, int32_t mem, const cph_csv_options* opt,
                              const int32_t* col_index, int32_t ncols, int32_t out_mem, cph_csv_table** out) {
    return csv_parse_any(ctx, data, size, mem, opt, col_index, ncols, out_mem, out, false);
}

CPH_API int32_t cph_csv_parse_lazy(cph_ctx* ctx, const uint8_t* data, uint64_t size, int32_t mem, const cph_csv_options* opt,
                                   const int32_t* col_index, int32_t ncols, int32_t out_mem, cph_csv_table** out) {
    return csv_parse_any(ctx, data, size, mem, opt, col_index, ncols, out_mem, out, true);
}

CPH_API void cph_csv_table_release(cph_csv_table* pub) { release_result<cph_csv_table_impl>(pub); }

}  // extern "C"

// Loads this translation unit's code object now (cph_ctx_create) instead of inside the first timed call.
namespace cph {
void warm_csv_ingest() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_csv_pick_counts));
    (void)hipGetLastError();
}
}  // namespace cph
