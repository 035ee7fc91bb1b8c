// tile_bitmap.hpp — "which rows?" as one bit per row: the layout Filter (k_pred_eval / k_pred_emit), Totals (k_agg_heads / k_agg_emit /
// k_agg_reduce), Resolve (k_resolve_tile / k_resolve_emit) and OrderBy (k_order_select_flag / k_order_select_emit / k_order_key_rank)
// share, and the device code that writes and reads it.  The host half (allocation, the scan, the total) is TileBitmap in cph_internal.hpp.
//
//   bitmap[tile * 32 + w] bit b = row tile * 2048 + 64 w + b is chosen (rows >= n: 0)
//   counts[tile]                = the tile's set bits; after the exclusive scan: the set bits in front of the tile, and
//   counts[ntiles]              = all of them (the scan's total)
//
// A tile is one workgroup of kTileWaves waves.  Its words are written either by ballots (a wave's ballot IS the word of its 64
// rows) or by lanes that hold kTileLaneRows CONSECUTIVE rows, which are one byte of a word.  A set bit's rank is the scanned count
// of its tile + the popcounts of the words in front of it + mbcnt inside its word: no atomics anywhere.
//
// These bodies replaced per-kernel copies under the rule that every kernel keeps its registers, LDS and occupancy
// (profiles/tile_bitmap_refactor.txt).  That is why the tile store and the word load read lane_id() in front of their `if`: read
// inside it, several kernels' VGPR counts moved.  Run tools/kernel_usage.sh over the users when changing them.
#pragma once

#include "device_utils.hpp"

namespace cph {

constexpr int kTileLaneRows  = 8;                                    // consecutive rows per lane
constexpr int kTileWaves     = 4;
constexpr int kTileRows      = kTileWaves * kWave * kTileLaneRows;   // 2048: tests/test_resolve.py and tests/test_totals.py call it T
constexpr int kTileWords     = kTileRows / 64;                       // 32
constexpr int kTileWaveWords = kTileWords / kTileWaves;              // 8 words = 512 rows per wave
static_assert(kTileRows == 2048 && kTileWords == 32 && kTileWaveWords == 8, "the layout every reader of these bitmaps assumes");
static_assert(kTileLaneRows == 8 && 64 % kTileLaneRows == 0, "a lane's 8 consecutive rows are one byte of a word");
static_assert(kTileWords <= kWave, "one lane of wave 0 per word");

__host__ __device__ constexpr uint64_t tile_count(uint64_t n) { return (n + kTileRows - 1) / kTileRows; }

// which of a lane's kTileLaneRows rows base .. base + 7 exist below tend, one past the tile's last row
__device__ __forceinline__ uint32_t tile_live_rows(uint64_t base, uint64_t tend) {
    return base >= tend ? 0u : (tend - base >= (uint64_t)kTileLaneRows ? (1u << kTileLaneRows) - 1 : (1u << (uint32_t)(tend - base)) - 1);
}

// The tile store: the 32 words the workgroup has put into s_word leave as one 256-byte store by wave 0, whose popcounts add up to
// counts[tile].  Every thread calls it behind its own writes to s_word; s_word may be written again when it returns.
__device__ __forceinline__ void tile_store_words(const uint64_t* s_word, uint64_t tile, uint64_t* bitmap, uint32_t* counts) {
    const int lane = lane_id();
    __syncthreads();
    if (wave_id() == 0) {
        const uint64_t word = lane < kTileWords ? s_word[lane & (kTileWords - 1)] : 0;
        if (lane < kTileWords) bitmap[tile * kTileWords + lane] = word;
        const uint32_t c = wave_sum((uint32_t)__popcll(word));
        if (lane == 0) counts[tile] = c;
    }
    __syncthreads();
}

// The rank walker: f(rank, r) for every set bit of the tile, r = its row inside the tile and rank = o0 + the set bits of the tile in
// front of it.  Every wave reads the 32 words and walks its own 8; the whole workgroup calls it.
template <class F>
__device__ __forceinline__ void tile_for_each_set(const uint64_t* bitmap, uint64_t tile, uint64_t o0, F f) {
    const int lane = lane_id(), wave = wave_id();
    const uint64_t word = lane < kTileWords ? bitmap[tile * kTileWords + lane] : 0;
    const uint32_t pc = (uint32_t)__popcll(word);
    const uint32_t before = wave_inclusive_sum(pc) - pc;
#pragma unroll
    for (int k = 0; k < kTileWaveWords; k++) {
        const int w = wave * kTileWaveWords + k;
        const uint32_t lo = __shfl((uint32_t)word, w, kWave), hi = __shfl((uint32_t)(word >> 32), w, kWave);
        const uint32_t pre = __shfl(before, w, kWave);
        const uint64_t bits = (uint64_t)lo | ((uint64_t)hi << 32);
        if ((bits >> lane) & 1ull) f(o0 + pre + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)), w * 64 + lane);
    }
}

// The reverse lookup, for lanes that hold 8 consecutive rows.  tile_load_words: the tile's words and their exclusive popcounts into
// LDS (32 entries each), by wave 0; every thread calls it and may read both when it returns.
__device__ __forceinline__ void tile_load_words(const uint64_t* bitmap, uint64_t tile, uint64_t* s_word, uint32_t* s_pre) {
    const int lane = lane_id();
    if (wave_id() == 0) {
        const uint64_t w = lane < kTileWords ? bitmap[tile * kTileWords + lane] : 0;
        const uint32_t pc = (uint32_t)__popcll(w);
        const uint32_t incl = wave_inclusive_sum(pc);
        if (lane < kTileWords) {
            s_word[lane] = w;
            s_pre[lane] = incl - pc;
        }
    }
    __syncthreads();
}
// ... *bits = the byte of the lane's rows r0 .. r0 + 7 (r0 = 8 * thread), *before = the tile's set bits in front of row r0
__device__ __forceinline__ void tile_lane_bits(const uint64_t* s_word, const uint32_t* s_pre, uint32_t r0, uint32_t* bits, uint32_t* before) {
    const uint64_t word = s_word[r0 >> 6];
    const uint32_t sh = r0 & 63u;   // <= 56: the lane's 8 rows never straddle a word
    *bits = (uint32_t)(word >> sh) & 0xFFu;
    *before = s_pre[r0 >> 6] + (uint32_t)__popcll(word & ((1ull << sh) - 1ull));
}

}  // namespace cph
