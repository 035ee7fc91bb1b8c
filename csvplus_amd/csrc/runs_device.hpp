// runs_device.hpp — the runs of equal keys of a sorted index, as resolve.hip (groups of >= 2 rows) and aggregate.hip (every
// run) see them: one tile of the sorted codes per workgroup, kResRows CONSECUTIVE rows per lane.
#pragma once

#include "numparse_device.hpp"
#include "tile_bitmap.hpp"

namespace cph {

// the tile of tile_bitmap.hpp under the names of the run kernels
constexpr int kResRows  = kTileLaneRows;              // consecutive rows per lane
constexpr int kResTile  = kTileRows;                  // 2048 rows = 32 bitmap words: tests/test_resolve.py and tests/test_totals.py call it T
constexpr int kResWords = kTileWords;
constexpr int kResWaves = kTileWaves;
static_assert(kMatThreads == kTileWaves * kWave, "one workgroup per tile");

// e[j] (j = 0..kResRows) = sorted positions base + j - 1 and base + j exist and carry the same key
template <bool KEY32>
__device__ __forceinline__ uint32_t equal_flags(const void* __restrict__ codes, uint64_t n, int nwords, uint64_t base) {
    uint32_t e = (1u << (kResRows + 1)) - 1;
    if constexpr (KEY32) {
        const uint32_t* c = reinterpret_cast<const uint32_t*>(codes);
        uint32_t prev = c[base ? base - 1 : 0];
#pragma unroll
        for (int j = 0; j <= kResRows; j++) {
            const uint64_t p = base + (uint64_t)j;
            const uint32_t cur = c[p < n ? p : n - 1];
            if (cur != prev) e &= ~(1u << j);
            prev = cur;
        }
    } else {
        const uint64_t* c = reinterpret_cast<const uint64_t*>(codes);
        for (int w = 0; w < nwords; w++) {
            const uint64_t* cw = c + (uint64_t)w * n;
            uint64_t prev = cw[base ? base - 1 : 0];
#pragma unroll
            for (int j = 0; j <= kResRows; j++) {
                const uint64_t p = base + (uint64_t)j;
                const uint64_t cur = cw[p < n ? p : n - 1];
                if (cur != prev) e &= ~(1u << j);
                prev = cur;
            }
        }
    }
    if (base == 0) e &= ~1u;
#pragma unroll
    for (int j = 0; j <= kResRows; j++)
        if (base + (uint64_t)j >= n) e &= ~(1u << j);
    return e;
}

}  // namespace cph
