// order_device.hpp — the value maps of OrderBy (order.hip): an int64 / a float64 as a uint64 whose UNSIGNED order is the order
// of Go's cmp.Compare on the value, so that a radix sort over the mapped keys is slices.SortStableFunc over the values.
//
//   int64    the sign bit flipped.
//   float64  cmp.Compare on float64: a NaN is less than every non-NaN, all NaNs are equal whatever their bits, -0 == +0.
//            -0 is folded into +0 and every NaN goes to 0; a non-negative value gets its sign bit set, a negative one has all
//            bits inverted.  The smallest number, -Inf (0xFFF0...0), lands at 0x000F...F > 0: NaN sorts below it.
//   descending   the bitwise complement of the ascending key: the order is reversed, and rows that compare equal still carry
//            equal keys, so the stable sort leaves them in input order (descending is not the reverse of ascending).
//
// Plain C++ behind CPH_ORDER_HD: hipcc compiles it for the device, g++ for the host (tests/cpp/test_orderkey.cpp checks every
// pair of edge values and random bit patterns against the comparison above).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CPH_ORDER_HD __host__ __device__ __forceinline__
#else
#define CPH_ORDER_HD inline
#endif

namespace cph {

CPH_ORDER_HD uint64_t order_map_int64(uint64_t bits) { return bits ^ 0x8000000000000000ull; }

CPH_ORDER_HD uint64_t order_map_float64(uint64_t bits) {
    const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
    if (mag > 0x7FF0000000000000ull) return 0ull;             // NaN, any sign, any payload
    if (mag == 0ull) return 0x8000000000000000ull;            // -0 and +0
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}

// the key a sort pass sees: kind is float (true) or int64, bits the value's 8-byte pattern
CPH_ORDER_HD uint64_t order_key64(uint64_t bits, bool is_float, bool descending) {
    const uint64_t k = is_float ? order_map_float64(bits) : order_map_int64(bits);
    return descending ? ~k : k;
}

}  // namespace cph
