// floatparse_device.hpp — decimal -> float64 beyond Clinger's exact cases: the Eisel-Lemire conversion (D. Lemire, "Number
// Parsing at a Gigabyte per Second", 2021; the algorithm of Go's strconv eiselLemire64) for numparse.hip's full float
// instantiation.  From the first 19 significant digits w and the decimal exponent q it computes the correctly rounded double
// of w * 10^q with one or two 64 x 64 -> 128-bit multiplies by a tabulated 128-bit power of five (pow5_table.inc, written by
// tools/gen_pow5_table.py) — or says that it cannot tell.  It never guesses: an undecided value stays deferred and the
// library's host side finishes it as before.
//
// Plain C++ behind CPH_FLTPARSE_HD, depending on nothing else in the tree: hipcc compiles it for the device, g++ for the host
// (tests/cpp/test_floatparse.cpp runs it against glibc's strtod bit for bit).
//
// The table is 651 x 16 bytes in global memory.  Every lane indexes it with its own q, so the read is one 16-byte vector load
// per multiply-by-table step, served by the vector cache / L2; the path is entered by few columns, which is why nothing is
// staged in LDS.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CPH_FLTPARSE_HD __host__ __device__ inline
#define CPH_FLTPARSE_TABLE __device__ const
#else
#define CPH_FLTPARSE_HD inline
#define CPH_FLTPARSE_TABLE static const
#endif

namespace cph {

constexpr int32_t kPow5MinQ = -342, kPow5MaxQ = 308;
constexpr uint64_t kFloatInfBits = 0x7FF0000000000000ull;

struct alignas(16) Pow5 {
    uint64_t hi, lo;
};

CPH_FLTPARSE_TABLE Pow5 kPow5Table[kPow5MaxQ - kPow5MinQ + 1] = {
#include "pow5_table.inc"
};

// a * b = *hi : *lo
CPH_FLTPARSE_HD void fp_mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
    const unsigned __int128 p = (unsigned __int128)a * b;   // host: one mul; device: the mul_hi / mul_lo pairs of __umul64hi
    *hi = (uint64_t)(p >> 64);
    *lo = (uint64_t)p;
}

CPH_FLTPARSE_HD int fp_clz64(uint64_t v) { return __builtin_clzll(v); }   // v != 0

// One value, all of its digits in w (w != 0, kPow5MinQ <= q <= kPow5MaxQ).
CPH_FLTPARSE_HD uint64_t fp_eisel_lemire_exact(uint64_t w, int32_t q) {
    const int lz = fp_clz64(w);
    w <<= lz;
    const Pow5 t = kPow5Table[q - kPow5MinQ];
    uint64_t hi, lo;
    fp_mul64(w, t.hi, &hi, &lo);
    if ((hi & 0x1FFull) == 0x1FFull) {   // the 55 kept bits could still change: the second product settles them
        uint64_t shi, slo;
        fp_mul64(w, t.lo, &shi, &slo);
        lo += shi;
        if (lo < shi) hi++;
    }
    const int ub = (int)(hi >> 63), shift = ub + 9;   // 64 - 52 - 3 = 9
    uint64_t m = hi >> shift;
    int32_t p2 = (int32_t)(((int64_t)(152170 + 65536) * (int64_t)q) >> 16) + 63 + ub - lz + 1023;   // floor(log2(10^q)) + ...; q may be negative
    if (p2 <= 0) {   // subnormal or zero
        if (1 - p2 >= 64) return 0;
        m >>= 1 - p2;
        m += m & 1ull;
        m >>= 1;
        return m;    // m == 2^52 is the smallest normal: the same bit pattern
    }
    if (lo <= 1ull && q >= -4 && q <= 23 && (m & 3ull) == 1ull && (m << shift) == hi) m &= ~1ull;   // an exact tie: to even
    m += m & 1ull;
    m >>= 1;
    if (m >= (1ull << 53)) {
        m = 1ull << 52;
        p2++;
    }
    if (p2 >= 0x7FF) return kFloatInfBits;
    return ((uint64_t)p2 << 52) | (m & ((1ull << 52) - 1ull));
}

// w: the first <= 19 significant decimal digits as an integer (w != 0), q: the decimal exponent so that value ~ w * 10^q,
// trunc: non-zero digits were dropped behind the 19th.  true: *bits = the correctly rounded double's magnitude bits (0 for
// underflow, kFloatInfBits for overflow).  false: undecided, the caller defers the value.
CPH_FLTPARSE_HD bool float_eisel_lemire(uint64_t w, int32_t q, bool trunc, uint64_t* bits) {
    if (w == 0) return false;   // the caller's business
    if (q < kPow5MinQ) {        // w < 2^64 < 10^20: below 10^-322, less than half the smallest subnormal
        *bits = 0;
        return true;
    }
    if (q > kPow5MaxQ) {        // at least 10^309
        *bits = kFloatInfBits;
        return true;
    }
    const uint64_t a = fp_eisel_lemire_exact(w, q);
    if (trunc) {   // the value lies strictly between w and w + 1 (<= 10^19 < 2^64): decided when both round alike
        if (fp_eisel_lemire_exact(w + 1ull, q) != a) return false;
    }
    *bits = a;
    return true;
}

}  // namespace cph
