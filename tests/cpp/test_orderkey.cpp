// The value maps of OrderBy (csvplus_amd/csrc/order_device.hpp) compiled for the host: for every pair of edge values and for
// random bit patterns, the unsigned order of the mapped keys must be Go's cmp.Compare on the values (int64; float64 with a NaN
// below every number, all NaNs equal, -0 == +0), and the descending map the same with the arguments swapped.
// CPU only: no GPU and no library needed.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "order_device.hpp"

using namespace cph;

namespace {

long g_checked = 0, g_failed = 0;

double from_bits(uint64_t b) {
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}
uint64_t to_bits(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

// cmp.Compare (Go 1.21+): -1 if x < y or x is a NaN and y is not; 0 if equal or both NaN; +1 otherwise
int compare_f64(double x, double y) {
    const bool xn = std::isnan(x), yn = std::isnan(y);
    if (xn) return yn ? 0 : -1;
    if (yn) return 1;
    return x < y ? -1 : (x > y ? 1 : 0);
}
int compare_i64(int64_t x, int64_t y) { return x < y ? -1 : (x > y ? 1 : 0); }
int compare_u64(uint64_t x, uint64_t y) { return x < y ? -1 : (x > y ? 1 : 0); }

void check_pair(uint64_t a, uint64_t b, bool flt) {
    const int want = flt ? compare_f64(from_bits(a), from_bits(b)) : compare_i64((int64_t)a, (int64_t)b);
    const int asc = compare_u64(order_key64(a, flt, false), order_key64(b, flt, false));
    const int desc = compare_u64(order_key64(a, flt, true), order_key64(b, flt, true));
    g_checked += 2;
    if (asc != want) {
        if (g_failed++ < 20) printf("FAIL asc %s a=%016llx b=%016llx: got %d want %d\n", flt ? "f64" : "i64", (unsigned long long)a, (unsigned long long)b, asc, want);
    }
    if (desc != -want) {   // descending = the comparison with its arguments swapped
        if (g_failed++ < 20) printf("FAIL desc %s a=%016llx b=%016llx: got %d want %d\n", flt ? "f64" : "i64", (unsigned long long)a, (unsigned long long)b, desc, -want);
    }
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

int main() {
    const std::vector<uint64_t> ints = {(uint64_t)INT64_MIN, (uint64_t)(INT64_MIN + 1), (uint64_t)-2, (uint64_t)-1, 0, 1, 2,
                                        (uint64_t)(INT64_MAX - 1), (uint64_t)INT64_MAX};
    const double denorm = from_bits(1ull), denorm_max = from_bits(0x000FFFFFFFFFFFFFull);
    std::vector<uint64_t> flts;
    for (double v : {0.0, -0.0, denorm, -denorm, denorm_max, -denorm_max, DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX, (double)INFINITY,
                     -(double)INFINITY, 1.0, -1.0, 1.5, -1.5, 1e300, -1e300})
        flts.push_back(to_bits(v));
    // NaNs: quiet / signalling, several payloads, both signs
    for (uint64_t nan : {0x7FF8000000000000ull, 0x7FF8000000000001ull, 0x7FF0000000000001ull, 0x7FFFFFFFFFFFFFFFull, 0xFFF8000000000000ull,
                         0xFFF8000000000001ull, 0xFFF0000000000001ull, 0xFFFFFFFFFFFFFFFFull})
        flts.push_back(nan);
    for (uint64_t a : ints)
        for (uint64_t b : ints) check_pair(a, b, false);
    for (uint64_t a : flts)
        for (uint64_t b : flts) check_pair(a, b, true);
    // the layout the select relies on: NaN is the all-zero key, nothing else is; INT64_MAX is the all-one key
    g_checked += 3;
    if (order_map_float64(0x7FF8000000000001ull) != 0 || order_map_float64(to_bits(-(double)INFINITY)) == 0) {
        g_failed++;
        printf("FAIL: NaN must map to 0 and -Inf above it\n");
    }
    if (order_map_int64((uint64_t)INT64_MAX) != ~0ull || order_map_int64((uint64_t)INT64_MIN) != 0) {
        g_failed++;
        printf("FAIL: INT64_MAX / INT64_MIN must map to the all-one / all-zero key\n");
    }
    // random bit patterns, against each other and against every edge value
    for (int i = 0; i < 500000; i++) {
        const uint64_t a = next_u64(), b = next_u64();
        check_pair(a, b, false);
        check_pair(a, b, true);
        check_pair(a, ints[(size_t)i % ints.size()], false);
        check_pair(flts[(size_t)i % flts.size()], a, true);
        // neighbours in the exponent field: patterns that differ in few bits
        check_pair(a, a ^ (1ull << (i & 63)), true);
        check_pair(a, a ^ (1ull << (i & 63)), false);
    }
    printf("%ld checks, %ld failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
