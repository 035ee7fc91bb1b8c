// The fixed-precision float formatter of the Map kernels (csvplus_amd/csrc/numformat_device.hpp) compiled for the host and
// run against glibc's snprintf("%.*f"), which is exact: every prec 0..22 on a table of edge values and on random bit
// patterns below 2^128, the reported character count against the bytes produced, and the values the formatter refuses.
// CPU only: no GPU and no library needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "numformat_device.hpp"

using namespace cph;

namespace {

struct BufSink {
    char* p;
    void put8(uint64_t chunk, uint32_t n) {
        for (uint32_t j = 0; j < n; j++) *p++ = (char)(chunk >> (8u * j));
    }
};

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

// Go's spelling: glibc's for finite values, "NaN" / "+Inf" / "-Inf" for the rest
std::string expected(double v, int prec) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-Inf" : "+Inf";
    char buf[512];
    const int n = snprintf(buf, sizeof buf, "%.*f", prec, v);
    return std::string(buf, (size_t)n);
}

void check(double v, int prec) {
    char buf[kFixedMaxChars + 17];
    memset(buf, '#', sizeof buf);
    const FixedParts r = fixed_split(v, prec);
    const uint32_t len = fixed_chars(r, prec);
    BufSink s{buf};
    fixed_put(s, r, prec);
    const size_t made = (size_t)(s.p - buf);
    const std::string want = expected(v, prec);
    g_checked++;
    if (r.kind == FIXED_RANGE || len != made || len > kFixedMaxChars || want != std::string(buf, made)) {
        if (g_failed++ < 20)
            printf("FAIL bits=%016llx prec=%d: got \"%.*s\" (%zu bytes, %u reported, kind %u), want \"%s\"\n",
                   (unsigned long long)to_bits(v), prec, (int)made, buf, made, len, r.kind, want.c_str());
    }
}

void check_refused(double v) {
    for (int prec = 0; prec <= kFixedMaxPrec; prec += 11) {
        char buf[kFixedMaxChars + 17];
        const FixedParts r = fixed_split(v, prec);
        BufSink s{buf};
        fixed_put(s, r, prec);
        g_checked++;
        if (r.kind != FIXED_RANGE || fixed_chars(r, prec) != 0 || s.p != buf) {
            if (g_failed++ < 20) printf("FAIL bits=%016llx prec=%d: not refused\n", (unsigned long long)to_bits(v), prec);
        }
    }
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

int main(int argc, char** argv) {
    const long nrandom = argc > 1 ? atol(argv[1]) : 1200000;
    const double two52 = 4503599627370496.0, two64 = 18446744073709551616.0, two128 = std::ldexp(1.0, 128);
    const double edges[] = {
        0.125, 0.375, 2.5, 3.5, 2.675, 1.005, 9.995, 0.1, 0.5, 1.5, 0.05, 0.25, 0.75,
        9.5, 0.999999, 999999.9999995, 99.5, 0.95, 0.995,
        0.0, -0.0, -0.001, 0.001, 1.0, 10.0, 123456.789,
        5e-324, 2.2250738585072014e-308, std::nextafter(2.2250738585072014e-308, 0.0),
        std::ldexp(1.0, -75), std::nextafter(std::ldexp(1.0, -75), 0.0), std::nextafter(std::ldexp(1.0, -75), 1.0),
        std::ldexp(1.0, -74), std::ldexp(1.0, -73), std::ldexp(1.0, -76), std::ldexp(1.0, -127), std::ldexp(1.0, -128),
        std::ldexp(1.0, -129), std::ldexp(4503599627370497.0, -52 - 74), std::ldexp(9007199254740991.0, -53 - 73),
        two52 + 0.5, two52 - 0.5, two52 + 1.5, two52 / 2 + 0.25, two52 / 2 + 0.75, two52,
        9007199254740993.0, 9007199254740992.0, 9223372036854775808.0,
        two64, std::nextafter(two64, 0.0), std::nextafter(two64, two128),
        9999999999999999999.0, 1e19, 1e20, 1e22, 1e23, 1e38,
        std::nextafter(two128, 0.0), std::ldexp(1.0, 127),
        from_bits(0xFFF8000000001234ull), from_bits(0x7FF0000000000001ull), (double)INFINITY, -(double)INFINITY,
    };
    for (double v : edges)
        for (int prec = 0; prec <= kFixedMaxPrec; prec++) {
            check(v, prec);
            check(-v, prec);
        }
    // random bit patterns, exponent field below 1023 + 128, every prec in turn
    for (long i = 0; i < nrandom; i++) {
        uint64_t b = next_u64();
        const uint64_t ef = ((b >> 52) & 0x7FF) % (1023 + 128);
        b = (b & ~(0x7FFull << 52)) | ef << 52;
        check(from_bits(b), (int)(i % (kFixedMaxPrec + 1)));
    }
    // magnitudes around 1, where integer and fraction digits meet: exponents 2^-80 .. 2^70
    for (long i = 0; i < nrandom / 4; i++) {
        uint64_t b = next_u64();
        const uint64_t ef = 1023 - 80 + ((b >> 52) & 0x7FF) % 150;
        b = (b & ~(0x7FFull << 52)) | ef << 52;
        check(from_bits(b), (int)((b >> 3) % (kFixedMaxPrec + 1)));
    }
    // short decimal fractions, many of them ties or near-ties at some prec
    for (long i = 0; i < 200000; i++) {
        const uint64_t r = next_u64();
        const double v = (double)(r % 2000001) / (double)(1ull << (r >> 60)) / 1000.0 * ((r >> 40 & 1) ? 1.0 : 0.125);
        check(v, (int)((r >> 32) % 8));
        check((double)(r % 4097) / 4096.0 + (double)((r >> 20) % 1000), (int)((r >> 32) % 14));
    }
    check_refused(two128);
    check_refused(-two128);
    check_refused(1e300);
    check_refused(1.7976931348623157e308);
    printf("%ld checks, %ld failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
