// The shortest float formatter of csvplus_amd/csrc/shortfmt_device.hpp — the code the Map kernels run for a
// CPH_MAP_FLOAT64_SHORTEST piece — compiled for the host (CPU only, no HIP).  Digits and exponent are compared with
// std::to_chars(v, chars_format::scientific), the shortest round-trip digits closest to the value; the 'e' text is compared
// with to_chars' text byte for byte, the 'f' / 'g' / 'E' / 'G' texts with a layout written here over std::string from
// to_chars' digits (Go's strconv/ftoa.go rules for prec = -1).  For every value and all five format bytes the length
// function must equal the number of bytes put.  Values:
//   * every power of two 2^-1074 .. 2^1023 with both neighbours; every subnormal binade's ends and random members;
//   * 10^k and both neighbours, k = -323..308;
//   * integers: small ones, random ones below 2^53, 2^53 and its neighbours;
//   * short decimals k / 10^j;
//   * 1e5 seeded random bit patterns per class: any finite, subnormal, near 1, both signs;
//   * zeros, infinities, NaNs with payloads.
// The 'f' maximum (kShortMaxCharsF) must be reached and never exceeded; likewise 'e' and 'g'.
// An argument N > 1 thins the random classes to 1 / N (the run under the sanitizers).
#include <charconv>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "shortfmt_device.hpp"

using namespace cph;

static int failures = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            if (++failures <= 20) {                   \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);             \
                std::printf("\n");                    \
            }                                         \
        }                                             \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double of_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

struct StringSink {
    std::string out;
    int bad = 0;
    void put8(uint64_t chunk, uint32_t n) {
        if (n < 1 || n > 8) bad++;
        for (uint32_t j = 0; j < n && j < 8; j++) out.push_back((char)(chunk >> (8 * j)));
    }
};

static std::string ours(double v, char fmt, uint32_t* chars) {
    const ShortParts r = short_split(v);
    *chars = short_chars(r, fmt);
    StringSink s;
    short_put(s, r, fmt);
    CHECK(s.bad == 0, "put8 with a count outside 1..8 for %a '%c'", v, fmt);
    return s.out;
}

// Go's layouts over the digits of to_chars' scientific text
static std::string expected(double v, char fmt, std::string* digits, int* dp) {
    const bool neg = std::signbit(v);
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return neg ? "-Inf" : "+Inf";
    char buf[64];
    const auto res = std::to_chars(buf, buf + sizeof buf, std::fabs(v), std::chars_format::scientific);
    const std::string sci(buf, res.ptr);
    const size_t epos = sci.find('e');
    std::string d;
    for (size_t i = 0; i < epos; i++)
        if (sci[i] != '.') d.push_back(sci[i]);
    const int exp = std::atoi(sci.c_str() + epos + 1);
    *digits = d, *dp = exp + 1;
    const std::string sign = neg ? "-" : "";
    const bool upper = fmt == 'E' || fmt == 'G';
    const bool eform = fmt == 'e' || fmt == 'E' || (fmt != 'f' && (exp < -4 || exp >= 6));
    if (eform) {
        std::string t = sign + sci;
        if (upper) t[t.find('e')] = 'E';
        return t;
    }
    const int nd = (int)d.size(), p = exp + 1;
    if (d == "0") return sign + "0";
    if (p <= 0) return sign + "0." + std::string((size_t)-p, '0') + d;
    if (p < nd) return sign + d.substr(0, (size_t)p) + "." + d.substr((size_t)p);
    return sign + d + std::string((size_t)(p - nd), '0');
}

static uint32_t max_e = 0, max_f = 0, max_g = 0;
static long checked = 0;

static void check_value(double v) {
    checked++;
    const char fmts[5] = {'e', 'E', 'f', 'g', 'G'};
    std::string d;
    int dp = 0;
    if (std::isfinite(v)) {
        expected(v, 'e', &d, &dp);
        const ShortParts r = short_split(v);
        CHECK(r.kind == SHORT_FINITE && r.neg == (std::signbit(v) ? 1u : 0u), "kind / sign of %a", v);
        CHECK(std::to_string(r.digits) == d && r.nd == (int)d.size() && r.dp == dp, "%a: digits %" PRIu64 " nd %d dp %d, want %s dp %d", v, r.digits,
              r.nd, r.dp, d.c_str(), dp);
    }
    for (char f : fmts) {
        uint32_t n = 0;
        const std::string got = ours(v, f, &n), want = expected(v, f, &d, &dp);
        CHECK(got == want, "%a '%c': got %s, want %s", v, f, got.c_str(), want.c_str());
        CHECK(n == got.size(), "%a '%c': the length function says %u, %zu bytes put", v, f, n, got.size());
        uint32_t& mx = f == 'f' ? max_f : (f == 'e' || f == 'E') ? max_e : max_g;
        if (n > mx) mx = n;
    }
}

static void both_signs(double v) {
    check_value(v);
    check_value(-v);
}

static void with_neighbours(double v) {
    both_signs(v);
    if (v > 0) both_signs(of_bits(bits_of(v) - 1));
    if (std::isfinite(v) && bits_of(v) + 1 < 0x7FF0000000000000ull) both_signs(of_bits(bits_of(v) + 1));
}

static void section(const char* name, long before) { std::printf("%-40s %ld values\n", name, checked - before); }

int main(int argc, char** argv) {
    const int thin = argc > 1 ? std::atoi(argv[1]) : 1;   // test_shortfmt 10: a tenth of the random values (the sanitizer run)
    if (thin < 1) return 2;
    long at = checked;
    for (int e = -1074; e <= 1023; e++) with_neighbours(std::ldexp(1.0, e));
    section("powers of two and neighbours", at);

    at = checked;
    for (int b = 0; b < 52; b++) {   // binade b: mantissas 2^b .. 2^(b+1) - 1 of 2^-1074
        both_signs(of_bits(1ull << b));
        both_signs(of_bits((2ull << b) - 1));
        for (int k = 0; k < 2000 / thin; k++) both_signs(of_bits((1ull << b) | (rnd() & ((1ull << b) - 1))));
    }
    section("subnormal binades", at);

    at = checked;
    for (int k = -323; k <= 308; k++) {
        char t[16];
        std::snprintf(t, sizeof t, "1e%d", k);
        with_neighbours(std::strtod(t, nullptr));
    }
    section("powers of ten and neighbours", at);

    at = checked;
    for (uint64_t i = 0; i <= 20000u / (unsigned)thin; i++) both_signs((double)i);
    for (int k = 0; k < 100000 / thin; k++) both_signs((double)(rnd() >> (11 + rnd() % 53)));
    with_neighbours(9007199254740992.0);
    for (uint64_t p = 1, k = 0; k <= 18; k++, p *= 10) {
        with_neighbours((double)p);
        with_neighbours((double)(p * 5));
    }
    section("integers", at);

    at = checked;
    for (int j = 0; j <= 22; j++) {
        char t[48];
        for (int k = 0; k < 4000 / thin; k++) {
            std::snprintf(t, sizeof t, "%" PRIu64 "e-%d", rnd() % 100000, j);
            both_signs(std::strtod(t, nullptr));
        }
    }
    section("short decimals k / 10^j", at);

    at = checked;
    for (int k = 0; k < 100000 / thin; k++) {
        uint64_t b = rnd();
        if (((b >> 52) & 0x7FF) == 0x7FF) b &= ~(1ull << 62);
        check_value(of_bits(b));
    }
    section("random finite bit patterns", at);
    at = checked;
    for (int k = 0; k < 100000 / thin; k++) check_value(of_bits(rnd() & 0x800FFFFFFFFFFFFFull));
    section("random subnormals", at);
    at = checked;
    for (int k = 0; k < 100000 / thin; k++) check_value(of_bits((rnd() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 30 + rnd() % 90) << 52)));
    section("random values of 2^-30 .. 2^60", at);
    at = checked;
    for (int k = 0; k < 100000 / thin; k++) check_value(of_bits((rnd() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1 + rnd() % 40) << 52)));
    section("random values near 1e-300", at);

    at = checked;
    both_signs(0.0);
    both_signs(INFINITY);
    both_signs(of_bits(0x7FF8000000000000ull));
    both_signs(of_bits(0x7FF0000000000001ull));
    both_signs(of_bits(0x7FFFFFFFFFFFFFFFull));
    both_signs(of_bits(0x7FF4000000ABCDEFull));
    both_signs(1.7976931348623157e308);
    both_signs(2.2250738585072014e-308);
    both_signs(5e-324);
    both_signs(std::ldexp(8511030020275656.0, -342));   // 9.5e-88: two digits
    both_signs(99999999999999974834176.0);
    section("specials and literals", at);

    // a few texts by hand, so that the layout above is itself pinned
    struct { double v; char f; const char* want; } pins[] = {
        {1.0, 'e', "1e+00"}, {1.0, 'f', "1"}, {1e5, 'g', "100000"}, {1e6, 'g', "1e+06"}, {1e6, 'G', "1E+06"}, {1e5, 'E', "1E+05"},
        {123456.7, 'g', "123456.7"}, {1234567.8, 'g', "1.2345678e+06"}, {1e-4, 'g', "0.0001"}, {1e-5, 'g', "1e-05"}, {1e-5, 'f', "0.00001"},
        {0.3, 'e', "3e-01"}, {1e23, 'f', "100000000000000000000000"}, {std::ldexp(1.0, 976), 'e', "6.386688990511104e+293"},
        {-0.0, 'e', "-0e+00"}, {-0.0, 'f', "-0"}, {-0.0, 'g', "-0"}, {5e-324, 'e', "5e-324"}, {9007199254740992.0, 'g', "9.007199254740992e+15"},
    };
    for (const auto& p : pins) {
        uint32_t n = 0;
        const std::string got = ours(p.v, p.f, &n);
        CHECK(got == p.want, "pinned %a '%c': got %s, want %s", p.v, p.f, got.c_str(), p.want);
    }
    {
        uint32_t n = 0;
        const std::string t = ours(5e-324, 'f', &n);
        CHECK(t == "0." + std::string(323, '0') + "5", "5e-324 'f': %s", t.c_str());
        CHECK(ours(-2.2250738585072014e-308, 'f', &n).size() == kShortMaxCharsF, "the longest 'f' text has %u characters", n);
    }

    std::printf("longest: 'e' %u (constant %u), 'f' %u (constant %u), 'g' %u (constant %u)\n", max_e, kShortMaxCharsE, max_f, kShortMaxCharsF, max_g,
                kShortMaxCharsG);
    CHECK(max_e == kShortMaxCharsE, "'e' maximum");
    CHECK(max_f == kShortMaxCharsF, "'f' maximum");
    CHECK(max_g == kShortMaxCharsG, "'g' maximum");
    if (failures) {
        std::printf("test_shortfmt: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("test_shortfmt: OK (%ld values)\n", checked);
    return 0;
}
