// The Eisel-Lemire conversion of csvplus_amd/csrc/floatparse_device.hpp — the code k_num_parse's full float instantiation
// runs behind Clinger's exact cases — compiled for the host (CPU only, no HIP).  Every decided value is compared bit for bit
// with glibc's strtod on the same text:
//   * "%.17g" of random bit patterns over the whole exponent range, both signs;
//   * subnormals;
//   * 19-digit mantissas with exponents -330..300;
//   * truncated values of 25 and 40 digits (the routine runs for w and w + 1);
//   * a literal list around the rounding, overflow and underflow edges.
// Conditions: no wrong bit anywhere, no undecided value in the classes that are not truncated, at most 1 % undecided in the
// truncated ones.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "floatparse_device.hpp"

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

// [+-] digits [. digits] [e [+-] digits] -> sign, the first 19 significant digits, the decimal exponent, trunc (what the
// device's byte loop hands to float_eisel_lemire).  The texts here are well formed.
struct Decimal {
    bool neg, trunc;
    uint64_t w;
    int32_t q;
};
static Decimal read_decimal(const std::string& s) {
    Decimal d{false, false, 0, 0};
    size_t i = 0;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) d.neg = s[i++] == '-';
    bool sawdot = false;
    int nd = 0, ndmant = 0, dp = 0;
    for (; i < s.size(); i++) {
        const char c = s[i];
        if (c == '.') {
            sawdot = true;
            dp = nd;
            continue;
        }
        if (c < '0' || c > '9') break;
        if (c == '0' && nd == 0) {
            dp--;
            continue;
        }
        nd++;
        if (ndmant < 19) {
            d.w = d.w * 10 + (uint64_t)(c - '0');
            ndmant++;
        } else if (c != '0') {
            d.trunc = true;
        }
    }
    if (!sawdot) dp = nd;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        int esign = 1;
        if (s[i] == '+' || s[i] == '-') esign = s[i++] == '-' ? -1 : 1;
        int e = 0;
        for (; i < s.size(); i++) e = e * 10 + (s[i] - '0');
        dp += e * esign;
    }
    if (i != s.size()) {
        std::printf("test bug: cannot read %s\n", s.c_str());
        std::exit(2);
    }
    d.q = dp - ndmant;
    return d;
}

struct Tally {
    uint64_t n = 0, undecided = 0, wrong = 0;
};

// true: decided (and compared)
static bool check_text(const std::string& s, Tally* t) {
    const Decimal d = read_decimal(s);
    t->n++;
    if (d.w == 0) {
        std::printf("test bug: zero mantissa in %s\n", s.c_str());
        std::exit(2);
    }
    uint64_t got = 0xDEADBEEFDEADBEEFull;
    if (!float_eisel_lemire(d.w, d.q, d.trunc, &got)) {
        t->undecided++;
        return false;
    }
    got |= (uint64_t)d.neg << 63;
    const uint64_t want = bits_of(std::strtod(s.c_str(), nullptr));
    if (got != want) t->wrong++;
    CHECK(got == want, "%s: %016" PRIx64 ", strtod %016" PRIx64, s.c_str(), got, want);
    return true;
}

static std::string fmt17(double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

static std::string random_digits(int n) {
    std::string s;
    s.push_back((char)('1' + rnd() % 9));
    for (int k = 1; k < n; k++) s.push_back((char)('0' + rnd() % 10));
    return s;
}

static void report(const char* name, const Tally& t, double max_undecided_share) {
    std::printf("%-28s %8" PRIu64 " values, %6" PRIu64 " undecided (%.3f %%), %" PRIu64 " wrong\n", name, t.n, t.undecided,
                100.0 * (double)t.undecided / (double)(t.n ? t.n : 1), t.wrong);
    CHECK(t.wrong == 0, "%s: %" PRIu64 " wrong bits", name, t.wrong);
    CHECK((double)t.undecided <= max_undecided_share * (double)t.n, "%s: %" PRIu64 " of %" PRIu64 " undecided", name, t.undecided, t.n);
}

int main(int argc, char** argv) {
    const int N = argc > 1 ? std::atoi(argv[1]) : 100000;

    {   // "%.17g" of random bit patterns: every exponent field 0..2046, both signs
        Tally t;
        for (int k = 0; k < N; k++) {
            uint64_t b = rnd();
            if (((b >> 52) & 0x7FF) == 0x7FF) b &= ~(1ull << 62);   // finite
            if ((b << 1) == 0) b |= 1;                              // not zero
            double v;
            std::memcpy(&v, &b, 8);
            const std::string s = fmt17(v);
            if (check_text(s, &t)) CHECK(bits_of(std::strtod(s.c_str(), nullptr)) == b, "%s does not round-trip", s.c_str());
        }
        report("%.17g of random doubles", t, 0.0);
    }
    {   // subnormals
        Tally t;
        for (int k = 0; k < N; k++) {
            uint64_t b = rnd() & ((1ull << 52) - 1);
            b >>= rnd() % 52;   // every width of a subnormal mantissa
            if (b == 0) b = 1;
            double v;
            std::memcpy(&v, &b, 8);
            check_text(fmt17(v), &t);
        }
        report("subnormals", t, 0.0);
    }
    {   // 19 digits, exponents -330..300
        Tally t;
        for (int k = 0; k < N; k++) {
            char e[16];
            std::snprintf(e, sizeof e, "e%d", (int)(rnd() % 631) - 330);
            check_text(random_digits(19) + e, &t);
        }
        report("19-digit mantissas", t, 0.0);
    }
    for (int nd : {25, 40}) {   // truncated: digits dropped behind the 19th; the value's magnitude spans the whole range
        Tally t;
        while (t.n < (uint64_t)N) {
            char e[16];
            std::snprintf(e, sizeof e, "e%d", (int)(rnd() % 631) - 330 - (nd - 19));
            std::string s = random_digits(nd);
            if (rnd() % 4 == 0) s.insert(1 + rnd() % (nd - 1), ".");
            const std::string text = s + e;
            const Decimal d = read_decimal(text);
            if (!d.trunc) continue;   // the dropped digits were all zeros: once in 10^6 and 10^21
            check_text(text, &t);
        }
        report(nd == 25 ? "truncated, 25 digits" : "truncated, 40 digits", t, 0.01);
    }
    {   // literals: decided, equal to strtod, and what the issue's list says about them
        struct Lit {
            const char* text;
            uint64_t want;
        };
        const Lit lits[] = {
            {"9007199254740993", 0x4340000000000000ull},          // 2^53 + 1: a tie, to even
            {"9007199254740992.5", 0x4340000000000000ull},
            {"1.7976931348623157e308", 0x7FEFFFFFFFFFFFFFull},
            {"1.7976931348623158e308", 0x7FEFFFFFFFFFFFFFull},    // the largest double
            {"1.7976931348623159e308", 0x7FF0000000000000ull},    // inf
            {"4.9406564584124654e-324", 0x0000000000000001ull},
            {"2.4703282292062327e-324", 0x0000000000000000ull},   // just below half the smallest subnormal
            {"2.4703282292062328e-324", 0x0000000000000001ull},   // just above it
            {"2.2250738585072011e-308", 0x000FFFFFFFFFFFFFull},   // the largest subnormal
            {"2.2250738585072014e-308", 0x0010000000000000ull},   // the smallest normal
            {"1e23", 0x44B52D02C7E14AF6ull},
            {"8.5e22", 0},                                        // 0: strtod alone says
            {"-122.41941550000001", 0},
            {"1e-30", 0},
        };
        Tally t;
        for (const Lit& l : lits) {
            CHECK(check_text(l.text, &t), "%s is undecided", l.text);
            if (l.want) CHECK(bits_of(std::strtod(l.text, nullptr)) == l.want, "%s: the literal's expectation is not strtod's", l.text);
        }
        {
            const Decimal d = read_decimal("2.4703282292062327e-324");
            uint64_t b = 1;
            CHECK(float_eisel_lemire(d.w, d.q, d.trunc, &b) && b == 0, "2.4703282292062327e-324 -> %016" PRIx64, b);
        }
        uint64_t b = 1;
        CHECK(float_eisel_lemire(1, -343, false, &b) && b == 0, "1e-343 -> %016" PRIx64, b);
        CHECK(float_eisel_lemire(1, 309, false, &b) && b == kFloatInfBits, "1e309 -> %016" PRIx64, b);
        CHECK(float_eisel_lemire(9999999999999999999ull, -343, true, &b) && b == 0, "9.99..e-325 (truncated) -> %016" PRIx64, b);
        CHECK(float_eisel_lemire(1, 308, false, &b) && b == bits_of(1e308), "1e308 -> %016" PRIx64, b);
        CHECK(float_eisel_lemire(1, -342, false, &b) && b == 0, "1e-342 -> %016" PRIx64, b);
        // a tie that only the dropped digits break: w rounds down to even, w + 1 up — the routine must not decide
        const Decimal d = read_decimal("9007199254740993.0000000000000000000001");
        CHECK(d.trunc && !float_eisel_lemire(d.w, d.q, d.trunc, &b), "9007199254740993.0000000000000000000001 was decided");
        report("literals", t, 0.0);
    }
    if (failures) {
        std::printf("test_floatparse: %d FAILED\n", failures);
        return 1;
    }
    std::printf("test_floatparse: OK\n");
    return 0;
}
