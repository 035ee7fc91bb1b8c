// The RFC 3339 routines of csvplus_amd/csrc/timeparse_device.hpp — the code k_num_parse and the Map kernels run per value —
// compiled for the host (CPU only, no HIP):
//   * days_from_civil / civil_from_days / days_in_month over EVERY day from 0000-01-01 to 9999-12-31 against a running counter;
//   * the formatter and the parser against gmtime_r / timegm on a stride of instants, and against each other in five zones;
//   * the classification table of include/csvplus_hip.h (cph_col_to_number), both kinds;
//   * one wrong byte at a time over the 25-byte form.
// The value's bytes past its end are filled with 0xAA on purpose: the routines must not look at them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "timeparse_device.hpp"

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

struct HostChunks {   // the functor V over an exact-size copy of the value: reading past it is a sanitizer finding
    const std::vector<unsigned char>& b;
    uint64_t operator()(int j) const {
        uint64_t w = 0xAAAAAAAAAAAAAAAAull;
        const size_t at = 8 * (size_t)j;
        if (at >= b.size()) std::abort();   // the contract: only chunks that hold a byte of the value
        const size_t n = b.size() - at < 8 ? b.size() - at : 8;
        std::memcpy(&w, b.data() + at, n);
        return w;
    }
};

static uint32_t parse(const std::string& s, bool nano, int64_t* out) {
    const std::vector<unsigned char> b(s.begin(), s.end());
    const HostChunks v{b};
    uint64_t c[2] = {0, 0}, t[2] = {0xAAAAAAAAAAAAAAAAull, 0xAAAAAAAAAAAAAAAAull};
    for (int j = 0; j < 2; j++)
        if (b.size() > 8 * (size_t)j) c[j] = v(j) & time_low_bytes((uint32_t)(b.size() - 8 * j < 8 ? b.size() - 8 * j : 8));
    for (int j = 2; j < 4; j++)
        if (b.size() > 8 * (size_t)j) t[j - 2] = v(j);
    return parse_rfc3339(b.size(), c[0], c[1], t[0], t[1], v, nano, out);
}

static std::string format(int64_t v, int32_t zone) {
    uint64_t w[4];
    rfc3339_words(v, zone, &w[0], &w[1], &w[2], &w[3]);
    char buf[32];
    std::memcpy(buf, w, 32);
    return std::string(buf, rfc3339_chars(zone));
}

static void every_day() {
    int32_t counter = -719528;   // 0000-01-01
    uint64_t ndays = 0;
    for (uint32_t y = 0; y <= 9999; y++) {
        const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
        static const uint32_t ml[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
        for (uint32_t m = 1; m <= 12; m++) {
            const uint32_t dim = ml[m - 1] + (m == 2 && leap ? 1 : 0);
            CHECK(days_in_month(y, m) == dim, "days_in_month(%u, %u) = %u", y, m, days_in_month(y, m));
            for (uint32_t d = 1; d <= dim; d++, counter++, ndays++) {
                CHECK(days_from_civil(y, m, d) == counter, "days_from_civil(%u-%u-%u) = %d, not %d", y, m, d, days_from_civil(y, m, d), counter);
                uint32_t yy, mm, dd;
                civil_from_days(counter, &yy, &mm, &dd);
                CHECK(yy == y && mm == m && dd == d, "civil_from_days(%d) = %u-%u-%u, not %u-%u-%u", counter, yy, mm, dd, y, m, d);
            }
        }
    }
    CHECK(ndays == 3652425, "%llu days", (unsigned long long)ndays);
    CHECK(days_from_civil(1970, 1, 1) == 0, "the epoch is day %d", days_from_civil(1970, 1, 1));
    CHECK(counter == 2932897, "the day behind 9999-12-31 is %d", counter);
}

static void against_libc() {
    // a prime stride over the whole range: every second of day, weekday and month phase turns up
    for (int64_t v = kTimeMinSeconds; v <= kTimeMaxSeconds; v += 86400ll * 37 + 3607) {
        const time_t tt = (time_t)v;
        struct tm g;
        if (!gmtime_r(&tt, &g)) continue;
        char want[40];
        std::snprintf(want, sizeof want, "%04d-%02d-%02dT%02d:%02d:%02dZ", g.tm_year + 1900, g.tm_mon + 1, g.tm_mday, g.tm_hour, g.tm_min, g.tm_sec);
        const std::string got = format(v, 0);
        CHECK(got == want, "format(%lld) = %s, gmtime_r says %s", (long long)v, got.c_str(), want);
        CHECK((int64_t)timegm(&g) == v, "timegm disagrees with gmtime_r at %lld", (long long)v);
        for (int32_t zone : {0, 60, -330, 1439, -1439}) {
            if (!rfc3339_in_range(v, zone)) continue;
            int64_t back = 0;
            const std::string s = format(v, zone);
            CHECK(parse(s, false, &back) == kTimeOk && back == v, "parse(format(%lld, %d) = %s) = %lld", (long long)v, zone, s.c_str(), (long long)back);
        }
    }
    CHECK(format(kTimeMinSeconds, 0) == "0000-01-01T00:00:00Z", "%s", format(kTimeMinSeconds, 0).c_str());
    CHECK(format(kTimeMaxSeconds, 0) == "9999-12-31T23:59:59Z", "%s", format(kTimeMaxSeconds, 0).c_str());
    CHECK(format(-1, 0) == "1969-12-31T23:59:59Z", "%s", format(-1, 0).c_str());
    CHECK(format(0, -330) == "1969-12-31T18:30:00-05:30", "%s", format(0, -330).c_str());
    CHECK(format(0, 1439) == "1970-01-01T23:59:00+23:59", "%s", format(0, 1439).c_str());
    CHECK(!rfc3339_in_range(kTimeMaxSeconds, 1) && !rfc3339_in_range(kTimeMinSeconds, -1), "a zone pushing the year out of 0000..9999 is in range");
    CHECK(rfc3339_in_range(kTimeMaxSeconds + 60, -1) && rfc3339_in_range(kTimeMinSeconds - 60, 1), "a zone pulling the year into 0000..9999 is not");
    CHECK(!rfc3339_in_range(INT64_MAX, 1439) && !rfc3339_in_range(INT64_MIN, -1439), "the int64 ends are in range");
}

struct Row {
    const char* text;
    uint32_t st_s;
    int64_t secs;
    uint32_t st_ns;
    int64_t ns;
};

static const Row kTable[] = {
    // valid forms
    {"2016-09-14T08:48:22Z", 0, 1473842902, 0, 1473842902000000000ll},
    {"2016-09-14T08:48:22+01:00", 0, 1473839302, 0, 1473839302000000000ll},
    {"2016-09-14T08:48:22-00:00", 0, 1473842902, 0, 1473842902000000000ll},
    {"2016-09-14T08:48:22+23:59", 0, 1473842902 - 86340, 0, (1473842902ll - 86340) * 1000000000ll},
    {"2016-09-14T08:48:22-23:59", 0, 1473842902 + 86340, 0, (1473842902ll + 86340) * 1000000000ll},
    {"2016-09-14T08:48:22.5Z", 0, 1473842902, 0, 1473842902500000000ll},
    {"2016-09-14T08:48:22.125Z", 0, 1473842902, 0, 1473842902125000000ll},
    {"2016-09-14T08:48:22.123456789Z", 0, 1473842902, 0, 1473842902123456789ll},
    {"2016-09-14T08:48:22.123456789-05:30", 0, 1473842902 + 19800, 0, (1473842902ll + 19800) * 1000000000ll + 123456789},
    {"2016-09-14T08:48:22.000000001+02:00", 0, 1473842902 - 7200, 0, (1473842902ll - 7200) * 1000000000ll + 1},
    {"0000-01-01T00:00:00Z", 0, -62167219200ll, 3, 0},
    {"9999-12-31T23:59:59Z", 0, 253402300799ll, 3, 0},
    {"1969-12-31T23:59:59.5Z", 0, -1, 0, -500000000ll},
    {"2000-02-29T12:00:00Z", 0, 951825600, 0, 951825600000000000ll},
    {"0000-02-29T00:00:00Z", 0, -62167219200ll + 59 * 86400ll, 3, 0},
    {"1970-01-01T00:00:00Z", 0, 0, 0, 0},
    // range errors
    {"1900-02-29T00:00:00Z", 2, 0, 2, 0},
    {"2001-02-29T00:00:00Z", 2, 0, 2, 0},
    {"2016-00-14T08:48:22Z", 2, 0, 2, 0},
    {"2016-13-14T08:48:22Z", 2, 0, 2, 0},
    {"2016-09-00T08:48:22Z", 2, 0, 2, 0},
    {"2016-09-32T08:48:22Z", 2, 0, 2, 0},
    {"2016-04-31T08:48:22Z", 2, 0, 2, 0},
    {"2016-09-14T24:00:00Z", 2, 0, 2, 0},
    {"2016-09-14T08:60:22Z", 2, 0, 2, 0},
    {"2016-09-14T23:59:60Z", 2, 0, 2, 0},
    {"2016-13-14T08:48:22+24:00", 2, 0, 2, 0},   // the range error is decided in front of the zone's
    // unsupported
    {"2016-09-14T8:48:22Z", 3, 0, 3, 0},
    {"2016-09-14T8:48:22+01:00", 3, 0, 3, 0},
    {"2016-13-14T8:48:22Z", 3, 0, 3, 0},        // ... and the relaxation in front of the range
    {"2016-09-14T08:48:22,5Z", 3, 0, 3, 0},
    {"2016-09-14T08:48:22.1234567890Z", 3, 0, 3, 0},
    {"2016-09-14T08:48:22.1234567890+01:00", 3, 0, 3, 0},
    {"2016-09-14T08:48:22.12345678901234567890123456789Z", 3, 0, 3, 0},
    {"2016-09-14T8:48:22,1234567890Z", 3, 0, 3, 0},
    {"2016-09-14T08:48:22+24:00", 3, 0, 3, 0},
    {"2016-09-14T08:48:22+01:60", 3, 0, 3, 0},
    {"1677-09-21T00:12:43Z", 0, -9223372037ll, 3, 0},
    {"1677-09-21T00:12:44Z", 0, -9223372036ll, 0, -9223372036000000000ll},
    {"1677-09-21T00:12:43.145224192Z", 0, -9223372037ll, 0, INT64_MIN},
    {"1677-09-21T00:12:43.145224191Z", 0, -9223372037ll, 3, 0},
    {"2262-04-11T23:47:17Z", 0, 9223372037ll, 3, 0},
    {"2262-04-11T23:47:16Z", 0, 9223372036ll, 0, 9223372036000000000ll},
    {"2262-04-11T23:47:16.854775807Z", 0, 9223372036ll, 0, INT64_MAX},
    {"2262-04-11T23:47:16.854775808Z", 0, 9223372036ll, 3, 0},
    // syntax errors
    {"", 1, 0, 1, 0},
    {"2016-09-14T08:48:22", 1, 0, 1, 0},
    {"2016-09-14t08:48:22Z", 1, 0, 1, 0},
    {"2016-09-14T08:48:22z", 1, 0, 1, 0},
    {"2016-09-14 08:48:22Z", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.Z", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.+01:00", 1, 0, 1, 0},
    {"2016-09-14T08:48:22+0100", 1, 0, 1, 0},
    {"2016-09-14T08:48:22Z ", 1, 0, 1, 0},
    {"2016-09-14T08:48:22+01:00x", 1, 0, 1, 0},
    {" 2016-09-14T08:48:22Z", 1, 0, 1, 0},
    {"2016-09-14T08:48Z", 1, 0, 1, 0},
    {"2016-09-14", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.5", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.12345678Z0", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.1234x6789+01:00", 1, 0, 1, 0},
    {"2016-09-14T08:48:22.12345678x+01:00", 1, 0, 1, 0},
    {"2016-09-14T08:48:22+1:00", 1, 0, 1, 0},
    {"Z", 1, 0, 1, 0},
    {"12345678901234567890", 1, 0, 1, 0},
};

static void table() {
    for (const Row& r : kTable) {
        int64_t v = 77;
        uint32_t st = parse(r.text, false, &v);
        CHECK(st == r.st_s && v == (st ? 0 : r.secs), "seconds of \"%s\": status %u value %lld, not %u / %lld", r.text, st, (long long)v, r.st_s, (long long)r.secs);
        v = 77;
        st = parse(r.text, true, &v);
        CHECK(st == r.st_ns && v == (st ? 0 : r.ns), "nanoseconds of \"%s\": status %u value %lld, not %u / %lld", r.text, st, (long long)v, r.st_ns, (long long)r.ns);
    }
}

static void mutations() {
    const std::string base = "2016-09-14T08:48:22+02:00";
    int64_t v;
    CHECK(parse(base, false, &v) == kTimeOk, "the base form does not parse");
    for (size_t p = 0; p < base.size(); p++) {
        const bool digit = base[p] >= '0' && base[p] <= '9';
        const char* wrong = digit ? "x/: -Z" : "x0/;tz ";
        for (const char* w = wrong; *w; w++) {
            if (*w == base[p]) continue;
            std::string s = base;
            s[p] = *w;
            const uint32_t st = parse(s, false, &v), sn = parse(s, true, &v);
            CHECK(st == kTimeSyntax && sn == kTimeSyntax, "\"%s\" (byte %zu wrong): status %u / %u, not a syntax error", s.c_str(), p, st, sn);
        }
    }
}

int main() {
    every_day();
    against_libc();
    table();
    mutations();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("test_timeparse: OK\n");
    return 0;
}
