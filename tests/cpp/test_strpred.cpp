// test_strpred.cpp — csrc/strpred_device.hpp compiled for the host (CPU only): strings.Compare / HasPrefix / HasSuffix /
// Contains as k_pred_eval runs them, against std::string's operations, and the span of a Map slice against hand-written cases.
//
// Values and literals of every length 0..26, the value at every start alignment 0..7, bytes from {a, b, c, 0x00, 0xFF}; the
// literal is random, a piece of the value, or such a piece with one byte changed, so that matches, near-matches and ties
// are dense.  The value functor restates load_value_chunk (device_utils.hpp): it touches whole aligned 8-byte words.  The
// column buffer is sized exactly (alignment + value), a byte of a touched word that lies outside the VALUE reads as noise,
// and a touched word that holds NO byte of the value — what the device must never load — aborts the test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "strpred_device.hpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

long failures = 0, checks = 0;

struct HostValue {
    const std::vector<uint8_t>& buf;   // the column: `begin` bytes in front of the value, then the value, then nothing
    uint64_t begin, vlen;
    uint8_t byte_at(uint64_t addr) const {   // inside the value: the byte; elsewhere in a touched word: noise
        if (addr >= begin && addr < begin + vlen) return buf[(size_t)addr];
        return (uint8_t)rnd();
    }
    uint64_t word_at(uint64_t waddr) const {   // the aligned word at waddr: it must hold a byte of the value
        if (!(waddr < begin + vlen && waddr + 8 > begin) || vlen == 0) {
            std::fprintf(stderr, "load outside the value's rounded span: word %llu, value [%llu, %llu)\n", (unsigned long long)waddr,
                         (unsigned long long)begin, (unsigned long long)(begin + vlen));
            std::abort();
        }
        uint64_t w = 0;
        for (int k = 0; k < 8; k++) w |= (uint64_t)byte_at(waddr + (uint64_t)k) << (8 * k);
        return w;
    }
    // load_value_chunk(data, begin + off, len, j)
    uint64_t operator()(uint64_t off, uint64_t len, int j) const {
        if (off + len > vlen || 8ull * (uint64_t)j >= len) {
            std::fprintf(stderr, "span (%llu, %llu) chunk %d leaves a value of %llu bytes\n", (unsigned long long)off, (unsigned long long)len, j,
                         (unsigned long long)vlen);
            std::abort();
        }
        const uint64_t a = begin + off + 8ull * (uint64_t)j;
        const uint64_t last = begin + off + (len < 8ull * (uint64_t)(j + 1) ? len : 8ull * (uint64_t)(j + 1)) - 1;
        const int sh = (int)(a & 7ull) * 8;
        uint64_t v = word_at(a & ~7ull) >> sh;
        if (sh != 0 && (last & ~7ull) != (a & ~7ull)) v |= word_at((a & ~7ull) + 8) << (64 - sh);
        return v;
    }
};

struct HostLiteral {
    std::vector<uint64_t> words;   // zero padded to whole words, as build_pred_prog packs it
    explicit HostLiteral(const std::string& s) : words((s.size() + 7) / 8 + 1, 0) {
        for (size_t i = 0; i < s.size(); i++) words[i / 8] |= (uint64_t)(uint8_t)s[i] << (8 * (i % 8));
    }
    uint64_t operator()(uint64_t j) const { return words.at((size_t)j); }
};

const char kAlphabet[5] = {'a', 'b', 'c', '\0', '\xFF'};

std::string random_string(size_t n) {
    std::string s(n, 'a');
    for (auto& c : s) c = kAlphabet[rnd() % 5];
    return s;
}

int sign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

void expect(bool ok, const char* what, const std::string& v, const std::string& l, int align) {
    checks++;
    if (ok) return;
    if (++failures <= 10) {
        std::fprintf(stderr, "%s wrong: align %d, value [", what, align);
        for (unsigned char c : v) std::fprintf(stderr, "%02x", c);
        std::fprintf(stderr, "] literal [");
        for (unsigned char c : l) std::fprintf(stderr, "%02x", c);
        std::fprintf(stderr, "]\n");
    }
}

void check_pair(const std::string& v, const std::string& l, int align) {
    std::vector<uint8_t> buf((size_t)align + v.size());   // exactly: nothing behind the value
    for (int k = 0; k < align; k++) buf[(size_t)k] = (uint8_t)kAlphabet[rnd() % 5];
    for (size_t i = 0; i < v.size(); i++) buf[(size_t)align + i] = (uint8_t)v[i];
    const HostValue hv{buf, (uint64_t)align, (uint64_t)v.size()};
    const HostLiteral hl(l);
    expect(cph::str_compare(hv, v.size(), hl, l.size()) == sign(v.compare(l)), "compare", v, l, align);
    expect(cph::str_has_prefix(hv, v.size(), hl, l.size()) == (l.size() <= v.size() && v.compare(0, l.size(), l) == 0), "prefix", v, l, align);
    expect(cph::str_has_suffix(hv, v.size(), hl, l.size()) == (l.size() <= v.size() && v.compare(v.size() - l.size(), l.size(), l) == 0), "suffix",
           v, l, align);
    expect(cph::str_contains(hv, v.size(), hl, l.size()) == (v.find(l) != std::string::npos), "contains", v, l, align);
}

void check_slice(uint64_t len, int64_t from, int64_t to, uint64_t want_off, uint64_t want_n) {
    uint64_t off = ~0ull, n = ~0ull;
    cph::slice_span(len, from, to, &off, &n);
    checks++;
    if ((n != want_n || (n && off != want_off)) && ++failures <= 10)
        std::fprintf(stderr, "slice_span(%llu, %lld, %lld) = (%llu, %llu), want (%llu, %llu)\n", (unsigned long long)len, (long long)from,
                     (long long)to, (unsigned long long)off, (unsigned long long)n, (unsigned long long)want_off, (unsigned long long)want_n);
}

}  // namespace

int main() {
    long outcomes[4][2] = {};
    for (int vlen = 0; vlen <= 26; vlen++)
        for (int llen = 0; llen <= 26; llen++)
            for (int align = 0; align < 8; align++)
                for (int trial = 0; trial < 12; trial++) {
                    const std::string v = random_string((size_t)vlen);
                    std::string l;
                    const int how = trial % 4;
                    if (how == 0 || llen > vlen) {
                        l = random_string((size_t)llen);
                        if (how != 0 && vlen) l.replace(0, (size_t)vlen, v);   // the value and more: a tie on the common prefix
                    } else {   // a piece of the value: its head, its tail, or anywhere
                        const size_t at = how == 1 ? 0 : how == 2 ? (size_t)(vlen - llen) : (size_t)(rnd() % (uint64_t)(vlen - llen + 1));
                        l = v.substr(at, (size_t)llen);
                        if (llen && trial >= 8) l[(size_t)(rnd() % (uint64_t)llen)] = kAlphabet[rnd() % 5];   // ... with one byte changed
                    }
                    check_pair(v, l, align);
                    outcomes[0][v.compare(l) < 0]++;
                    outcomes[1][l.size() <= v.size() && v.compare(0, l.size(), l) == 0]++;
                    outcomes[2][l.size() <= v.size() && v.compare(v.size() - l.size(), l.size(), l) == 0]++;
                    outcomes[3][v.find(l) != std::string::npos]++;
                }
    // the adversarial search: the literal's first byte everywhere, the mismatch at its end
    for (int align = 0; align < 8; align++) {
        check_pair(std::string(25, 'a'), std::string(8, 'a') + "b", align);
        check_pair(std::string(24, 'a') + "b", std::string(8, 'a') + "b", align);
        check_pair(std::string(26, '\xFF'), std::string(25, '\xFF') + std::string(1, '\0'), align);
    }
    for (int k = 0; k < 4; k++)
        if (outcomes[k][0] < 1000 || outcomes[k][1] < 1000) {
            std::fprintf(stderr, "op %d: outcomes %ld / %ld are not both dense\n", k, outcomes[k][0], outcomes[k][1]);
            failures++;
        }

    const int64_t kMax = INT64_MAX, kMin = INT64_MIN;
    check_slice(25, 0, 10, 0, 10);
    check_slice(25, 0, kMax, 0, 25);
    check_slice(25, -6, kMax, 19, 6);
    check_slice(25, 11, 19, 11, 8);
    check_slice(25, 20, 30, 20, 5);
    check_slice(25, 30, 40, 25, 0);
    check_slice(25, 10, 10, 0, 0);
    check_slice(25, 12, 3, 0, 0);
    check_slice(25, -100, 3, 0, 3);
    check_slice(25, -3, -1, 22, 2);
    check_slice(25, -1, -3, 0, 0);
    check_slice(25, kMin, kMax, 0, 25);
    check_slice(25, kMin, kMin, 0, 0);
    check_slice(25, kMax, kMax, 0, 0);
    check_slice(0, 0, kMax, 0, 0);
    check_slice(0, -1, 1, 0, 0);
    check_slice(1, -1, kMax, 0, 1);

    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
