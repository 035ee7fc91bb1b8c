// test_span.cpp — csrc/span_device.hpp compiled for the host (CPU only): the operations of a CPH_MAP_SPAN piece as the Map
// kernels run them, against a naive per-byte reference written here from Go's own definitions: utf8.DecodeRune /
// DecodeLastRune and unicode.IsSpace for TrimSpace (strings.TrimLeftFunc / TrimRightFunc, with lastIndexFunc's forward
// re-decode), a byte loop for the cutset trims, std::string::find for Split / SplitN.
//
//   * every byte string of length <= 6 over {20, 61, 2C, C2, 85, E2, 80}, the start alignment rotating through 0..7;
//   * value lengths 0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65 at every begin offset mod 8, padded front and back with
//     0..3 spaces drawn from all 25 sequences;
//   * separators of 1, 2, 8 and 9 bytes put at EVERY position of such values, so that matches straddle every chunk edge and
//     one ends at the value's very end;
//   * programs of four operations through span_run.
// The value functor restates load_value_chunk (device_utils.hpp) over a buffer of exactly alignment + value bytes: a byte of a
// touched word outside the VALUE reads as noise, and a touched word that holds no byte of the requested span — what the
// device must never load — aborts the test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "span_device.hpp"

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
    uint8_t byte_at(uint64_t addr) const {
        if (addr >= begin && addr < begin + vlen) return buf.at((size_t)addr);
        return (uint8_t)rnd();
    }
    uint64_t word_at(uint64_t waddr, uint64_t s0, uint64_t s1) const {   // the aligned word at waddr: it must hold a byte of the span [s0, s1)
        if (!(waddr < s1 && waddr + 8 > s0)) {
            std::fprintf(stderr, "load outside the span's rounded words: word %llu, span [%llu, %llu)\n", (unsigned long long)waddr,
                         (unsigned long long)s0, (unsigned long long)s1);
            std::abort();
        }
        uint64_t w = 0;
        for (int k = 0; k < 8; k++) w |= (uint64_t)byte_at(waddr + (uint64_t)k) << (8 * k);
        return w;
    }
    // load_value_chunk(data, begin + off, len, j)
    uint64_t operator()(uint64_t off, uint64_t len, int j) const {
        if (len == 0 || off + len > vlen || 8ull * (uint64_t)j >= len) {
            std::fprintf(stderr, "span (%llu, %llu) chunk %d leaves a value of %llu bytes\n", (unsigned long long)off, (unsigned long long)len, j,
                         (unsigned long long)vlen);
            std::abort();
        }
        const uint64_t a = begin + off + 8ull * (uint64_t)j;
        const uint64_t last = begin + off + (len < 8ull * (uint64_t)(j + 1) ? len : 8ull * (uint64_t)(j + 1)) - 1;
        const int sh = (int)(a & 7ull) * 8;
        uint64_t v = word_at(a & ~7ull, begin + off, begin + off + len) >> sh;
        if (sh != 0 && (last & ~7ull) != (a & ~7ull)) v |= word_at((a & ~7ull) + 8, begin + off, begin + off + len) << (64 - sh);
        return v;
    }
};

struct HostLit {   // a literal of exactly its bytes: a word past them reads as noise
    const std::string* s;
    uint64_t operator()(uint64_t j) const {
        if (8 * j >= s->size()) {
            std::fprintf(stderr, "word %llu of a literal of %zu bytes\n", (unsigned long long)j, s->size());
            std::abort();
        }
        uint64_t w = 0;
        for (size_t k = 0; k < 8; k++) {
            const size_t i = (size_t)j * 8 + k;
            w |= (uint64_t)(i < s->size() ? (uint8_t)(*s)[i] : (uint8_t)rnd()) << (8 * k);
        }
        return w;
    }
};
struct HostLits {   // the literal block: literal q "starts at offset q"
    const std::vector<std::string>& lits;
    HostLit operator()(uint32_t off, uint32_t len) const {
        if (lits.at(off).size() != len) std::abort();
        return HostLit{&lits.at(off)};
    }
};

// ---- the reference: Go's definitions, a byte at a time -----------------------------------------------------------------------

constexpr uint32_t kRuneError = 0xFFFD;

// utf8.DecodeRune(p[i:end]): (rune, size); an invalid or short encoding is (RuneError, 1)
void decode_rune(const std::string& p, size_t i, size_t end, uint32_t* r, size_t* size) {
    *r = kRuneError, *size = 1;
    if (i >= end) {
        *size = 0;
        return;
    }
    const uint8_t b0 = (uint8_t)p[i];
    if (b0 < 0x80) {
        *r = b0;
        return;
    }
    size_t need;
    uint8_t lo = 0x80, hi = 0xBF;
    if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
    else if (b0 >= 0xE0 && b0 <= 0xEF) need = 3, lo = b0 == 0xE0 ? 0xA0 : 0x80, hi = b0 == 0xED ? 0x9F : 0xBF;
    else if (b0 >= 0xF0 && b0 <= 0xF4) need = 4, lo = b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xF4 ? 0x8F : 0xBF;
    else return;
    if (end - i < need) return;
    uint32_t v = need == 2 ? b0 & 0x1Fu : need == 3 ? b0 & 0x0Fu : b0 & 0x07u;
    for (size_t k = 1; k < need; k++) {
        const uint8_t c = (uint8_t)p[i + k];
        if (c < (k == 1 ? lo : 0x80) || c > (k == 1 ? hi : 0xBF)) return;
        v = (v << 6) | (c & 0x3Fu);
    }
    *r = v, *size = need;
}

// utf8.DecodeLastRune(p[:end])
void decode_last_rune(const std::string& p, size_t end, uint32_t* r, size_t* size) {
    *r = kRuneError, *size = 0;
    if (end == 0) return;
    size_t start = end - 1;
    if ((uint8_t)p[start] < 0x80) {
        *r = (uint8_t)p[start], *size = 1;
        return;
    }
    // Go: lim := max(end - UTFMax, 0); for start--; start >= lim; start-- { if RuneStart(p[start]) { break } }; if start < lim { start = lim }
    const long lim = end >= 4 ? (long)end - 4 : 0;
    long st = (long)start;
    for (st--; st >= lim; st--)
        if (((uint8_t)p[(size_t)st] & 0xC0) != 0x80) break;
    if (st < lim) st = lim;
    decode_rune(p, (size_t)st, end, r, size);
    if ((size_t)st + *size != end) *r = kRuneError, *size = 1;
}

bool is_space(uint32_t r) {
    return (r >= 9 && r <= 13) || r == 0x20 || r == 0x85 || r == 0xA0 || r == 0x1680 || (r >= 0x2000 && r <= 0x200A) || r == 0x2028 || r == 0x2029 ||
           r == 0x202F || r == 0x205F || r == 0x3000;
}

struct Span {
    size_t off, len;
};

Span ref_trim_space(const std::string& s, Span sp, int mode) {
    const std::string v = s.substr(sp.off, sp.len);
    size_t a = 0, e = v.size();
    if (mode & 1)
        while (a < e) {
            uint32_t r;
            size_t n;
            decode_rune(v, a, e, &r, &n);
            if (!is_space(r)) break;
            a += n;
        }
    if (mode & 2) {   // strings.TrimRightFunc over v[a:]
        const std::string t = v.substr(a);
        size_t i = t.size();
        bool found = false;
        while (i > 0) {   // lastIndexFunc(t, IsSpace, false)
            uint32_t r;
            size_t n;
            decode_last_rune(t, i, &r, &n);
            i -= n;
            if (!is_space(r)) {
                found = true;
                break;
            }
        }
        size_t keep = 0;
        if (found) {
            if ((uint8_t)t[i] >= 0x80) {
                uint32_t r;
                size_t n;
                decode_rune(t, i, t.size(), &r, &n);
                keep = i + n;
            } else {
                keep = i + 1;
            }
        }
        e = a + keep;
    }
    return Span{sp.off + a, e - a};
}

Span ref_trim_set(const std::string& s, Span sp, const std::string& set, int mode) {
    size_t a = sp.off, e = sp.off + sp.len;
    if (mode & 1)
        while (a < e && set.find(s[a]) != std::string::npos) a++;
    if (mode & 2)
        while (e > a && set.find(s[e - 1]) != std::string::npos) e--;
    return Span{a, e - a};
}

Span ref_affix(const std::string& s, Span sp, const std::string& lit, bool suffix) {
    if (lit.size() > sp.len) return sp;
    if (!suffix && s.compare(sp.off, lit.size(), lit) == 0) return Span{sp.off + lit.size(), sp.len - lit.size()};
    if (suffix && s.compare(sp.off + sp.len - lit.size(), lit.size(), lit) == 0) return Span{sp.off, sp.len - lit.size()};
    return sp;
}

Span ref_field(const std::string& s, Span sp, const std::string& sep, int64_t k, int32_t limit) {
    const std::string v = s.substr(sp.off, sp.len);
    std::vector<Span> parts;   // strings.SplitN(v, sep, limit)
    size_t at = 0;
    while (limit < 0 || (int64_t)parts.size() < (int64_t)limit - 1) {
        const size_t m = v.find(sep, at);
        if (m == std::string::npos) break;
        parts.push_back(Span{at, m - at});
        at = m + sep.size();
    }
    parts.push_back(Span{at, v.size() - at});
    const int64_t n = (int64_t)parts.size();
    const int64_t idx = k < 0 ? n + k : k;
    if (idx < 0 || idx >= n) return Span{sp.off, 0};
    return Span{sp.off + parts[(size_t)idx].off, parts[(size_t)idx].len};
}

Span ref_slice(Span sp, int64_t from, int64_t to) {
    const int64_t l = (int64_t)sp.len;
    const int64_t f = from < 0 ? (from + l < 0 ? 0 : from + l) : (from < l ? from : l);
    const int64_t t = to < 0 ? (to + l < 0 ? 0 : to + l) : (to < l ? to : l);
    return t > f ? Span{sp.off + (size_t)f, (size_t)(t - f)} : Span{sp.off, 0};
}

// ---- one program on one value, both ways -------------------------------------------------------------------------------------

struct TestOp {
    int32_t op, mode;
    int64_t a, b;
    std::string lit;
};

void check_program(const std::string& v, int align, const std::vector<TestOp>& prog, const char* what) {
    std::vector<uint8_t> buf((size_t)align + v.size());   // exactly: nothing behind the value
    for (int k = 0; k < align; k++) buf[(size_t)k] = (uint8_t)rnd();
    for (size_t i = 0; i < v.size(); i++) buf[(size_t)align + i] = (uint8_t)v[i];
    const HostValue hv{buf, (uint64_t)align, (uint64_t)v.size()};
    std::vector<std::string> lits;
    std::vector<cph::SpanOp> ops;
    Span want{0, v.size()};
    for (const TestOp& t : prog) {
        cph::SpanOp o{};
        o.op = t.op, o.mode = t.mode;
        if (t.op == cph::kSpanTrimSpace) {
            want = ref_trim_space(v, want, t.mode);
        } else if (t.op == cph::kSpanTrimCutset) {
            uint64_t lo = 0, hi = 0;
            for (unsigned char c : t.lit) (c < 64 ? lo : hi) |= 1ull << (c & 63);
            o.a = (int64_t)lo, o.b = (int64_t)hi;
            want = ref_trim_set(v, want, t.lit, t.mode);
        } else if (t.op == cph::kSpanSlice) {
            o.a = t.a, o.b = t.b;
            want = ref_slice(want, t.a, t.b);
        } else {
            o.a = t.a;
            o.lit_off = (uint32_t)lits.size(), o.lit_len = (uint32_t)t.lit.size();
            lits.push_back(t.lit);
            want = t.op == cph::kSpanField ? ref_field(v, want, t.lit, t.a, t.mode) : ref_affix(v, want, t.lit, t.op == cph::kSpanTrimSuffix);
        }
        ops.push_back(o);
    }
    const HostLits lb{lits};
    uint64_t off = ~0ull, len = ~0ull;
    cph::span_run(ops.data(), (int)ops.size(), hv, v.size(), lb, &off, &len);
    checks++;
    const bool ok = len == want.len && (len == 0 || off == want.off) && off + len <= v.size();
    if (!ok && ++failures <= 12) {
        std::fprintf(stderr, "%s wrong: align %d, value [", what, align);
        for (unsigned char c : v) std::fprintf(stderr, "%02x", c);
        std::fprintf(stderr, "] ops");
        for (const TestOp& t : prog) std::fprintf(stderr, " (%d mode %d a %lld lit %zu bytes)", t.op, t.mode, (long long)t.a, t.lit.size());
        std::fprintf(stderr, ": got (%llu, %llu), want (%zu, %zu)\n", (unsigned long long)off, (unsigned long long)len, want.off, want.len);
    }
}

const char* const kSpaces[25] = {"\t", "\n", "\v", "\f", "\r", " ", "\xC2\x85", "\xC2\xA0", "\xE1\x9A\x80", "\xE2\x80\x80", "\xE2\x80\x81",
                                 "\xE2\x80\x82", "\xE2\x80\x83", "\xE2\x80\x84", "\xE2\x80\x85", "\xE2\x80\x86", "\xE2\x80\x87", "\xE2\x80\x88",
                                 "\xE2\x80\x89", "\xE2\x80\x8A", "\xE2\x80\xA8", "\xE2\x80\xA9", "\xE2\x80\xAF", "\xE2\x81\x9F", "\xE3\x80\x80"};

// what every value goes through: each operation and mode alone
void check_all_ops(const std::string& v, int align) {
    using namespace cph;
    for (int mode = 1; mode <= 3; mode++) {
        check_program(v, align, {{kSpanTrimSpace, mode, 0, 0, ""}}, "trim_space");
        check_program(v, align, {{kSpanTrimCutset, mode, 0, 0, " ,"}}, "trim_cutset");
        check_program(v, align, {{kSpanTrimCutset, mode, 0, 0, "a\x7F"}}, "trim_cutset");
    }
    check_program(v, align, {{kSpanTrimCutset, 3, 0, 0, ""}}, "empty cutset");
    for (const char* lit : {"", " ", "a,", "\xE2\x80", "\xC2\x85 a", "aaaaaaaa", "a,a,a,a,a"}) {
        check_program(v, align, {{kSpanTrimPrefix, 0, 0, 0, lit}}, "trim_prefix");
        check_program(v, align, {{kSpanTrimSuffix, 0, 0, 0, lit}}, "trim_suffix");
    }
    check_program(v, align, {{kSpanTrimPrefix, 0, 0, 0, v}}, "trim_prefix of itself");
    for (const char* sep : {",", "a,", "\x80"})
        for (int limit : {-1, 1, 2, 3, 4})
            for (int k = -4; k <= 4; k++) check_program(v, align, {{kSpanField, limit, k, 0, sep}}, "field");
}

std::string filler(size_t n, const char* alphabet, size_t na) {
    std::string s(n, 'x');
    for (auto& c : s) c = alphabet[rnd() % na];
    return s;
}

}  // namespace

int main() {
    using namespace cph;
    // 1. every byte string of length <= 6 over the alphabet that holds pieces of the space sequences
    const unsigned char kAlpha[7] = {0x20, 0x61, 0x2C, 0xC2, 0x85, 0xE2, 0x80};
    long count = 0;
    for (int len = 0; len <= 6; len++) {
        long total = 1;
        for (int k = 0; k < len; k++) total *= 7;
        for (long code = 0; code < total; code++, count++) {
            std::string v((size_t)len, ' ');
            long c = code;
            for (int k = 0; k < len; k++, c /= 7) v[(size_t)k] = (char)kAlpha[c % 7];
            const int align = (int)(count & 7);
            for (int mode = 1; mode <= 3; mode++) check_program(v, align, {{kSpanTrimSpace, mode, 0, 0, ""}}, "trim_space (exhaustive)");
            check_program(v, align, {{kSpanTrimCutset, 3, 0, 0, " ,"}}, "trim_cutset (exhaustive)");
            for (int k = -3; k <= 3; k++) {
                check_program(v, align, {{kSpanField, -1, k, 0, ","}}, "field (exhaustive)");
                check_program(v, align, {{kSpanField, 2, k, 0, "\x80\x80"}}, "field (exhaustive)");
            }
            check_program(v, align, {{kSpanTrimPrefix, 0, 0, 0, "\xE2\x80"}, {kSpanTrimSuffix, 0, 0, 0, "\x80"}}, "affixes (exhaustive)");
        }
    }
    // the tail cases by name
    for (int align = 0; align < 8; align++) {
        check_program("\xE2\x80\x80\x80", align, {{kSpanTrimSpace, 2, 0, 0, ""}}, "E2 80 80 80");
        check_program("\xE2\xC2\x85", align, {{kSpanTrimSpace, 2, 0, 0, ""}}, "E2 C2 85");
        check_program("a\x85", align, {{kSpanTrimSpace, 3, 0, 0, ""}}, "a lone 85");
        check_program("a\x80", align, {{kSpanTrimSpace, 3, 0, 0, ""}}, "a lone 80");
    }

    // 2. the lengths around the chunk edges at every alignment, padded with spaces of all 25 kinds
    const int kLens[13] = {0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65};
    const char kCore[8] = {'a', ',', ' ', 'a', ',', 'a', '\x80', '\xE2'};
    for (int len : kLens)
        for (int align = 0; align < 8; align++)
            for (int trial = 0; trial < 16; trial++) {
                std::string v;
                for (uint64_t k = rnd() % 4; k > 0; k--) v += kSpaces[rnd() % 25];
                v += filler((size_t)len, kCore, trial % 2 ? 8 : 2);
                for (uint64_t k = rnd() % 4; k > 0; k--) v += kSpaces[rnd() % 25];
                check_all_ops(v, align);
                check_program(v, align,
                              {{kSpanTrimSpace, 3, 0, 0, ""}, {kSpanTrimPrefix, 0, 0, 0, "a,"}, {kSpanField, -1, -1, 0, ","}, {kSpanSlice, 0, 0, 8, ""}},
                              "a program of four");
                check_program(v, align, {{kSpanField, 2, 1, 0, ","}, {kSpanTrimCutset, 3, 0, 0, "a "}, {kSpanSlice, 0, -5, INT64_MAX, ""}, {kSpanTrimSpace, 1, 0, 0, ""}},
                              "a program of four");
                // a value that is all spaces, of exactly len bytes or a little more
                std::string sp;
                while (sp.size() < (size_t)len) sp += kSpaces[rnd() % 25];
                for (int mode = 1; mode <= 3; mode++) check_program(sp, align, {{kSpanTrimSpace, mode, 0, 0, ""}}, "all spaces");
            }

    // 3. separators of 1, 2, 8 and 9 bytes at every position: a match across every chunk edge, one at the very end
    const std::string kSeps[4] = {"|", "|-", "|1234567", "|12345678"};
    for (int len : kLens)
        for (const std::string& sep : kSeps)
            for (int align = 0; align < 8; align++)
                for (size_t at = 0; at + sep.size() <= (size_t)len; at++) {
                    std::string v = filler((size_t)len, "ab|1", (at + (size_t)align) % 3 ? 2 : 4);   // with and without near-matches
                    v.replace(at, sep.size(), sep);
                    if (at % 2 && at >= sep.size()) v.replace(at - sep.size(), sep.size(), sep);   // two in a row
                    for (int k = -3; k <= 3; k++)
                        for (int limit : {-1, 2}) check_program(v, align, {{kSpanField, limit, k, 0, sep}}, "field (separator placed)");
                    check_program(v, align, {{kSpanTrimSuffix, 0, 0, 0, sep}}, "trim_suffix (separator placed)");
                    check_program(v, align, {{kSpanTrimPrefix, 0, 0, 0, sep}}, "trim_prefix (separator placed)");
                }
    // Go's own examples
    check_program("aaa", 3, {{kSpanField, -1, 1, 0, "aa"}}, "aaa split on aa");
    check_program("", 5, {{kSpanField, -1, 0, 0, "x"}}, "the empty value");
    check_program("a man a plan a canal panama", 1, {{kSpanField, -1, 3, 0, "a "}}, "a man a plan");

    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
