// The LazyQuotes separator automaton of csvplus_amd/csrc/csv_lazy_device.hpp — the code k_csv_lazy_tile_maps / k_csv_lazy_marks
// run per 16-byte chunk — compiled for the host (v_perm_b32 emulated).  Usage: test_csv_lazy <comma> <comment|0> <trim 0|1>,
// texts on stdin as one hex string per line; per text it prints the positions of the record separators found by
//   chunk maps (lz_walk16 from the identity) -> exclusive compose-scan over the chunks, packed and unpacked on the way
//   -> second walk from lz_constant(entry state) collecting the separator masks
// which tests/test_csv_lazy.py compares with the Python automaton.  It also checks, per text, that the scan's entry states equal a
// plain byte-by-byte walk with lz_next, and exits 1 if they ever differ.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "csv_lazy_device.hpp"

using namespace cph;

template <bool TRIM, bool CMT>
static bool run(const std::string& text, const LzTable& tb, std::vector<size_t>* seps) {
    const size_t nchunks = (text.size() + 15) / 16;
    std::vector<uint32_t> w(nchunks * 4 + 4, 0);
    for (size_t i = 0; i < text.size(); i++) w[i >> 2] |= (uint32_t)(uint8_t)text[i] << (8 * (i & 3));
    std::vector<uint32_t> packed(nchunks);
    for (size_t c = 0; c < nchunks; c++) {
        const uint32_t (&cw)[4] = *reinterpret_cast<const uint32_t (*)[4]>(&w[4 * c]);
        packed[c] = lz_pack(lz_walk16<TRIM, CMT, false>(cw, tb, lz_identity(), nullptr));
    }
    // the byte-by-byte walk
    std::vector<uint32_t> plain(text.size() + 1);
    uint32_t s = kLzRS;
    for (size_t i = 0; i < text.size(); i++) {
        plain[i] = s;
        const uint32_t c = (uint8_t)text[i];
        int cls = kLzOther;
        if (TRIM && (c == ' ' || (c >= 9 && c <= 13))) cls = kLzSpace;
        if (CMT && c == tb.comment) cls = kLzComment;
        if (c == '\r') cls = kLzCR;
        if (c == tb.comma) cls = kLzComma;
        if (c == '"') cls = kLzQuote;
        if (c == '\n') cls = kLzNewline;
        s = lz_next(s, cls, TRIM);
    }
    bool ok = true;
    LzMap before = lz_identity();
    for (size_t c = 0; c < nchunks; c++) {
        const uint32_t entry = lz_apply(before, kLzRS);
        ok &= entry == plain[16 * c];
        const uint32_t (&cw)[4] = *reinterpret_cast<const uint32_t (*)[4]>(&w[4 * c]);
        uint32_t mk = 0;
        lz_walk16<TRIM, CMT, true>(cw, tb, lz_constant(entry), &mk);
        for (int b = 0; b < 16; b++)
            if ((mk >> b) & 1u) seps->push_back(16 * c + b);
        before = lz_compose(before, lz_unpack(packed[c]));
    }
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int comma = atoi(argv[1]), comment = atoi(argv[2]), trim = atoi(argv[3]);
    const LzTable tb = lz_table((uint8_t)comma, (uint8_t)comment, trim != 0);
    std::string line;
    bool ok = true;
    while (std::getline(std::cin, line)) {
        std::string text;
        for (size_t i = 0; i + 1 < line.size(); i += 2) text.push_back((char)strtol(line.substr(i, 2).c_str(), nullptr, 16));
        std::vector<size_t> seps;
        if (trim) ok &= comment ? run<true, true>(text, tb, &seps) : run<true, false>(text, tb, &seps);
        else ok &= comment ? run<false, true>(text, tb, &seps) : run<false, false>(text, tb, &seps);
        for (size_t i = 0; i < seps.size(); i++) printf(i ? ",%zu" : "%zu", seps[i]);
        printf("\n");
    }
    return ok ? 0 : 1;
}
