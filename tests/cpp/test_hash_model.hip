// The hash of the Join hash table (csvplus_amd/csrc/hash_device.hpp) evaluated on the host: prints, for a table of inputs,
// what hash_one / hash_tag, the multi-word hash (seed, hash_step over the words most significant first, hash_finish),
// hash_home and hash_next_sector return.  tests/test_hash_model_cpp.py recomputes every line with the Python restatement in
// tests/hash_model.py — the model the GPU edge tests (tests/test_gpu_hash_edges.py) design their tables with.
// Host code only: no HIP call, runs on a machine without a GPU.  Line formats (all numbers decimal):
//   one   <code> <hash_one> <hash_tag>
//   multi <nwords> <w0> .. <w(n-1)> <hash>
//   home  <hash> <nsectors> <home>
//   next  <s> <nsectors> <slice_mask> <next>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../csvplus_amd/csrc/hash_device.hpp"

using namespace cph;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {   // splitmix64: inputs only, the Python side reads them from the lines
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t words_hash(const std::vector<uint64_t>& w) {
    uint64_t s = kHashSeed;
    for (uint64_t v : w) s = hash_step(s, v);
    return hash_finish(s);
}

int main() {
    static_assert(kHashSeed == 0x9E3779B97F4A7C15ull && kHashEmpty == ~0ull, "constants the model restates");
    std::vector<uint64_t> codes = {0ull, 1ull, 2ull, 35ull, 36ull, 0xFFFFFFFFull, 0x100000000ull, 0x7FFFFFFFFFFFFFFFull,
                                   0x8000000000000000ull, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull, 4738381338321616895ull /* 36^12 - 1 */};
    for (int i = 0; i < 400; i++) codes.push_back(rnd() >> (i % 64));
    std::vector<uint64_t> hashes;
    for (uint64_t c : codes) {
        const uint64_t h = hash_one(c);
        hashes.push_back(h);
        printf("one %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c, h, hash_tag(h));
        // one word through the multi-word route is hash_one
        if (words_hash({c}) != h) {
            fprintf(stderr, "hash_one differs from the one-word multi-word hash for %" PRIu64 "\n", c);
            return 1;
        }
    }
    for (int nw = 1; nw <= 9; nw++)
        for (int i = 0; i < 40; i++) {
            std::vector<uint64_t> w((size_t)nw);
            for (auto& v : w) v = i == 0 ? 0ull : i == 1 ? ~0ull : rnd() >> ((i * 7) % 64);
            printf("multi %d", nw);
            for (uint64_t v : w) printf(" %" PRIu64, v);
            const uint64_t h = words_hash(w);
            hashes.push_back(h);
            printf(" %" PRIu64 "\n", h);
        }
    hashes.push_back(0ull);
    hashes.push_back(~0ull);
    hashes.push_back(0xFFFFFFFF00000000ull);
    hashes.push_back(0x00000000FFFFFFFFull);
    hashes.push_back(0x8000000000000000ull);
    const uint32_t nsecs[] = {1u, 2u, 3u, 4u, 85u, 1023u, 1024u, 1025u, 2047u, 2048u, 2049u, 65536u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t ns : nsecs)
        for (uint64_t h : hashes) printf("home %" PRIu64 " %u %u\n", h, ns, hash_home(h, ns));
    // the sector after s: whole-table wrap (mask 0) and the wrap inside a slice of mask + 1 sectors
    const uint32_t masks[] = {0u, 1u, 3u, 1023u, 4095u};
    const uint32_t tables[] = {2u, 3u, 4u, 85u, 1024u, 1025u, 2048u, 3072u, 8192u, 0xFFFFFFFFu};
    for (uint32_t ns : tables)
        for (uint32_t mask : masks) {
            if (mask && (ns % (mask + 1u) != 0 || ns == 0xFFFFFFFFu)) continue;   // a sliced table is whole slices
            std::vector<uint32_t> ss = {0u, 1u, ns - 2u, ns - 1u, ns / 2u};
            if (mask) {
                ss.push_back(mask - 1u);
                ss.push_back(mask);                     // last sector of slice 0 -> sector 0
                if (ns >= 2u * (mask + 1u)) {
                    ss.push_back(mask + 1u);            // first sector of slice 1
                    ss.push_back(mask + 1u + mask);     // last sector of slice 1 -> mask + 1, not 2 * (mask + 1)
                    ss.push_back(mask + mask);
                }
            }
            for (uint32_t s : ss)
                if (s < ns) printf("next %u %u %u %u\n", s, ns, mask, hash_next_sector(s, ns, mask));
        }
    return 0;
}
