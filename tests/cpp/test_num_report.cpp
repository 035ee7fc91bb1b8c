// The error report's packing (csvplus_amd/csrc/num_report.hpp) on the host: err_pack / err_row / err_tag / err_kind round trip at
// the ends of every field, packed words order by (row, tag, kind), and err_unpack hands on what the device left.  CPU only.
#include <cstdio>
#include <vector>

#include "num_report.hpp"

using namespace cph;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                            \
        }                                                          \
    } while (0)

int main() {
    const uint64_t rows[] = {0ull, 1ull, (1ull << 32) - 1, 1ull << 32, (1ull << 48) - 1};
    const uint32_t bytes[] = {0u, 1u, 7u, 31u, 255u};
    struct Triple {
        uint64_t row;
        uint32_t tag, kind;
    };
    std::vector<Triple> all;   // in ascending (row, tag, kind) order
    for (uint64_t row : rows)
        for (uint32_t tag : bytes)
            for (uint32_t kind : bytes) all.push_back({row, tag, kind});
    for (const Triple& t : all) {
        const unsigned long long w = err_pack(t.row, t.tag, t.kind);
        CHECK(err_row(w) == t.row && err_tag(w) == t.tag && err_kind(w) == t.kind);
        CHECK((w == kErrNone) == (t.row == (1ull << 48) - 1 && t.tag == 255u && t.kind == 255u));   // the one word "no error" takes
        CHECK((uint32_t)(w & 0xFFFFu) == err_tag_kind(t.tag, t.kind));
    }
    for (size_t i = 0; i + 1 < all.size(); i++)
        CHECK(err_pack(all[i].row, all[i].tag, all[i].kind) < err_pack(all[i + 1].row, all[i + 1].tag, all[i + 1].kind));
    // the lowest row wins whatever its tag and kind; on one row the lowest tag; on one row and tag the lowest kind
    CHECK(err_pack(5, 255, 255) < err_pack(6, 0, 0));
    CHECK(err_pack(5, 3, 255) < err_pack(5, 4, 0));
    CHECK(err_pack(5, 3, 1) < err_pack(5, 3, 2));

    const ErrFirst none = err_unpack(ErrWord{0ull, kErrNone});
    CHECK(none.nerrors == 0 && none.row == UINT64_MAX && none.tag == 0 && none.kind == 0);
    const ErrFirst some = err_unpack(ErrWord{3ull, err_pack((1ull << 48) - 1, CPH_EXPR_MAX_OPS - 1, CPH_NUM_ERR_CONVERT)});
    CHECK(some.nerrors == 3 && some.row == (1ull << 48) - 1 && some.tag == CPH_EXPR_MAX_OPS - 1 && some.kind == CPH_NUM_ERR_CONVERT);

    std::printf("%zu triples\n", all.size());
    if (failures) {
        std::printf("test_num_report: %d FAILED\n", failures);
        return 1;
    }
    std::printf("test_num_report: OK\n");
    return 0;
}
