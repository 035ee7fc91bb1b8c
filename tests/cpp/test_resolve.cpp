// test_resolve.cpp — Index::ResolveDuplicates with NAMED resolvers through the C++ facade (csvplus_amd/host/csvplus.hpp,
// cph_index_resolve), in the shape of the reference's TestResolver (csvplus_test.go:695-752): every named resolver must leave
// the rows the callback overload leaves for the callback that states the same rule.  Run by tests/test_resolve_cpp.py under
// `-m gpu`.
#include <cstdio>
#include <random>

#include "csvplus.hpp"

using namespace csvplus;

static int g_failed = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            g_failed++;                                                                \
            return;                                                                    \
        }                                                                              \
    } while (0)

static std::vector<Row> peopleRows;

static void makeFixtures() {
    static const char* names[] = {"Amelia", "Ava", "Emily", "Isla", "Jack", "Mia", "Noah", "Oliver", "Olivia", "William"};
    static const char* surnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies", "Evans", "Wilson"};
    int id = 0;
    for (const char* n : names)
        for (const char* s : surnames) peopleRows.push_back(Row{{"id", std::to_string(id++)}, {"name", n}, {"surname", s}});
}

// one duplicated person, n extra copies with fresh ids scattered over the table (TestResolver's shape)
static std::vector<Row> withDuplicates(std::mt19937_64& rng, int n, Row* dup) {
    std::vector<Row> src = peopleRows;
    *dup = src[rng() % src.size()];
    for (int j = 0; j < n; j++) {
        Row copy = *dup;
        copy["id"] = std::to_string(1000 + (int)(rng() % 9000));
        const size_t k = rng() % src.size();
        src.push_back(copy);
        std::swap(src[k], src.back());
    }
    return src;
}

static std::vector<Row> viaCallback(const std::vector<Row>& src, const Index::ResolveFunc& fn, Error* err) {
    auto [index, e] = TakeRows(src).IndexOn({"name", "surname"});
    if (e) {
        *err = e;
        return {};
    }
    *err = index->ResolveDuplicates(fn);
    return index->rows();
}
static std::vector<Row> viaNamed(const std::vector<Row>& src, const Resolver& rs, Error* err) {
    auto [index, e] = TakeRows(src).IndexOn({"name", "surname"});
    if (e) {
        *err = e;
        return {};
    }
    *err = index->ResolveDuplicates(rs);
    return index->rows();
}

static void TestNamedResolvers() {   // csvplus_test.go:695-752
    std::mt19937_64 rng(695);
    for (int i = 0; i < 12; i++) {
        Row dup;
        const std::vector<Row> src = withDuplicates(rng, (int)(rng() % 100) + 1, &dup);
        Error e1, e2;
        // KeepFirst() == the reference's resolver returning rows[0]
        auto want = viaCallback(src, [](const std::vector<Row>& rows) -> std::pair<Row, Error> { return {rows[0], Error()}; }, &e1);
        auto got = viaNamed(src, KeepFirst(), &e2);
        CHECK(!e1 && !e2 && got == want && got.size() >= peopleRows.size() - 1);
        // KeepLast()
        want = viaCallback(src, [](const std::vector<Row>& rows) -> std::pair<Row, Error> { return {rows.back(), Error()}; }, &e1);
        got = viaNamed(src, KeepLast(), &e2);
        CHECK(!e1 && !e2 && got == want);
        // KeepMaxInt("id") == a max-by-id callback (ties: the first)
        auto maxById = [](const std::vector<Row>& rows) -> std::pair<Row, Error> {
            size_t best = 0;
            for (size_t k = 1; k < rows.size(); k++)
                if (std::stoll(rows[k].at("id")) > std::stoll(rows[best].at("id"))) best = k;
            return {rows[best], Error()};
        };
        want = viaCallback(src, maxById, &e1);
        got = viaNamed(src, KeepMaxInt("id"), &e2);
        CHECK(!e1 && !e2 && got == want);
        got = viaNamed(src, KeepMaxFloat("id"), &e2);
        CHECK(!e2 && got == want);
        auto minById = [](const std::vector<Row>& rows) -> std::pair<Row, Error> {
            size_t best = 0;
            for (size_t k = 1; k < rows.size(); k++)
                if (std::stoll(rows[k].at("id")) < std::stoll(rows[best].at("id"))) best = k;
            return {rows[best], Error()};
        };
        want = viaCallback(src, minById, &e1);
        got = viaNamed(src, KeepMinInt("id"), &e2);
        CHECK(!e1 && !e2 && got == want);
        // KeepMax("id"): the ids as STRINGS ("999" > "1000")
        auto maxStr = [](const std::vector<Row>& rows) -> std::pair<Row, Error> {
            size_t best = 0;
            for (size_t k = 1; k < rows.size(); k++)
                if (rows[k].at("id") > rows[best].at("id")) best = k;
            return {rows[best], Error()};
        };
        want = viaCallback(src, maxStr, &e1);
        got = viaNamed(src, KeepMax("id"), &e2);
        CHECK(!e1 && !e2 && got == want);
        // DropDuplicates() == the empty-row callback
        want = viaCallback(src, [](const std::vector<Row>&) -> std::pair<Row, Error> { return {Row{}, Error()}; }, &e1);
        got = viaNamed(src, DropDuplicates(), &e2);
        CHECK(!e1 && !e2 && got == want && got.size() <= peopleRows.size() - 1);
    }
    // no duplicates: untouched; and the deduplicated index keeps working as a join target
    Error e;
    CHECK(viaNamed(peopleRows, KeepMaxInt("id"), &e).size() == peopleRows.size() && !e);
    Row dup;
    const std::vector<Row> src = withDuplicates(rng, 5, &dup);
    auto [index, err] = TakeRows(src).IndexOn({"name", "surname"});
    CHECK(!err && !index->ResolveDuplicates(KeepFirst()));
    size_t hits = 0;
    CHECK(!TakeRows(peopleRows).Join(index)([&](Row) { hits++; return Error(); }));
    CHECK(hits == index->rows().size());
}

static void TestTailRule() {   // csvplus.go:851-859, hand-derived in SURVEY.md §2
    auto keysAfter = [&](const std::string& keys, const Resolver& rs) -> std::string {
        std::vector<Row> rows;
        for (size_t k = 0; k < keys.size(); k++) rows.push_back(Row{{"k", std::string(1, keys[k])}, {"id", std::to_string(k)}});
        auto [ix, er] = TakeRows(rows).IndexOn({"k"});
        if (er) return "IndexOn failed";
        if (ix->ResolveDuplicates(rs)) return "ResolveDuplicates failed";
        std::string out;
        for (const Row& r : ix->rows()) out += r.at("k") + r.at("id");
        return out;
    };
    CHECK(keysAfter("AAB", KeepFirst()) == "A0");
    CHECK(keysAfter("BAAC", KeepFirst()) == "A1B0");
    CHECK(keysAfter("ABB", KeepLast()) == "A0B2");
    CHECK(keysAfter("CAB", KeepFirst()) == "A1B2C0");
    CHECK(keysAfter("AABCC", DropDuplicates()) == "B2");
    CHECK(keysAfter("AAAB", KeepMaxInt("id")) == "A2");
    CHECK(keysAfter("AAAB", KeepMinInt("id")) == "A0");
}

static void TestConversionError() {   // the message of csvplus.go:176 / :198, as a Go resolver returning ValueAsInt's error gives it
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}},   Row{{"k", "a"}, {"v", "2"}}, Row{{"k", "b"}, {"v", "oops"}},
                             Row{{"k", "c"}, {"v", "3"}},   Row{{"k", "c"}, {"v", "xyz"}}, Row{{"k", "c"}, {"v", "99999999999999999999"}},
                             Row{{"k", "d"}, {"v", "4"}}};
    auto [ix, er] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er);
    Error e = ix->ResolveDuplicates(KeepMaxInt("v"));
    CHECK(e && e.message() == "column \"v\": cannot convert \"xyz\" to integer: invalid syntax");
    CHECK(ix->rows().size() == rows.size());   // nothing changed
    e = ix->ResolveDuplicates(KeepMinFloat("v"));
    CHECK(e && e.message() == "column \"v\": cannot convert \"xyz\" to float: invalid syntax");
    // rows that reach IndexOn unsorted: the order values are still read from the right rows, and the reported one is the
    // lowest bad row of the pack in index order (the range error now comes first)
    std::vector<Row> reversed(rows.rbegin(), rows.rend());
    auto [ixr, err] = TakeRows(reversed).IndexOn({"k"});
    CHECK(!err);
    e = ixr->ResolveDuplicates(KeepMaxInt("v"));
    CHECK(e && e.message() == "column \"v\": cannot convert \"99999999999999999999\" to integer: value out of range");
    CHECK(ixr->rows().size() == rows.size());
    // the bad value outside every pack is never looked at
    rows.erase(rows.begin() + 4, rows.begin() + 6);
    auto [ix2, er2] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er2 && !ix2->ResolveDuplicates(KeepMaxInt("v")));
    CHECK(ix2->rows().size() == 3 && ix2->rows()[0].at("v") == "2" && ix2->rows()[1].at("v") == "oops");
}

static void TestMissingColumnFallback() {
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}}, Row{{"k", "a"}, {"v", "7"}}, Row{{"k", "b"}},   // no "v", outside every pack
                             Row{{"k", "c"}, {"v", "3"}}, Row{{"k", "c"}, {"v", "2"}}, Row{{"k", "d"}, {"v", "4"}}};
    auto [ix, er] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er && !ix->ResolveDuplicates(KeepMaxInt("v")));
    CHECK(ix->rows().size() == 3 && ix->rows()[0].at("v") == "7" && ix->rows()[1].count("v") == 0 && ix->rows()[2].at("v") == "3");
    rows[4].erase("v");   // now inside a pack
    auto [ix2, er2] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er2);
    Error e = ix2->ResolveDuplicates(KeepMaxInt("v"));
    CHECK(e && e.message() == "missing column \"v\"");
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestNamedResolvers", TestNamedResolvers}, {"TestTailRule", TestTailRule},
                       {"TestConversionError", TestConversionError}, {"TestMissingColumnFallback", TestMissingColumnFallback}};
    int bad = 0;
    for (auto& t : tests) {
        int before = g_failed;
        try {
            t.fn();
        } catch (const std::exception& e) {
            std::printf("  exception: %s\n", e.what());
            g_failed++;
        } catch (const Error& e) {
            std::printf("  error: %s\n", e.message().c_str());
            g_failed++;
        }
        std::printf("%s %s\n", g_failed == before ? "PASS" : "FAIL", t.name);
        if (g_failed != before) bad++;
    }
    std::printf("%d of %zu resolve tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
