// test_totals.cpp — Index::Totals through the C++ facade (csvplus_amd/host/csvplus.hpp, cph_index_aggregate), in the shape of
// the reference's TestSimpleTotals (csvplus_test.go:516-571): per key of an index the row count and named aggregates, against a
// std::map group-by over the same rows.  Run by tests/test_totals_cpp.py under `-m gpu`.
#include <cmath>
#include <cstdio>
#include <map>
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

static std::vector<Row> peopleRows, orderRows;
static const double prices[] = {0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08};

static void makeFixtures() {
    static const char* names[] = {"Amelia", "Ava", "Emily", "Isla", "Jack", "Mia", "Noah", "Oliver", "Olivia", "William"};
    static const char* surnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies", "Evans", "Wilson"};
    int id = 0;
    for (const char* s : surnames)   // surname-major: the rows reach IndexOn("name") unsorted
        for (const char* n : names) peopleRows.push_back(Row{{"id", std::to_string(id++)}, {"name", n}, {"surname", s}});
    std::mt19937_64 rng(516);
    char price[16];
    for (int i = 0; i < 5000; i++) {   // makeOrderCsvFile (csvplus_test.go:1300-1333), joined with the stock's price
        const int prod = (int)(rng() % 8);
        std::snprintf(price, sizeof price, "%.2f", prices[prod]);
        orderRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string(rng() % peopleRows.size())},
                                {"qty", std::to_string(rng() % 100 + 1)}, {"price", price}});
    }
}

static void TestCountPerName() {
    auto [index, err] = TakeRows(peopleRows).IndexOn({"name"});
    CHECK(!err);
    auto [t, e] = index->Totals({});   // no aggregates: the distinct keys and their frequencies
    CHECK(!e && t.keys.size() == 10 && t.counts.size() == 10 && t.ints.empty() && t.floats.empty());
    for (size_t g = 0; g < t.keys.size(); g++) {
        CHECK(t.counts[g] == 8 && t.keys[g].size() == 1 && t.keys[g].count("name") == 1);
        CHECK(g == 0 || t.keys[g - 1].at("name") < t.keys[g].at("name"));   // key order
    }
    auto [t2, e2] = index->Totals({MinInt("id"), MaxInt("id"), SumInt("id")});
    CHECK(!e2 && t2.keys.size() == 10);
    std::map<std::string, std::vector<long long>> ids;
    for (const Row& r : peopleRows) ids[r.at("name")].push_back(std::stoll(r.at("id")));
    for (size_t g = 0; g < 10; g++) {
        const auto& v = ids.at(t2.keys[g].at("name"));
        long long lo = v[0], hi = v[0], sum = 0;
        for (long long x : v) lo = std::min(lo, x), hi = std::max(hi, x), sum += x;
        CHECK(t2.ints[0][g] == lo && t2.ints[1][g] == hi && t2.ints[2][g] == sum && t2.floats[0].empty());
    }
    // two key columns: every key is its own group; the rows of the index are untouched
    auto [full, e3] = TakeRows(peopleRows).IndexOn({"name", "surname"});
    CHECK(!e3);
    auto [t3, e4] = full->Totals({SumInt("id")});
    CHECK(!e4 && t3.keys.size() == peopleRows.size() && full->rows().size() == peopleRows.size());
    for (size_t g = 0; g < t3.keys.size(); g++)
        CHECK(t3.counts[g] == 1 && t3.keys[g].size() == 2 && t3.keys[g] == Row({{"name", full->rows()[g].at("name")}, {"surname", full->rows()[g].at("surname")}}) &&
              t3.ints[0][g] == std::stoll(full->rows()[g].at("id")));
    // an index without rows
    auto [none, e5] = TakeRows(std::vector<Row>{}).IndexOn({"name"});
    CHECK(!e5);
    auto [t4, e6] = none->Totals({SumInt("id")});
    CHECK(!e6 && t4.keys.empty() && t4.counts.empty() && t4.ints.size() == 1 && t4.ints[0].empty());
}

static void TestSumPerCustomer() {   // csvplus_test.go:516-571 with the sum its loop is named after
    auto [index, err] = TakeRows(orderRows).IndexOn({"cust_id"});
    CHECK(!err);
    auto [t, e] = index->Totals({SumInt("qty"), MaxFloat("price"), MinFloat("price"), SumFloat("price")});
    CHECK(!e);
    struct Acc { uint64_t n = 0; long long qty = 0; double hi = -1, lo = 1e9, sum = 0; };
    std::map<std::string, Acc> want;
    for (const Row& r : orderRows) {
        Acc& a = want[r.at("cust_id")];
        const double p = std::stod(r.at("price"));
        a.n++, a.qty += std::stoll(r.at("qty")), a.hi = std::max(a.hi, p), a.lo = std::min(a.lo, p), a.sum += p;
    }
    CHECK(t.keys.size() == want.size() && t.ints[0].size() == want.size() && t.floats[1].size() == want.size() && t.ints[1].empty());
    size_t g = 0;
    for (const auto& [cust, a] : want) {   // std::map iterates in byte order: the index's key order
        CHECK(t.keys[g].at("cust_id") == cust && t.counts[g] == a.n && t.ints[0][g] == a.qty && t.floats[1][g] == a.hi && t.floats[2][g] == a.lo);
        CHECK(std::fabs((t.floats[3][g] - a.sum) / a.sum) <= 1e-6);   // the reference's own check (:566)
        g++;
    }
}

static void TestMissingColumn() {
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}}, Row{{"k", "a"}, {"v", "7"}}, Row{{"k", "b"}}, Row{{"k", "c"}, {"v", "3"}}};
    auto [ix, er] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er);
    auto [t, e] = ix->Totals({SumInt("v")});   // every row lies in a group: one row without the column is enough
    CHECK(e && e.message() == "missing column \"v\"" && t.keys.empty());
    auto [t2, e2] = ix->Totals({SumInt("k2")});
    CHECK(e2 && e2.message() == "missing column \"k2\"");
    auto [t3, e3] = ix->Totals({});
    CHECK(!e3 && t3.counts == std::vector<uint64_t>({2, 1, 1}));
}

static void TestConversionError() {   // the message of csvplus.go:176 / :198
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}}, Row{{"k", "a"}, {"v", "2"}},   Row{{"k", "b"}, {"v", "oops"}},
                             Row{{"k", "c"}, {"v", "3"}}, Row{{"k", "c"}, {"v", "1.5"}}, Row{{"k", "d"}, {"v", "99999999999999999999"}}};
    auto [ix, er] = TakeRows(rows).IndexOn({"k"});
    CHECK(!er);
    auto [t, e] = ix->Totals({SumInt("v")});
    CHECK(e && e.message() == "column \"v\": cannot convert \"oops\" to integer: invalid syntax" && t.keys.empty());
    auto [t2, e2] = ix->Totals({MaxInt("k"), MaxFloat("v")});   // "k" fails first, at the first row
    CHECK(e2 && e2.message() == "column \"k\": cannot convert \"a\" to integer: invalid syntax");
    // rows that reach IndexOn unsorted: the values are still read from the right rows, the first bad row in index order is reported
    std::vector<Row> reversed(rows.rbegin(), rows.rend());
    auto [ixr, err] = TakeRows(reversed).IndexOn({"k"});
    CHECK(!err);
    auto [t3, e3] = ixr->Totals({MinFloat("v")});
    CHECK(e3 && e3.message() == "column \"v\": cannot convert \"oops\" to float: invalid syntax");
    rows.erase(rows.begin() + 2);
    rows.pop_back();
    std::vector<Row> rev2(rows.rbegin(), rows.rend());
    auto [ix2, er2] = TakeRows(rev2).IndexOn({"k"});
    CHECK(!er2);
    auto [t4, e4] = ix2->Totals({SumFloat("v"), MinFloat("v")});
    CHECK(!e4 && t4.floats[0] == std::vector<double>({3.0, 4.5}) && t4.floats[1] == std::vector<double>({1.0, 1.5}) && ix2->rows().size() == 4);
    auto [t5, e5] = ix2->Totals({SumInt("v")});
    CHECK(e5 && e5.message() == "column \"v\": cannot convert \"1.5\" to integer: invalid syntax");
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestCountPerName", TestCountPerName}, {"TestSumPerCustomer", TestSumPerCustomer},
                       {"TestMissingColumn", TestMissingColumn}, {"TestConversionError", TestConversionError}};
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
    std::printf("%d of %zu totals tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
