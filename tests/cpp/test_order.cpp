// test_order.cpp — DataSource::OrderBy through the C++ facade (csvplus_amd/host/csvplus.hpp, cph_order_rows) over the people /
// orders fixtures, against std::stable_sort with the comparisons written out (cmp.Compare per key; Desc swaps its arguments).
// Run by tests/test_order_cpp.py under `-m gpu`.
#include <algorithm>
#include <cmath>
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

static std::vector<Row> peopleRows, orderRows;
static const double prices[] = {0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08};

static void makeFixtures() {
    static const char* names[] = {"Amelia", "Ava", "Emily", "Isla", "Jack", "Mia", "Noah", "Oliver", "Olivia", "William"};
    static const char* surnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies", "Evans", "Wilson"};
    int id = 0;
    for (const char* s : surnames)
        for (const char* n : names) peopleRows.push_back(Row{{"id", std::to_string(id++)}, {"name", n}, {"surname", s}});
    std::mt19937_64 rng(794);
    char price[16];
    for (int i = 0; i < 5000; i++) {   // makeOrderCsvFile (csvplus_test.go:1300-1333), joined with the stock's price
        const int prod = (int)(rng() % 8);
        std::snprintf(price, sizeof price, "%.2f", prices[prod]);
        orderRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string(rng() % peopleRows.size())},
                                {"qty", std::to_string(rng() % 100 + 1)}, {"price", price}});
    }
}

template <class T>
static int compare(const T& a, const T& b) { return a < b ? -1 : (b < a ? 1 : 0); }

static std::vector<std::string> column(const std::vector<Row>& rows, const char* name) {
    std::vector<std::string> out;
    for (const Row& r : rows) out.push_back(r.at(name));
    return out;
}

static void TestTopFiveByQty() {   // "the five largest orders": Desc int key, Top(5) becomes the sort's limit
    std::vector<Row> want = orderRows;
    std::stable_sort(want.begin(), want.end(), [](const Row& a, const Row& b) { return compare(std::stoll(b.at("qty")), std::stoll(a.at("qty"))) < 0; });
    const uint64_t calls = DataSource::order_calls();
    auto [got, err] = TakeRows(orderRows).OrderBy({Desc(IntKey("qty"))}).Top(5).ToRows();
    CHECK(!err && got.size() == 5 && DataSource::order_calls() == calls + 1);
    CHECK(column(got, "order_id") == column(std::vector<Row>(want.begin(), want.begin() + 5), "order_id"));
    CHECK(DataSource::order_candidates() < orderRows.size());   // the device selected: not every row entered the sort
    // Drop and Top in either order, and the whole order
    auto [got2, err2] = TakeRows(orderRows).OrderBy({Desc(IntKey("qty"))}).Drop(3).Top(4).ToRows();
    CHECK(!err2 && column(got2, "order_id") == column(std::vector<Row>(want.begin() + 3, want.begin() + 7), "order_id"));
    auto [got3, err3] = TakeRows(orderRows).OrderBy({Desc(IntKey("qty"))}).Top(10).Drop(8).ToRows();
    CHECK(!err3 && column(got3, "order_id") == column(std::vector<Row>(want.begin() + 8, want.begin() + 10), "order_id"));
    auto [all, err4] = TakeRows(orderRows).OrderBy({Desc(IntKey("qty"))}).ToRows();
    CHECK(!err4 && column(all, "order_id") == column(want, "order_id"));
    auto [none, err5] = TakeRows(std::vector<Row>{}).OrderBy({Asc(IntKey("qty"))}).Top(3).ToRows();
    CHECK(!err5 && none.empty());
    // a consumer that stops early ends the iteration cleanly
    size_t seen = 0;
    Error stop = TakeRows(orderRows).OrderBy({Asc(IntKey("qty"))})([&](Row) { return ++seen == 3 ? io_EOF : Error(); });
    CHECK(!stop && seen == 3);
}

static void TestMixedThreeKeys() {   // bytes descending, float ascending, an int expression descending; the input order decides the rest
    std::vector<Row> want = orderRows;
    std::stable_sort(want.begin(), want.end(), [](const Row& a, const Row& b) {
        if (int c = compare(b.at("cust_id"), a.at("cust_id"))) return c < 0;                       // strings.Compare: "10" < "9"
        if (int c = compare(std::stod(a.at("price")), std::stod(b.at("price")))) return c < 0;
        return compare(std::stoll(b.at("qty")) % 10, std::stoll(a.at("qty")) % 10) < 0;
    });
    auto [got, err] = TakeRows(orderRows).OrderBy({Desc(StrKey("cust_id")), Asc(FloatKey("price")), Desc(IntKey(AsInt(Col("qty")) % 10))}).ToRows();
    CHECK(!err && got.size() == want.size());
    CHECK(column(got, "order_id") == column(want, "order_id"));
    // people by name, then surname descending: two bytes keys
    std::vector<Row> people = peopleRows;
    std::stable_sort(people.begin(), people.end(), [](const Row& a, const Row& b) {
        if (int c = compare(a.at("name"), b.at("name"))) return c < 0;
        return compare(b.at("surname"), a.at("surname")) < 0;
    });
    auto [got2, err2] = TakeRows(peopleRows).OrderBy({Asc(StrKey("name")), Desc(StrKey("surname"))}).ToRows();
    CHECK(!err2 && column(got2, "id") == column(people, "id"));
}

static void TestMissingColumn() {
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}}, Row{{"k", "b"}, {"v", "7"}}, Row{{"k", "c"}}, Row{{"k", "d"}, {"v", "3"}}};
    size_t seen = 0;
    Error e = TakeRows(rows).OrderBy({Desc(IntKey("v"))})([&](Row) { seen++; return Error(); });
    CHECK(e && e.is_data_source_error() && e.line() == 2 && e.message() == "row 2: missing column \"v\"" && seen == 0);
    Error e2 = TakeRows(rows).OrderBy({Asc(StrKey("k")), Asc(StrKey("k2"))})([&](Row) { seen++; return Error(); });
    CHECK(e2 && e2.message() == "row 0: missing column \"k2\"" && seen == 0);
    auto [ok, e3] = TakeRows(rows).OrderBy({Desc(StrKey("k"))}).ToRows();
    CHECK(!e3 && column(ok, "k") == std::vector<std::string>({"d", "c", "b", "a"}));
}

static void TestConversionError() {   // the message of csvplus.go:176 / :198, for the first such row
    std::vector<Row> rows = {Row{{"k", "a"}, {"v", "1"}}, Row{{"k", "b"}, {"v", "2.5"}}, Row{{"k", "c"}, {"v", "oops"}}, Row{{"k", "d"}, {"v", "3"}}};
    size_t seen = 0;
    Error e = TakeRows(rows).OrderBy({Asc(IntKey("v"))})([&](Row) { seen++; return Error(); });
    CHECK(e && e.line() == 1 && e.message() == "row 1: column \"v\": cannot convert \"2.5\" to integer: invalid syntax" && seen == 0);
    Error e2 = TakeRows(rows).OrderBy({Asc(StrKey("k")), Desc(FloatKey("v"))})([&](Row) { seen++; return Error(); });
    CHECK(e2 && e2.message() == "row 2: column \"v\": cannot convert \"oops\" to float: invalid syntax" && seen == 0);
    // a conversion error in front of a missing column wins; behind it, the missing column does
    rows.push_back(Row{{"k", "e"}});
    Error e3 = TakeRows(rows).OrderBy({Asc(FloatKey("v"))})([&](Row) { seen++; return Error(); });
    CHECK(e3 && e3.message() == "row 2: column \"v\": cannot convert \"oops\" to float: invalid syntax");
    rows.erase(rows.begin() + 2);
    Error e4 = TakeRows(rows).OrderBy({Asc(FloatKey("v"))})([&](Row) { seen++; return Error(); });
    CHECK(e4 && e4.message() == "row 3: missing column \"v\"" && seen == 0);
    rows.pop_back();
    auto [ok, e5] = TakeRows(rows).OrderBy({Desc(FloatKey("v"))}).ToRows();
    CHECK(!e5 && column(ok, "k") == std::vector<std::string>({"d", "b", "a"}));
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestTopFiveByQty", TestTopFiveByQty}, {"TestMixedThreeKeys", TestMixedThreeKeys},
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
    std::printf("%d of %zu order tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
