// test_join_totals.cpp — DataSource::TotalsBy through the C++ facade (csvplus_amd/host/csvplus.hpp, cph_chain_aggregate), in the
// shape of the reference's TestTransformedSource (csvplus_test.go:754-806): orders joined with people and with the stock, then
// per customer the row count, the int Sum of qty and the float Sum of price * float64(qty), against a std::map group-by computed
// here over the same rows.  Run by tests/test_join_totals_cpp.py under `-m gpu`.
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

static std::vector<Row> peopleRows, stockRows, orderRows;
static const double prices[] = {0.25, 1.5, 3.0, 4.75, 10.0, 12.5, 0.5, 100.0};   // binary fractions: price * qty and its sums are exact

static void makeFixtures() {
    for (int id = 0; id < 90; id++) peopleRows.push_back(Row{{"id", std::to_string(id)}, {"name", "n" + std::to_string(id % 7)}});
    char price[16];
    for (int p = 0; p < 8; p++) {
        std::snprintf(price, sizeof price, "%.2f", prices[p]);
        stockRows.push_back(Row{{"prod_id", std::to_string(p)}, {"price", price}});
    }
    std::mt19937_64 rng(754);
    for (int i = 0; i < 4000; i++)   // customers 80..89 never order
        orderRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string(rng() % 80)}, {"prod_id", std::to_string(rng() % 8)},
                                {"qty", std::to_string(rng() % 100 + 1)}});
}

struct Acc {
    uint64_t n = 0;
    long long qty = 0, most = 0;
    double amount = 0;
};

static void TestAmountPerCustomer() {
    auto [people, e1] = TakeRows(peopleRows).UniqueIndexOn({"id"});
    auto [stock, e2] = TakeRows(stockRows).UniqueIndexOn({"prod_id"});
    CHECK(!e1 && !e2);
    DataSource joined = TakeRows(orderRows).Join(people, {"cust_id"}).Join(stock, {"prod_id"});
    auto [t, e] = joined.TotalsBy(0, {SumInt("qty"), SumFloat(AsFloat64(Col("price")) * Float64(AsInt(Col("qty")))), MaxInt(AsInt(Col("qty")))});
    CHECK(!e);
    std::map<std::string, Acc> want;
    for (const Row& r : orderRows) {
        Acc& a = want[r.at("cust_id")];
        const long long q = std::stoll(r.at("qty"));
        a.n++, a.qty += q, a.most = std::max(a.most, q), a.amount += prices[std::stoi(r.at("prod_id"))] * (double)q;
    }
    const auto& rows = people->rows();   // group g = row g of the index, key order
    CHECK(t.counts.size() == rows.size() && t.ints[0].size() == rows.size() && t.floats[1].size() == rows.size() && t.ints[1].empty() &&
          t.floats[0].empty() && t.ints[2].size() == rows.size());
    size_t empty = 0;
    for (size_t g = 0; g < rows.size(); g++) {
        auto it = want.find(rows[g].at("id"));
        if (it == want.end()) {
            CHECK(t.counts[g] == 0 && t.ints[0][g] == 0 && t.floats[1][g] == 0.0 && t.ints[2][g] == 0);
            empty++;
            continue;
        }
        const Acc& a = it->second;
        CHECK(t.counts[g] == a.n && t.ints[0][g] == a.qty && t.ints[2][g] == a.most);
        CHECK(t.floats[1][g] == a.amount);   // every product and every partial sum is exact: any order gives these bits
    }
    CHECK(empty == 10);
    // by the second Join: per product
    auto [tp, ep] = joined.TotalsBy(1, {SumInt("qty")});
    CHECK(!ep && tp.counts.size() == 8);
    std::map<std::string, Acc> per;
    for (const Row& r : orderRows) per[r.at("prod_id")].n++, per[r.at("prod_id")].qty += std::stoll(r.at("qty"));
    for (size_t g = 0; g < 8; g++) CHECK(tp.counts[g] == per.at(stock->rows()[g].at("prod_id")).n && tp.ints[0][g] == per.at(stock->rows()[g].at("prod_id")).qty);
    // no aggregates: the counts only
    auto [tc, ec] = joined.TotalsBy(0, {});
    CHECK(!ec && tc.counts == t.counts && tc.ints.empty() && tc.floats.empty());
}

static void TestErrorsAndEdges() {
    auto [people, e1] = TakeRows(peopleRows).UniqueIndexOn({"id"});
    CHECK(!e1);
    std::vector<Row> orders = {Row{{"cust_id", "3"}, {"qty", "2"}}, Row{{"cust_id", "3"}, {"qty", "oops"}}, Row{{"cust_id", "5"}, {"qty", "4"}},
                               Row{{"cust_id", "zz"}, {"qty", "9"}}};
    DataSource joined = TakeRows(orders).Join(people, {"cust_id"});
    auto [t, e] = joined.TotalsBy(0, {SumInt("qty")});
    CHECK(e && e.message() == "column \"qty\": cannot convert \"oops\" to integer: invalid syntax" && t.counts.empty());
    auto [t2, e2] = joined.TotalsBy(0, {SumInt("nope")});
    CHECK(e2 && e2.message() == "missing column \"nope\"");
    auto [t3, e3] = joined.TotalsBy(0, {MaxInt("id")});   // a column of the index row; the stream row without a match joins nothing
    CHECK(!e3);
    uint64_t total = 0;
    for (size_t g = 0; g < t3.counts.size(); g++) {
        const std::string& id = people->rows()[g].at("id");
        CHECK(t3.counts[g] == (id == "3" ? 2u : id == "5" ? 1u : 0u) && t3.ints[0][g] == (t3.counts[g] ? std::stoll(id) : 0));
        total += t3.counts[g];
    }
    CHECK(total == 3);
    auto [t4, e4] = TakeRows(std::vector<Row>{}).Join(people, {"id"}).TotalsBy(0, {SumFloat("x")});   // no stream rows: zeros
    CHECK(!e4 && t4.counts == std::vector<uint64_t>(peopleRows.size(), 0) && t4.floats[0] == std::vector<double>(peopleRows.size(), 0.0));
    bool panicked = false;
    try {
        (void)TakeRows(orders).TotalsBy(0, {});
    } catch (const Panic&) {
        panicked = true;
    }
    CHECK(panicked);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestAmountPerCustomer", TestAmountPerCustomer}, {"TestErrorsAndEdges", TestErrorsAndEdges}};
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
    std::printf("%d of %zu join totals tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
