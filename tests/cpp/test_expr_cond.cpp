// test_expr_cond.cpp — conditions that compare two expressions or two columns, against csvplus_amd/host/csvplus.hpp:
// ExprCmp(lhs, REL, rhs) and ColCmp(a, REL, b) as Filter, TakeWhile / DropWhile, Validate and Switch conditions (cph_filter_rows ops
// 56..61 and 72..77), over an orders fixture with prices, quantities, an amount and two city columns.  The device's answers are
// compared with the facade's own host evaluation (Pred::operator(): Expr::eval and std::string::compare).  Run by
// tests/test_expr_cond_cpp.py under `-m gpu`.
#include <algorithm>
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

static const int numOrders = 5000;
static std::vector<Row> ordersRows;

static void makeFixtures() {
    std::mt19937_64 rng(20261021);
    const char* prices[] = {"12.5", "0.5", "100", "99.99", "1e2", "0.1", "33.333", "25", "4", "n/a", "NaN", "1e38"};
    const char* cities[] = {"Leeds", "York", "Hull", "Yo", "", "York\x80"};
    for (int i = 0; i < numOrders; i++) {
        const std::string price = prices[rng() % 12];
        const int qty = (int)(rng() % 41) - 2;   // -2..38: zero and negatives among them
        double p = 0;
        std::string amount = "none";
        if (ParseFloat(price, &p) == CPH_NUM_OK && rng() % 4) amount = std::to_string(p * (double)qty + (rng() % 5 == 0 ? 0.5 : 0.0));
        ordersRows.push_back(Row{{"order_id", std::to_string(i)}, {"price", price}, {"qty", std::to_string(qty)}, {"amount", amount},
                                 {"ship", cities[rng() % 6]}, {"bill", cities[rng() % 6]}});
    }
    ordersRows[11]["qty"] = "7x";
}

static std::vector<Row> hostFilter(const std::vector<Row>& rows, const Pred& p) {
    std::vector<Row> out;
    for (const Row& r : rows)
        if (p(r)) out.push_back(r);
    return out;
}

static Expr amountExpr() { return AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))); }

static void TestHostModel() {
    const Pred ge = ExprCmp(amountExpr(), GE, 100.0);
    CHECK(ge(Row{{"price", "12.5"}, {"qty", "8"}}) && !ge(Row{{"price", "12.5"}, {"qty", "7"}}));
    CHECK(!ge(Row{{"price", "x"}, {"qty", "8"}}) && !ExprCmp(amountExpr(), NE, 100.0)(Row{{"price", "x"}, {"qty", "8"}}));   // an error: false under NE too
    CHECK(!ExprCmp(amountExpr(), NE, 100.0)(Row{{"qty", "8"}}));                                                             // a missing column
    CHECK(ExprCmp(AsFloat64(Col("p")), NE, 1.0)(Row{{"p", "NaN"}}) && !ExprCmp(AsFloat64(Col("p")), EQ, AsFloat64(Col("p")))(Row{{"p", "NaN"}}));
    CHECK(ExprCmp(AsFloat64(Col("p")), EQ, 0.0)(Row{{"p", "-0.0"}}));
    CHECK(ExprCmp(AsInt(Col("a")) / 2, EQ, -3)(Row{{"a", "-7"}}) && ExprCmp(AsInt(Col("a")) % -2, EQ, 1)(Row{{"a", "7"}}));
    CHECK(!ExprCmp(AsInt(Col("a")) / AsInt(Col("b")), NE, 0)(Row{{"a", "7"}, {"b", "0"}}));                                  // a zero divisor
    CHECK(ExprCmp(AsInt(Col("a")) + 1, LT, AsInt(Col("a")))(Row{{"a", "9223372036854775807"}}));                             // int64 wraps
    CHECK(!ExprCmp(Int(AsFloat64(Col("p"))), GE, 0)(Row{{"p", "1e19"}}));                                                    // Int() out of range
    CHECK(ColCmp("a", LT, "b")(Row{{"a", "10"}, {"b", "9"}}) && ColCmp("a", LT, "b")(Row{{"a", "a"}, {"b", std::string("a\0", 2)}}));
    CHECK(ColCmp("a", LT, "b")(Row{{"a", "\x7f"}, {"b", "\x80"}}) && ColCmp("a", EQ, "b")(Row{{"a", ""}, {"b", ""}}));
    CHECK(!ColCmp("a", NE, "b")(Row{{"a", "x"}}) && !ColCmp("a", NE, "b")(Row{{"b", "x"}}));
    bool panicked = false;
    try {
        ExprCmp(AsInt(Col("qty")), LT, 1.5);
    } catch (const Panic&) {
        panicked = true;
    }
    CHECK(panicked);
}

// every relation as a Filter: the device's rows are the host evaluation's rows, and both outcomes occur
static void TestFilters() {
    std::vector<Pred> preds;
    for (Rel rel : {LT, LE, EQ, NE, GE, GT}) {
        preds.push_back(ExprCmp(amountExpr(), rel, 100.0));
        preds.push_back(ExprCmp(amountExpr(), rel, AsFloat64(Col("amount"))));
        preds.push_back(ExprCmp(AsInt(Col("qty")) * 3 - 7, rel, AsInt(Col("order_id")) % 50));
        preds.push_back(ColCmp("ship", rel, "bill"));
    }
    preds.push_back(All(ExprCmp(AsInt(Col("qty")), GT, 0), ExprCmp(amountExpr(), EQ, AsFloat64(Col("amount")))));   // the issue's Validate
    preds.push_back(All(Not(ExprCmp(amountExpr(), GE, 100.0)), Like(Row{{"ship", "York"}}), HasPrefix("bill", "Y"), ColCmp("ship", NE, "bill")));
    preds.push_back(Any(ExprCmp(Int(AsFloat64(Col("price"))), EQ, AsInt(Col("qty"))), IntCmp("qty", LT, 0)));
    for (size_t k = 0; k < preds.size(); k++) {
        const std::vector<Row> want = hostFilter(ordersRows, preds[k]);
        CHECK(!want.empty() && want.size() < ordersRows.size());
        for (size_t batch : {(size_t)100, (size_t)8192}) {
            Gpu::Default().join_batch_rows = batch;
            auto [got, e] = TakeRows(ordersRows).Filter(preds[k]).ToRows();
            if (e) std::printf("  %s\n", e.message().c_str());
            if (!e && got != want) std::printf("  predicate %zu, batch %zu: %zu rows, want %zu\n", k, batch, got.size(), want.size());
            CHECK(!e && got == want);
        }
    }
    Gpu::Default().join_batch_rows = 8192;
}

// a row that lacks a column is false under every relation, NE included — and true under Not; a Col default stands in
static void TestMissingColumn() {
    std::vector<Row> rows(ordersRows.begin(), ordersRows.begin() + 300);
    for (size_t i = 0; i < rows.size(); i += 3) rows[i].erase("qty");
    for (size_t i = 1; i < rows.size(); i += 5) rows[i].erase("bill");
    const std::vector<Pred> preds = {ExprCmp(amountExpr(), NE, 100.0), Not(ExprCmp(amountExpr(), NE, 100.0)), ExprCmp(AsInt(Col("qty")), GE, AsInt(Col("qty"))),
                                     ExprCmp(AsInt(Col("qty", "5")), EQ, 5), ColCmp("ship", NE, "bill"), ColCmp("bill", GE, "bill"), Not(ColCmp("ship", LT, "bill"))};
    for (const Pred& p : preds) {
        const std::vector<Row> want = hostFilter(rows, p);
        CHECK(!want.empty() && want.size() < rows.size());
        auto [got, e] = TakeRows(rows).Filter(p).ToRows();
        CHECK(!e && got == want);
    }
    for (const Row& r : hostFilter(rows, preds[0])) CHECK(r.count("qty") == 1);
    CHECK(hostFilter(rows, preds[3]).size() >= rows.size() / 3);   // the rows without qty take the default
}

static void TestWhileAndValidate() {
    std::vector<Row> rows = hostFilter(ordersRows, All(ExprCmp(AsInt(Col("qty")), GT, 0), ExprCmp(amountExpr(), LT, 1e30)));
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
        double x = 0, y = 0;
        amountExpr().eval(a, nullptr, &x, nullptr, nullptr);
        amountExpr().eval(b, nullptr, &y, nullptr, nullptr);
        return x < y;
    });
    const Pred cheap = ExprCmp(amountExpr(), LT, 100.0);
    size_t stop = 0;
    while (stop < rows.size() && cheap(rows[stop])) stop++;
    CHECK(stop > 0 && stop < rows.size());
    auto [head, he] = TakeRows(rows).TakeWhile(cheap).ToRows();
    CHECK(!he && head == std::vector<Row>(rows.begin(), rows.begin() + (std::ptrdiff_t)stop));
    auto [tail, te] = TakeRows(rows).DropWhile(cheap).ToRows();
    CHECK(!te && tail.size() == rows.size() - stop && tail[0] == rows[stop]);
    // Validate(qty > 0 && price * float64(qty) < 100): the iteration ends at the first row that fails, behind the rows in front of it
    const Pred ok = All(ExprCmp(AsInt(Col("qty")), GT, 0), cheap);
    std::vector<Row> seen;
    Error err = TakeRows(rows).Validate(ok, "too dear")([&](Row r) {
        seen.push_back(std::move(r));
        return Error();
    });
    CHECK(err && err.message().find("too dear") != std::string::npos && seen.size() == stop);
    auto [all, ae] = TakeRows(head).Validate(ok, "too dear").ToRows();
    CHECK(!ae && all == head);
}

static void TestSwitchTiers() {   // if amount >= 1000 { gold } else if amount >= 100 { silver } else { std }
    const Switch sw = Switch({Case(ExprCmp(amountExpr(), GE, 1000.0), Format({"gold"})), Case(ExprCmp(amountExpr(), GE, 100.0), Format({"silver ", Col("qty")})),
                              Case(ColCmp("ship", EQ, "bill"), Format({"local ", Col("ship")}))},
                             Format({"std"}));
    std::vector<Row> want = ordersRows;
    size_t seen[4] = {0, 0, 0, 0};
    for (Row& r : want) {
        const size_t a = sw.which(r);
        seen[a]++;
        std::string v, missing;
        CHECK((a < sw.cases.size() ? sw.cases[a].then : sw.otherwise).render(r, &v, &missing));
        r["tier"] = v;
    }
    CHECK(seen[0] && seen[1] && seen[2] && seen[3]);
    for (size_t batch : {(size_t)64, (size_t)8192}) {
        Gpu::Default().join_batch_rows = batch;
        auto [got, e] = TakeRows(ordersRows).Map(Set("tier", sw)).ToRows();
        if (e) std::printf("  %s\n", e.message().c_str());
        CHECK(!e && got == want);
    }
    Gpu::Default().join_batch_rows = 8192;
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestHostModel", TestHostModel}, {"TestFilters", TestFilters}, {"TestMissingColumn", TestMissingColumn},
                       {"TestWhileAndValidate", TestWhileAndValidate}, {"TestSwitchTiers", TestSwitchTiers}};
    int bad = 0;
    for (auto& t : tests) {
        int before = g_failed;
        try {
            t.fn();
        } catch (const std::exception& e) {
            std::printf("  exception: %s\n", e.what());
            g_failed++;
        }
        std::printf("%s %s\n", g_failed == before ? "PASS" : "FAIL", t.name);
        if (g_failed != before) bad++;
    }
    std::printf("%d of %zu expression condition tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
