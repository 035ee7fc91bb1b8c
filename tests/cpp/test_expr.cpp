// test_expr.cpp — numeric expressions through the C++ facade (csvplus_amd/host/csvplus.hpp): the reference's two numeric flows,
// the amounts table (csvplus_test.go:1391-1421) and TestSimpleTotals (:516-571), as one chain each —
//     orders.Join(products).Map(Set("amount", Fixed(AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))), 2)))
//     Totals per cust_id with SumFloat(the same product)
// — evaluated by cph_num_eval and compared with Expr::eval / Format::render, the per-row host model, and with a plain host
// loop.  Run by tests/test_expr_cpp.py under `-m gpu`.
#include <chrono>
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

static const int kStock = 8, kCustomers = 37, numOrders = 3000;
static const char* stockNames[] = {"banana", "apple", "orange", "pea", "tomato", "potato", "cucumber", "iPhone"};
static const char* stockPrices[] = {"0.99", "2.675", "9.995", "1.50", "0.10", "1234.89", ".5", "799.00"};
static std::vector<Row> stockRows, ordersRows;

static void makeFixtures() {
    std::mt19937_64 rng(20250611);
    for (int i = 0; i < kStock; i++) stockRows.push_back(Row{{"prod_id", std::to_string(i)}, {"product", stockNames[i]}, {"price", stockPrices[i]}});
    for (int i = 0; i < numOrders; i++)
        ordersRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string((int)(rng() % kCustomers))},
                                 {"prod_id", std::to_string((int)(rng() % kStock))}, {"qty", std::to_string((int)(rng() % 100) + 1)}});
}

static Expr amount() { return AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))); }

static int32_t evalInt(const Expr& e, const Row& row, int64_t* v, int* op = nullptr) { return e.eval(row, v, nullptr, op, nullptr); }
static int32_t evalFlt(const Expr& e, const Row& row, double* v, int* op = nullptr) { return e.eval(row, nullptr, v, op, nullptr); }

static void TestExprHostModel() {   // no device call: Expr::eval alone
    const Row none;
    int64_t i = 0;
    double f = 0;
    int op = 0;
    CHECK(evalInt(Expr(INT64_MAX) + 1, none, &i) == CPH_NUM_OK && i == INT64_MIN);
    CHECK(evalInt(Expr(INT64_MIN) * -1, none, &i) == CPH_NUM_OK && i == INT64_MIN);
    CHECK(evalInt(-Expr(INT64_MIN), none, &i) == CPH_NUM_OK && i == INT64_MIN);
    CHECK(evalInt(Expr(INT64_MIN) / -1, none, &i) == CPH_NUM_OK && i == INT64_MIN);
    CHECK(evalInt(Expr(INT64_MIN) % -1, none, &i) == CPH_NUM_OK && i == 0);
    CHECK(evalInt(Expr(-7) / 2, none, &i) == CPH_NUM_OK && i == -3 && evalInt(Expr(-7) % 2, none, &i) == CPH_NUM_OK && i == -1);
    CHECK(evalInt(Expr(7) / -2, none, &i) == CPH_NUM_OK && i == -3 && evalInt(Expr(7) % -2, none, &i) == CPH_NUM_OK && i == 1);
    CHECK(evalInt(Expr(5) / 0, none, &i, &op) == CPH_NUM_ERR_DIV_ZERO && i == 0 && op == 2);
    CHECK(evalInt(Expr(5) % 0, none, &i) == CPH_NUM_ERR_DIV_ZERO);
    CHECK(evalFlt(Float64(Expr((1ll << 53) + 1)), none, &f) == CPH_NUM_OK && f == 9007199254740992.0);
    CHECK(evalInt(Int(Expr(-0.9)), none, &i) == CPH_NUM_OK && i == 0);
    CHECK(evalInt(Int(Expr(-9223372036854775808.0)), none, &i) == CPH_NUM_OK && i == INT64_MIN);
    CHECK(evalInt(Int(Expr(9223372036854775808.0)), none, &i) == CPH_NUM_ERR_CONVERT && i == 0);
    CHECK(evalInt(Int(Expr(std::nan(""))), none, &i) == CPH_NUM_ERR_CONVERT);
    CHECK(evalFlt(Expr(1.0) / 0.0, none, &f) == CPH_NUM_OK && std::isinf(f) && f > 0);
    const double a = 1.0 + std::ldexp(1.0, -30), c = -(1.0 + std::ldexp(1.0, -29));
    CHECK(evalFlt(Expr(a) * a + c, none, &f) == CPH_NUM_OK && f == 0.0);   // never fused
    // the reference's shape, and the first failing op in program order
    const Expr e = amount();
    CHECK(e.ops.size() == 4 && e.cols.size() == 2 && e.cols[0].name == "price" && e.cols[1].name == "qty" && e.kind == CPH_NUM_FLOAT64);
    CHECK(evalFlt(e, Row{{"price", "2.5"}, {"qty", "3"}}, &f) == CPH_NUM_OK && f == 7.5);
    CHECK(evalFlt(e, Row{{"price", "2,5"}, {"qty", "x"}}, &f, &op) == CPH_NUM_ERR_SYNTAX && op == 0 && f == 0.0);
    CHECK(evalFlt(e, Row{{"price", "2.5"}, {"qty", "x"}}, &f, &op) == CPH_NUM_ERR_SYNTAX && op == 1);
    CHECK(e.errorText(CPH_NUM_ERR_SYNTAX, 1, Row{{"price", "2.5"}, {"qty", "x"}}) == "column \"qty\": cannot convert \"x\" to integer: invalid syntax");
    std::string missing;
    CHECK(e.eval(Row{{"price", "1"}}, nullptr, &f, &op, &missing) == -1 && missing == "qty");
    CHECK(evalFlt(AsFloat64(Col("tax", "0.25")) + 1.0, none, &f) == CPH_NUM_OK && f == 1.25);
    int panics = 0;
    for (int k = 0; k < 5; k++) {
        try {
            if (k == 0) AsInt(Col("a")) + AsFloat64(Col("b"));
            if (k == 1) AsFloat64(Col("a")) % 2.0;
            if (k == 2) Float64(AsFloat64(Col("a")));
            if (k == 3) Fixed(AsInt(Col("a")), 2);
            if (k == 4) Itoa(AsFloat64(Col("a")));
        } catch (const Panic&) {
            panics++;
        }
    }
    CHECK(panics == 5);
    std::string v, invalid;
    const Format t({Col("product"), ": ", Fixed(amount(), 2), " #", Itoa(AsInt(Col("qty")) % 7)});
    CHECK(t.render(Row{{"product", "bolt"}, {"price", "2.675"}, {"qty", "1"}}, &v, &missing) && v == "bolt: 2.67 #1");
    CHECK(!t.render(Row{{"product", "bolt"}, {"price", "2.675"}, {"qty", "1O"}}, &v, &missing, &invalid));
    CHECK(invalid == "column \"qty\": cannot convert \"1O\" to integer: invalid syntax");
}

static void TestAmountsTable() {   // createAmountsTable (:1391-1421) as one chain, against a host loop
    auto [products, pe] = TakeRows(stockRows).UniqueIndexOn({"prod_id"});
    CHECK(!pe);
    std::vector<Row> want;
    for (const Row& o : ordersRows) {
        Row r = mergeRows(o, stockRows[(size_t)std::stoi(o.at("prod_id"))]);
        r["amount"] = FormatFixed(std::strtod(r.at("price").c_str(), nullptr) * (double)std::stoi(r.at("qty")), 2);
        want.push_back(std::move(r));
    }
    for (size_t batch : {(size_t)1, (size_t)1000, (size_t)8192}) {
        if (batch == 1 && numOrders > 500) continue;   // row at a time over 3000 rows only costs time: covered by TestExprErrors
        Gpu::Default().join_batch_rows = batch;
        auto [rows, e] = TakeRows(ordersRows).Join(products).Map(Set("amount", Fixed(amount(), 2))).ToRows();
        if (e) std::printf("  %s\n", e.message().c_str());
        CHECK(!e && rows == want);
    }
    Gpu::Default().join_batch_rows = 8192;
    // beside other parts, an integer expression, and a later assignment reading an earlier one
    const std::vector<Assign> mixed = {Set("amount", Fixed(amount(), 2)),
                                       Set("line", Format({Col("product"), " x", Itoa(AsInt(Col("qty")) * 1), " = ", Fixed(AsFloat64(Col("amount")) + 0.0, 3)})),
                                       Set("dozens", Itoa(AsInt(Col("qty")) / 12))};
    auto joined = TakeRows(ordersRows).Join(products);
    auto [all, ae] = joined.ToRows();
    CHECK(!ae && all.size() == (size_t)numOrders);
    std::vector<Row> host = all;
    for (Row& r : host)
        for (const Assign& a : mixed) {
            std::string v, missing;
            CHECK(a.value.render(r, &v, &missing));
            r[a.name] = v;
        }
    auto [rows, e] = joined.Map(mixed).ToRows();
    CHECK(!e && rows == host);
    // Evaluate: the numbers themselves
    DataSource::Numbers nums = joined.Evaluate(amount());
    CHECK(nums.kind == CPH_NUM_FLOAT64 && nums.floats.size() == (size_t)numOrders && nums.ints.empty());
    for (size_t i = 0; i < all.size(); i++)
        CHECK(nums.floats[i] == std::strtod(all[i].at("price").c_str(), nullptr) * (double)std::stoi(all[i].at("qty")));
    DataSource::Numbers ints = joined.Evaluate(AsInt(Col("qty")) % 7 - 3);
    CHECK(ints.kind == CPH_NUM_INT64 && ints.ints.size() == (size_t)numOrders);
    for (size_t i = 0; i < all.size(); i++) CHECK(ints.ints[i] == std::stoi(all[i].at("qty")) % 7 - 3);
}

static void TestSimpleTotalsExpr() {   // TestSimpleTotals (:516-571): sum(price * qty) per cust_id
    auto [products, pe] = TakeRows(stockRows).UniqueIndexOn({"prod_id"});
    CHECK(!pe);
    auto [byCust, ie] = TakeRows(ordersRows).Join(products).IndexOn({"cust_id"});
    CHECK(!ie);
    auto [t, te] = byCust->Totals({SumFloat(amount()), SumInt(AsInt(Col("qty"))), MaxInt(AsInt(Col("qty")) * 2), SumInt("qty")});
    if (te) std::printf("  %s\n", te.message().c_str());
    CHECK(!te && t.keys.size() == (size_t)kCustomers);
    std::map<std::string, double> sums;
    std::map<std::string, int64_t> qty, top;
    for (const Row& o : ordersRows) {
        const int q = std::stoi(o.at("qty"));
        sums[o.at("cust_id")] += std::strtod(stockPrices[std::stoi(o.at("prod_id"))], nullptr) * (double)q;
        qty[o.at("cust_id")] += q;
        top[o.at("cust_id")] = std::max<int64_t>(top[o.at("cust_id")], 2 * q);
    }
    for (size_t g = 0; g < t.keys.size(); g++) {
        const std::string& c = t.keys[g].at("cust_id");
        CHECK(std::fabs(t.floats[0][g] - sums.at(c)) <= 1e-6 * std::fabs(sums.at(c)));   // the reference's own bound (:566)
        CHECK(t.ints[1][g] == qty.at(c) && t.ints[2][g] == top.at(c) && t.ints[3][g] == qty.at(c));
    }
    // a value that does not convert: the reference's message
    std::vector<Row> broken = ordersRows;
    broken[77]["qty"] = "7 ";
    auto [bad, be] = TakeRows(broken).Join(products).IndexOn({"cust_id"});
    CHECK(!be);
    auto [t2, te2] = bad->Totals({SumFloat(amount())});
    CHECK(te2 && te2.message().find("column \"qty\": cannot convert \"7 \" to integer: invalid syntax") != std::string::npos);
}

static void TestExprErrors() {   // a failing row ends the iteration at its row, after the rows in front of it
    std::vector<Row> rows;
    for (int i = 0; i < 40; i++) rows.push_back(Row{{"n", std::to_string(i + 1)}, {"d", std::to_string(i % 5 + 1)}, {"price", "1.25"}});
    const Assign ratio = Set("ratio", Itoa(AsInt(Col("n")) / AsInt(Col("d"))));
    for (size_t bad : {(size_t)0, (size_t)9, (size_t)39}) {
        for (int what = 0; what < 2; what++) {
            std::vector<Row> broken = rows;
            if (what == 0) broken[bad]["d"] = "0";          // division by zero
            else broken[bad]["n"] = "1e3";                  // a leaf that does not parse
            const std::string msg = what == 0 ? "integer divide by zero" : "column \"n\": cannot convert \"1e3\" to integer: invalid syntax";
            std::vector<Row> want(rows.begin(), rows.begin() + (long)bad);
            for (Row& r : want) r["ratio"] = std::to_string(std::stoi(r.at("n")) / std::stoi(r.at("d")));
            for (size_t batch : {(size_t)1, (size_t)7, (size_t)8192}) {
                Gpu::Default().join_batch_rows = batch;
                std::vector<Row> seen;
                Error e = TakeRows(broken).Map(ratio)([&](Row r) {
                    seen.push_back(std::move(r));
                    return Error();
                });
                CHECK(e && e.message().find(msg) != std::string::npos);
                CHECK(seen == want);
                if (batch == 1) CHECK(e.is_data_source_error() && e.line() == bad);   // row at a time: the reference's row number
            }
            Gpu::Default().join_batch_rows = 8192;
            bool thrown = false;
            try {
                TakeRows(broken).Evaluate(AsInt(Col("n")) / AsInt(Col("d")));
            } catch (const Error& ee) {
                thrown = ee.is_data_source_error() && ee.line() == bad && ee.message().find(msg) != std::string::npos;
            }
            CHECK(thrown);
        }
    }
    // a row without the column: the reference's `missing column`
    std::vector<Row> lacking = rows;
    lacking[3].erase("d");
    Error e = TakeRows(lacking).Map(ratio)([](Row) { return Error(); });
    CHECK(e && e.message().find("missing column \"d\"") != std::string::npos);
    bool thrown = false;
    try {
        TakeRows(lacking).Evaluate(AsInt(Col("n")) / AsInt(Col("d")));
    } catch (const Error& ee) {
        thrown = ee.is_data_source_error() && ee.line() == 3 && ee.message().find("missing column \"d\"") != std::string::npos;
    }
    CHECK(thrown);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestExprHostModel", TestExprHostModel}, {"TestAmountsTable", TestAmountsTable},
                       {"TestSimpleTotalsExpr", TestSimpleTotalsExpr}, {"TestExprErrors", TestExprErrors}};
    int bad = 0;
    for (auto& t : tests) {
        int before = g_failed;
        const auto t0 = std::chrono::steady_clock::now();
        try {
            t.fn();
        } catch (const std::exception& e) {
            std::printf("  exception: %s\n", e.what());
            g_failed++;
        } catch (const Error& e) {
            std::printf("  error: %s\n", e.message().c_str());
            g_failed++;
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s %s (%.2f s)\n", g_failed == before ? "PASS" : "FAIL", t.name, sec);
        if (g_failed != before) bad++;
    }
    std::printf("%d of %zu expr tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
