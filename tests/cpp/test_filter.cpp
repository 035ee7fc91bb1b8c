// test_filter.cpp — the reference's tests around Filter and the named predicates (csvplus_test.go: TestSimpleDataSource :118,
// TestFilterMap :155, the Filter(Like(surname)).Top(10) tail of TestLongChain :270-293, the combinator cases :468-504)
// restated against csvplus_amd/host/csvplus.hpp, whose Filter / TakeWhile / DropWhile evaluate a declarative Pred on the GPU
// (cph_filter_rows).  Fixtures as in test_host.cpp.  Run by tests/test_filter_cpp.py under `-m gpu`.
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

static const char* peopleNames[] = {"Amelia", "Olivia", "Emily", "Ava", "Isla", "Oliver", "Jack", "Harry", "Jacob", "Charlie"};
static const char* peopleSurnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies",
                                       "Evans", "Wilson", "Thomas", "Roberts", "Johnson", "Lewis"};
static const int kNames = 10, kSurnames = 12, numOrders = 10000, kStock = 8;
static const char* stockNames[] = {"banana", "apple", "orange", "pea", "tomato", "potato", "cucumber", "iPhone"};
static std::vector<Row> peopleRows, ordersRows, stockRows;

static void makeFixtures() {
    std::mt19937_64 rng(20250523);
    for (int i = 0; i < kNames; i++)
        for (int j = 0; j < kSurnames; j++)
            peopleRows.push_back(Row{{"id", std::to_string(i * kSurnames + j)}, {"name", peopleNames[i]}, {"surname", peopleSurnames[j]},
                                     {"born", std::to_string(1916 + (int)(rng() % 90))}});
    for (int i = 0; i < kStock; i++) {
        char price[16];
        std::snprintf(price, sizeof price, "%.2f", 0.01 * (i + 1));
        stockRows.push_back(Row{{"prod_id", std::to_string(i)}, {"product", stockNames[i]}, {"price", price}});
    }
    for (int i = 0; i < numOrders; i++)
        ordersRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string((int)(rng() % (kNames * kSurnames)))},
                                 {"prod_id", std::to_string((int)(rng() % kStock))}, {"qty", std::to_string((int)(rng() % 100) + 1)}});
}

// the same combinators applied row by row on the host: what the device answers are compared with
static std::vector<Row> hostRows(const std::vector<Row>& rows, const Pred& p, int mode) {
    std::vector<Row> out;
    bool yield = false;
    for (const Row& r : rows) {
        const bool ok = p(r);
        if (mode == CPH_FILTER_WHERE) {
            if (ok) out.push_back(r);
        } else if (mode == CPH_FILTER_TAKE_WHILE) {
            if (!ok) break;
            out.push_back(r);
        } else {
            yield = yield || !ok;
            if (yield) out.push_back(r);
        }
    }
    return out;
}

static void TestSimpleDataSource() {   // :118-152
    int n = 0;
    auto src = TakeRows(peopleRows).SelectColumns({"born", "id", "name", "surname"})
                   .Filter(Any(Like(Row{{"name", "Jack"}}), Like(Row{{"name", "Amelia"}})));
    Error err = src([&](Row row) -> Error {
        const std::string& name = row.at("name");
        if (name != "Jack" && name != "Amelia") return Error("Unexpected name: " + name);
        if (row.size() != 4) return Error("Unexpected number of columns: " + std::to_string(row.size()));
        n++;
        return Error();
    });
    if (err) std::printf("  %s\n", err.message().c_str());
    CHECK(!err);
    CHECK(n == kSurnames * 2);
}

static void TestFilterMap() {   // :155-172 (Map stays a host closure)
    auto src = TakeRows(peopleRows).SelectColumns({"name", "surname", "id"}).Filter(Like(Row{{"name", "Amelia"}}));
    int n = 0;
    Error err = src([&](Row row) -> Error {
        if (row["name"] == "Amelia") row["name"] = "Julia";
        n++;
        return row["name"] == "Julia" ? Error() : Error("Unexpected name: " + row["name"] + " instead of Julia");
    });
    CHECK(!err);
    CHECK(n == kSurnames);
}

static void TestLongChainTail() {   // :270-293: ...Join(orders).Join(products)...Filter(Like(surname: Smith)).Top(10)
    auto [orders, err] = TakeRows(ordersRows).IndexOn({"cust_id"});
    CHECK(!err);
    auto [products, err2] = TakeRows(stockRows).UniqueIndexOn({"prod_id"});
    CHECK(!err2);
    auto joined = TakeRows(peopleRows).SelectColumns({"id", "name", "surname"}).Join(orders, {"id"}).Join(products);
    int n = 0;
    Error e = joined.Filter(Like(Row{{"surname", "Smith"}})).Top(10).DropColumns({"id"})([&](Row row) -> Error {
        if (++n > 10) return Error("Too many rows");
        if (row.at("surname") != "Smith") return Error("Surname \"Smith\" not found");
        return row.count("id") ? Error("id is still there") : Error();
    });
    if (e) std::printf("  chain: %s\n", e.message().c_str());
    CHECK(!e);
    CHECK(n == 10);
    // all of them, against the predicate run on the host over the same joined rows
    auto [all, ae] = joined.ToRows();
    CHECK(!ae && all.size() == (size_t)numOrders);
    const Pred smith = Like(Row{{"surname", "Smith"}});
    auto [got, ge] = joined.Filter(smith).ToRows();
    CHECK(!ge && got == hostRows(all, smith, CPH_FILTER_WHERE) && !got.empty() && got.size() < all.size());
    auto [dt, de] = joined.Filter(smith).Drop(3).Top(5).ToRows();
    auto want = hostRows(all, smith, CPH_FILTER_WHERE);
    CHECK(!de && dt == std::vector<Row>(want.begin() + 3, want.begin() + 8));
}

static void TestCombinators() {   // :468-504 and the rules of :1243-1293
    const std::vector<Pred> preds = {
        Like(Row{{"name", "Amelia"}}), Like(Row{{"name", "Amelia"}, {"surname", "Smith"}}), Not(Like(Row{{"name", "Amelia"}})),
        All(), Any(), Not(Any()), All(Like(Row{{"name", "Ava"}}), Not(Like(Row{{"surname", "Smith"}}))),
        Any(Like(Row{{"id", "5"}}), Like(Row{{"id", "77"}}), All(Like(Row{{"name", "Jack"}}), Like(Row{{"surname", "Lewis"}}))),
        Like(Row{{"nope", "x"}}), Not(Like(Row{{"nope", ""}})), Like(Row{{"name", ""}}), Like(Row{{"name", "Ameli"}}),
        Like(Row{{"name", std::string("Amelia\0", 7)}})};
    // rows that lack a named column are false for its Like (:1286), row by row: every third row loses its surname
    std::vector<Row> ragged = peopleRows;
    for (size_t i = 0; i < ragged.size(); i += 3) ragged[i].erase("surname");
    ragged[4]["surname"] = "";
    for (const auto* rows : {&peopleRows, &ragged})
        for (size_t batch : {(size_t)1, (size_t)7, (size_t)8192}) {
            Gpu::Default().join_batch_rows = batch;
            for (const Pred& p : preds) {
                auto [f, fe] = TakeRows(*rows).Filter(p).ToRows();
                CHECK(!fe && f == hostRows(*rows, p, CPH_FILTER_WHERE));
                auto [t, te] = TakeRows(*rows).TakeWhile(p).ToRows();
                CHECK(!te && t == hostRows(*rows, p, CPH_FILTER_TAKE_WHILE));
                auto [d, dde] = TakeRows(*rows).DropWhile(p).ToRows();
                CHECK(!dde && d == hostRows(*rows, p, CPH_FILTER_DROP_WHILE));
            }
        }
    Gpu::Default().join_batch_rows = 8192;
    const uint64_t c0 = DataSource::filter_calls();
    auto [f, fe] = TakeRows(peopleRows).Filter(preds[0]).ToRows();
    CHECK(!fe && f.size() == (size_t)kSurnames && DataSource::filter_calls() == c0 + 1);   // one batch: one device call
    // Top stops the source: TakeWhile behind Top(30) sees 30 rows only
    auto [tt, tte] = TakeRows(peopleRows).Top(30).TakeWhile(Not(Like(Row{{"id", "500"}}))).ToRows();
    CHECK(!tte && tt.size() == 30);
    auto [dd, dre] = TakeRows(peopleRows).Drop(115).ToRows();
    CHECK(!dre && dd.size() == 5 && dd[0].at("id") == "115");
    bool panicked = false;
    try {
        Like(Row{});
    } catch (const Panic&) {
        panicked = true;
    }
    CHECK(panicked);                                                                         // :1280-1282
    // an error from the consumer surfaces, io.EOF from it ends the iteration cleanly
    Error ce = TakeRows(peopleRows).Filter(All())([](Row) { return Error("stop"); });
    CHECK(ce && ce.message().find("stop") != std::string::npos);
    int seen = 0;
    Error ee = TakeRows(peopleRows).Filter(All())([&](Row) { return ++seen == 3 ? io_EOF : Error(); });
    CHECK(!ee && seen == 3);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestSimpleDataSource", TestSimpleDataSource}, {"TestFilterMap", TestFilterMap},
                       {"TestLongChainTail", TestLongChainTail}, {"TestCombinators", TestCombinators}};
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
    std::printf("%d of %zu filter tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
