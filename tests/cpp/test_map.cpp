// test_map.cpp — the reference's Map and Validate (csvplus.go:290-310; csvplus_test.go: TestFilterMap :153-170, the Printf over
// a joined row of the README's second example) restated against csvplus_amd/host/csvplus.hpp, whose Map renders a row template
// on the GPU (cph_map_format) and whose Validate evaluates a declarative Pred there (cph_filter_rows, TAKE_WHILE).  Fixtures
// as in test_filter.cpp.  Run by tests/test_map_cpp.py under `-m gpu`.
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
static const int kNames = 10, kSurnames = 12, numOrders = 3000, kStock = 8;
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

// the assignments applied row by row on the host: what the device answers are compared with
static bool hostMap(std::vector<Row> rows, const std::vector<Assign>& assigns, std::vector<Row>* out) {
    for (Row& r : rows)
        for (const Assign& a : assigns) {
            std::string v, missing;
            if (!a.value.render(r, &v, &missing)) return false;
            r[a.name] = v;
        }
    *out = std::move(rows);
    return true;
}

static void TestMapConstant() {   // :153-170, the README's first example: Amelia -> Julia
    auto src = TakeRows(peopleRows).SelectColumns({"name", "surname", "id"}).Filter(Like(Row{{"name", "Amelia"}})).Map(Set("name", "Julia"));
    int n = 0;
    Error err = src([&](Row row) -> Error {
        n++;
        if (row.size() != 3) return Error("Unexpected number of columns: " + std::to_string(row.size()));
        return row["name"] == "Julia" ? Error() : Error("Unexpected name: " + row["name"] + " instead of Julia");
    });
    if (err) std::printf("  %s\n", err.message().c_str());
    CHECK(!err);
    CHECK(n == kSurnames);
    // a new column, the empty literal, bytes of every kind; one device call per batch
    const std::string odd("\0\x80\xff,\"\n", 6);
    for (size_t batch : {(size_t)1, (size_t)7, (size_t)8192}) {
        Gpu::Default().join_batch_rows = batch;
        const uint64_t c0 = DataSource::map_calls();
        auto [rows, e] = TakeRows(peopleRows).Map({Set("odd", odd), Set("none", "")}).ToRows();
        CHECK(!e && rows.size() == peopleRows.size());
        for (size_t i = 0; i < rows.size(); i++) {
            Row want = peopleRows[i];
            want["odd"] = odd;
            want["none"] = "";
            CHECK(rows[i] == want);
        }
        CHECK(DataSource::map_calls() == c0 + 2 * ((peopleRows.size() + batch - 1) / batch));
    }
    Gpu::Default().join_batch_rows = 8192;
}

static void TestMapFormat() {   // row["full"] = row["name"] + " " + row["surname"]; the README's Printf over a joined row
    const std::vector<Assign> assigns = {
        Set("full", Format({Col("name"), " ", Col("surname")})),
        Set("line", Format({Col("full"), " (", Col("id"), ") born ", Col("born"), Col("nope", "?"), Col("id")})),
        Set("name", Format({Col("surname"), Col("name")}))};   // replaces a source column, reading its old value
    std::vector<Row> want;
    CHECK(hostMap(peopleRows, assigns, &want));
    CHECK(want[13].at("full") == "Olivia Jones" && want[13].at("line") == "Olivia Jones (13) born " + peopleRows[13].at("born") + "?13");
    for (size_t batch : {(size_t)1, (size_t)5, (size_t)8192}) {
        Gpu::Default().join_batch_rows = batch;
        auto [rows, e] = TakeRows(peopleRows).Map(assigns).ToRows();
        CHECK(!e && rows == want);
    }
    Gpu::Default().join_batch_rows = 8192;
    // rows that lack a column: the default where there is one, row by row ...
    std::vector<Row> ragged = peopleRows;
    for (size_t i = 0; i < ragged.size(); i += 3) ragged[i].erase("surname");
    ragged[4]["surname"] = "";
    const std::vector<Assign> safe = {Set("full", Format({Col("name"), "-", Col("surname", "n/a"), "-"}))};
    CHECK(hostMap(ragged, safe, &want));
    auto [got, ge] = TakeRows(ragged).Map(safe).ToRows();
    CHECK(!ge && got == want && got[0].at("full") == "Amelia-n/a-" && got[4].at("full") == "Amelia--");
    // ... and without one the reference's error at that row, after the rows in front of it
    std::vector<Row> seen;
    Error me = TakeRows(ragged).Drop(1).Map(Set("full", Format({Col("name"), " ", Col("surname")})))([&](Row r) {
        seen.push_back(std::move(r));
        return Error();
    });
    CHECK(me && me.is_data_source_error() && me.line() == 3 && me.message().find("missing column \"surname\"") != std::string::npos);
    CHECK(seen.size() == 2 && seen[1].at("full") == "Amelia Taylor");
    // over a joined row: "<name> <surname> bought <qty> <product>s"
    auto [customers, ce] = TakeRows(peopleRows).UniqueIndexOn({"id"});
    CHECK(!ce);
    auto [products, pe] = TakeRows(stockRows).UniqueIndexOn({"prod_id"});
    CHECK(!pe);
    auto joined = TakeRows(ordersRows).Join(customers, {"cust_id"}).Join(products);
    auto [all, ae] = joined.ToRows();
    CHECK(!ae && all.size() == (size_t)numOrders);
    const std::vector<Assign> bought = {Set("text", Format({Col("name"), " ", Col("surname"), " bought ", Col("qty"), " ", Col("product"), "s"}))};
    CHECK(hostMap(all, bought, &want));
    auto [texts, te] = joined.Map(bought).ToRows();
    CHECK(!te && texts == want);
    // an error from the consumer surfaces, io.EOF from it ends the iteration cleanly
    Error cerr = TakeRows(peopleRows).Map(Set("x", "y"))([](Row) { return Error("stop"); });
    CHECK(cerr && cerr.message().find("stop") != std::string::npos);
    int cnt = 0;
    Error eof = TakeRows(peopleRows).Map(Set("x", "y"))([&](Row) { return ++cnt == 3 ? io_EOF : Error(); });
    CHECK(!eof && cnt == 3);
    bool panicked = false;
    try {
        TakeRows(peopleRows).Map(std::vector<Assign>{});
    } catch (const Panic&) {
        panicked = true;
    }
    CHECK(panicked);
}

static void TestValidate() {   // :300-310
    const Pred young = IntCmp("born", GT, 1800);
    auto [okRows, oe] = TakeRows(peopleRows).Validate(young, "born too early").ToRows();
    CHECK(!oe && okRows == peopleRows);
    std::vector<Row> rows = peopleRows;
    for (size_t bad : {(size_t)0, (size_t)57, rows.size() - 1}) {
        std::vector<Row> broken = rows;
        broken[bad]["born"] = "1492";
        for (size_t batch : {(size_t)1, (size_t)16, (size_t)8192}) {
            Gpu::Default().join_batch_rows = batch;
            std::vector<Row> seen;
            Error e = TakeRows(broken).Validate(young, "born too early")([&](Row r) {
                seen.push_back(std::move(r));
                return Error();
            });
            CHECK(e && e.message().find("born too early") != std::string::npos);
            CHECK(seen.size() == bad && seen == std::vector<Row>(broken.begin(), broken.begin() + (long)bad));
            if (batch == 1) CHECK(e.is_data_source_error() && e.line() == bad);   // row at a time: the reference's row number
        }
    }
    Gpu::Default().join_batch_rows = 8192;
    // a row that lacks the column fails a Like / IntCmp over it, hence the validation
    rows[5].erase("born");
    Error e = TakeRows(rows).Validate(young, "no year")([](Row) { return Error(); });
    CHECK(e && e.message().find("no year") != std::string::npos);
    // Transform = Map, Filter and Validate composed
    auto [tr, te] = TakeRows(peopleRows).Validate(young, "bad").Filter(Like(Row{{"name", "Jack"}})).Map(Set("name", "John")).ToRows();
    CHECK(!te && tr.size() == (size_t)kSurnames && tr[0].at("name") == "John");
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestMapConstant", TestMapConstant}, {"TestMapFormat", TestMapFormat}, {"TestValidate", TestValidate}};
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
    std::printf("%d of %zu map tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
