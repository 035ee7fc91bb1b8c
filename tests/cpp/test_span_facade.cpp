// test_span_facade.cpp — the values NARROWED from a column, against csvplus_amd/host/csvplus.hpp: TrimSpace / TrimLeft /
// TrimRight / Trim / TrimPrefix / TrimSuffix / Field / Before / After as Map parts (CPH_MAP_SPAN), nested with each other and
// with Substr, as alternatives of a Switch, and over a Join.  The device's answers are compared with the facade's host row
// model (Format::render -> Span::of, which runs csrc/span_device.hpp's routines on the host); the model itself is pinned
// with Go's documented results first.  Run by tests/test_span_facade_cpp.py under `-m gpu`.
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

static const char* kPads[] = {"", " ", "\t", "  ", "\xC2\xA0", "\xE2\x80\x83 ", "\n\xE3\x80\x80", " \xC2\x85\r"};
static const char* kColours[] = {"red", "blue", "green", ""};
static std::vector<Row> peopleRows, ordersRows;

static void makeFixtures() {
    std::mt19937_64 rng(20261021);
    for (int i = 0; i < 120; i++)
        peopleRows.push_back(Row{{"id", std::to_string(i)}, {"email", "user" + std::to_string(i) + "@host" + std::to_string(i % 7) + ".example"}});
    for (int i = 0; i < 3000; i++) {
        const std::string cust = std::to_string((int)(rng() % 120));
        ordersRows.push_back(Row{{"order_id", std::to_string(i)},
                                 {"cust_id", cust},
                                 {"cust_raw", std::string(kPads[rng() % 8]) + cust + kPads[rng() % 8]},
                                 {"sku", std::string(i % 5 ? "SKU-" : "") + std::to_string(1000 + (int)(rng() % 9000)) + "-" + kColours[rng() % 4]},
                                 {"ts", std::string(kPads[rng() % 8]) + "2016-09-" + std::to_string(10 + (int)(rng() % 10)) + "T08:00:00Z" + kPads[rng() % 8]}});
    }
}

static std::string one(const Span& s, const std::string& v) { return Span::of(s.ops, v); }

// the host row model against Go's documented results
static void TestHostModel() {
    const Col x("x");
    CHECK(one(TrimSpace(x), " \t\n Hello, Gophers \n\t\r\n") == "Hello, Gophers");
    CHECK(one(TrimRightSpace(x), "\xE2\x80\x80\x80") == "\xE2\x80\x80\x80" && one(TrimRightSpace(x), "\xE2\xC2\x85") == "\xE2");
    CHECK(one(TrimLeftSpace(x), "\xC2\xA0 a ") == "a " && one(TrimSpace(x), "a\x85") == "a\x85" && one(TrimSpace(x), " \xE2\x80\xA8 ").empty());
    CHECK(one(Field(x, ",", 1, 2), "a,b,c,d") == "b,c,d" && one(Field(x, ",", 0, 2), "a,b,c,d") == "a");
    CHECK(one(Field(x, "a ", 3), "a man a plan a canal panama") == "canal panama" && one(Field(x, "a ", 0), "a man a plan a canal panama").empty());
    CHECK(one(Field(x, "aa", 1), "aaa") == "a" && one(Field(x, "x", 0), "").empty() && one(Field(x, ",", 5), "a,b").empty());
    CHECK(one(Field(x, ",", -1), "a,b,c") == "c" && one(Field(x, ",", -3), "a,b,c") == "a" && one(Field(x, ",", -4), "a,b,c").empty());
    CHECK(one(TrimPrefix(x, "\xC2\xA1\xC2\xA1\xC2\xA1Hello"), "\xC2\xA1\xC2\xA1\xC2\xA1Hello").empty());
    CHECK(one(TrimSuffix(x, "absent"), "value") == "value" && one(TrimSuffix(x, ".go"), "main.go.go") == "main.go");
    CHECK(one(Before(x, "Go"), "Gopher").empty() && one(After(x, "Go"), "Gopher") == "pher");
    CHECK(one(Before(x, "ph"), "Gopher") == "Go" && one(After(x, "ph"), "Gopher") == "er");
    CHECK(one(Before(x, "Badger"), "Gopher") == "Gopher" && one(After(x, "Badger"), "Gopher").empty());
    CHECK(one(Trim(x, "-+"), "-+-a+b-+") == "a+b" && one(TrimLeft(x, "-"), "--a--") == "a--" && one(TrimRight(x, "-"), "--a--") == "--a" &&
          one(Trim(x, ""), " a ") == " a ");
    CHECK(one(Span(Substr(TrimSpace(Col("ts")), 0, 10)), "  2016-09-14T10:00:00Z ") == "2016-09-14");
    CHECK(one(TrimSuffix(Substr(TrimSpace(x), 1, -1), "e"), " abcdef ") == "bcd");
    int panics = 0;
    for (int k = 0; k < 6; k++) {
        try {
            if (k == 0) Trim(x, "\xC2\xA0");
            if (k == 1) Field(x, "", 0);
            if (k == 2) Field(x, ",", 0, 0);
            if (k == 3) TrimSpace(TrimSpace(TrimSpace(TrimSpace(TrimSpace(x)))));
            if (k == 4) Trim(x, std::string(33, '-'));
            if (k == 5) Substr(TrimSpace(TrimSpace(TrimSpace(TrimSpace(x)))), 0, 1);
        } catch (const Panic&) {
            panics++;
        }
    }
    CHECK(panics == 6);
}

static bool mapMatchesModel(const std::vector<Row>& rows, const Format& f) {
    std::vector<Row> want = rows;
    for (Row& r : want) {
        std::string v, missing;
        if (!f.render(r, &v, &missing)) return false;
        r["x"] = v;
    }
    for (size_t batch : {(size_t)1, (size_t)64, (size_t)8192}) {
        if (batch == 1 && rows.size() > 100) continue;   // one call per row: for a few rows only
        Gpu::Default().join_batch_rows = batch;
        auto [got, e] = TakeRows(rows).Map(Set("x", f)).ToRows();
        Gpu::Default().join_batch_rows = 8192;
        if (e) std::printf("  %s\n", e.message().c_str());
        if (e || got != want) return false;
    }
    return true;
}

// every form as a Map part
static void TestForms() {
    std::vector<Row> rows(ordersRows.begin(), ordersRows.begin() + 300);
    rows[7]["ts"] = "";
    rows[8]["ts"] = " \t ";
    rows[9].erase("ts");
    const Col ts("ts", " none "), sku("sku");
    CHECK(mapMatchesModel(rows, Format({TrimSpace(ts)})));
    CHECK(mapMatchesModel(std::vector<Row>(rows.begin(), rows.begin() + 40), Format({TrimSpace(ts), Field(sku, "-", -1)})));
    CHECK(mapMatchesModel(rows, Format({"[", TrimLeftSpace(ts), "|", TrimRightSpace(ts), "|", Col("order_id"), "]"})));
    CHECK(mapMatchesModel(rows, Format({Trim(sku, "SKU-"), "|", TrimLeft(sku, "SKU"), "|", TrimRight(sku, "denrgbul")})));
    CHECK(mapMatchesModel(rows, Format({TrimPrefix(sku, "SKU-"), "|", TrimSuffix(sku, "-red"), "|", TrimSuffix(sku, "")})));
    CHECK(mapMatchesModel(rows, Format({Field(sku, "-", 0), "|", Field(sku, "-", 1), "|", Field(sku, "-", -1), "|", Field(sku, "-", 1, 2), "|", Field(sku, "-", 7)})));
    CHECK(mapMatchesModel(rows, Format({Before(sku, "-"), "|", After(sku, "-"), "|", After(sku, "@")})));
    std::vector<Row> seen;   // a column without default that a row lacks: the reference's missing-column error, behind the rows in front of it
    Error err = TakeRows(rows).Map(Set("day", Format({TrimSpace(Col("ts"))})))([&](Row r) {
        seen.push_back(std::move(r));
        return Error();
    });
    CHECK(err && err.message().find("missing column") != std::string::npos && seen.size() == 9);
}

// nested forms: programs of up to four operations, Substr inside and outside
static void TestNested() {
    const Col ts("ts"), sku("sku");
    const Format f({Substr(TrimSpace(ts), 0, 10), "|", Field(TrimPrefix(sku, "SKU-"), "-", 0), "|", TrimSuffix(Substr(TrimSpace(ts), 11), "Z"), "|",
                    Substr(After(Before(TrimSpace(ts), "T"), "-"), -2), "|", Substr(sku, 0, 3), "|", Fixed(Col("order_id"), 1)});
    std::string v, missing;
    Row r{{"ts", " \xC2\xA0" "2016-09-14T08:00:00Z\t"}, {"sku", "SKU-1234-red"}, {"order_id", "7"}};
    CHECK(f.render(r, &v, &missing) && v == "2016-09-14|1234|08:00:00|14|SKU|7.0");
    CHECK(mapMatchesModel(ordersRows, f));
}

// SPAN pieces in the alternatives of a Switch
static void TestSwitch() {
    const Col sku("sku"), ts("ts");
    const Switch sw = Switch({Case(HasSuffix("sku", "-red"), Format({"red ", Field(TrimPrefix(sku, "SKU-"), "-", 0)})),
                              Case(HasPrefix("sku", "SKU-"), Format({After(sku, "-"), " on ", Substr(TrimSpace(ts), 0, 10)}))},
                             Format({TrimSpace(ts), "?", Col("order_id")}));
    std::vector<Row> want = ordersRows;
    size_t seen[3] = {0, 0, 0};
    for (Row& r : want) {
        const size_t a = sw.which(r);
        seen[a]++;
        std::string v, missing;
        CHECK((a < sw.cases.size() ? sw.cases[a].then : sw.otherwise).render(r, &v, &missing));
        r["what"] = v;
    }
    CHECK(seen[0] && seen[1] && seen[2]);
    auto [got, e] = TakeRows(ordersRows).Map(Set("what", sw)).ToRows();
    if (e) std::printf("  %s\n", e.message().c_str());
    CHECK(!e && got == want);
}

// a padded key trimmed by a Map feeds a Join; a span over the joined rows reads the build side's column
static void TestOverAJoin() {
    auto [customers, ce] = TakeRows(peopleRows).UniqueIndexOn({"id"});
    CHECK(!ce);
    auto [rows, e] = TakeRows(ordersRows).Map(Set("key", Format({TrimSpace(Col("cust_raw"))}))).Join(customers, {"key"})
                         .Map(Set("host", Format({Before(After(Col("email"), "@"), "."), "/", TrimSpace(Col("ts"))}))).ToRows();
    if (e) std::printf("  %s\n", e.message().c_str());
    CHECK(!e && rows.size() == ordersRows.size());
    std::map<std::string, size_t> per_host;
    for (size_t i = 0; i < rows.size(); i++) {
        const Row& o = ordersRows[i];
        CHECK(rows[i].at("order_id") == o.at("order_id") && rows[i].at("key") == o.at("cust_id"));
        const std::string want = "host" + std::to_string(std::stoi(o.at("cust_id")) % 7) + "/" + Span::of(TrimSpace(Col("ts")).ops, o.at("ts"));
        CHECK(rows[i].at("host") == want);
        per_host[rows[i].at("host").substr(0, 5)]++;
    }
    CHECK(per_host.size() == 7);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestHostModel", TestHostModel}, {"TestForms", TestForms}, {"TestNested", TestNested}, {"TestSwitch", TestSwitch},
                       {"TestOverAJoin", TestOverAJoin}};
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
    std::printf("%d of %zu span tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
