// test_numeric.cpp — typed column values through the C++ facade (csvplus_amd/host/csvplus.hpp): the reference's flagship filter
// `year, _ := row.ValueAsInt("born"); return year > 1970` (csvplus_test.go:272-281) as Filter(IntCmp("born", GT, 1970)),
// DataSource::ColumnAsInt / ColumnAsFloat64 (Row.ValueAsInt / ValueAsFloat64 for a whole column, cph_col_to_number), and the
// error of TestNumericalConversions (:911-958).  Run by tests/test_numeric_cpp.py under `-m gpu`.
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
    static const char* surnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies"};
    std::mt19937_64 rng(20250523);
    for (int i = 0; i < 600; i++) {
        char price[32];
        std::snprintf(price, sizeof price, "%d.%02d", (int)(rng() % 1000), (int)(rng() % 100));
        peopleRows.push_back(Row{{"id", std::to_string(i)}, {"surname", surnames[i % 6]}, {"born", std::to_string(1916 + (int)(rng() % 90))},
                                 {"price", price}});
    }
}

static std::vector<Row> hostWhere(const std::vector<Row>& rows, const Pred& p) {
    std::vector<Row> out;
    for (const Row& r : rows)
        if (p(r)) out.push_back(r);
    return out;
}

static void TestFilterIntCmp() {   // :272-281
    const Pred young = IntCmp("born", GT, 1970);
    auto [got, err] = TakeRows(peopleRows).Filter(young).ToRows();
    CHECK(!err);
    size_t want = 0;
    for (const Row& r : peopleRows) want += std::stoi(r.at("born")) > 1970;
    CHECK(got.size() == want && want > 0 && want < peopleRows.size());
    for (const Row& r : got) CHECK(std::stoi(r.at("born")) > 1970);
    CHECK(got == hostWhere(peopleRows, young));
    // composed with Like / All / Any / Not, every relation, rows that lack the column or hold no number
    std::vector<Row> ragged = peopleRows;
    for (size_t i = 0; i < ragged.size(); i += 5) ragged[i].erase("born");
    ragged[1]["born"] = "xyz";
    ragged[2]["born"] = "";
    ragged[3]["price"] = "1e400";
    ragged[4]["price"] = "0.1000000000000000055511151231257827";
    for (Rel rel : {LT, LE, EQ, NE, GE, GT}) {
        const std::vector<Pred> preds = {IntCmp("born", rel, 1960), Not(IntCmp("born", rel, 1960)), FloatCmp("price", rel, 500.25),
                                         FloatCmp("price", rel, 0.1), All(IntCmp("born", rel, 1950), Like(Row{{"surname", "Smith"}})),
                                         Any(FloatCmp("price", rel, 100.0), Not(IntCmp("born", GE, 1930)), Like(Row{{"surname", "Brown"}})),
                                         IntCmp("nope", rel, 0)};
        for (const Pred& p : preds) {
            auto [f, fe] = TakeRows(ragged).Filter(p).ToRows();
            CHECK(!fe && f == hostWhere(ragged, p));
        }
    }
    auto [top, te] = TakeRows(peopleRows).Filter(All(young, Like(Row{{"surname", "Smith"}}))).Top(10).ToRows();
    CHECK(!te && top.size() == 10);
    for (const Row& r : top) CHECK(r.at("surname") == "Smith" && std::stoi(r.at("born")) > 1970);
}

static void TestColumnAsNumber() {
    const std::vector<int64_t> born = TakeRows(peopleRows).ColumnAsInt("born");
    CHECK(born.size() == peopleRows.size());
    for (size_t i = 0; i < born.size(); i++) CHECK(born[i] == std::stoll(peopleRows[i].at("born")));
    const std::vector<double> price = TakeRows(peopleRows).ColumnAsFloat64("price");
    CHECK(price.size() == peopleRows.size());
    for (size_t i = 0; i < price.size(); i++) CHECK(price[i] == std::strtod(peopleRows[i].at("price").c_str(), nullptr));
    CHECK(TakeRows(std::vector<Row>{}).ColumnAsInt("born").empty());
}

static void TestConversionError() {   // :911-958
    std::vector<Row> rows = {Row{{"int", "12345"}, {"float", "3.1415926"}, {"string", "xyz"}}};
    CHECK(TakeRows(rows).ColumnAsInt("int") == std::vector<int64_t>{12345});
    const std::vector<double> f = TakeRows(rows).ColumnAsFloat64("float");
    CHECK(f.size() == 1 && f[0] == 3.1415926);
    std::string msg;
    uint64_t line = 99;
    try {
        TakeRows(rows).ColumnAsInt("string");
    } catch (const Error& e) {
        msg = e.message();
        line = e.line();
    }
    CHECK(msg == "row 0: column \"string\": cannot convert \"xyz\" to integer: invalid syntax" && line == 0);
    msg.clear();
    try {
        TakeRows(rows).ColumnAsFloat64("string");
    } catch (const Error& e) {
        msg = e.message();
    }
    CHECK(msg == "row 0: column \"string\": cannot convert \"xyz\" to float: invalid syntax");
    // the FIRST failing row is the one reported
    std::vector<Row> many = peopleRows;
    many[417]["born"] = "99999999999999999999";
    many[500]["born"] = "xyz";
    msg.clear();
    try {
        TakeRows(many).ColumnAsInt("born");
    } catch (const Error& e) {
        msg = e.message();
        line = e.line();
    }
    CHECK(line == 417 && msg == "row 417: column \"born\": cannot convert \"99999999999999999999\" to integer: value out of range");
    msg.clear();
    try {
        TakeRows(rows).ColumnAsInt("nope");
    } catch (const Error& e) {
        msg = e.message();
    }
    CHECK(msg == "row 0: missing column \"nope\"");
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestFilterIntCmp", TestFilterIntCmp}, {"TestColumnAsNumber", TestColumnAsNumber},
                       {"TestConversionError", TestConversionError}};
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
    std::printf("%d of %zu numeric tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
