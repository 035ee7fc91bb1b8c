// test_strpred_facade.cpp — the conditions and values that look inside a string, against csvplus_amd/host/csvplus.hpp:
// StrCmp / HasPrefix / HasSuffix / Contains as Filter, TakeWhile and Switch conditions (cph_filter_rows ops 32..37, 40..42)
// and Substr as a Map part (CPH_MAP_SLICE), over the people / orders fixtures with an RFC3339 `ts` column.  The device's
// answers are compared with the facade's own host evaluation (Pred::operator(), Format::render), which is std::string's
// compare / find / substr.  Run by tests/test_strpred_facade_cpp.py under `-m gpu`.
#include <algorithm>
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

static const char* peopleNames[] = {"Amelia", "Olivia", "Emily", "Ava", "Isla", "Oliver", "Jack", "Harry", "Jacob", "Charlie"};
static const char* peopleSurnames[] = {"Smith", "Jones", "Taylor", "Williams", "Brown", "Davies",
                                       "Evans", "Wilson", "Thomas", "Roberts", "Johnson", "Lewis"};
static const int kNames = 10, kSurnames = 12, numOrders = 3000;
static std::vector<Row> peopleRows, ordersRows;

static void makeFixtures() {
    std::mt19937_64 rng(20261020);
    for (int i = 0; i < kNames; i++)
        for (int j = 0; j < kSurnames; j++)
            peopleRows.push_back(Row{{"id", std::to_string(i * kSurnames + j)}, {"name", peopleNames[i]}, {"surname", peopleSurnames[j]}});
    peopleRows[5]["surname"] = "Smithson";
    peopleRows[17]["surname"] = "Goldsmith";
    for (int i = 0; i < numOrders; i++) {
        char ts[32];
        std::snprintf(ts, sizeof ts, "2016-09-%02dT%02d:%02d:%02d+01:00", 10 + (int)(rng() % 10), (int)(rng() % 24), (int)(rng() % 60), (int)(rng() % 60));
        ordersRows.push_back(Row{{"order_id", std::to_string(i)}, {"cust_id", std::to_string((int)(rng() % (kNames * kSurnames)))},
                                 {"qty", std::to_string((int)(rng() % 100) + 1)}, {"ts", ts}});
    }
}

static std::vector<Row> hostFilter(const std::vector<Row>& rows, const Pred& p) {
    std::vector<Row> out;
    for (const Row& r : rows)
        if (p(r)) out.push_back(r);
    return out;
}

// every constructor as a Filter: the device's rows are the host evaluation's rows, and both outcomes occur
static void TestFilters() {
    const std::vector<Pred> preds = {
        StrCmp("ts", GE, "2016-09-14"), StrCmp("ts", LT, "2016-09-14T12"), StrCmp("ts", LE, "2016-09-12"), StrCmp("ts", GT, "2016-09-18T23:00:00+01:00"),
        StrCmp("ts", NE, ordersRows[3].at("ts")), StrCmp("ts", EQ, ordersRows[3].at("ts")), StrCmp("qty", LT, "5"),   // "10" < "5": bytes, not numbers
        HasPrefix("ts", "2016-09-14"), HasSuffix("ts", ":00+01:00"), Contains("ts", "T08:"), HasPrefix("ts", ""), Contains("ts", ""),
        All(StrCmp("ts", GE, "2016-09-14"), Not(HasPrefix("ts", "2016-09-16"))), Any(HasSuffix("qty", "7"), Contains("order_id", "99")),
    };
    for (size_t k = 0; k < preds.size(); k++) {
        const std::vector<Row> want = hostFilter(ordersRows, preds[k]);
        const bool trivially_true = k == 10 || k == 11;
        CHECK(trivially_true ? want.size() == ordersRows.size() : (!want.empty() && want.size() < ordersRows.size()));
        for (size_t batch : {(size_t)100, (size_t)8192}) {
            Gpu::Default().join_batch_rows = batch;
            auto [got, e] = TakeRows(ordersRows).Filter(preds[k]).ToRows();
            if (e) std::printf("  %s\n", e.message().c_str());
            CHECK(!e && got == want);
        }
    }
    Gpu::Default().join_batch_rows = 8192;
    // the surnames: Smith, Smithson, Goldsmith
    auto [smiths, se] = TakeRows(peopleRows).Filter(Contains("surname", "Smith")).ToRows();
    CHECK(!se && smiths == hostFilter(peopleRows, Contains("surname", "Smith")) && smiths.size() == (size_t)kNames + 1);
    auto [sons, ne] = TakeRows(peopleRows).Filter(HasSuffix("surname", "son")).ToRows();
    CHECK(!ne && sons == hostFilter(peopleRows, HasSuffix("surname", "son")) && !sons.empty());
    auto [lower, le] = TakeRows(peopleRows).Filter(Contains("surname", "smith")).ToRows();   // bytes: no case folding
    CHECK(!le && lower.size() == 1 && lower[0].at("surname") == "Goldsmith");
}

// a row that lacks the column is false under every op, NE and the empty literal included — and true under Not
static void TestMissingColumn() {
    std::vector<Row> rows(ordersRows.begin(), ordersRows.begin() + 200);
    for (size_t i = 0; i < rows.size(); i += 3) rows[i].erase("ts");
    const std::vector<Pred> preds = {StrCmp("ts", NE, "x"), StrCmp("ts", LT, "\xff"), StrCmp("ts", GE, ""), StrCmp("ts", EQ, ""),
                                     HasPrefix("ts", ""), HasSuffix("ts", ""), Contains("ts", ""), Not(StrCmp("ts", NE, "x")), Not(Contains("ts", ""))};
    for (const Pred& p : preds) {
        const std::vector<Row> want = hostFilter(rows, p);
        auto [got, e] = TakeRows(rows).Filter(p).ToRows();
        CHECK(!e && got == want);
        for (const Row& r : got) CHECK((p.kind() == Pred::kNot) == (r.count("ts") == 0));
    }
    CHECK(hostFilter(rows, StrCmp("ts", NE, "x")).size() == rows.size() - (rows.size() + 2) / 3);
}

static void TestWhile() {   // sorted by ts: TakeWhile / DropWhile split the rows at a day
    std::vector<Row> rows = ordersRows;
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.at("ts") < b.at("ts"); });
    const Pred before = StrCmp("ts", LT, "2016-09-15");
    size_t stop = 0;
    while (stop < rows.size() && before(rows[stop])) stop++;
    CHECK(stop > 0 && stop < rows.size());
    auto [head, he] = TakeRows(rows).TakeWhile(before).ToRows();
    CHECK(!he && head.size() == stop && head == std::vector<Row>(rows.begin(), rows.begin() + (std::ptrdiff_t)stop));
    auto [tail, te] = TakeRows(rows).DropWhile(before).ToRows();
    CHECK(!te && tail.size() == rows.size() - stop && tail[0] == rows[stop]);
    CHECK(HasPrefix("ts", "2016-09-15")(tail[0]) || StrCmp("ts", GT, "2016-09-15")(tail[0]));
}

static void TestSubstr() {   // Map(row["day"] = row["ts"][:10]) and friends, against Format::render
    std::vector<Row> rows(ordersRows.begin(), ordersRows.begin() + 500);
    rows[7]["ts"] = "";
    rows[8]["ts"] = "2016";
    rows[9].erase("ts");
    const Format f({Substr(Col("ts", "none"), 0, 10), "|", Substr(Col("ts", "none"), -6), "|", Substr(Col("ts", "none"), 11, 19), "|",
                    Col("qty"), "|", Substr(Col("ts", "none"), 5, 2), Substr(Col("ts", "none"), -100, 4), Substr(Col("ts", "none"), 30, 40)});
    std::vector<Row> want = rows;
    for (Row& r : want) {
        std::string v, missing;
        CHECK(f.render(r, &v, &missing));
        r["x"] = v;
    }
    CHECK(want[0].at("x") == want[0].at("ts").substr(0, 10) + "|+01:00|" + want[0].at("ts").substr(11, 8) + "|" + want[0].at("qty") + "|2016");
    CHECK(want[7].at("x") == "|||" + want[7].at("qty") + "|" && want[8].at("x") == "2016|2016||" + want[8].at("qty") + "|2016");
    CHECK(want[9].at("x") == "none|none||" + want[9].at("qty") + "|none");
    for (size_t batch : {(size_t)1, (size_t)64, (size_t)8192}) {
        Gpu::Default().join_batch_rows = batch;
        auto [got, e] = TakeRows(rows).Map(Set("x", f)).ToRows();
        if (e) std::printf("  %s\n", e.message().c_str());
        CHECK(!e && got == want);
    }
    Gpu::Default().join_batch_rows = 8192;
    // a Substr of a column without default that a row lacks: the reference's missing-column error, behind the rows in front of it
    std::vector<Row> seen;
    Error err = TakeRows(rows).Map(Set("day", Format({Substr(Col("ts"), 0, 10)})))([&](Row r) {
        seen.push_back(std::move(r));
        return Error();
    });
    CHECK(err && err.message().find("missing column") != std::string::npos && seen.size() == 9 && seen[0].at("day") == rows[0].at("ts").substr(0, 10));
}

static void TestSwitchAndTotalsPerDay() {   // a HasPrefix case with Substr alternatives; then orders joined to people, counted per day
    const Switch sw = Switch({Case(HasPrefix("ts", "2016-09-14"), Format({"today ", Substr(Col("ts"), 11, 19)})),
                              Case(StrCmp("ts", LT, "2016-09-14"), Format({Substr(Col("ts"), 0, 10), " (past)"}))},
                             Format({Substr(Col("ts"), 5, 10)}));
    std::vector<Row> want = ordersRows;
    size_t seen[3] = {0, 0, 0};
    for (Row& r : want) {
        const size_t a = sw.which(r);
        seen[a]++;
        std::string v, missing;
        CHECK((a < sw.cases.size() ? sw.cases[a].then : sw.otherwise).render(r, &v, &missing));
        r["when"] = v;
    }
    CHECK(seen[0] && seen[1] && seen[2]);
    auto [got, e] = TakeRows(ordersRows).Map(Set("when", sw)).ToRows();
    if (e) std::printf("  %s\n", e.message().c_str());
    CHECK(!e && got == want);
    auto [customers, ce] = TakeRows(peopleRows).UniqueIndexOn({"id"});
    CHECK(!ce);
    auto [days, de] = TakeRows(ordersRows).Join(customers, {"cust_id"}).Filter(Contains("surname", "Smith"))
                          .Map(Set("day", Format({Substr(Col("ts"), 0, 10)}))).ToRows();
    CHECK(!de && !days.empty());
    std::map<std::string, size_t> per_day, host_per_day;
    for (const Row& r : days) per_day[r.at("day")]++;
    for (const Row& r : ordersRows) {
        const Row& c = peopleRows[(size_t)std::stoi(r.at("cust_id"))];
        if (c.at("surname").find("Smith") != std::string::npos) host_per_day[r.at("ts").substr(0, 10)]++;
    }
    CHECK(per_day == host_per_day && per_day.size() == 10);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestFilters", TestFilters}, {"TestMissingColumn", TestMissingColumn}, {"TestWhile", TestWhile}, {"TestSubstr", TestSubstr},
                       {"TestSwitchAndTotalsPerDay", TestSwitchAndTotalsPerDay}};
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
    std::printf("%d of %zu string predicate tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
