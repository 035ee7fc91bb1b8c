// test_time.cpp — RFC 3339 timestamps through the C++ facade (csvplus_amd/host/csvplus.hpp): DataSource::ColumnAsTime /
// ColumnAsTimeNano (cph_col_to_number, CPH_NUM_TIME_*), Filter(TimeCmp("ts", GE, "...")) (CPH_PRED_TIME_*) and
// Map(Set("utc", Rfc3339(...))) (CPH_MAP_TIME) on a dozen rows whose stamps mix zone offsets, so that their bytes and their
// instants order differently.  Run by tests/test_time_cpp.py under `-m gpu`.
#include <cstdio>

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

struct Stamp {
    const char* text;
    int64_t secs, nanos;
};
// 2016-09-14T00:00:00Z = 1473811200
static const Stamp kStamps[] = {
    {"2016-09-14T00:00:00Z", 1473811200, 1473811200000000000ll},
    {"2016-09-14T02:00:00+02:00", 1473811200, 1473811200000000000ll},
    {"2016-09-13T18:30:00-05:30", 1473811200, 1473811200000000000ll},
    {"2016-09-14T00:30:00+02:00", 1473805800, 1473805800000000000ll},
    {"2016-09-13T22:30:00Z", 1473805800, 1473805800000000000ll},
    {"2016-09-13T23:59:59.5-01:00", 1473814799, 1473814799500000000ll},
    {"2016-09-14T08:48:22.123456789Z", 1473842902, 1473842902123456789ll},
    {"2016-09-14T08:48:22+23:59", 1473756562, 1473756562000000000ll},
    {"1969-12-31T23:59:59.5Z", -1, -500000000ll},
    {"2000-02-29T12:00:00Z", 951825600, 951825600000000000ll},
    {"2016-09-14T00:00:01Z", 1473811201, 1473811201000000000ll},
    {"2016-09-13T23:59:59Z", 1473811199, 1473811199000000000ll},
};
static std::vector<Row> rows;

static void makeFixtures() {
    int i = 0;
    for (const Stamp& s : kStamps) rows.push_back(Row{{"id", std::to_string(i++)}, {"ts", s.text}, {"t", std::to_string(s.secs)}});
}

static std::vector<Row> hostWhere(const std::vector<Row>& in, const Pred& p) {
    std::vector<Row> out;
    for (const Row& r : in)
        if (p(r)) out.push_back(r);
    return out;
}

static void TestColumnAsTime() {
    const std::vector<int64_t> secs = TakeRows(rows).ColumnAsTime("ts");
    const std::vector<int64_t> nanos = TakeRows(rows).ColumnAsTimeNano("ts");
    CHECK(secs.size() == rows.size() && nanos.size() == rows.size());
    for (size_t i = 0; i < rows.size(); i++) {
        CHECK(secs[i] == kStamps[i].secs && nanos[i] == kStamps[i].nanos);
        int64_t v;
        CHECK(ParseRfc3339(kStamps[i].text, false, &v) == CPH_NUM_OK && v == kStamps[i].secs);
        CHECK(ParseRfc3339(kStamps[i].text, true, &v) == CPH_NUM_OK && v == kStamps[i].nanos);
    }
    CHECK(TakeRows(std::vector<Row>{}).ColumnAsTime("ts").empty());
    struct Bad { const char* text; const char* what; };
    const Bad bad[] = {{"2016-09-14 00:00:00Z", "invalid syntax"}, {"2016-02-30T00:00:00Z", "a field out of range"}};
    for (const Bad& b : bad) {
        std::vector<Row> some = rows;
        some[7]["ts"] = b.text;
        some[9]["ts"] = "";
        std::string msg;
        uint64_t line = 99;
        try {
            TakeRows(some).ColumnAsTime("ts");
        } catch (const Error& e) {
            msg = e.message();
            line = e.line();
        }
        CHECK(line == 7 && msg == std::string("row 7: column \"ts\": cannot convert \"") + b.text + "\" to time: " + b.what);
    }
    int64_t v;
    CHECK(ParseRfc3339("2016-09-14T8:48:22Z", false, &v) == CPH_NUM_ERR_UNSUPPORTED && ParseRfc3339("2016-09-14T08:48:22,5Z", false, &v) == CPH_NUM_ERR_UNSUPPORTED);
    CHECK(ParseRfc3339("2262-04-11T23:47:17Z", true, &v) == CPH_NUM_ERR_UNSUPPORTED && ParseRfc3339("2262-04-11T23:47:17Z", false, &v) == CPH_NUM_OK);
}

static void TestFilterTimeCmp() {
    std::vector<Row> ragged = rows;
    ragged[3].erase("ts");
    ragged[8]["ts"] = "2016-09-14T0:00:00Z";
    size_t differs = 0;
    for (Rel rel : {LT, LE, EQ, NE, GE, GT}) {
        const Pred p = TimeCmp("ts", rel, "2016-09-14T00:00:00Z");
        auto [got, err] = TakeRows(rows).Filter(p).ToRows();
        CHECK(!err && got == hostWhere(rows, p) && !got.empty() && got.size() < rows.size());
        differs += got != hostWhere(rows, StrCmp("ts", rel, "2016-09-14T00:00:00Z"));
        const std::vector<Pred> preds = {p, Not(p), All(p, Like(Row{{"id", "1"}})), Any(p, TimeCmp("nope", rel, "2016-09-14T00:00:00Z")),
                                         All(TimeCmp("ts", GE, "2016-09-13T22:30:00Z"), TimeCmp("ts", rel, "2016-09-14T02:00:00+02:00"))};
        for (const Pred& q : preds) {
            auto [f, fe] = TakeRows(ragged).Filter(q).ToRows();
            CHECK(!fe && f == hostWhere(ragged, q));
        }
    }
    CHECK(differs == 6);   // the byte comparison selects other rows under every relation
    auto [same, se] = TakeRows(rows).Filter(TimeCmp("ts", EQ, "2016-09-14T00:00:00Z")).ToRows();
    CHECK(!se && same.size() == 3 && same[1].at("ts") == "2016-09-14T02:00:00+02:00");
    int panics = 0;
    for (const char* lit : {"2016-09-14T00:00:00.5Z", "2016-09-14", "2016-13-14T00:00:00Z", ""}) {
        try {
            TimeCmp("ts", LT, lit);
        } catch (const Panic&) {
            panics++;
        }
    }
    CHECK(panics == 4);
}

static void TestMapRfc3339() {
    auto [utc, e1] = TakeRows(rows).Map(Set("utc", Rfc3339(Col("t")))).ToRows();
    CHECK(!e1 && utc.size() == rows.size());
    CHECK(utc[0].at("utc") == "2016-09-14T00:00:00Z" && utc[1].at("utc") == "2016-09-14T00:00:00Z" && utc[8].at("utc") == "1969-12-31T23:59:59Z");
    const Format line({"hour ", Rfc3339(AsInt(Col("t")) / 3600 * 3600, -330), " #", Col("id")});
    auto [bucket, e2] = TakeRows(rows).Map(Set("line", line)).ToRows();
    CHECK(!e2 && bucket.size() == rows.size());
    for (size_t i = 0; i < rows.size(); i++) {
        std::string want, missing;
        CHECK(line.render(rows[i], &want, &missing) && bucket[i].at("line") == want);
        std::string t;
        CHECK(FormatRfc3339(kStamps[i].secs, 0, &t) && utc[i].at("utc") == t);
        int64_t back;
        CHECK(ParseRfc3339(t, false, &back) == CPH_NUM_OK && back == kStamps[i].secs);
    }
    CHECK(bucket[0].at("line") == "hour 2016-09-13T18:30:00-05:30 #0");
    const Switch sw = When(TimeCmp("ts", LT, "2016-09-14T00:00:00Z"), Format({"before"}), Format({"at ", Rfc3339(Col("t"), 60)}));
    auto [cond, e3] = TakeRows(rows).Map(Set("when", sw)).ToRows();
    CHECK(!e3 && cond.size() == rows.size());
    CHECK(cond[3].at("when") == "before" && cond[0].at("when") == "at 2016-09-14T01:00:00+01:00" && cond[8].at("when") == "before");
    std::vector<Row> far = rows;
    far[5]["t"] = "253402300800";   // 10000-01-01T00:00:00Z
    auto [none, e4] = TakeRows(far).Map(Set("utc", Rfc3339(Col("t")))).ToRows();
    CHECK(e4 && e4.message().find("TIME piece 0, row 5") != std::string::npos);
    int panics = 0;
    try {
        Rfc3339(Col("t"), 1440);
    } catch (const Panic&) {
        panics++;
    }
    try {
        Rfc3339(AsFloat64(Col("t")));
    } catch (const Panic&) {
        panics++;
    }
    CHECK(panics == 2);
}

int main() {
    makeFixtures();
    struct T { const char* name; void (*fn)(); };
    const T tests[] = {{"TestColumnAsTime", TestColumnAsTime}, {"TestFilterTimeCmp", TestFilterTimeCmp}, {"TestMapRfc3339", TestMapRfc3339}};
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
    std::printf("%d of %zu time tests failed\n", bad, sizeof tests / sizeof tests[0]);
    return bad ? 1 : 0;
}
