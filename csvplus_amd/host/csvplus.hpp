// csvplus.hpp — C++ host side of the hot path, mirroring the reference's Go method set
// (maxim2266/csvplus, csvplus.go) for Index build + Join on top of the C ABI
// (include/csvplus_hip.h).  The Go toolchain is absent from this image, so this header is
// what the cgo shim of INTEGRATION.md would be in Go: same names, argument meaning and
// error behaviour.
//
//   Go (csvplus.go)                              here
//   type Row map[string]string            :59    csvplus::Row
//   Row.HasColumn/SelectValues/...      :62-161  free functions of the same names
//   type DataSource func(RowFunc) error  :215    csvplus::DataSource
//   TakeRows / Take                    :218,:252 csvplus::TakeRows / Take
//   DataSource.IndexOn / UniqueIndexOn :529,:535 DataSource::IndexOn / UniqueIndexOn
//   DataSource.Join / Except           :545,:588 DataSource::Join / Except
//   DataSource.Filter / TakeWhile / DropWhile / Top / Drop :276-374  DataSource::Filter / TakeWhile / DropWhile (over a
//                                                declarative csvplus::Pred, evaluated on the GPU) / Top / Drop
//   Like / All / Any / Not           :1243-1293  csvplus::Like / All / Any / Not (plain data, also callable on a Row)
//   DataSource.Map                     :290-296  DataSource::Map over csvplus::Set(name, literal or Format{...}): a row
//                                                template instead of a closure, rendered on the GPU (cph_map_format);
//                                                Fixed(expr, prec) / Shortest(expr, fmt) / Itoa(expr): an Expr's value
//                                                (cph_num_eval);
//                                                Set(name, Switch({Case(pred, Format)...}, otherwise)) / When(pred, then,
//                                                otherwise): the `if` inside the closure — the template of the first case
//                                                whose Pred holds (cph_map_switch)
//   DataSource.Validate                :300-310  DataSource::Validate(pred, message): a declarative Pred instead of a closure
//   DataSource.Transform               :262-272  no entry of its own: it is the composition of Map, Filter and Validate
//   Row.ValueAsInt / ValueAsFloat64  :165-205    csvplus::ValueAsInt / ValueAsFloat64 (one row, on the host);
//                                                DataSource::ColumnAsInt / ColumnAsFloat64 (a whole column, on the GPU);
//                                                csvplus::IntCmp / FloatCmp: `v, err := row.ValueAsInt(c); err == nil && v REL k`
//                                                as a predicate that composes with Like / All / Any / Not;
//                                                csvplus::ExprCmp(lhs, REL, rhs): two numeric expressions compared (`price(r) *
//                                                float64(qty(r)) >= 100`, `died(r) > born(r)`); csvplus::ColCmp(a, REL, b): two
//                                                columns of a row compared as strings (`r["ship"] != r["bill"]`)
//   time.Parse(time.RFC3339, row[c])   (closures) DataSource::ColumnAsTime / ColumnAsTimeNano (t.Unix() / t.UnixNano() of a whole
//                                                column, on the GPU); csvplus::TimeCmp(c, REL, "2016-09-14T00:00:00Z"): instants, not
//                                                bytes; Rfc3339(expr or Col, zone_minutes) as a Format part: Unix seconds written
//                                                back as RFC 3339; ParseRfc3339 / FormatRfc3339 (one value, on the host)
//   Index.Iterate / Find / SubIndex    :618-641  Index::Iterate / Find / SubIndex
//   Index.ResolveDuplicates            :643-653  Index::ResolveDuplicates (groups found on the GPU)
//   Index.WriteTo / LoadIndex          :655-705  Index::WriteTo / LoadIndex (own binary format, not gob)
//   DataSourceError                   :1229-1238 csvplus::DataSourceError
//
// Go `error` values become csvplus::Error (nil == ok()); Go panics (programmer errors:
// empty / duplicate column lists, too many join columns, :710, :715, :549, :634) become
// csvplus::Panic exceptions.  io.EOF keeps its role: returned from a RowFunc it stops the
// iteration cleanly (:213-214, :238-239).
//
// What runs where: rows stay host-side maps exactly as in the reference; the key columns of
// a batch are staged into pinned SoA buffers and the sort / unique check / probe run on the
// GPU.  There is no CPU implementation of those steps here.
//
// Chained Joins (round 4): `src.Join(a, ka).Join(b, kb)...` (README.md:56; csvplus.go:545-569 nested: the second Join's
// source IS the first Join's closure) is recognised — a DataSource returned by Join remembers its upstream and its steps
// — and a batch of stream rows goes through ONE cph_join_chain_ex(CPH_CHAIN_POSITIONS) call, the entry point bench.py
// times, as long as every row of the batch carries the later steps' key columns itself: mergeRows
// lets the stream's value win, so that is the value the later Join sees.  Round 5: a later key that NO stream row of the
// batch carries but every row of an earlier index does — people.Join(orders, "id").DropColumns(...).Join(products),
// csvplus_test.go:280-285: prod_id is a column of the orders index rows — is fused too: the step names its source
// (cph_chain_step.source) and the device gathers the key from the row that earlier step matched.  DropColumns between the
// Joins of a chain is part of the chain (the columns are dropped when the merged row is built).  A batch whose rows
// disagree about where a key comes from runs the steps one after the other over the merged rows (same emission order,
// same errors).
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <locale.h>

#include "csvplus_hip.h"
#include "../csrc/span_device.hpp"   // the SPAN piece's routines: the host row model runs the code the kernels run

namespace csvplus {

// ---- errors ------------------------------------------------------------------------------------
class Error {
public:
    Error() = default;                                        // nil
    explicit Error(std::string msg) : set_(true), msg_(std::move(msg)) {}
    static Error Eof() { Error e("EOF"); e.eof_ = true; return e; }   // io.EOF
    bool ok() const { return !set_; }
    bool is_eof() const { return set_ && eof_; }
    explicit operator bool() const { return set_; }           // `if (err)` == `if err != nil`
    const std::string& message() const { return msg_; }       // err.Error()
    // DataSourceError (:1229-1238)
    bool is_data_source_error() const { return has_line_; }
    uint64_t line() const { return line_; }
    static Error DataSourceError(uint64_t line, const Error& inner) {
        Error e("row " + std::to_string(line) + ": " + inner.message());
        e.has_line_ = true;
        e.line_ = line;
        return e;
    }

private:
    bool set_ = false, eof_ = false, has_line_ = false;
    uint64_t line_ = 0;
    std::string msg_;
};
inline const Error io_EOF = Error::Eof();

struct Panic : std::logic_error {   // Go panic(...)
    using std::logic_error::logic_error;
};

// ---- Row (:59) -----------------------------------------------------------------------------------
using Row = std::map<std::string, std::string>;

inline bool HasColumn(const Row& row, const std::string& col) { return row.count(col) != 0; }   // :62-65

inline std::string quote(const std::string& s) { return "\"" + s + "\""; }   // %q for plain names

// SelectValues (:138-150)
inline Error SelectValues(const Row& row, const std::vector<std::string>& cols, std::vector<const std::string*>* out) {
    out->resize(cols.size());
    for (size_t i = 0; i < cols.size(); i++) {
        auto it = row.find(cols[i]);
        if (it == row.end()) return Error("missing column " + quote(cols[i]));
        (*out)[i] = &it->second;
    }
    return Error();
}

// SelectExisting (:108-118)
inline Row SelectExisting(const Row& row, const std::vector<std::string>& cols) {
    Row r;
    for (const auto& name : cols) {
        auto it = row.find(name);
        if (it != row.end()) r[name] = it->second;
    }
    return r;
}

// Row.String (:90-104): `{ "a" : "1", "b" : "2" }`, columns sorted
inline std::string String(const Row& row) {
    if (row.empty()) return "{}";
    std::string s = "{ ";
    bool first = true;
    for (const auto& kv : row) {   // std::map iterates in sorted key order == Header()
        if (!first) s += ", ";
        first = false;
        s += "\"" + kv.first + "\" : \"" + kv.second + "\"";
    }
    return s + " }";
}

// mergeRows (:571-583): index row first, then the stream row: the stream wins on a name collision
inline Row mergeRows(const Row& left, const Row& right) {
    Row r = left;
    for (const auto& kv : right) r[kv.first] = kv.second;
    return r;
}

// ---- the named predicates (:1243-1293) as DATA ---------------------------------------------------------------------------
// A Go closure cannot run on a GPU; Like / All / Any / Not are declarative and can: DataSource::Filter / TakeWhile / DropWhile
// compile a Pred to the postfix program of cph_filter_rows.  A Pred is also callable on a Row (the reference's semantics on
// the host), so it fits wherever a std::function<bool(const Row&)> is wanted.
enum Rel { LT = 0, LE = 1, EQ = 2, NE = 3, GE = 4, GT = 5 };   // the order of CPH_PRED_INT_LT.. / CPH_PRED_FLT_LT..

// Row.ValueAsInt (:165-183) / Row.ValueAsFloat64 (:187-205) on the host: strconv.Atoi / strconv.ParseFloat as the header's
// cph_col_to_number comment restates them.  Returns CPH_NUM_*; *out = what Go returns beside the error.
inline int32_t Atoi(const std::string& s, int64_t* out) {
    *out = 0;
    size_t i = 0;
    const bool neg = !s.empty() && s[0] == '-';
    if (!s.empty() && (s[0] == '+' || s[0] == '-')) i = 1;
    if (i == s.size()) return CPH_NUM_ERR_SYNTAX;
    uint64_t n = 0;
    for (; i < s.size(); i++) {
        const unsigned d = (unsigned char)s[i] - (unsigned)'0';
        if (d > 9) return CPH_NUM_ERR_SYNTAX;
        const uint64_t n10 = n * 10u, n1 = n10 + d;
        if (n > UINT64_MAX / 10u || n1 < n10) {
            *out = neg ? INT64_MIN : INT64_MAX;
            return CPH_NUM_ERR_RANGE;
        }
        n = n1;
    }
    if (neg ? n > (1ull << 63) : n >= (1ull << 63)) {
        *out = neg ? INT64_MIN : INT64_MAX;
        return CPH_NUM_ERR_RANGE;
    }
    *out = neg ? (int64_t)(0ull - n) : (int64_t)n;
    return CPH_NUM_OK;
}
inline int32_t ParseFloat(const std::string& s, double* out) {
    *out = 0.0;
    if (s.empty()) return CPH_NUM_ERR_SYNTAX;
    size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
    const bool neg = s[0] == '-';
    if (s.find('_') != std::string::npos || (s.size() - i >= 2 && s[i] == '0' && (s[i + 1] | 0x20) == 'x')) return CPH_NUM_ERR_UNSUPPORTED;
    std::string low = s.substr(i);
    for (char& c : low)
        if (c >= 'A' && c <= 'Z') c = (char)(c | 0x20);
    if (low == "inf" || low == "infinity") {
        *out = neg ? -HUGE_VAL : HUGE_VAL;
        return CPH_NUM_OK;
    }
    if (i == 0 && low == "nan") {
        *out = std::nan("");
        return CPH_NUM_OK;
    }
    size_t j = i, digits = 0;
    while (j < s.size() && s[j] >= '0' && s[j] <= '9') j++, digits++;
    if (j < s.size() && s[j] == '.') {
        j++;
        while (j < s.size() && s[j] >= '0' && s[j] <= '9') j++, digits++;
    }
    if (!digits) return CPH_NUM_ERR_SYNTAX;
    if (j < s.size() && (s[j] | 0x20) == 'e') {
        j++;
        if (j < s.size() && (s[j] == '+' || s[j] == '-')) j++;
        if (j >= s.size() || s[j] < '0' || s[j] > '9') return CPH_NUM_ERR_SYNTAX;
        while (j < s.size() && s[j] >= '0' && s[j] <= '9') j++;
    }
    if (j != s.size()) return CPH_NUM_ERR_SYNTAX;
    static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    *out = c_locale ? strtod_l(s.c_str(), nullptr, c_locale) : strtod(s.c_str(), nullptr);   // correctly rounded (glibc)
    return std::isinf(*out) ? CPH_NUM_ERR_RANGE : CPH_NUM_OK;
}
// the reference's message for a value that does not convert (:176 / :198); err = CPH_NUM_ERR_*
inline std::string conversionError(const std::string& column, const std::string& value, int32_t kind, int32_t err) {
    const char* what = err == CPH_NUM_ERR_SYNTAX  ? "invalid syntax"
                       : err == CPH_NUM_ERR_RANGE ? "value out of range"
                                                  : "not decided by this library (digit separators, hexadecimal floats)";
    if (kind == CPH_NUM_TIME_UNIX || kind == CPH_NUM_TIME_UNIXNANO)
        return "column " + quote(column) + ": cannot convert " + quote(value) + " to time: " +
               (err == CPH_NUM_ERR_SYNTAX  ? "invalid syntax"
                : err == CPH_NUM_ERR_RANGE ? "a field out of range"
                                           : "not decided by this library (one-digit hour, ',' fraction, more than 9 fraction digits, zone beyond 23:59, UnixNano overflow)");
    return "column " + quote(column) + ": cannot convert " + quote(value) + " to " + (kind == CPH_NUM_INT64 ? "integer" : "float") + ": " + what;
}
// strconv.FormatFloat(v, 'f', prec, 64) on the host: glibc's exact "%.*f" and Go's spellings of NaN and the infinities
inline std::string FormatFixed(double v, int prec) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-Inf" : "+Inf";
    std::string out((size_t)snprintf(nullptr, 0, "%.*f", prec, v), '\0');
    snprintf(&out[0], out.size() + 1, "%.*f", prec, v);
    return out;
}

// `t, err := time.Parse(time.RFC3339, s)` then t.Unix() (nano false: whole seconds, the floor) or t.UnixNano() on the host, by the
// rules of the header's cph_col_to_number comment (CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO): returns CPH_NUM_*, *out = 0 at an error.
inline int64_t DaysFromCivil(int64_t y, int64_t m, int64_t d) {   // days since 1970-01-01, proleptic Gregorian
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400, yoe = y - era * 400;
    const int64_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
    return era * 146097 + yoe * 365 + yoe / 4 - yoe / 100 + doy - 719468;
}
inline int32_t ParseRfc3339(const std::string& s, bool nano, int64_t* out) {
    *out = 0;
    size_t i = 0;
    bool relaxed = false;
    auto digit = [&](size_t at) { return at < s.size() && s[at] >= '0' && s[at] <= '9'; };
    auto number = [&](size_t n, int64_t* v) {   // exactly n digits at i
        *v = 0;
        for (size_t k = 0; k < n; k++, i++) {
            if (!digit(i)) return false;
            *v = *v * 10 + (s[i] - '0');
        }
        return true;
    };
    auto byte = [&](char c) { return i < s.size() && s[i] == c ? (i++, true) : false; };
    int64_t year, month, day, hour, minute, second, frac = 0, zh = 0, zm = 0, sign = 1;
    if (!number(4, &year) || !byte('-') || !number(2, &month) || !byte('-') || !number(2, &day) || !byte('T')) return CPH_NUM_ERR_SYNTAX;
    if (digit(i) && !digit(i + 1)) {   // the hour written with one digit: not decided
        relaxed = true;
        number(1, &hour);
    } else if (!number(2, &hour)) {
        return CPH_NUM_ERR_SYNTAX;
    }
    if (!byte(':') || !number(2, &minute) || !byte(':') || !number(2, &second)) return CPH_NUM_ERR_SYNTAX;
    if (i < s.size() && (s[i] == '.' || s[i] == ',')) {
        relaxed = relaxed || s[i] == ',';
        i++;
        size_t nd = 0;
        for (; digit(i); i++, nd++)
            if (nd < 9) frac = frac * 10 + (s[i] - '0');
        if (nd == 0) return CPH_NUM_ERR_SYNTAX;
        relaxed = relaxed || nd > 9;
        for (; nd < 9; nd++) frac *= 10;
    }
    if (byte('Z')) {
        if (i != s.size()) return CPH_NUM_ERR_SYNTAX;
    } else {
        if (i >= s.size() || (s[i] != '+' && s[i] != '-')) return CPH_NUM_ERR_SYNTAX;
        sign = s[i++] == '-' ? -1 : 1;
        if (!number(2, &zh) || !byte(':') || !number(2, &zm) || i != s.size()) return CPH_NUM_ERR_SYNTAX;
    }
    if (relaxed) return CPH_NUM_ERR_UNSUPPORTED;
    static const int mdays[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    const bool leap = (year % 4 == 0 && year % 100 != 0) || year % 400 == 0;
    if (month < 1 || month > 12 || day < 1 || day > mdays[month - 1] + (month == 2 && leap) || hour > 23 || minute > 59 || second > 59)
        return CPH_NUM_ERR_RANGE;
    if (zh > 23 || zm > 59) return CPH_NUM_ERR_UNSUPPORTED;
    const int64_t secs = DaysFromCivil(year, month, day) * 86400 + hour * 3600 + minute * 60 + second - sign * (zh * 3600 + zm * 60);
    if (!nano) {
        *out = secs;
        return CPH_NUM_OK;
    }
    const __int128 ns = (__int128)secs * 1000000000 + frac;
    if (ns < (__int128)INT64_MIN || ns > (__int128)INT64_MAX) return CPH_NUM_ERR_UNSUPPORTED;
    *out = (int64_t)ns;
    return CPH_NUM_OK;
}
// strconv.FormatFloat(v, fmt, -1, 64) on the host for fmt 'e' 'E' 'f' 'g' 'G': the shortest round-trip digits from std::to_chars,
// laid out by Go's rules (strconv/ftoa.go: %e, %f, and 'g' choosing %e when the exponent is below -4 or at least 6)
inline std::string FormatShortest(double v, char fmt) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-Inf" : "+Inf";
    char buf[40];
    const auto res = std::to_chars(buf, buf + sizeof buf, std::fabs(v), std::chars_format::scientific);   // d[.ddd]e±XX[X]
    std::string sci(buf, res.ptr), digits;
    const size_t epos = sci.find('e');
    for (size_t i = 0; i < epos; i++)
        if (sci[i] != '.') digits.push_back(sci[i]);
    const int exp = atoi(sci.c_str() + epos + 1), nd = (int)digits.size(), dp = exp + 1;
    const std::string sign = std::signbit(v) ? "-" : "";
    if (fmt == 'e' || fmt == 'E' || (fmt != 'f' && (exp < -4 || exp >= 6))) {
        if (fmt == 'E' || fmt == 'G') sci[epos] = 'E';
        return sign + sci;
    }
    if (dp <= 0) return sign + "0." + std::string((size_t)-dp, '0') + digits;
    if (dp < nd) return sign + digits.substr(0, (size_t)dp) + "." + digits.substr((size_t)dp);
    return sign + digits + std::string((size_t)(dp - nd), '0');
}

// time.Unix(v, 0).In(time.FixedZone("", 60 * zone)).Format(time.RFC3339) on the host; false where the local year leaves 0000..9999
inline bool FormatRfc3339(int64_t v, int zone, std::string* out) {
    if (v < -62167219200ll - 86400 || v > 253402300799ll + 86400) return false;
    const int64_t local = v + 60ll * zone;
    if (local < -62167219200ll || local > 253402300799ll) return false;
    int64_t days = local / 86400, sod = local % 86400;
    if (sod < 0) sod += 86400, days--;
    int64_t z = days + 719468;   // civil from days
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097, doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365, doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153, d = doy - (153 * mp + 2) / 5 + 1, m = mp < 10 ? mp + 3 : mp - 9, y = yoe + era * 400 + (m <= 2);
    char buf[40];
    int len = snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02d", (int)y, (int)m, (int)d, (int)(sod / 3600), (int)(sod / 60 % 60), (int)(sod % 60));
    if (zone == 0) len += snprintf(buf + len, sizeof buf - (size_t)len, "Z");
    else len += snprintf(buf + len, sizeof buf - (size_t)len, "%c%02d:%02d", zone < 0 ? '-' : '+', std::abs(zone) / 60, std::abs(zone) % 60);
    out->assign(buf, (size_t)len);
    return true;
}

class Expr;
class Pred {
public:
    enum Kind { kLike, kNot, kAll, kAny, kIntCmp, kFloatCmp, kStrCmp, kHasPrefix, kHasSuffix, kContains, kTimeCmp, kExprCmp, kColCmp };
    bool operator()(const Row& row) const {
        switch (kind_) {
            case kExprCmp: return exprHolds(row);   // a row that lacks a column, or in which an op fails, is false under every relation
            case kColCmp: {                         // bytes, as kStrCmp; a row without either column is false under every relation
                auto a = row.find(column_), b = row.find(slit_);
                return a != row.end() && b != row.end() && holds(a->second.compare(b->second), 0);
            }
            case kTimeCmp: {   // a row without the column, or whose stamp does not convert, is false under every relation
                auto it = row.find(column_);
                int64_t v;
                return it != row.end() && ParseRfc3339(it->second, false, &v) == CPH_NUM_OK && holds(v, ilit_);
            }
            case kStrCmp:
            case kHasPrefix:
            case kHasSuffix:
            case kContains: {   // byte operations, as Go's; a row without the column is false under every one of them, NE included
                auto it = row.find(column_);
                if (it == row.end()) return false;
                const std::string& v = it->second;
                if (kind_ == kStrCmp) return holds(v.compare(slit_), 0);   // char_traits<char>::compare: bytewise, unsigned, the shorter first
                if (slit_.size() > v.size()) return false;
                if (kind_ == kHasPrefix) return v.compare(0, slit_.size(), slit_) == 0;
                if (kind_ == kHasSuffix) return v.compare(v.size() - slit_.size(), slit_.size(), slit_) == 0;
                return v.find(slit_) != std::string::npos;
            }
            case kIntCmp:
            case kFloatCmp: {   // a row without the column, or whose value does not convert, is false under every relation
                auto it = row.find(column_);
                if (it == row.end()) return false;
                if (kind_ == kIntCmp) {
                    int64_t v;
                    return Atoi(it->second, &v) == CPH_NUM_OK && holds(v, ilit_);
                }
                double v;
                return ParseFloat(it->second, &v) == CPH_NUM_OK && holds(v, flit_);
            }
            case kLike:
                for (const auto& kv : match_) {                                             // :1285-1289
                    auto it = row.find(kv.first);
                    if (it == row.end() || it->second != kv.second) return false;
                }
                return true;
            case kNot: return !kids_[0](row);
            case kAll:
                for (const auto& k : kids_)
                    if (!k(row)) return false;
                return true;
            default:
                for (const auto& k : kids_)
                    if (k(row)) return true;
                return false;
        }
    }
    Kind kind() const { return kind_; }
    const Row& match() const { return match_; }
    const std::vector<Pred>& operands() const { return kids_; }
    const std::string& column() const { return column_; }
    Rel rel() const { return rel_; }
    const void* literal() const { return kind_ == kIntCmp ? (const void*)&ilit_ : (const void*)&flit_; }   // 8 bytes
    const std::string& text() const { return slit_; }   // kStrCmp .. kContains: the literal's bytes; kColCmp: the second column's name
    const Expr& lhs() const { return *lhs_; }           // kExprCmp
    const Expr& rhs() const { return *rhs_; }

private:
    template <class T>
    bool holds(T v, T k) const {
        switch (rel_) {
            case LT: return v < k;
            case LE: return v <= k;
            case EQ: return v == k;
            case NE: return v != k;
            case GE: return v >= k;
            default: return v > k;
        }
    }
    friend Pred IntCmp(std::string column, Rel rel, int64_t k);
    friend Pred FloatCmp(std::string column, Rel rel, double x);
    friend Pred StrCmp(std::string column, Rel rel, std::string literal);
    friend Pred StrTest(Pred::Kind kind, std::string column, std::string literal);
    friend Pred TimeCmp(std::string column, Rel rel, std::string literal);
    friend Pred ExprCmp(Expr lhs, Rel rel, Expr rhs);
    friend Pred ColCmp(std::string a, Rel rel, std::string b);
    bool exprHolds(const Row& row) const;   // defined behind Expr
    std::shared_ptr<const Expr> lhs_, rhs_;
    std::string column_, slit_;
    Rel rel_ = EQ;
    int64_t ilit_ = 0;
    double flit_ = 0.0;
    friend Pred Like(Row match);
    friend Pred Not(Pred p);
    friend Pred All(std::vector<Pred> preds);
    friend Pred Any(std::vector<Pred> preds);
    Kind kind_ = kAll;
    Row match_;
    std::vector<Pred> kids_;
};
inline Pred Like(Row match) {
    if (match.empty()) throw Panic("empty match row in Like() predicate");                // :1280-1282
    Pred p;
    p.kind_ = Pred::kLike;
    p.match_ = std::move(match);
    return p;
}
inline Pred IntCmp(std::string column, Rel rel, int64_t k) {
    Pred p;
    p.kind_ = Pred::kIntCmp;
    p.column_ = std::move(column);
    p.rel_ = rel;
    p.ilit_ = k;
    return p;
}
inline Pred FloatCmp(std::string column, Rel rel, double x) {
    Pred p;
    p.kind_ = Pred::kFloatCmp;
    p.column_ = std::move(column);
    p.rel_ = rel;
    p.flit_ = x;
    return p;
}
// Conditions that look INSIDE a string, as data: StrCmp("ts", GE, "2016-09") is `row["ts"] >= "2016-09"`, HasPrefix / HasSuffix /
// Contains are strings.HasPrefix / HasSuffix / Contains — all byte operations.  On the device each of them also checks that the
// row HAS the column (a staged presence flag), so one such term costs two of the 32 terms and its column two of the 16 columns.
inline Pred StrCmp(std::string column, Rel rel, std::string literal) {
    Pred p;
    p.kind_ = Pred::kStrCmp;
    p.column_ = std::move(column);
    p.rel_ = rel;
    p.slit_ = std::move(literal);
    return p;
}
inline Pred StrTest(Pred::Kind kind, std::string column, std::string literal) {
    Pred p;
    p.kind_ = kind;
    p.column_ = std::move(column);
    p.slit_ = std::move(literal);
    return p;
}
// TimeCmp("ts", GE, "2016-09-14T00:00:00Z") is `t, err := time.Parse(time.RFC3339, row["ts"]); err == nil && t.Unix() >= u.Unix()`:
// instants, not bytes — two stamps of one instant in different zones are equal.  The literal is RFC 3339 text without a fraction
// (the term compares whole seconds); anything else panics here, as the C ABI would refuse it.
inline Pred TimeCmp(std::string column, Rel rel, std::string literal) {
    Pred p;
    p.kind_ = Pred::kTimeCmp;
    p.column_ = std::move(column);
    p.rel_ = rel;
    if (ParseRfc3339(literal, false, &p.ilit_) != CPH_NUM_OK) throw Panic("TimeCmp(): the literal is no RFC 3339 timestamp this library converts");
    if (literal.find('.') != std::string::npos) throw Panic("TimeCmp(): the literal has a fraction (the term compares whole seconds)");
    p.slit_ = std::move(literal);
    return p;
}
// ColCmp("ship_city", NE, "bill_city") is `row["ship_city"] != row["bill_city"]`: StrCmp's byte comparison with the second column's
// value in the literal's place.  On the device it is AND-ed with the presence flags of both columns (see StrCmp): three terms.
inline Pred ColCmp(std::string a, Rel rel, std::string b) {
    Pred p;
    p.kind_ = Pred::kColCmp;
    p.column_ = std::move(a);
    p.rel_ = rel;
    p.slit_ = std::move(b);
    return p;
}
inline Pred HasPrefix(std::string column, std::string literal) { return StrTest(Pred::kHasPrefix, std::move(column), std::move(literal)); }
inline Pred HasSuffix(std::string column, std::string literal) { return StrTest(Pred::kHasSuffix, std::move(column), std::move(literal)); }
inline Pred Contains(std::string column, std::string literal) { return StrTest(Pred::kContains, std::move(column), std::move(literal)); }
inline Pred Not(Pred q) {
    Pred p;
    p.kind_ = Pred::kNot;
    p.kids_.push_back(std::move(q));
    return p;
}
inline Pred All(std::vector<Pred> preds = {}) {
    Pred p;
    p.kind_ = Pred::kAll;
    p.kids_ = std::move(preds);
    return p;
}
inline Pred Any(std::vector<Pred> preds = {}) {
    Pred p;
    p.kind_ = Pred::kAny;
    p.kids_ = std::move(preds);
    return p;
}
template <class... P>
inline Pred All(const Pred& first, const P&... more) { return All(std::vector<Pred>{first, more...}); }
template <class... P>
inline Pred Any(const Pred& first, const P&... more) { return Any(std::vector<Pred>{first, more...}); }

// ---- Map (:290-296) as DATA ----------------------------------------------------------------------------------------------
// `row["name"] = "Julia"` is Set("name", "Julia"); `row["full"] = row["name"] + " " + row["surname"]` is
// Set("full", Format({Col("name"), " ", Col("surname")})).  A row that lacks a Col's column takes the Col's default
// (Row.SafeGetValue, :69-75); without a default the iteration ends with the reference's `missing column` error at that row.
// Fixed(Col("price"), 2) is the column's value read as Row.ValueAsFloat64 reads it and written back as
// strconv.FormatFloat(v, 'f', 2, 64) writes it (prec 0..22; a finite value of 2^128 or more is refused by the device); a value
// that does not parse ends the iteration at that row with ValueAsFloat64's error.  Arithmetic between columns is an Expr:
// Fixed(AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))), 2) is the reference's amount column (csvplus_test.go:1404-1412),
// Itoa(expr) writes an integer expression as strconv.Itoa does.
struct Col {
    std::string name, fallback;
    bool has_default = false;
    explicit Col(std::string n) : name(std::move(n)) {}
    Col(std::string n, std::string dflt) : name(std::move(n)), fallback(std::move(dflt)), has_default(true) {}
};

// ---- numeric expressions as DATA (cph_num_eval) ---------------------------------------------------------------------------
// `price * float64(qty)` of the reference's closures, as a value: AsInt(Col) / AsFloat64(Col) read a column as Row.ValueAsInt /
// Row.ValueAsFloat64 do, literals are C++ integers (int64) and doubles (float64), Float64(e) / Int(e) are Go's conversions, and
// + - * / % and unary - are Go's operators: no implicit conversions (mixing the types is a Panic when the expression is built),
// int64 wraps, / truncates toward zero, % has the dividend's sign, INT64_MIN / -1 == INT64_MIN; every float op is one IEEE
// operation, never fused.  A zero integer divisor and an Int() of a NaN or of a value outside [-2^63, 2^63) are errors of
// their row, like a value that does not convert; the first failing op in program order decides (include/csvplus_hip.h).
class Expr {
public:
    struct Op {
        int32_t op = 0;     // CPH_EXPR_*
        int32_t arg = 0;    // COL_*: index into cols
        bool flt = false;   // NEG and the binary ops: float64 operands
        int64_t i = 0;
        double f = 0;
    };
    std::vector<Op> ops;        // postfix
    std::vector<Col> cols;      // the columns read, in order of first use
    int32_t kind = 0;           // CPH_NUM_INT64 / CPH_NUM_FLOAT64: the result's type

    Expr(int v) : Expr((long long)v) {}    // NOLINT: implicit, so that `AsInt(Col("qty")) * 2` reads like the expression
    Expr(long v) : Expr((long long)v) {}   // NOLINT
    Expr(long long v) : kind(CPH_NUM_INT64) {   // NOLINT
        Op o;
        o.op = CPH_EXPR_LIT_INT;
        o.i = (int64_t)v;
        ops.push_back(o);
    }
    Expr(double v) : kind(CPH_NUM_FLOAT64) {   // NOLINT
        Op o;
        o.op = CPH_EXPR_LIT_FLT;
        o.f = v;
        ops.push_back(o);
    }
    static Expr column(Col c, bool flt) {
        Expr e(0);
        e.ops[0].op = flt ? CPH_EXPR_COL_FLT : CPH_EXPR_COL_INT;
        e.kind = flt ? CPH_NUM_FLOAT64 : CPH_NUM_INT64;
        e.cols.push_back(std::move(c));
        return e;
    }
    static Expr unary(int32_t op, Expr x) {
        if (op == CPH_EXPR_TO_FLT && x.kind != CPH_NUM_INT64) throw Panic("Float64() of a float64 expression");
        if (op == CPH_EXPR_TO_INT && x.kind != CPH_NUM_FLOAT64) throw Panic("Int() of an int64 expression");
        Op o;
        o.op = op;
        o.flt = x.kind == CPH_NUM_FLOAT64;
        x.ops.push_back(o);
        x.kind = op == CPH_EXPR_TO_FLT ? CPH_NUM_FLOAT64 : op == CPH_EXPR_TO_INT ? CPH_NUM_INT64 : x.kind;
        x.check();
        return x;
    }
    static Expr binary(int32_t op, Expr a, const Expr& b) {
        if (a.kind != b.kind) throw Panic("mismatched types int64 and float64 in an expression (there are no implicit conversions)");
        if (op == CPH_EXPR_MOD && a.kind != CPH_NUM_INT64) throw Panic("operator % on float64 expressions");
        for (Op o : b.ops) {
            if (o.op == CPH_EXPR_COL_INT || o.op == CPH_EXPR_COL_FLT) {
                const Col& c = b.cols[(size_t)o.arg];
                size_t k = 0;
                while (k < a.cols.size() && a.cols[k].name != c.name) k++;
                if (k == a.cols.size()) a.cols.push_back(c);
                o.arg = (int32_t)k;
            }
            a.ops.push_back(o);
        }
        Op o;
        o.op = op;
        o.flt = a.kind == CPH_NUM_FLOAT64;
        a.ops.push_back(o);
        a.check();
        return a;
    }
    // the expression on one row, on the host (what the device computes for a whole batch).  Returns CPH_NUM_*: the status
    // of the first failing op, whose index goes to *bad_op; -1 with *missing set for a row that lacks a column without default.
    int32_t eval(const Row& row, int64_t* iv, double* fv, int* bad_op, std::string* missing) const {
        int64_t si[CPH_EXPR_MAX_STACK] = {};
        double sf[CPH_EXPR_MAX_STACK] = {};
        int sp = 0, bad = -1;
        int32_t status = CPH_NUM_OK;
        for (size_t q = 0; q < ops.size(); q++) {
            const Op& o = ops[q];
            int32_t st = CPH_NUM_OK;
            switch (o.op) {
                case CPH_EXPR_COL_INT:
                case CPH_EXPR_COL_FLT: {
                    const Col& c = cols[(size_t)o.arg];
                    auto it = row.find(c.name);
                    const std::string* v = it != row.end() ? &it->second : c.has_default ? &c.fallback : nullptr;
                    if (!v) {
                        if (missing) *missing = c.name;
                        return -1;
                    }
                    st = o.op == CPH_EXPR_COL_INT ? Atoi(*v, &si[sp]) : ParseFloat(*v, &sf[sp]);
                    sp++;
                    break;
                }
                case CPH_EXPR_LIT_INT: si[sp++] = o.i; break;
                case CPH_EXPR_LIT_FLT: sf[sp++] = o.f; break;
                case CPH_EXPR_TO_FLT: sf[sp - 1] = (double)si[sp - 1]; break;
                case CPH_EXPR_TO_INT: {
                    const double v = sf[sp - 1];
                    const bool fits = v >= -9223372036854775808.0 && v < 9223372036854775808.0;   // false for a NaN
                    si[sp - 1] = fits ? (int64_t)v : 0;
                    if (!fits) st = CPH_NUM_ERR_CONVERT;
                    break;
                }
                case CPH_EXPR_NEG:
                    if (o.flt) sf[sp - 1] = -sf[sp - 1];
                    else si[sp - 1] = (int64_t)(0ull - (uint64_t)si[sp - 1]);
                    break;
                default: {
                    sp--;
                    if (o.flt) {
                        const double a = sf[sp - 1], b = sf[sp];
                        sf[sp - 1] = o.op == CPH_EXPR_ADD ? a + b : o.op == CPH_EXPR_SUB ? a - b : o.op == CPH_EXPR_MUL ? a * b : a / b;
                        break;
                    }
                    const uint64_t a = (uint64_t)si[sp - 1], b = (uint64_t)si[sp];
                    uint64_t r = 0;
                    if (o.op == CPH_EXPR_ADD) r = a + b;
                    else if (o.op == CPH_EXPR_SUB) r = a - b;
                    else if (o.op == CPH_EXPR_MUL) r = a * b;
                    else if (b == 0) st = CPH_NUM_ERR_DIV_ZERO;
                    else if (b == ~0ull) r = o.op == CPH_EXPR_DIV ? 0ull - a : 0ull;   // INT64_MIN / -1 wraps, % -1 is 0
                    else r = (uint64_t)(o.op == CPH_EXPR_DIV ? (int64_t)a / (int64_t)b : (int64_t)a % (int64_t)b);
                    si[sp - 1] = (int64_t)r;
                    break;
                }
            }
            if (st != CPH_NUM_OK && status == CPH_NUM_OK) status = st, bad = (int)q;
        }
        if (bad_op) *bad_op = bad;
        if (iv) *iv = status == CPH_NUM_OK ? si[0] : 0;
        if (fv) *fv = status == CPH_NUM_OK ? sf[0] : 0.0;
        return status;
    }
    // the message of a row whose op `op` failed with `status`; value(column index) = the row's value of that column
    std::string errorText(int32_t status, int op, const std::function<std::string(size_t)>& value) const {
        const Op& o = ops[(size_t)op];
        if (o.op == CPH_EXPR_COL_INT || o.op == CPH_EXPR_COL_FLT)
            return conversionError(cols[(size_t)o.arg].name, value((size_t)o.arg), o.op == CPH_EXPR_COL_INT ? CPH_NUM_INT64 : CPH_NUM_FLOAT64, status);
        return status == CPH_NUM_ERR_DIV_ZERO ? "integer divide by zero" : "float64 value does not fit an int64";
    }
    std::string errorText(int32_t status, int op, const Row& row) const {
        return errorText(status, op, [&](size_t c) {
            auto it = row.find(cols[c].name);
            return it != row.end() ? it->second : cols[c].fallback;
        });
    }

private:
    void check() const {   // the ABI's limits
        if (ops.size() > (size_t)CPH_EXPR_MAX_OPS) throw Panic("expression of more than 32 ops");
        if (cols.size() > (size_t)CPH_MAX_KEY_COLS) throw Panic("expression over more than 16 columns");
        int sp = 0;
        for (const Op& o : ops) {
            if (o.op <= CPH_EXPR_LIT_FLT) sp++;
            else if (o.op >= CPH_EXPR_ADD) sp--;
            if (sp > CPH_EXPR_MAX_STACK) throw Panic("expression needs a stack deeper than 8");
        }
    }
};
inline Expr AsInt(Col c) { return Expr::column(std::move(c), false); }       // row.ValueAsInt(name)
inline Expr AsFloat64(Col c) { return Expr::column(std::move(c), true); }    // row.ValueAsFloat64(name)
inline Expr Float64(Expr e) { return Expr::unary(CPH_EXPR_TO_FLT, std::move(e)); }   // float64(x)
inline Expr Int(Expr e) { return Expr::unary(CPH_EXPR_TO_INT, std::move(e)); }       // int64(x)
inline Expr operator-(Expr e) { return Expr::unary(CPH_EXPR_NEG, std::move(e)); }
inline Expr operator+(Expr a, const Expr& b) { return Expr::binary(CPH_EXPR_ADD, std::move(a), b); }
inline Expr operator-(Expr a, const Expr& b) { return Expr::binary(CPH_EXPR_SUB, std::move(a), b); }
inline Expr operator*(Expr a, const Expr& b) { return Expr::binary(CPH_EXPR_MUL, std::move(a), b); }
inline Expr operator/(Expr a, const Expr& b) { return Expr::binary(CPH_EXPR_DIV, std::move(a), b); }
inline Expr operator%(Expr a, const Expr& b) { return Expr::binary(CPH_EXPR_MOD, std::move(a), b); }

// ExprCmp(AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))), GE, 100.0) is `price(r) * float64(qty(r)) >= 100`, and
// ExprCmp(AsInt(Col("died")), GT, AsInt(Col("born"))) a column against a column as numbers: both sides of one type (mixing them is a
// Panic here, there are no implicit conversions), int64 compared signed, float64 as IEEE (with a NaN only NE holds).  A row in which
// any op fails — a value that does not convert, a zero divisor, an Int() out of range — or that lacks a column without default is
// false under every relation, NE included.  One term on the device (cph_filter_rows: CPH_PRED_EXPR_*), whatever the expressions.
inline Pred ExprCmp(Expr lhs, Rel rel, Expr rhs) {
    if (lhs.kind != rhs.kind) throw Panic("mismatched types int64 and float64 in ExprCmp() (there are no implicit conversions)");
    if (lhs.ops.size() + rhs.ops.size() > (size_t)CPH_EXPR_MAX_OPS) throw Panic("ExprCmp(): more than 32 ops on both sides together");
    Expr::binary(CPH_EXPR_SUB, lhs, rhs);   // the stack of rhs on top of lhs, and the columns of both: Panics beyond the ABI's limits
    Pred p;
    p.kind_ = Pred::kExprCmp;
    p.rel_ = rel;
    p.lhs_ = std::make_shared<const Expr>(std::move(lhs));
    p.rhs_ = std::make_shared<const Expr>(std::move(rhs));
    return p;
}
inline bool Pred::exprHolds(const Row& row) const {
    int64_t ai = 0, bi = 0;
    double af = 0, bf = 0;
    if (lhs_->eval(row, &ai, &af, nullptr, nullptr) != CPH_NUM_OK || rhs_->eval(row, &bi, &bf, nullptr, nullptr) != CPH_NUM_OK) return false;
    return lhs_->kind == CPH_NUM_INT64 ? holds(ai, bi) : holds(af, bf);
}

struct Fixed {
    Col col;
    int prec;
    std::shared_ptr<const Expr> expr;   // Fixed(expression, prec)
    Fixed(Col c, int p) : col(std::move(c)), prec(p) {
        if (p < 0 || p > 22) throw Panic("Fixed(): prec outside 0..22");
    }
    Fixed(Expr e, int p) : col(""), prec(p), expr(std::make_shared<const Expr>(std::move(e))) {
        if (p < 0 || p > 22) throw Panic("Fixed(): prec outside 0..22");
        if (expr->kind != CPH_NUM_FLOAT64) throw Panic("Fixed() of an int64 expression (use Itoa, or Float64)");
    }
};
// Shortest(Col("price"), 'g') is the column's value read as Row.ValueAsFloat64 reads it and written back as
// strconv.FormatFloat(v, fmt, -1, 64) writes it: the shortest digits that read back to the same float64, as 'e' / 'E', 'f' or
// 'g' / 'G' (a CPH_MAP_FLOAT64_SHORTEST piece).  Shortest(expression, fmt) writes a float64 expression's value.  No value is refused.
struct Shortest {
    Col col;
    char fmt;
    std::shared_ptr<const Expr> expr;
    static void check(char f) {
        if (f != 'e' && f != 'E' && f != 'f' && f != 'g' && f != 'G') throw Panic("Shortest(): fmt is none of 'e' 'E' 'f' 'g' 'G'");
    }
    Shortest(Col c, char f = 'g') : col(std::move(c)), fmt(f) { check(f); }
    Shortest(Expr e, char f = 'g') : col(""), fmt(f), expr(std::make_shared<const Expr>(std::move(e))) {
        check(f);
        if (expr->kind != CPH_NUM_FLOAT64) throw Panic("Shortest() of an int64 expression (use Itoa, or Float64)");
    }
};
struct Itoa {   // an int64 expression written as strconv.Itoa writes it
    std::shared_ptr<const Expr> expr;
    explicit Itoa(Expr e) : expr(std::make_shared<const Expr>(std::move(e))) {
        if (expr->kind != CPH_NUM_INT64) throw Panic("Itoa() of a float64 expression (use Fixed, or Int)");
    }
};
// Rfc3339(expr, zone_minutes) writes an int64 expression — Unix seconds, e.g. AsInt(Col("t")) / 3600 * 3600 — as
// time.Unix(v, 0).In(time.FixedZone("", 60 * zone_minutes)).Format(time.RFC3339) does: "...Z" for zone 0, "...+HH:MM" otherwise
// (a CPH_MAP_TIME piece).  Rfc3339(Col("t")) reads the column as ValueAsInt reads it.  A value whose local year leaves 0000..9999
// fails the Map with the library's message.
struct Rfc3339 {
    std::shared_ptr<const Expr> expr;
    int zone;
    explicit Rfc3339(Expr e, int zone_minutes = 0) : expr(std::make_shared<const Expr>(std::move(e))), zone(zone_minutes) {
        if (expr->kind != CPH_NUM_INT64) throw Panic("Rfc3339() of a float64 expression (Unix seconds are an int64: use Int)");
        if (zone < -1439 || zone > 1439) throw Panic("Rfc3339(): zone outside -1439..1439 minutes");
    }
    explicit Rfc3339(Col c, int zone_minutes = 0) : Rfc3339(AsInt(std::move(c)), zone_minutes) {}
};
// Substr(Col("ts"), 0, 10) is Go's `row["ts"][0:10]`: the bytes [from, to) of the column's value (of its default where the row
// lacks the column).  Python's slice rules: a negative index counts from the end, both ends are clamped into the value, from >=
// to gives "", to == INT64_MAX (the default) means "to the end".  One deviation from Go: an index out of range clamps, no panic.
struct SpanStep {   // one cph_span_op with its literal owned
    int32_t op, mode;
    int64_t a, b;
    std::string lit;
};
struct Span;
struct Substr {
    Col col;
    int64_t from, to;
    std::vector<SpanStep> pre;   // Substr(TrimSpace(col), 0, 10): the operations in front of the slice
    Substr(Col c, int64_t f, int64_t t = INT64_MAX) : col(std::move(c)), from(f), to(t) {}
    inline Substr(Span s, int64_t f, int64_t t = INT64_MAX);
    static std::string of(const std::string& v, int64_t from, int64_t to) {
        const int64_t l = (int64_t)v.size();
        const int64_t f = from < 0 ? (from + l < 0 ? 0 : from + l) : (from < l ? from : l);
        const int64_t t = to < 0 ? (to + l < 0 ? 0 : to + l) : (to < l ? to : l);
        return t > f ? v.substr((size_t)f, (size_t)(t - f)) : std::string();
    }
};
// A column's value NARROWED by a short program of span operations (CPH_MAP_SPAN): TrimSpace(Col("id")) is strings.TrimSpace,
// TrimLeft / TrimRight / Trim(col, cutset) strings.TrimLeft / TrimRight / Trim with an ASCII cutset of at most 32 bytes,
// TrimPrefix / TrimSuffix(col, lit) once and only if the literal is there, Field(col, sep, k, limit) is strings.Split(s, sep)[k]
// (limit -1) or strings.SplitN(s, sep, limit)[k] — k < 0 counts from the last part, an index outside the parts gives "" where
// Go panics — and Before / After(col, sep) are strings.Cut's two halves.  They nest, Substr included:
// Substr(TrimSpace(Col("ts")), 0, 10); at most 4 operations per part.  Accepted wherever a Part is.
struct Span {
    Col col;
    std::vector<SpanStep> ops;
    Span(Col c) : col(std::move(c)) {}   // NOLINT: implicit, so that the functions take a Col, a Substr or another Span
    Span(Substr s) : col(std::move(s.col)), ops(std::move(s.pre)) { ops.push_back(SpanStep{CPH_SPAN_SLICE, 0, s.from, s.to, ""}); }   // NOLINT
    Span then(SpanStep step) && {
        if (ops.size() >= (size_t)CPH_SPAN_MAX_OPS) throw Panic("more than 4 span operations on one column value");
        ops.push_back(std::move(step));
        return std::move(*this);
    }
    // the program on one value, on the host: span_device.hpp's routines over the value's bytes
    static std::string of(const std::vector<SpanStep>& steps, const std::string& v) {
        struct Value {
            const std::string& s;
            uint64_t operator()(uint64_t off, uint64_t len, int j) const {
                uint64_t w = 0;
                for (uint64_t k = 0; k < 8 && 8 * (uint64_t)j + k < len; k++) w |= (uint64_t)(uint8_t)s[(size_t)(off + 8 * (uint64_t)j + k)] << (8 * k);
                return w;
            }
        };
        struct Literal {
            const std::string& block;
            uint32_t off, len;
            uint64_t operator()(uint64_t j) const {
                uint64_t w = 0;
                for (uint64_t k = 0; k < 8 && 8 * j + k < len; k++) w |= (uint64_t)(uint8_t)block[(size_t)(off + 8 * j + k)] << (8 * k);
                return w;
            }
        };
        struct Literals {
            const std::string& block;
            Literal operator()(uint32_t off, uint32_t len) const { return Literal{block, off, len}; }
        };
        std::string block;
        std::vector<cph::SpanOp> ops;
        for (const SpanStep& st : steps) {
            cph::SpanOp o{};
            o.op = st.op, o.mode = st.mode, o.a = st.a;
            if (st.op == CPH_SPAN_SLICE) {
                o.b = st.b;
            } else if (st.op == CPH_SPAN_TRIM_CUTSET) {
                uint64_t set[2] = {0, 0};
                for (unsigned char c : st.lit) set[c >> 6] |= 1ull << (c & 63);
                o.a = (int64_t)set[0], o.b = (int64_t)set[1];
            } else if (st.op != CPH_SPAN_TRIM_SPACE) {
                o.lit_off = (uint32_t)block.size(), o.lit_len = (uint32_t)st.lit.size();
                block += st.lit;
            }
            ops.push_back(o);
        }
        uint64_t off = 0, len = 0;
        cph::span_run(ops.data(), (int)ops.size(), Value{v}, v.size(), Literals{block}, &off, &len);
        return v.substr((size_t)off, (size_t)len);
    }
};
inline Substr::Substr(Span s, int64_t f, int64_t t) : col(std::move(s.col)), from(f), to(t), pre(std::move(s.ops)) {
    if (pre.size() >= (size_t)CPH_SPAN_MAX_OPS) throw Panic("more than 4 span operations on one column value");
}
namespace detail {
inline std::string spanCutset(std::string cutset) {
    if (cutset.size() > (size_t)CPH_SPAN_MAX_CUTSET) throw Panic("a trim cutset of more than 32 bytes");
    for (unsigned char c : cutset)
        if (c >= 0x80) throw Panic("a trim cutset byte of 0x80 or above (only an ASCII cutset trims bytewise as Go trims runes)");
    return cutset;
}
inline std::string spanLiteral(std::string lit, size_t least) {
    if (lit.size() < least) throw Panic("an empty separator in Field()");
    if (lit.size() > (size_t)CPH_SPAN_MAX_LITERAL) throw Panic("a span literal of more than 255 bytes");
    return lit;
}
}  // namespace detail
inline Span TrimSpace(Span s) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_SPACE, CPH_SPAN_BOTH, 0, 0, ""}); }
inline Span TrimLeftSpace(Span s) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_SPACE, CPH_SPAN_LEFT, 0, 0, ""}); }
inline Span TrimRightSpace(Span s) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_SPACE, CPH_SPAN_RIGHT, 0, 0, ""}); }
inline Span Trim(Span s, std::string cutset) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_CUTSET, CPH_SPAN_BOTH, 0, 0, detail::spanCutset(std::move(cutset))}); }
inline Span TrimLeft(Span s, std::string cutset) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_CUTSET, CPH_SPAN_LEFT, 0, 0, detail::spanCutset(std::move(cutset))}); }
inline Span TrimRight(Span s, std::string cutset) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_CUTSET, CPH_SPAN_RIGHT, 0, 0, detail::spanCutset(std::move(cutset))}); }
inline Span TrimPrefix(Span s, std::string lit) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_PREFIX, 0, 0, 0, detail::spanLiteral(std::move(lit), 0)}); }
inline Span TrimSuffix(Span s, std::string lit) { return std::move(s).then(SpanStep{CPH_SPAN_TRIM_SUFFIX, 0, 0, 0, detail::spanLiteral(std::move(lit), 0)}); }
inline Span Field(Span s, std::string sep, int64_t k, int32_t limit = -1) {
    if (limit == 0 || limit < -1) throw Panic("Field(): limit is -1 (all parts) or at least 1");
    return std::move(s).then(SpanStep{CPH_SPAN_FIELD, limit, k, 0, detail::spanLiteral(std::move(sep), 1)});
}
inline Span Before(Span s, std::string sep) { return Field(std::move(s), std::move(sep), 0, 2); }
inline Span After(Span s, std::string sep) { return Field(std::move(s), std::move(sep), 1, 2); }
struct Part {   // a literal, a column, a slice of a column, a narrowed column, a column as a fixed-precision number, or an expression's value
    bool is_col = false;
    bool is_slice = false;        // Substr: bytes [slice.from, slice.to) of the column
    cph_map_slice slice{0, 0};
    std::string text;   // the literal's bytes
    Col col{""};
    std::vector<SpanStep> span;   // TrimSpace(col) and its kin: the column's value narrowed by these operations
    mutable std::vector<cph_span_op> span_abi;   // ... as the C ABI takes them, filled while a batch is mapped (the literals stay in `span`)
    int prec = -1;      // >= 0: Fixed, or Shortest (0)
    char shortest = 0;  // Shortest: the format byte; the float64 value is written with its shortest round-trip digits
    std::shared_ptr<const Expr> expr;   // Fixed(expr, prec) (prec >= 0), Itoa(expr) or Rfc3339(expr, zone) (prec < 0)
    bool is_time = false;               // Rfc3339: the int64 value is Unix seconds, written in the zone `zone`
    int zone = 0;
    Part(Rfc3339 t) : expr(std::move(t.expr)), is_time(true), zone(t.zone) {}   // NOLINT
    Part(const char* lit) : text(lit) {}                 // NOLINT: implicit, so that a template reads like the expression
    Part(std::string lit) : text(std::move(lit)) {}      // NOLINT
    Part(Col c) : is_col(true), col(std::move(c)) {}     // NOLINT
    Part(Fixed f) : is_col(!f.expr), col(std::move(f.col)), prec(f.prec), expr(std::move(f.expr)) {}   // NOLINT
    Part(Shortest f) : is_col(!f.expr), col(std::move(f.col)), prec(0), shortest(f.fmt), expr(std::move(f.expr)) {}   // NOLINT
    Part(Itoa i) : expr(std::move(i.expr)) {}            // NOLINT
    std::string floatText(double v) const { return shortest ? FormatShortest(v, shortest) : FormatFixed(v, prec); }
    Part(Substr s) : is_col(true), is_slice(s.pre.empty()), slice{s.from, s.to}, col(s.col) {   // NOLINT
        if (!s.pre.empty()) span = Span(std::move(s)).ops;
    }
    Part(Span s) : is_col(true), col(std::move(s.col)), span(std::move(s.ops)) {}   // NOLINT
};
struct Format {
    std::vector<Part> parts;
    explicit Format(std::vector<Part> p) : parts(std::move(p)) {
        if (parts.empty()) throw Panic("empty template in Format()");
    }
    // the template on one row, on the host (what the device computes for a whole batch); *missing gets the first absent column,
    // *invalid (when given) ValueAsFloat64's message for a Fixed part's value that does not parse
    bool render(const Row& row, std::string* out, std::string* missing, std::string* invalid = nullptr) const {
        out->clear();
        for (const Part& p : parts) {
            if (p.expr) {
                int64_t iv = 0;
                double fv = 0;
                int op = -1;
                const int32_t rc = p.expr->eval(row, &iv, &fv, &op, missing);
                if (rc != CPH_NUM_OK) {
                    if (rc > 0 && invalid) *invalid = p.expr->errorText(rc, op, row);
                    return false;
                }
                if (p.is_time) {
                    std::string t;
                    if (!FormatRfc3339(iv, p.zone, &t)) {
                        if (invalid) *invalid = "the local year of " + std::to_string(iv) + " is outside 0000..9999";
                        return false;
                    }
                    *out += t;
                    continue;
                }
                *out += p.prec >= 0 ? p.floatText(fv) : std::to_string(iv);
                continue;
            }
            if (!p.is_col) {
                *out += p.text;
                continue;
            }
            auto it = row.find(p.col.name);
            const std::string* v = it != row.end() ? &it->second : p.col.has_default ? &p.col.fallback : nullptr;
            if (!v) {
                *missing = p.col.name;
                return false;
            }
            if (p.is_slice) {
                *out += Substr::of(*v, p.slice.from, p.slice.to);
                continue;
            }
            if (!p.span.empty()) {
                *out += Span::of(p.span, *v);
                continue;
            }
            if (p.prec < 0) {
                *out += *v;
                continue;
            }
            double d;
            const int32_t rc = ParseFloat(*v, &d);
            if (rc != CPH_NUM_OK) {
                if (invalid) *invalid = conversionError(p.col.name, *v, CPH_NUM_FLOAT64, rc);
                return false;
            }
            *out += p.floatText(d);
        }
        return true;
    }
};
// A value that depends on a condition — `if row["name"] == "Amelia" { row["name"] = "Julia" }` (csvplus_test.go:283-288) — is a
// Switch: the template of the FIRST case whose predicate holds for the row, else `otherwise` (cph_map_switch).  A Switch stands
// where a whole template stands; it is no part of a Format and does not nest.  Every Col without default of EVERY alternative
// must be present in a row, whichever alternative the row selects.
struct Case {
    Pred when;
    Format then;
    Case(Pred p, Format f) : when(std::move(p)), then(std::move(f)) {}
};
struct Switch {
    std::vector<Case> cases;
    Format otherwise;
    Switch(std::vector<Case> c, Format o) : cases(std::move(c)), otherwise(std::move(o)) {
        if (cases.empty()) throw Panic("no cases in Switch()");
        if (cases.size() > (size_t)CPH_MAP_MAX_CASES) throw Panic("more than 8 cases in Switch()");
    }
    // the alternative a row selects: the index of the first case that holds, or cases.size() for `otherwise`
    size_t which(const Row& row) const {
        size_t a = 0;
        while (a < cases.size() && !cases[a].when(row)) a++;
        return a;
    }
};
inline Switch When(Pred when, Format then, Format otherwise) { return Switch({Case(std::move(when), std::move(then))}, std::move(otherwise)); }
struct Assign {
    std::string name;
    Format value;              // with cases: the value where none of them holds
    std::vector<Case> cases;   // Set(name, Switch)
};
inline Assign Set(std::string name, std::string literal) { return Assign{std::move(name), Format({Part(std::move(literal))})}; }
inline Assign Set(std::string name, const char* literal) { return Set(std::move(name), std::string(literal)); }
inline Assign Set(std::string name, Format value) { return Assign{std::move(name), std::move(value)}; }
inline Assign Set(std::string name, Fixed value) { return Assign{std::move(name), Format({Part(std::move(value))})}; }
inline Assign Set(std::string name, Shortest value) { return Assign{std::move(name), Format({Part(std::move(value))})}; }
inline Assign Set(std::string name, Itoa value) { return Assign{std::move(name), Format({Part(std::move(value))})}; }
inline Assign Set(std::string name, Rfc3339 value) { return Assign{std::move(name), Format({Part(std::move(value))})}; }
inline Assign Set(std::string name, Switch value) { return Assign{std::move(name), std::move(value.otherwise), std::move(value.cases)}; }

using RowFunc = std::function<Error(Row)>;

// ---- GPU context shared by the process (the Go API has no context argument) -------------------------
class Gpu {
public:
    static Gpu& Default() {
        static Gpu g;
        return g;
    }
    cph_ctx* ctx() {
        if (!ctx_) {
            int dev = 0;
            if (const char* e = std::getenv("CSVPLUS_HIP_DEVICE")) dev = std::atoi(e);
            int32_t rc = cph_ctx_create(dev, &ctx_);
            if (rc != CPH_OK) throw std::runtime_error("csvplus: no usable GPU (cph_ctx_create failed, status " +
                                                       std::to_string(rc) + "); there is no CPU fallback");
        }
        return ctx_;
    }
    // cph_ctx_set_option on the process-wide ctx, e.g. SetOption("float_device", 1): ColumnAsFloat64, FloatCmp and float totals
    // then convert the values outside Clinger's exact cases on the device too.
    void SetOption(const char* name, int64_t value) {
        if (cph_ctx_set_option(ctx(), name, value) != CPH_OK) throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx()));
    }
    // The process-wide ctx is deliberately never destroyed: indexes held in static storage may
    // outlive it during exit, and they return their device blocks to this ctx's pool.
    // Rows read ahead per GPU probe call in Join/Except.  1 reproduces the reference's
    // row-at-a-time order of side effects exactly.
    size_t join_batch_rows = 8192;

private:
    cph_ctx* ctx_ = nullptr;
};

namespace detail {

// Key columns of a batch of rows, staged as Arrow-style SoA in pinned host memory.
class StagedColumns {
public:
    StagedColumns(cph_ctx* ctx, size_t ncols) : ctx_(ctx), data_(ncols), offs_(ncols), cols_(ncols) {}
    StagedColumns(const StagedColumns&) = delete;
    ~StagedColumns() {
        for (void* p : pinned_) cph_pinned_free(ctx_, p);
    }
    // values[c][i] = value of key column c in row i
    void stage(const std::vector<std::vector<const std::string*>>& values, size_t nrows) {
        for (size_t c = 0; c < cols_.size(); c++) {
            uint64_t total = 0;
            for (size_t i = 0; i < nrows; i++) total += values[c][i]->size();
            uint8_t* d = static_cast<uint8_t*>(pinned(total + 8));
            uint64_t* o = static_cast<uint64_t*>(pinned((nrows + 1) * sizeof(uint64_t)));
            uint64_t pos = 0;
            for (size_t i = 0; i < nrows; i++) {
                o[i] = pos;
                const std::string& v = *values[c][i];
                if (!v.empty()) std::memcpy(d + pos, v.data(), v.size());
                pos += v.size();
            }
            o[nrows] = pos;
            cols_[c].data = d;
            cols_[c].offsets = o;
            cols_[c].nrows = nrows;
            cols_[c].offset_bits = 64;
            cols_[c].mem = CPH_MEM_HOST;
        }
    }
    const cph_strcol* cols() const { return cols_.data(); }

private:
    void* pinned(size_t bytes) {
        void* p = nullptr;
        if (cph_pinned_alloc(ctx_, bytes, &p) != CPH_OK)
            throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx_));
        pinned_.push_back(p);
        return p;
    }
    cph_ctx* ctx_;
    std::vector<void*> data_, offs_;
    std::vector<cph_strcol> cols_;
    std::vector<void*> pinned_;
};

// An expression over n rows by ONE cph_num_eval call: vals[c][i] = the value of the expression's column c in row i.
inline int32_t evalStaged(cph_ctx* ctx, const Expr& e, const std::vector<std::vector<const std::string*>>& vals, size_t n, cph_numcol** out,
                          int32_t* bad_op) {
    std::vector<cph_expr_op> prog(e.ops.size());
    for (size_t q = 0; q < prog.size(); q++) {
        prog[q].op = e.ops[q].op;
        prog[q].arg = e.ops[q].arg;
        if (e.ops[q].op == CPH_EXPR_LIT_FLT) prog[q].lit.f = e.ops[q].f;
        else prog[q].lit.i = e.ops[q].i;
    }
    StagedColumns st(ctx, vals.size());
    st.stage(vals, n);
    return cph_num_eval(ctx, vals.empty() ? nullptr : st.cols(), nullptr, (int32_t)vals.size(), n, nullptr, 0, prog.data(), (int32_t)prog.size(),
                        CPH_MEM_HOST, out, bad_op);
}

struct DeviceIndex {   // owns a cph_index
    cph_index* h = nullptr;
    ~DeviceIndex() {
        if (h) cph_index_destroy(h);
    }
};

// allColumnsUnique (:770-782)
inline bool allColumnsUnique(const std::vector<std::string>& columns) {
    std::set<std::string> s(columns.begin(), columns.end());
    return s.size() == columns.size();
}

// A Pred as the postfix program of cph_filter_rows over its own column list.  A row that LACKS a named column must make that
// Like false (:1286 `!found`), and presence differs row by row, so it cannot be the program's column -1: the staging
// carries it instead — such a row gets the column's `absent` value, which is one byte longer than the longest literal any
// Like compares that column with and therefore equals none of them (equality is on the whole value, length first) — and, being
// NUL bytes, converts to no number either, which is what IntCmp / FloatCmp need of it.
struct PredProgram {
    std::vector<std::string> columns;   // distinct names, in order of first use
    std::vector<std::string> absent;    // per column
    std::vector<int> flag_of;           // per column: -1, or this staged column is the PRESENCE FLAG of that column ("1" / "")
    std::vector<cph_pred_op> ops;       // literal pointers point into `pred`
    std::shared_ptr<const Pred> pred;
    std::deque<std::vector<cph_expr_op>> expr_progs;   // an ExprCmp's two sides as one program ...
    std::deque<cph_pred_expr> exprs;                   // ... and the struct its op's value points at (a deque: addresses stay)
    std::deque<int32_t> second_cols;                   // a ColCmp's second column, its op's value
    // what column c holds for `row` on the device
    const std::string* value(size_t c, const Row& row) const {
        static const std::string one("1"), none;
        if (c < flag_of.size() && flag_of[c] >= 0) return row.find(columns[(size_t)flag_of[c]]) == row.end() ? &none : &one;
        auto it = row.find(columns[c]);
        return it == row.end() ? &absent[c] : &it->second;
    }
    size_t column(const std::string& name) {
        size_t c = (size_t)(std::find(columns.begin(), columns.end(), name) - columns.begin());
        if (c == columns.size()) {
            columns.push_back(name);
            absent.emplace_back();
        }
        flag_of.resize(columns.size(), -1);
        return c;
    }
    void emit(const Pred& p) {
        switch (p.kind()) {
            case Pred::kStrCmp:
            case Pred::kHasPrefix:
            case Pred::kHasSuffix:
            case Pred::kContains: {
                // No `absent` value is false under all of these (NE wants it equal to the literal, LT above it, ...): the term is
                // AND-ed with a presence flag, a staged column that holds "1" where the row has the column and "" where not.
                const size_t c = column(p.column());
                const size_t f = column(std::string("\0present\0", 9) + p.column());
                flag_of[f] = (int)c;
                const int32_t op = p.kind() == Pred::kStrCmp      ? (int32_t)CPH_PRED_STR_LT + (int32_t)p.rel()
                                   : p.kind() == Pred::kHasPrefix ? (int32_t)CPH_PRED_HAS_PREFIX
                                   : p.kind() == Pred::kHasSuffix ? (int32_t)CPH_PRED_HAS_SUFFIX
                                                                  : (int32_t)CPH_PRED_CONTAINS;
                ops.push_back(cph_pred_op{op, (int32_t)c, {reinterpret_cast<const uint8_t*>(p.text().data()), p.text().size()}});
                ops.push_back(cph_pred_op{CPH_PRED_LIKE, (int32_t)f, {reinterpret_cast<const uint8_t*>("1"), 1}});
                ops.push_back(cph_pred_op{CPH_PRED_ALL, 2, {nullptr, 0}});
                break;
            }
            case Pred::kExprCmp: {
                // one program, lhs below rhs, over this program's columns.  A row that lacks a column reads the Col's default, or
                // a NUL, which converts to no number: the row is false under every relation, as on the host.
                expr_progs.emplace_back();
                std::vector<cph_expr_op>& prog = expr_progs.back();
                for (const Expr* e : {&p.lhs(), &p.rhs()})
                    for (const Expr::Op& o : e->ops) {
                        cph_expr_op d{};
                        d.op = o.op;
                        if (o.op == CPH_EXPR_COL_INT || o.op == CPH_EXPR_COL_FLT) {
                            const Col& col = e->cols[(size_t)o.arg];
                            const size_t c = column(col.name);
                            if (col.has_default) absent[c] = col.fallback;
                            else if (absent[c].empty()) absent[c].assign(1, '\0');
                            d.arg = (int32_t)c;
                        }
                        if (o.op == CPH_EXPR_LIT_FLT) d.lit.f = o.f;
                        else d.lit.i = o.i;
                        prog.push_back(d);
                    }
                exprs.push_back(cph_pred_expr{prog.data(), (int32_t)prog.size(), 0, nullptr});
                ops.push_back(cph_pred_op{(int32_t)CPH_PRED_EXPR_LT + (int32_t)p.rel(), 0,
                                          {reinterpret_cast<const uint8_t*>(&exprs.back()), sizeof(cph_pred_expr)}});
                break;
            }
            case Pred::kColCmp: {   // like kStrCmp: AND-ed with the presence flags of both columns
                const size_t a = column(p.column()), b = column(p.text());
                const size_t fa = column(std::string("\0present\0", 9) + p.column()), fb = column(std::string("\0present\0", 9) + p.text());
                flag_of[fa] = (int)a;
                flag_of[fb] = (int)b;
                second_cols.push_back((int32_t)b);
                ops.push_back(cph_pred_op{(int32_t)CPH_PRED_COLS_LT + (int32_t)p.rel(), (int32_t)a,
                                          {reinterpret_cast<const uint8_t*>(&second_cols.back()), 4}});
                ops.push_back(cph_pred_op{CPH_PRED_LIKE, (int32_t)fa, {reinterpret_cast<const uint8_t*>("1"), 1}});
                ops.push_back(cph_pred_op{CPH_PRED_LIKE, (int32_t)fb, {reinterpret_cast<const uint8_t*>("1"), 1}});
                ops.push_back(cph_pred_op{CPH_PRED_ALL, 3, {nullptr, 0}});
                break;
            }
            case Pred::kLike:
                for (const auto& kv : p.match()) {
                    size_t c = (size_t)(std::find(columns.begin(), columns.end(), kv.first) - columns.begin());
                    if (c == columns.size()) {
                        columns.push_back(kv.first);
                        absent.emplace_back();
                    }
                    if (absent[c].size() <= kv.second.size()) absent[c].assign(kv.second.size() + 1, '\0');
                    cph_pred_op op{CPH_PRED_LIKE, (int32_t)c, {reinterpret_cast<const uint8_t*>(kv.second.data()), kv.second.size()}};
                    ops.push_back(op);
                }
                if (p.match().size() > 1) ops.push_back(cph_pred_op{CPH_PRED_ALL, (int32_t)p.match().size(), {nullptr, 0}});
                break;
            case Pred::kIntCmp:
            case Pred::kFloatCmp: {
                size_t c = (size_t)(std::find(columns.begin(), columns.end(), p.column()) - columns.begin());
                if (c == columns.size()) {
                    columns.push_back(p.column());
                    absent.emplace_back();
                }
                if (absent[c].empty()) absent[c].assign(1, '\0');   // a NUL converts to no number
                const int32_t base = p.kind() == Pred::kIntCmp ? (int32_t)CPH_PRED_INT_LT : (int32_t)CPH_PRED_FLT_LT;
                ops.push_back(cph_pred_op{base + (int32_t)p.rel(), (int32_t)c, {static_cast<const uint8_t*>(p.literal()), 8}});
                break;
            }
            case Pred::kTimeCmp: {   // a row without the column gets a NUL, which is no timestamp: false under every relation
                const size_t c = column(p.column());
                if (absent[c].empty()) absent[c].assign(1, '\0');
                ops.push_back(cph_pred_op{(int32_t)CPH_PRED_TIME_LT + (int32_t)p.rel(), (int32_t)c,
                                          {reinterpret_cast<const uint8_t*>(p.text().data()), p.text().size()}});
                break;
            }
            case Pred::kNot:
                emit(p.operands()[0]);
                ops.push_back(cph_pred_op{CPH_PRED_NOT, 0, {nullptr, 0}});
                break;
            default:
                for (const auto& k : p.operands()) emit(k);
                ops.push_back(cph_pred_op{p.kind() == Pred::kAll ? CPH_PRED_ALL : CPH_PRED_ANY, (int32_t)p.operands().size(), {nullptr, 0}});
        }
    }
};
inline std::shared_ptr<const PredProgram> compilePred(const Pred& p) {
    auto prog = std::make_shared<PredProgram>();
    prog->pred = std::make_shared<const Pred>(p);
    prog->emit(*prog->pred);
    if (prog->columns.size() > (size_t)CPH_MAX_KEY_COLS) throw Panic("predicate over more than 16 columns");
    return prog;
}

}  // namespace detail

class DataSource;

// ---- Index (:612-641) ------------------------------------------------------------------------------
// ---- named resolvers for Index::ResolveDuplicates, as DATA ---------------------------------------------------------------
// The resolvers people write are a handful of fixed rules; like the named predicates they are declarative, so the device can
// run them (cph_index_resolve): keep the first / last row of a pack, drop the pack, keep the row whose column is smallest /
// largest as an integer, a float or a string.  Ties go to the first row of the pack; a NaN loses to every number.
struct Resolver {
    int32_t rule = 0;         // CPH_RESOLVE_*
    int32_t order_kind = 0;   // CPH_NUM_INT64 / CPH_NUM_FLOAT64 / CPH_ORDER_BYTES (MIN / MAX only)
    std::string column;       // the order column (MIN / MAX only)
};
inline Resolver KeepFirst() { return {CPH_RESOLVE_FIRST, 0, {}}; }
inline Resolver KeepLast() { return {CPH_RESOLVE_LAST, 0, {}}; }
inline Resolver DropDuplicates() { return {CPH_RESOLVE_DROP, 0, {}}; }
inline Resolver KeepMinInt(std::string col) { return {CPH_RESOLVE_MIN, CPH_NUM_INT64, std::move(col)}; }
inline Resolver KeepMaxInt(std::string col) { return {CPH_RESOLVE_MAX, CPH_NUM_INT64, std::move(col)}; }
inline Resolver KeepMinFloat(std::string col) { return {CPH_RESOLVE_MIN, CPH_NUM_FLOAT64, std::move(col)}; }
inline Resolver KeepMaxFloat(std::string col) { return {CPH_RESOLVE_MAX, CPH_NUM_FLOAT64, std::move(col)}; }
inline Resolver KeepMin(std::string col) { return {CPH_RESOLVE_MIN, CPH_ORDER_BYTES, std::move(col)}; }
inline Resolver KeepMax(std::string col) { return {CPH_RESOLVE_MAX, CPH_ORDER_BYTES, std::move(col)}; }

// ---- aggregates for Index::Totals, as DATA ---------------------------------------------------------------------------------
// The reference's TestSimpleTotals (csvplus_test.go:516-571) accumulates per key in a closure; the sums people write are a
// handful of fixed reductions, so they are declarative here and the device runs them (cph_index_aggregate): per key of the index
// the row count and the sum / smallest / largest value of a column read as an integer or a float.
struct Aggregate {
    int32_t op = 0;       // CPH_AGG_*
    int32_t kind = 0;     // CPH_NUM_INT64 / CPH_NUM_FLOAT64
    std::string column;
    std::shared_ptr<const Expr> expr;   // instead of a column: an expression over the rows' columns, SumFloat(price * Float64(qty))
};
inline Aggregate aggregateOf(int32_t op, int32_t kind, Expr e, const char* who) {
    if (e.kind != kind) throw Panic(std::string(who) + "() of an expression of the other type");
    return {op, kind, std::string(), std::make_shared<const Expr>(std::move(e))};
}
inline Aggregate SumInt(Expr e) { return aggregateOf(CPH_AGG_SUM, CPH_NUM_INT64, std::move(e), "SumInt"); }
inline Aggregate SumFloat(Expr e) { return aggregateOf(CPH_AGG_SUM, CPH_NUM_FLOAT64, std::move(e), "SumFloat"); }
inline Aggregate MinInt(Expr e) { return aggregateOf(CPH_AGG_MIN, CPH_NUM_INT64, std::move(e), "MinInt"); }
inline Aggregate MaxInt(Expr e) { return aggregateOf(CPH_AGG_MAX, CPH_NUM_INT64, std::move(e), "MaxInt"); }
inline Aggregate MinFloat(Expr e) { return aggregateOf(CPH_AGG_MIN, CPH_NUM_FLOAT64, std::move(e), "MinFloat"); }
inline Aggregate MaxFloat(Expr e) { return aggregateOf(CPH_AGG_MAX, CPH_NUM_FLOAT64, std::move(e), "MaxFloat"); }
inline Aggregate SumInt(std::string col) { return {CPH_AGG_SUM, CPH_NUM_INT64, std::move(col)}; }
inline Aggregate SumFloat(std::string col) { return {CPH_AGG_SUM, CPH_NUM_FLOAT64, std::move(col)}; }
inline Aggregate MinInt(std::string col) { return {CPH_AGG_MIN, CPH_NUM_INT64, std::move(col)}; }
inline Aggregate MaxInt(std::string col) { return {CPH_AGG_MAX, CPH_NUM_INT64, std::move(col)}; }
inline Aggregate MinFloat(std::string col) { return {CPH_AGG_MIN, CPH_NUM_FLOAT64, std::move(col)}; }
inline Aggregate MaxFloat(std::string col) { return {CPH_AGG_MAX, CPH_NUM_FLOAT64, std::move(col)}; }
// ---- keys for DataSource::OrderBy, as DATA ----------------------------------------------------------------------------------
// The reference orders rows only through an Index (by bytes, ascending).  A key here names a column read as an integer, as a
// float or as bytes — or an int64 / float64 expression over the row — and a direction; the device sorts (cph_order_rows).
// The statement is slices.SortStableFunc over cmp.Compare per key (a NaN below every number, -0 == +0; bytes: strings.Compare);
// Desc swaps the comparison's arguments, and rows equal on every key keep their input order either way.
struct OrderKey {
    int32_t kind = 0;     // CPH_NUM_INT64 / CPH_NUM_FLOAT64 / CPH_ORDER_BYTES
    bool descending = false;
    std::string column;
    std::shared_ptr<const Expr> expr;   // instead of a column: an expression over the rows' columns, FloatKey(price * Float64(qty))
};
inline OrderKey orderKeyOf(int32_t kind, Expr e, const char* who) {
    if (e.kind != kind) throw Panic(std::string(who) + "() of an expression of the other type");
    return {kind, false, std::string(), std::make_shared<const Expr>(std::move(e))};
}
inline OrderKey IntKey(std::string col) { return {CPH_NUM_INT64, false, std::move(col), nullptr}; }
inline OrderKey IntKey(const char* col) { return IntKey(std::string(col)); }
inline OrderKey FloatKey(std::string col) { return {CPH_NUM_FLOAT64, false, std::move(col), nullptr}; }
inline OrderKey FloatKey(const char* col) { return FloatKey(std::string(col)); }
inline OrderKey StrKey(std::string col) { return {CPH_ORDER_BYTES, false, std::move(col), nullptr}; }
inline OrderKey IntKey(Expr e) { return orderKeyOf(CPH_NUM_INT64, std::move(e), "IntKey"); }
inline OrderKey FloatKey(Expr e) { return orderKeyOf(CPH_NUM_FLOAT64, std::move(e), "FloatKey"); }
inline OrderKey Asc(OrderKey k) { k.descending = false; return k; }
inline OrderKey Desc(OrderKey k) { k.descending = true; return k; }

// Group g (key order): keys[g] = the index columns of its rows, counts[g] its rows, and per aggregate a its value in ints[a][g]
// (integer aggregates; floats[a] is empty) or floats[a][g] (float aggregates; ints[a] is empty).
struct TotalsResult {
    std::vector<Row> keys;
    std::vector<uint64_t> counts;
    std::vector<std::vector<int64_t>> ints;
    std::vector<std::vector<double>> floats;
};

class Index {
public:
    // Iterate (:618-620): rows sorted on the index columns, each handed out as a copy (:230)
    Error Iterate(const RowFunc& fn) const;
    // Find (:625-627)
    DataSource Find(const std::vector<std::string>& values) const;
    // SubIndex (:632-641)
    std::shared_ptr<Index> SubIndex(const std::vector<std::string>& values) const;

    // ResolveDuplicates (:643-653): `resolve` is called once per pack of rows with equal key, in key order;
    // it returns one of the rows (kept as the only row with that key), an empty row (the pack is dropped) or an
    // error (returned to the caller).  Compaction follows dedup (:810-867) to the letter.
    using ResolveFunc = std::function<std::pair<Row, Error>(const std::vector<Row>&)>;
    Error ResolveDuplicates(const ResolveFunc& resolve);
    // The same with a named resolver (KeepFirst, KeepMaxInt("id"), ...): choice, compaction and tail rule run on the device,
    // nothing crosses to the host per pack.  An order value inside a pack that does not convert returns the error a Go
    // resolver handing back row.ValueAsInt's error would produce (:176 / :198) and leaves the rows as they were.  When some
    // row lacks the order column the same rule runs through the callback overload: a missing column inside a pack is the
    // reference's `missing column` error (:170), one outside a pack is never looked at.
    Error ResolveDuplicates(const Resolver& resolver);
    static ResolveFunc resolver_func(const Resolver& resolver);   // the rule as a callback
    // Totals: per key of the index (every run of equal keys, runs of one row included) the row count and the named aggregates
    // (SumInt("qty"), MaxFloat("price"), ...), reduced on the device; no aggregates: the distinct keys and their frequencies.
    // Integer sums wrap around as Go's `+=` does; float Min / Max follow math.Min / math.Max.  A row that lacks an aggregate's
    // column is the reference's `missing column` error (:170 / :192), a value that does not convert the error of :176 / :198
    // for the first such row in index order.  The index is left as it was.
    std::pair<TotalsResult, Error> Totals(const std::vector<Aggregate>& aggregates) const;
    // WriteTo (:655-680) / LoadIndex (:682-705).  The reference gob-encodes columns + rows; this file is a
    // length-prefixed little-endian dump of the same two values and is NOT readable by the Go library.
    Error WriteTo(const std::string& fileName) const;

    const std::vector<Row>& rows() const { return impl_rows; }
    const std::vector<std::string>& columns() const { return impl_columns; }

    // ---- indexImpl (:785-788): the sorted rows ARE the index ----
    std::vector<Row> impl_rows;
    std::vector<std::string> impl_columns;

    // find (:870-891): [lower, upper) over impl_rows
    std::pair<size_t, size_t> find(const std::vector<std::string>& values) const {
        if (values.empty()) return {0, impl_rows.size()};                                  // :872-874
        if (values.size() > impl_columns.size()) throw Panic("too many columns in indexImpl.find()");   // :876-878
        std::vector<cph_strval> v(values.size());
        for (size_t i = 0; i < values.size(); i++) {
            v[i].data = reinterpret_cast<const uint8_t*>(values[i].data());
            v[i].len = values[i].size();
        }
        uint64_t lo = 0, hi = 0;
        cph_ctx* ctx = Gpu::Default().ctx();
        if (cph_index_find(ctx, device().h, v.data(), (int32_t)v.size(), &lo, &hi) != CPH_OK)
            throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
        return {(size_t)lo, (size_t)hi};
    }

    // The GPU-resident twin of impl_rows' key columns; built on demand for sub-indices.
    detail::DeviceIndex& device() const {
        if (!dev_) {
            dev_ = std::make_shared<detail::DeviceIndex>();
            cph_ctx* ctx = Gpu::Default().ctx();
            std::vector<std::vector<const std::string*>> vals(impl_columns.size());
            for (size_t c = 0; c < impl_columns.size(); c++) {
                vals[c].resize(impl_rows.size());
                for (size_t i = 0; i < impl_rows.size(); i++) vals[c][i] = &impl_rows[i].at(impl_columns[c]);
            }
            detail::StagedColumns st(ctx, impl_columns.size());
            st.stage(vals, impl_rows.size());
            uint64_t dup = 0;
            int32_t rc = cph_index_build(ctx, st.cols(), (int32_t)impl_columns.size(), 0, &dev_->h, &dup);
            if (rc != CPH_OK) throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
        }
        return *dev_;
    }
    mutable std::shared_ptr<detail::DeviceIndex> dev_;

    // A column of impl_rows as pinned SoA in SORTED order (row i = impl_rows[i]), staged once: what a later Join of a chain reads
    // its key from when the key is a column of THIS index's rows (cph_chain_step.source < 0).  nullptr when some row lacks it.
    // How many rows of impl_rows carry column `name`: kAll / kNone / kSome — ONE pass over the rows per column, cached until the rows
    // change (a chain asks per batch of stream rows: at 1e7 index rows the uncached walk dwarfed the 60-80 us device call)
    enum Presence { kNone = 0, kSome = 1, kAll = 2 };
    Presence column_presence(const std::string& name) const {
        auto it = col_presence_.find(name);
        if (it != col_presence_.end()) return it->second;
        size_t have = 0;
        for (const Row& r : impl_rows) have += r.count(name) ? 1 : 0;
        Presence p = have == 0 ? kNone : have == impl_rows.size() ? kAll : kSome;
        col_presence_.emplace(name, p);
        return p;
    }
    const cph_strcol* side_column(cph_ctx* ctx, const std::string& name) const {
        auto it = side_cols_.find(name);
        if (it == side_cols_.end()) {
            std::shared_ptr<detail::StagedColumns> st;
            const bool all = column_presence(name) == kAll;
            if (all) {
                std::vector<std::vector<const std::string*>> vals(1);
                vals[0].resize(impl_rows.size());
                for (size_t i = 0; i < impl_rows.size(); i++) vals[0][i] = &impl_rows[i].at(name);
                st = std::make_shared<detail::StagedColumns>(ctx, 1);
                st->stage(vals, impl_rows.size());
            }
            it = side_cols_.emplace(name, std::move(st)).first;
        }
        return it->second ? it->second->cols() : nullptr;
    }
    void invalidate_device() {   // impl_rows changed (ResolveDuplicates): the device twin and the staged columns are rebuilt on next use
        dev_.reset();
        side_cols_.clear();
        col_presence_.clear();
    }
    mutable std::map<std::string, std::shared_ptr<detail::StagedColumns>> side_cols_;
    mutable std::map<std::string, Presence> col_presence_;
};

// ---- DataSource (:215) ---------------------------------------------------------------------------------
class DataSource {
public:
    using Fn = std::function<Error(const RowFunc&)>;
    DataSource() = default;
    DataSource(Fn f) : fn_(std::move(f)) {}   // NOLINT: implicit like a Go func value
    Error operator()(const RowFunc& fn) const { return fn_(fn); }

    // IndexOn (:529-531) / UniqueIndexOn (:535-537): (index, error); index is null on error
    std::pair<std::shared_ptr<Index>, Error> IndexOn(const std::vector<std::string>& columns) const {
        return createIndex(columns, false);
    }
    std::pair<std::shared_ptr<Index>, Error> UniqueIndexOn(const std::vector<std::string>& columns) const {
        return createIndex(columns, true);
    }

    // Join (:545-569).  `columns` empty = natural join on the index columns.
    DataSource Join(std::shared_ptr<Index> index, std::vector<std::string> columns = {}) const {
        if (columns.empty()) columns = index->impl_columns;                                  // :546-547
        else if (columns.size() > index->impl_columns.size()) throw Panic("too many source columns in Join()");  // :548-550
        // a Join over a Join: one more step of the same chain (at most CPH_MAX_CHAIN fused; a longer chain starts a new one)
        auto spec = std::make_shared<ChainSpec>();
        if (chain_ && chain_->steps.size() < (size_t)CPH_MAX_CHAIN) *spec = *chain_;
        else spec->upstream = fn_;
        spec->steps.push_back(ChainStepSpec{std::move(index), std::move(columns)});
        DataSource out = spec->steps.size() == 1 ? probeSource(spec->upstream, spec->steps[0].index, spec->steps[0].columns, /*anti=*/false)
                                                 : chainSource(spec);   // (a one-step chain gets its drops in DropColumns)
        out.chain_ = spec;
        return out;
    }

    // Except (:588-608)
    DataSource Except(std::shared_ptr<Index> index, std::vector<std::string> columns = {}) const {
        if (columns.empty()) columns = index->impl_columns;
        else if (columns.size() > index->impl_columns.size()) throw Panic("too many source columns in Except()");
        return probeSource(fn_, std::move(index), std::move(columns), /*anti=*/true);
    }

    // DropColumns (:493-509).  Between the Joins of a chain it stays part of the chain: the columns leave the merged row when
    // it is built, and a later Join that needs one of them fails as in the reference (missing column).
    DataSource DropColumns(std::vector<std::string> columns) const {
        if (columns.empty()) throw Panic("no columns specified in DropColumns()");
        if (chain_) {
            auto spec = std::make_shared<ChainSpec>(*chain_);
            auto& d = spec->steps.back().drop_after;
            d.insert(d.end(), columns.begin(), columns.end());
            DataSource out = chainSource(spec);
            out.chain_ = spec;
            return out;
        }
        Fn src = fn_;
        return DataSource([src, columns](const RowFunc& fn) {
            return src([&](Row row) {
                for (const auto& c : columns) row.erase(c);
                return fn(std::move(row));
            });
        });
    }
    // SelectColumns (:511-525)
    DataSource SelectColumns(std::vector<std::string> columns) const {
        if (columns.empty()) throw Panic("no columns specified in SelectColumns()");
        Fn src = fn_;
        return DataSource([src, columns](const RowFunc& fn) {
            return src([&](Row row) {
                Row r;
                for (const auto& c : columns) {
                    auto it = row.find(c);
                    if (it == row.end()) return Error("missing column " + quote(c));   // Row.Select :122-135
                    r[c] = it->second;
                }
                return fn(std::move(r));
            });
        });
    }

    // Filter (:276-286), TakeWhile (:346-358), DropWhile (:362-374) over a declarative predicate: the predicate's columns of a
    // batch of rows (Gpu::join_batch_rows, read ahead as Join does) are staged and evaluated by ONE cph_filter_rows call; the
    // rows come out in the source's order.  (A predicate that is a closure stays a host affair: `pred(row)` works for a Pred too.)
    DataSource Filter(const Pred& pred) const { return filterSource(fn_, detail::compilePred(pred), CPH_FILTER_WHERE); }
    DataSource TakeWhile(const Pred& pred) const { return filterSource(fn_, detail::compilePred(pred), CPH_FILTER_TAKE_WHILE); }
    DataSource DropWhile(const Pred& pred) const { return filterSource(fn_, detail::compilePred(pred), CPH_FILTER_DROP_WHILE); }
    // Map (:290-296) with row templates: per batch of rows (Gpu::join_batch_rows) and assignment, the template's columns are
    // staged and ONE cph_map_format call renders the new column; the assignments are applied in order (a later one reads what
    // an earlier one wrote).  A row that lacks a column of a Col without default ends the iteration with `missing column`
    // — after the rows in front of it went through, as in Join.
    DataSource Map(const Assign& a) const { return Map(std::vector<Assign>{a}); }
    DataSource Map(std::vector<Assign> assigns) const {
        if (assigns.empty()) throw Panic("no assignments specified in Map()");
        std::vector<std::string> required, written;
        for (const Assign& a : assigns) {
            std::set<std::string> cols;
            std::vector<const Part*> parts;   // of every alternative
            for (const Part& p : a.value.parts) parts.push_back(&p);
            size_t pred_cols = 0;
            if (!a.cases.empty()) {
                detail::PredProgram prog;
                for (const Case& c : a.cases) {
                    prog.emit(c.when);
                    if (c.then.parts.size() > (size_t)CPH_MAP_MAX_PIECES) throw Panic("template of more than 16 parts in Map()");
                    for (const Part& p : c.then.parts) parts.push_back(&p);
                }
                pred_cols = prog.columns.size();
                if (a.cases.size() > (size_t)CPH_MAP_MAX_CASES) throw Panic("more than 8 cases in Map()");
                if (parts.size() > (size_t)CPH_MAP_SWITCH_MAX_PIECES) throw Panic("Switch of more than 32 parts in Map()");
            }
            for (const Part* pp : parts) {
                const Part& p = *pp;
                if (p.expr) {
                    for (const Col& c : p.expr->cols) {
                        const bool known = std::find(written.begin(), written.end(), c.name) != written.end() ||
                                           std::find(required.begin(), required.end(), c.name) != required.end();
                        if (!c.has_default && !known) required.push_back(c.name);
                    }
                    continue;
                }
                if (!p.is_col) continue;
                cols.insert(p.col.name);
                const bool known = std::find(written.begin(), written.end(), p.col.name) != written.end() ||
                                   std::find(required.begin(), required.end(), p.col.name) != required.end();
                if (!p.col.has_default && !known) required.push_back(p.col.name);
            }
            if (a.value.parts.size() > (size_t)CPH_MAP_MAX_PIECES) throw Panic("template of more than 16 parts in Map()");
            if (pred_cols + cols.size() > (size_t)CPH_MAX_KEY_COLS) throw Panic("template over more than 16 columns in Map()");
            written.push_back(a.name);
        }
        Fn src = fn_;
        auto shared = std::make_shared<const std::vector<Assign>>(std::move(assigns));
        return DataSource([src, shared, required](const RowFunc& fn) -> Error {
            cph_ctx* ctx = Gpu::Default().ctx();
            return batched(src, required, [&](std::vector<Row>* batch) -> Error {
                Error pending;   // a Fixed part's value did not parse: the rows in front of it go through, then this surfaces
                for (const Assign& a : *shared) {
                    size_t good = 0;
                    Error e = mapBatch(ctx, a, batch, &good);
                    if (!e) continue;
                    if (good == 0) {
                        batch->clear();
                        return e;
                    }
                    batch->resize(good);
                    pending = e;
                }
                Error err;
                for (size_t i = 0; i < batch->size() && !err; i++) err = fn(std::move((*batch)[i]));
                batch->clear();
                return err ? err : pending;
            });
        });
    }
    // Validate (:300-310) over a declarative predicate: the rows in front of the first row where `pred` fails are delivered,
    // then the iteration ends with Error(message).  A batch is evaluated by ONE cph_filter_rows call in TAKE_WHILE mode, so the
    // error surfaces when the failing row's batch is evaluated: like an error from a Join's batch it is wrapped by the source
    // with the row it had reached (the failing row itself when Gpu::join_batch_rows is 1; a failure in the last, partial
    // batch surfaces after the source has ended and comes back as it is).
    DataSource Validate(const Pred& pred, std::string message) const {
        return filterSource(fn_, detail::compilePred(pred), CPH_FILTER_TAKE_WHILE, std::make_shared<const std::string>(std::move(message)));
    }
    // cph_map_format / cph_map_switch calls made so far (tests: one per batch and assignment)
    static uint64_t map_calls() { return map_calls_counter(); }

    // Top (:313-325) / Drop (:329-342): counters, no data involved
    DataSource Top(uint64_t n) const {
        if (order_) {   // behind an OrderBy: the sort's limit (the device then selects before it sorts)
            auto spec = std::make_shared<OrderSpec>(*order_);
            spec->limit = std::min(spec->limit, n);
            return orderSource(spec);
        }
        Fn src = fn_;
        return DataSource([src, n](const RowFunc& fn) {
            uint64_t counter = n;
            return src([&](Row row) -> Error {
                if (counter == 0) return io_EOF;
                counter--;
                return fn(std::move(row));
            });
        });
    }
    DataSource Drop(uint64_t n) const {
        if (order_) {   // behind an OrderBy: the sort's skip
            auto spec = std::make_shared<OrderSpec>(*order_);
            const uint64_t room = UINT64_MAX - spec->skip;
            spec->skip += std::min(n, room);
            if (spec->limit != UINT64_MAX) spec->limit -= std::min(spec->limit, n);
            return orderSource(spec);
        }
        Fn src = fn_;
        return DataSource([src, n](const RowFunc& fn) {
            uint64_t counter = n;
            return src([&](Row row) -> Error {
                if (counter == 0) return fn(std::move(row));
                counter--;
                return Error();
            });
        });
    }

    // OrderBy: the rows of the source in the order of the keys — OrderBy({Desc(IntKey("qty")), Asc(FloatKey("price")),
    // Asc(StrKey("name"))}) — sorted on the device by ONE cph_order_rows call over all rows (a sort reads its whole input before
    // its first row comes out).  Stable: rows equal on every key keep the source's order, under Asc and Desc alike.  Top / Drop
    // directly behind it become the sort's limit / skip: OrderBy(...).Top(10) lets the device select the ten rows before it sorts.
    // A row without a key's column ends the iteration with the reference's `missing column %q` (:170 / :192), a value that does
    // not convert with the ValueAsInt / ValueAsFloat64 error of its row (:176 / :198) — the first such row, as a
    // DataSourceError(row number, counted from 0); no row is handed out then.
    DataSource OrderBy(std::vector<OrderKey> keys) const {
        if (keys.empty()) throw Panic("empty key list in OrderBy()");
        if (keys.size() > (size_t)CPH_ORDER_MAX_KEYS) throw Panic("too many keys in OrderBy()");
        auto spec = std::make_shared<OrderSpec>();
        spec->upstream = fn_;
        spec->keys = std::move(keys);
        return orderSource(spec);
    }

    // Row.ValueAsInt (:165-183) / Row.ValueAsFloat64 (:187-205) for every row of the source: the column is staged once and
    // converted by ONE cph_col_to_number call.  As the reference's iteration stops at the first row whose conversion fails,
    // the first such row throws Error::DataSourceError(row number, counted from 0) with the reference's message (:176 / :198);
    // a row without the column throws its `missing column` error (:170 / :192).
    std::vector<int64_t> ColumnAsInt(const std::string& name) const {
        std::vector<int64_t> out;
        columnAsNumber(name, CPH_NUM_INT64, &out);
        return out;
    }
    std::vector<double> ColumnAsFloat64(const std::string& name) const {
        std::vector<double> out;
        columnAsNumber(name, CPH_NUM_FLOAT64, &out);
        return out;
    }
    // `t, err := time.Parse(time.RFC3339, row[name])` for every row, the same way: t.Unix() (whole seconds, the floor) or
    // t.UnixNano().  The accepted set is the strict RFC 3339 profile of the header's cph_col_to_number comment; the first row whose
    // stamp does not convert throws Error::DataSourceError(row number) — `column "ts": cannot convert "..." to time: ...`.
    std::vector<int64_t> ColumnAsTime(const std::string& name) const {
        std::vector<int64_t> out;
        columnAsNumber(name, CPH_NUM_TIME_UNIX, &out);
        return out;
    }
    std::vector<int64_t> ColumnAsTimeNano(const std::string& name) const {
        std::vector<int64_t> out;
        columnAsNumber(name, CPH_NUM_TIME_UNIXNANO, &out);
        return out;
    }

    // An expression for every row of the source — `price * float64(qty)` — by ONE cph_num_eval call over the staged columns:
    // ints (an int64 expression) or floats (a float64 one), one value per row.  As the reference's iteration stops at the first
    // row whose closure returns an error, the first failing row throws Error::DataSourceError(row number, counted from 0) with
    // the reference's message for a value that does not convert (:176 / :198), "integer divide by zero" for a zero divisor; a row
    // without a column throws its `missing column` error (:170 / :192).
    struct Numbers {
        int32_t kind = 0;   // CPH_NUM_INT64 / CPH_NUM_FLOAT64
        std::vector<int64_t> ints;
        std::vector<double> floats;
    };
    Numbers Evaluate(const Expr& e) const {
        const size_t nc = e.cols.size();
        std::vector<std::vector<std::string>> values(nc);
        uint64_t missing = UINT64_MAX;
        std::string missing_name;
        uint64_t seen = 0;
        Error err = fn_([&](Row row) -> Error {
            for (size_t c = 0; c < nc; c++) {
                auto it = row.find(e.cols[c].name);
                if (it == row.end() && !e.cols[c].has_default) {
                    missing = seen;
                    missing_name = e.cols[c].name;
                    for (size_t k = 0; k < c; k++) values[k].pop_back();
                    return io_EOF;
                }
                values[c].push_back(it == row.end() ? e.cols[c].fallback : std::move(it->second));
            }
            seen++;
            return Error();
        });
        if (err && !err.is_eof()) throw err;
        const size_t n = (size_t)seen;
        cph_ctx* ctx = Gpu::Default().ctx();
        std::vector<std::vector<const std::string*>> vals(nc);
        for (size_t c = 0; c < nc; c++) {
            vals[c].resize(n);
            for (size_t i = 0; i < n; i++) vals[c][i] = &values[c][i];
        }
        cph_numcol* res = nullptr;
        int32_t op = -1;
        if (detail::evalStaged(ctx, e, vals, n, &res, &op) != CPH_OK) throw Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        struct Release { cph_numcol* r; ~Release() { cph_numcol_release(r); } } rel{res};
        if (res->nerrors) {
            const size_t row = (size_t)res->first_error_row;
            throw Error::DataSourceError(row, Error(e.errorText(res->first_error_kind, op, [&](size_t c) { return values[c][row]; })));
        }
        if (missing != UINT64_MAX) throw Error::DataSourceError(missing, Error("missing column " + quote(missing_name)));
        Numbers out;
        out.kind = e.kind;
        if (e.kind == CPH_NUM_INT64) {
            out.ints.resize(n);
            if (n) std::memcpy(out.ints.data(), res->values, n * sizeof(int64_t));
        } else {
            out.floats.resize(n);
            if (n) std::memcpy(out.floats.data(), res->values, n * sizeof(double));
        }
        return out;
    }

    // Totals over a Join — `custAmounts[cid] += amount` of the reference's TestTransformedSource (csvplus_test.go:754-806) without
    // a second index: on the result of Join(...)[.Join(...)] the row count and the named aggregates per ROW of the index of
    // Join number `step` (0 = the first), reduced on the device over the joined rows (cph_chain_aggregate).  Group g is row g of
    // that index (index->rows()[g], key order); a row no stream row matched has count 0 and values 0.  Over an index with
    // duplicate keys every row of a run is its own group: add the rows of a run for a total per key.  An aggregate's column or
    // expression (SumFloat(AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))))) reads the JOINED row: a name is looked up in
    // the stream row first, then in the rows of the first Join's index, the second's, ... (mergeRows).  A joined row that lacks
    // a column is the reference's `missing column` error, a value that does not convert the error of :176 / :198 for the first
    // such joined row.  All stream rows go through ONE device call; a chain with DropColumns between its Joins, or whose later
    // keys come from different places row by row, is a Panic here (take ToRows() and an Index::Totals instead).
    struct JoinTotalsResult {
        std::vector<uint64_t> counts;                 // [index rows]
        std::vector<std::vector<int64_t>> ints;       // [aggregate][index row]; empty for a float aggregate
        std::vector<std::vector<double>> floats;      // likewise
    };
    std::pair<JoinTotalsResult, Error> TotalsBy(size_t step, const std::vector<Aggregate>& aggs) const {
        JoinTotalsResult out;
        if (!chain_) throw Panic("TotalsBy() on a source that is not the result of a Join()");
        const ChainSpec& spec = *chain_;
        const size_t S = spec.steps.size();
        if (step >= S) throw Panic("TotalsBy() of a Join the chain does not have");
        if (aggs.size() > (size_t)CPH_AGG_MAX_SPECS) return {out, Error("too many aggregates in TotalsBy()")};
        for (const auto& st : spec.steps)
            if (!st.drop_after.empty()) throw Panic("TotalsBy() over a chain with DropColumns between its Joins");
        std::vector<Row> rows;
        Error err = spec.upstream([&](Row row) -> Error {
            std::vector<const std::string*> tmp;
            if (Error e = SelectValues(row, spec.steps[0].columns, &tmp)) return e;   // :556
            rows.push_back(std::move(row));
            return Error();
        });
        if (err && !err.is_eof()) return {out, err};
        cph_ctx* ctx = Gpu::Default().ctx();
        const Index& index = *spec.steps[step].index;
        const size_t ng = index.impl_rows.size();
        out.ints.resize(aggs.size());
        out.floats.resize(aggs.size());
        out.counts.assign(ng, 0);
        for (size_t a = 0; a < aggs.size(); a++) {
            if (aggs[a].kind == CPH_NUM_INT64) out.ints[a].assign(ng, 0);
            else out.floats[a].assign(ng, 0.0);
        }
        if (rows.empty() || ng == 0) return {out, Error()};
        std::vector<int> origin(S, 0);
        for (size_t k = 1; k < S; k++) {
            int org = -2;
            for (const auto& col : spec.steps[k].columns) {
                const int o = columnOrigin(ctx, spec, k, col, rows);
                if (o < 0 || (org != -2 && o != org)) throw Panic("TotalsBy() over a chain whose key columns have no single origin");
                org = o;
            }
            origin[k] = org;
        }
        cph_chain* ch = nullptr;
        if (Error je = fusedJoin(ctx, spec, origin, rows, &ch)) return {out, je};
        struct ReleaseChain { cph_chain* c; ~ReleaseChain() { cph_chain_release(c); } } relc{ch};
        const size_t n = (size_t)ch->nrows;
        // the value of a column in joined row m: the stream's, else the first index row of the chain that carries it
        auto value_of = [&](const Col& c, size_t m) -> const std::string* {
            const Row& srow = rows[(size_t)(ch->stream_row ? ch->stream_row[m] : m)];
            auto it = srow.find(c.name);
            if (it != srow.end()) return &it->second;
            for (size_t k = 0; k < S; k++) {
                const Row& r = spec.steps[k].index->impl_rows[ch->build_row[k][m]];
                auto jt = r.find(c.name);
                if (jt != r.end()) return &jt->second;
            }
            return c.has_default ? &c.fallback : nullptr;
        };
        std::vector<cph_numcol*> nums;
        struct ReleaseNums { std::vector<cph_numcol*>* v; ~ReleaseNums() { for (cph_numcol* p : *v) cph_numcol_release(p); } } reln{&nums};
        std::vector<cph_chain_agg_spec> specs(aggs.size());
        for (size_t a = 0; a < aggs.size() && n; a++) {
            const Expr e = aggs[a].expr ? *aggs[a].expr : Expr::column(Col(aggs[a].column), aggs[a].kind == CPH_NUM_FLOAT64);
            std::vector<std::vector<const std::string*>> vals(e.cols.size());
            for (size_t c = 0; c < e.cols.size(); c++) {
                vals[c].resize(n);
                for (size_t m = 0; m < n; m++)
                    if (!(vals[c][m] = value_of(e.cols[c], m))) return {JoinTotalsResult(), Error("missing column " + quote(e.cols[c].name))};
            }
            cph_numcol* nc = nullptr;
            int32_t op = -1;
            if (detail::evalStaged(ctx, e, vals, n, &nc, &op) != CPH_OK) throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
            nums.push_back(nc);
            if (nc->nerrors) {
                const size_t row = (size_t)nc->first_error_row;
                return {JoinTotalsResult(), Error(e.errorText(nc->first_error_kind, op, [&](size_t c) { return *vals[c][row]; }))};
            }
            specs[a] = cph_chain_agg_spec{aggs[a].op, aggs[a].kind, nc->values, nullptr, CPH_MEM_HOST, 0};
        }
        if (!n) return {out, Error()};
        cph_chain_aggregated* res = nullptr;
        if (cph_chain_aggregate(ctx, ch, (int32_t)step, index.device().h, specs.data(), (int32_t)specs.size(), CPH_MEM_HOST, &res) != CPH_OK)
            throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
        struct Release { cph_chain_aggregated* r; ~Release() { cph_chain_aggregated_release(r); } } rel{res};
        if (res->ngroups != ng) throw std::runtime_error("csvplus: cph_chain_aggregate returned another number of groups than the index has rows");
        out.counts.assign(res->count, res->count + ng);
        for (size_t a = 0; a < aggs.size(); a++) {
            if (aggs[a].kind == CPH_NUM_INT64) {
                const int64_t* v = static_cast<const int64_t*>(res->values[a]);
                out.ints[a].assign(v, v + ng);
            } else {
                const double* v = static_cast<const double*>(res->values[a]);
                out.floats[a].assign(v, v + ng);
            }
        }
        return {out, Error()};
    }

    // cph_filter_rows calls made so far (tests: one per batch)
    static uint64_t filter_calls() { return filter_calls_counter(); }
    // cph_order_rows calls made so far, and the rows that entered the sort of the last one (tests: Top behind OrderBy selects)
    static uint64_t order_calls() { return order_calls_counter(); }
    static uint64_t order_candidates() { return last_order_candidates(); }

    // ToRows (:481-490)
    std::pair<std::vector<Row>, Error> ToRows() const {
        std::vector<Row> rows;
        Error err = fn_([&](Row row) { rows.push_back(std::move(row)); return Error(); });
        return {std::move(rows), err};
    }

private:
    Fn fn_;
    template <class T>
    void columnAsNumber(const std::string& name, int32_t kind, std::vector<T>* out) const {
        std::vector<std::string> values;
        uint64_t missing = UINT64_MAX;
        Error err = fn_([&](Row row) -> Error {
            auto it = row.find(name);
            if (it == row.end()) {
                missing = values.size();
                return io_EOF;
            }
            values.push_back(std::move(it->second));
            return Error();
        });
        if (err && !err.is_eof()) throw err;
        const size_t n = values.size();
        cph_ctx* ctx = Gpu::Default().ctx();
        std::vector<std::vector<const std::string*>> vals(1);
        vals[0].resize(n);
        for (size_t i = 0; i < n; i++) vals[0][i] = &values[i];
        cph_numcol* nc = nullptr;
        int32_t rc;
        {
            detail::StagedColumns st(ctx, 1);
            st.stage(vals, n);
            rc = cph_col_to_number(ctx, st.cols(), nullptr, n, kind, CPH_MEM_HOST, &nc);
        }
        if (rc != CPH_OK) throw Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        if (nc->nerrors) {
            const uint64_t row = nc->first_error_row;
            const std::string msg = conversionError(name, values[(size_t)row], kind, nc->first_error_kind);
            cph_numcol_release(nc);
            throw Error::DataSourceError(row, Error(msg));
        }
        out->resize(n);
        if (n) std::memcpy(out->data(), nc->values, n * sizeof(T));
        cph_numcol_release(nc);
        if (missing != UINT64_MAX) throw Error::DataSourceError(missing, Error("missing column " + quote(name)));
    }
    struct ChainStepSpec {
        std::shared_ptr<Index> index;
        std::vector<std::string> columns;
        std::vector<std::string> drop_after;   // DropColumns applied to this step's output rows
    };
    struct ChainSpec {   // this source == upstream.Join(steps[0])...Join(steps.back())
        Fn upstream;
        std::vector<ChainStepSpec> steps;
    };
    std::shared_ptr<const ChainSpec> chain_;
    struct OrderSpec {   // this source == upstream.OrderBy(keys).Drop(skip).Top(limit)
        Fn upstream;
        std::vector<OrderKey> keys;
        uint64_t skip = 0, limit = UINT64_MAX;
    };
    std::shared_ptr<const OrderSpec> order_;

    static DataSource orderSource(std::shared_ptr<const OrderSpec> spec) {
        DataSource out([spec](const RowFunc& fn) -> Error {
            std::vector<Row> rows;
            if (Error err = spec->upstream([&](Row row) { rows.push_back(std::move(row)); return Error(); })) return err;
            if (rows.size() > 0xFFFFFFFFull) return Error("too many rows for a GPU sort (2^32-1 max)");
            const size_t nk = spec->keys.size();
            // the first row that lacks a key's column: the rows behind it are never reached
            size_t n = rows.size();
            std::string missing;
            for (size_t i = 0; i < n && missing.empty(); i++)
                for (size_t k = 0; k < nk && missing.empty(); k++) {
                    const OrderKey& key = spec->keys[k];
                    if (!key.expr) {
                        if (!rows[i].count(key.column)) missing = key.column;
                    } else {
                        for (const Col& c : key.expr->cols)
                            if (!c.has_default && !rows[i].count(c.name) && missing.empty()) missing = c.name;
                    }
                    if (!missing.empty()) n = i;
                }
            cph_ctx* ctx = Gpu::Default().ctx();
            auto fail = [&]() { return Error(std::string("csvplus_hip: ") + cph_last_error(ctx)); };
            // every key on the device (numbers: values + status bytes; bytes: an index over the column), over rows [0, n)
            std::vector<cph_order_key> ck(nk);
            std::vector<cph_numcol*> nums(nk, nullptr);
            std::vector<int32_t> bad_op(nk, -1);
            std::vector<std::unique_ptr<detail::DeviceIndex>> indexes;
            struct Release {
                std::vector<cph_numcol*>* v;
                ~Release() { for (cph_numcol* c : *v) if (c) cph_numcol_release(c); }
            } release{&nums};
            for (size_t k = 0; k < nk && n; k++) {
                const OrderKey& key = spec->keys[k];
                ck[k] = cph_order_key{key.kind, key.descending ? 1 : 0, nullptr, nullptr, CPH_MEM_HOST, 0, nullptr};
                if (key.expr) {
                    const Expr& e = *key.expr;
                    std::vector<std::vector<const std::string*>> vals(e.cols.size());
                    for (size_t c = 0; c < e.cols.size(); c++) {
                        vals[c].resize(n);
                        for (size_t i = 0; i < n; i++) {
                            auto it = rows[i].find(e.cols[c].name);
                            vals[c][i] = it == rows[i].end() ? &e.cols[c].fallback : &it->second;
                        }
                    }
                    if (detail::evalStaged(ctx, e, vals, n, &nums[k], &bad_op[k]) != CPH_OK) return fail();
                    continue;
                }
                std::vector<std::vector<const std::string*>> vals(1);
                vals[0].resize(n);
                for (size_t i = 0; i < n; i++) vals[0][i] = &rows[i].at(key.column);
                detail::StagedColumns st(ctx, 1);
                st.stage(vals, n);
                if (key.kind == CPH_ORDER_BYTES) {
                    indexes.push_back(std::make_unique<detail::DeviceIndex>());
                    uint64_t dup = 0;
                    if (cph_index_build(ctx, st.cols(), 1, 0, &indexes.back()->h, &dup) != CPH_OK) return fail();
                    ck[k].index = indexes.back()->h;
                } else if (cph_col_to_number(ctx, st.cols(), nullptr, n, key.kind, CPH_MEM_DEVICE, &nums[k]) != CPH_OK) {
                    return fail();
                }
            }
            // the first row with a value that does not convert, the lowest key there
            size_t bad_row = SIZE_MAX, bad_key = 0;
            for (size_t k = 0; k < nk; k++)
                if (nums[k] && nums[k]->nerrors && (size_t)nums[k]->first_error_row < bad_row) {
                    bad_row = (size_t)nums[k]->first_error_row;
                    bad_key = k;
                }
            if (bad_row != SIZE_MAX) {
                const OrderKey& key = spec->keys[bad_key];
                const int32_t kind = nums[bad_key]->first_error_kind;
                if (key.expr) return Error::DataSourceError(bad_row, Error(key.expr->errorText(kind, bad_op[bad_key], rows[bad_row])));
                return Error::DataSourceError(bad_row, Error(conversionError(key.column, rows[bad_row].at(key.column), key.kind, kind)));
            }
            if (!missing.empty()) return Error::DataSourceError(n, Error("missing column " + quote(missing)));
            if (!n) return Error();
            for (size_t k = 0; k < nk; k++)
                if (nums[k]) {
                    ck[k].values = nums[k]->values;
                    ck[k].status = nums[k]->status;
                    ck[k].values_mem = nums[k]->mem;
                }
            cph_ordered* res = nullptr;
            if (cph_order_rows(ctx, ck.data(), (int32_t)nk, n, spec->skip, spec->limit, CPH_MEM_HOST, &res) != CPH_OK) return fail();
            struct ReleaseOrdered { cph_ordered* r; ~ReleaseOrdered() { cph_ordered_release(r); } } rel{res};
            order_calls_counter()++;
            last_order_candidates() = res->candidates;
            for (uint64_t i = 0; i < res->nrows; i++)
                if (Error e = fn(std::move(rows[res->ids[i]]))) return e.is_eof() ? Error() : e;
            return Error();
        });
        out.order_ = std::move(spec);
        return out;
    }
    static uint64_t& order_calls_counter() {
        static uint64_t n = 0;
        return n;
    }
    static uint64_t& last_order_candidates() {
        static uint64_t n = 0;
        return n;
    }

    // createIndex (:707-738) + createUniqueIndex (:740-756)
    std::pair<std::shared_ptr<Index>, Error> createIndex(const std::vector<std::string>& columns, bool unique) const {
        if (columns.empty()) throw Panic("empty column list in CreateIndex()");                    // :709-710
        if (columns.size() > 1 && !detail::allColumnsUnique(columns))
            throw Panic("duplicate column name(s) in CreateIndex()");                                // :714-716
        auto index = std::make_shared<Index>();
        index->impl_columns = columns;
        std::vector<Row> rows;
        // copy Rows with validation (:722-733)
        Error err = fn_([&](Row row) {
            for (const auto& col : columns)
                if (!HasColumn(row, col)) return Error("missing column " + quote(col) + " while creating an index");
            rows.push_back(std::move(row));
            return Error();
        });
        if (err) return {nullptr, err};
        if (rows.size() > 0xFFFFFFFFull) return {nullptr, Error("too many rows for a GPU index (2^32-1 max)")};

        // sort (:736) on the GPU: stage key columns, build, fetch the permutation
        cph_ctx* ctx = Gpu::Default().ctx();
        std::vector<std::vector<const std::string*>> vals(columns.size());
        for (size_t c = 0; c < columns.size(); c++) {
            vals[c].resize(rows.size());
            for (size_t i = 0; i < rows.size(); i++) vals[c][i] = &rows[i].at(columns[c]);
        }
        auto dev = std::make_shared<detail::DeviceIndex>();
        uint64_t first_dup = UINT64_MAX;
        int32_t rc;
        {
            detail::StagedColumns st(ctx, columns.size());
            st.stage(vals, rows.size());
            rc = cph_index_build(ctx, st.cols(), (int32_t)columns.size(), unique ? 1 : 0, &dev->h, &first_dup);
        }
        if (rc != CPH_OK && rc != CPH_ERR_DUPLICATE) return {nullptr, Error(std::string("csvplus_hip: ") + cph_last_error(ctx))};
        const uint32_t* perm = nullptr;
        uint64_t n = 0;
        if (cph_index_perm(dev->h, CPH_MEM_HOST, &perm, &n) != CPH_OK)
            return {nullptr, Error(std::string("csvplus_hip: ") + cph_last_error(ctx))};
        if (rc == CPH_ERR_DUPLICATE) {
            // :751  "duplicate value while creating unique index: " + rows[i].SelectExisting(columns...).String()
            return {nullptr, Error("duplicate value while creating unique index: " +
                                   String(SelectExisting(rows[perm[first_dup]], columns)))};
        }
        index->impl_rows.resize(rows.size());
        for (size_t i = 0; i < rows.size(); i++) index->impl_rows[i] = std::move(rows[perm[i]]);
        index->dev_ = dev;
        return {index, Error()};
    }

    // One step over a batch of rows that all carry `columns`: the per-row `first()` + forward scan (:557-563) / `has()`
    // (:599-602) as one GPU probe; `emit` gets every output row in the reference's order.  The batch is consumed.
    static Error probeBatch(cph_ctx* ctx, const std::shared_ptr<Index>& index, const std::vector<std::string>& columns, bool anti,
                            std::vector<Row>* batch, const RowFunc& emit) {
        if (batch->empty()) return Error();
        std::vector<std::vector<const std::string*>> vals(columns.size());
        for (auto& v : vals) v.resize(batch->size());
        for (size_t i = 0; i < batch->size(); i++)
            for (size_t c = 0; c < columns.size(); c++) vals[c][i] = &(*batch)[i].at(columns[c]);
        cph_matches* m = nullptr;
        {
            detail::StagedColumns st(ctx, columns.size());
            st.stage(vals, batch->size());
            int32_t rc = cph_join_probe(ctx, index->device().h, st.cols(), (int32_t)columns.size(), nullptr, 32,
                                        0, 0, 0, /*want_pairs=*/0, CPH_MEM_HOST, &m);
            if (rc != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        }
        Error err;
        // index.impl.rows is read live at iteration time (:557), as in the reference
        const std::vector<Row>& irows = index->impl_rows;
        for (size_t i = 0; i < batch->size() && !err; i++) {
            if (anti) {
                if (m->cnt[i] == 0) err = emit(std::move((*batch)[i]));                        // :600-602
            } else {
                for (uint32_t j = 0; j < m->cnt[i] && !err; j++)                              // :559-563
                    err = emit(mergeRows(irows[(size_t)m->lo[i] + j], (*batch)[i]));
            }
        }
        cph_matches_release(m);
        batch->clear();
        return err;
    }

    // One batch through cph_filter_rows (mode WHERE: the rows kept; the WHILE modes: a range).  Emits the kept rows to `fn`;
    // *first / *count describe the answer (WHERE: count only).
    static Error filterBatch(cph_ctx* ctx, const detail::PredProgram& prog, int32_t mode, std::vector<Row>* batch, const RowFunc& fn,
                             uint64_t* first, uint64_t* count) {
        const size_t n = batch->size(), nc = prog.columns.size();
        *first = 0;
        *count = 0;
        if (n == 0) return Error();
        std::vector<std::vector<const std::string*>> vals(nc);
        for (size_t c = 0; c < nc; c++) {
            vals[c].resize(n);
            for (size_t i = 0; i < n; i++) {
                vals[c][i] = prog.value(c, (*batch)[i]);   // see detail::PredProgram
            }
        }
        cph_rowlist* rl = nullptr;
        int32_t rc;
        {
            detail::StagedColumns st(ctx, nc);
            st.stage(vals, n);
            cph_filter_opts o{mode, 32, 0, 0, UINT64_MAX};
            rc = cph_filter_rows(ctx, nc ? st.cols() : nullptr, nullptr, (int32_t)nc, n, prog.ops.data(), (int32_t)prog.ops.size(), &o,
                                 CPH_MEM_HOST, &rl);
        }
        if (rc != CPH_OK) {
            batch->clear();
            return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        }
        filter_calls_counter()++;
        const uint32_t* ids = static_cast<const uint32_t*>(rl->ids);
        Error err;
        for (uint64_t k = 0; k < rl->nrows && !err; k++) err = fn(std::move((*batch)[ids ? ids[k] : rl->first + k]));
        *first = rl->first;
        *count = rl->nrows;
        cph_rowlist_release(rl);
        batch->clear();
        return err;
    }
    static uint64_t& filter_calls_counter() {
        static uint64_t n = 0;
        return n;
    }

    // What mapBatch and switchBatch hand to the device for one template part.  A number part (an expression, or a Fixed
    // column) shows the converted values `num`; a Col or Substr part reads staged column `col`; a literal needs neither.
    static cph_map_piece partPiece(const Part& p, const cph_numcol* num, size_t col) {
        if (p.expr && p.prec < 0)
            return cph_map_piece{p.is_time ? CPH_MAP_TIME : CPH_MAP_INT64, CPH_MEM_HOST, {nullptr, 0}, static_cast<const int64_t*>(num->values), nullptr,
                                 p.is_time ? p.zone : 0, 0};
        if (p.expr || p.prec >= 0)
            return cph_map_piece{p.shortest ? CPH_MAP_FLOAT64_SHORTEST : CPH_MAP_FLOAT64, CPH_MEM_HOST, {nullptr, 0}, nullptr, static_cast<const double*>(num->values),
                                 p.shortest ? (int32_t)p.shortest : p.prec, 0};
        if (!p.is_col) return cph_map_piece{CPH_MAP_LITERAL, 0, {reinterpret_cast<const uint8_t*>(p.text.data()), p.text.size()}, nullptr};
        if (p.is_slice) return cph_map_piece{CPH_MAP_SLICE, (int32_t)col, {reinterpret_cast<const uint8_t*>(&p.slice), sizeof p.slice}, nullptr};
        if (!p.span.empty()) {
            p.span_abi.clear();
            for (const SpanStep& st : p.span)
                p.span_abi.push_back(cph_span_op{st.op, st.mode, st.a, st.b, {st.lit.empty() ? nullptr : reinterpret_cast<const uint8_t*>(st.lit.data()), st.lit.size()}});
            return cph_map_piece{CPH_MAP_SPAN, (int32_t)col, {reinterpret_cast<const uint8_t*>(p.span_abi.data()), p.span_abi.size() * sizeof(cph_span_op)}, nullptr};
        }
        return cph_map_piece{CPH_MAP_COLUMN, (int32_t)col, {nullptr, 0}, nullptr};
    }
    // the columns a number part converts
    static std::vector<const Col*> numberColumns(const Part& p) {
        std::vector<const Col*> cols;
        if (!p.expr) cols.push_back(&p.col);
        else
            for (const Col& c : p.expr->cols) cols.push_back(&c);
        return cols;
    }
    // vals[c][i] = the value of column cols[c] in row i of the batch (rows 0 .. n-1), its default where the row lacks the column
    static std::vector<std::vector<const std::string*>> columnValues(const std::vector<Row>& batch, size_t n, const std::vector<const Col*>& cols) {
        std::vector<std::vector<const std::string*>> vals(cols.size());
        for (size_t c = 0; c < cols.size(); c++) {
            vals[c].resize(n);
            for (size_t i = 0; i < n; i++) {
                auto it = batch[i].find(cols[c]->name);
                vals[c][i] = it == batch[i].end() ? &cols[c]->fallback : &it->second;
            }
        }
        return vals;
    }
    // the index of a template's column in `cols`, appended where it is new (the first mention's default counts)
    static size_t columnIndex(std::vector<const Col*>* cols, const Col& col) {
        size_t c = 0;
        while (c < cols->size() && (*cols)[c]->name != col.name) c++;
        if (c == cols->size()) cols->push_back(&col);
        return c;
    }

    // One assignment over a batch: row[a.name] = the template's value, for every row, by one cph_map_format call.  A row that
    // lacks a column gets the Col's default in its place (the caller has turned away rows that lack a column without one).
    // A Fixed part's column goes through cph_col_to_number first (ColumnAsFloat64's path) and into a FLOAT64 piece.  Where
    // such a value does not parse, the rows in front of it are mapped, *good is their number and ValueAsFloat64's error
    // comes back; on any other error *good is 0.
    static Error mapBatch(cph_ctx* ctx, const Assign& a, std::vector<Row>* batch, size_t* good) {
        size_t n = batch->size();
        *good = 0;
        if (n == 0) return Error();
        if (!a.cases.empty()) return switchBatch(ctx, a, batch, good);
        std::vector<const Col*> columns;
        std::vector<cph_map_piece> pieces;
        struct NumCols {   // the converted columns live until the template has run
            std::vector<cph_numcol*> v;
            ~NumCols() {
                for (cph_numcol* c : v) cph_numcol_release(c);
            }
        } nums;
        Error pending;
        for (const Part& p : a.value.parts) {
            if (!p.expr && p.prec < 0) continue;
            const std::vector<std::vector<const std::string*>> vals = columnValues(*batch, n, numberColumns(p));
            if (p.expr) {   // an expression's value: ONE cph_num_eval call over its columns, then an INT64 / FLOAT64 piece
                const Expr& e = *p.expr;
                cph_numcol* nc = nullptr;
                int32_t op = -1;
                if (detail::evalStaged(ctx, e, vals, n, &nc, &op) != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
                nums.v.push_back(nc);
                if (nc->nerrors) {
                    const size_t row = (size_t)nc->first_error_row;
                    pending = Error(e.errorText(nc->first_error_kind, op, [&](size_t c) { return *vals[c][row]; }));
                    n = row;
                    if (n == 0) return pending;
                }
                continue;
            }
            cph_numcol* nc = nullptr;
            int32_t rc;
            {
                detail::StagedColumns st(ctx, 1);
                st.stage(vals, n);
                rc = cph_col_to_number(ctx, st.cols(), nullptr, n, CPH_NUM_FLOAT64, CPH_MEM_HOST, &nc);
            }
            if (rc != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
            nums.v.push_back(nc);
            if (nc->nerrors) {   // an earlier part's later row no longer counts
                const size_t row = (size_t)nc->first_error_row;
                pending = Error(conversionError(p.col.name, *vals[0][row], CPH_NUM_FLOAT64, nc->first_error_kind));
                n = row;
                if (n == 0) return pending;
            }
        }
        size_t fixed_seen = 0;
        for (const Part& p : a.value.parts) {
            if (p.expr || p.prec >= 0) pieces.push_back(partPiece(p, nums.v[fixed_seen++], 0));
            else pieces.push_back(partPiece(p, nullptr, p.is_col ? columnIndex(&columns, p.col) : 0));
        }
        const size_t nc = columns.size();
        const std::vector<std::vector<const std::string*>> vals = columnValues(*batch, n, columns);
        cph_colbuf* cb = nullptr;
        int32_t rc;
        {
            detail::StagedColumns st(ctx, nc);
            st.stage(vals, n);
            rc = cph_map_format(ctx, nc ? st.cols() : nullptr, nullptr, (int32_t)nc, n, pieces.data(), (int32_t)pieces.size(), CPH_MEM_HOST, &cb);
        }
        if (rc != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        map_calls_counter()++;
        const uint64_t* offs = static_cast<const uint64_t*>(cb->col.offsets);
        const char* data = reinterpret_cast<const char*>(cb->col.data);
        for (size_t i = 0; i < n; i++) (*batch)[i][a.name].assign(data + offs[i], (size_t)(offs[i + 1] - offs[i]));
        cph_colbuf_release(cb);
        *good = pending ? n : batch->size();
        return pending;
    }
    // The same for Set(name, Switch): ONE cph_map_switch call.  The predicates' columns are staged as a Filter stages them (a row
    // that lacks one gets a value that equals no literal and converts to no number), the templates' columns behind them with
    // their defaults.  Fixed / Itoa parts are evaluated over all rows; a row where one fails counts only if the row selects
    // the alternative that holds the part (`which`): the rows in front of the lowest such row are mapped, then its error surfaces.
    static Error switchBatch(cph_ctx* ctx, const Assign& a, std::vector<Row>* batch, size_t* good) {
        const size_t n = batch->size(), ncases = a.cases.size();
        detail::PredProgram prog;   // every case's program over one column list
        std::vector<size_t> op_first(ncases + 1);
        for (size_t c = 0; c < ncases; c++) {
            op_first[c] = prog.ops.size();
            prog.emit(a.cases[c].when);
        }
        op_first[ncases] = prog.ops.size();
        const size_t npred = prog.columns.size();
        std::vector<const Col*> columns;   // the templates' columns, staged behind the predicates'
        struct NumPart {   // a Fixed / Itoa part's values over the batch
            size_t alt;
            const Part* part;
            cph_numcol* nc;
            std::vector<std::vector<const std::string*>> vals;
        };
        struct NumParts {   // they live until the switch has run
            std::vector<NumPart> v;
            ~NumParts() {
                for (NumPart& p : v) cph_numcol_release(p.nc);
            }
        } nums;
        std::vector<std::vector<cph_map_piece>> pieces(ncases + 1);
        for (size_t alt = 0; alt <= ncases; alt++) {
            for (const Part& p : (alt < ncases ? a.cases[alt].then : a.value).parts) {
                if (!p.expr && p.prec < 0) {
                    pieces[alt].push_back(partPiece(p, nullptr, p.is_col ? npred + columnIndex(&columns, p.col) : 0));
                    continue;
                }
                NumPart np{alt, &p, nullptr, columnValues(*batch, n, numberColumns(p))};
                int32_t rc, op = -1;
                if (p.expr) {
                    rc = detail::evalStaged(ctx, *p.expr, np.vals, n, &np.nc, &op);
                } else {
                    detail::StagedColumns st(ctx, 1);
                    st.stage(np.vals, n);
                    rc = cph_col_to_number(ctx, st.cols(), nullptr, n, CPH_NUM_FLOAT64, CPH_MEM_HOST, &np.nc);
                }
                if (rc != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
                pieces[alt].push_back(partPiece(p, np.nc, 0));
                nums.v.push_back(std::move(np));
            }
        }
        const size_t nc = npred + columns.size();
        std::vector<std::vector<const std::string*>> vals(npred);
        for (size_t c = 0; c < npred; c++) {
            vals[c].resize(n);
            for (size_t i = 0; i < n; i++) vals[c][i] = prog.value(c, (*batch)[i]);
        }
        for (auto& v : columnValues(*batch, n, columns)) vals.push_back(std::move(v));
        std::vector<cph_map_case> cases(ncases);
        for (size_t c = 0; c < ncases; c++)
            cases[c] = cph_map_case{prog.ops.data() + op_first[c], (int32_t)(op_first[c + 1] - op_first[c]), pieces[c].data(), (int32_t)pieces[c].size()};
        std::vector<uint8_t> which(n);
        cph_colbuf* cb = nullptr;
        int32_t rc;
        {
            detail::StagedColumns st(ctx, nc);
            st.stage(vals, n);
            rc = cph_map_switch(ctx, nc ? st.cols() : nullptr, nullptr, (int32_t)nc, n, cases.data(), (int32_t)ncases, pieces[ncases].data(),
                                (int32_t)pieces[ncases].size(), CPH_MEM_HOST, &cb, which.data());
        }
        if (rc != CPH_OK) return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        map_calls_counter()++;
        size_t bad = n;   // the lowest row whose own alternative holds a part that failed there
        const NumPart* culprit = nullptr;
        for (const NumPart& np : nums.v) {
            if (!np.nc->nerrors) continue;
            const uint8_t* st = static_cast<const uint8_t*>(np.nc->status);
            for (size_t i = (size_t)np.nc->first_error_row; i < bad; i++) {
                if (st[i] == CPH_NUM_OK || which[i] != np.alt) continue;
                bad = i;
                culprit = &np;
                break;
            }
        }
        Error pending;
        if (culprit) {
            const Part& p = *culprit->part;
            const int32_t kind = static_cast<const uint8_t*>(culprit->nc->status)[bad];
            if (p.expr) {
                int64_t iv = 0;
                double fv = 0;
                int op = 0;
                (void)p.expr->eval((*batch)[bad], &iv, &fv, &op, nullptr);   // the host model names the op that fails in that row
                pending = Error(p.expr->errorText(kind, op < 0 ? 0 : op, [&](size_t c) { return *culprit->vals[c][bad]; }));
            } else {
                pending = Error(conversionError(p.col.name, *culprit->vals[0][bad], CPH_NUM_FLOAT64, kind));
            }
        }
        const uint64_t* offs = static_cast<const uint64_t*>(cb->col.offsets);
        const char* data = reinterpret_cast<const char*>(cb->col.data);
        for (size_t i = 0; i < bad; i++) (*batch)[i][a.name].assign(data + offs[i], (size_t)(offs[i + 1] - offs[i]));
        cph_colbuf_release(cb);
        *good = culprit ? bad : batch->size();
        return pending;
    }
    static uint64_t& map_calls_counter() {
        static uint64_t n = 0;
        return n;
    }

    // invalid != null: Validate — a failing row ends the iteration with that message instead of ending it cleanly
    static DataSource filterSource(Fn src, std::shared_ptr<const detail::PredProgram> prog, int32_t mode,
                                   std::shared_ptr<const std::string> invalid = nullptr) {
        return DataSource([src, prog, mode, invalid](const RowFunc& fn) -> Error {
            cph_ctx* ctx = Gpu::Default().ctx();
            const size_t batch_rows = std::max<size_t>(1, Gpu::Default().join_batch_rows);
            std::vector<Row> batch;
            batch.reserve(batch_rows);
            bool yield = false;   // DropWhile: a row has failed, everything passes from here on (:366-368)
            auto flush = [&]() -> Error {
                const uint64_t n = batch.size();
                uint64_t first = 0, count = 0;
                Error e = filterBatch(ctx, *prog, mode, &batch, fn, &first, &count);
                if (e) return e;
                if (mode == CPH_FILTER_TAKE_WHILE && count < n)   // the predicate failed: the iteration stops (:350-352; Validate: :303)
                    return invalid ? Error(*invalid) : io_EOF;
                if (mode == CPH_FILTER_DROP_WHILE && count) yield = true;
                return Error();
            };
            Error err = src([&](Row row) -> Error {
                if (yield) return fn(std::move(row));
                batch.push_back(std::move(row));
                return batch.size() >= batch_rows ? flush() : Error();
            });
            if (err) return err;
            err = flush();
            return err.is_eof() ? Error() : err;   // as the source would have mapped it (:238-239)
        });
    }

    // Reads `src` in batches of Gpu::join_batch_rows rows that carry `columns` (SelectValues, :556 / :599: a row without one
    // of them ends the iteration with that error — after the rows in front of it went through `flush`) and hands each batch
    // to `flush`.
    static Error batched(const Fn& src, const std::vector<std::string>& columns, const std::function<Error(std::vector<Row>*)>& flush) {
        const size_t batch_rows = std::max<size_t>(1, Gpu::Default().join_batch_rows);
        std::vector<Row> batch;
        batch.reserve(batch_rows);
        Error err = src([&](Row row) -> Error {
            std::vector<const std::string*> tmp;
            Error e = SelectValues(row, columns, &tmp);                                       // :556 / :599
            if (e) {
                // rows before this one must be delivered first, then the error surfaces
                Error fe = flush(&batch);
                return fe ? fe : e;
            }
            batch.push_back(std::move(row));
            if (batch.size() >= batch_rows) return flush(&batch);
            return Error();
        });
        if (err) return err;
        err = flush(&batch);
        // an io.EOF from `fn` in the tail batch ends the iteration cleanly, as the source
        // would have mapped it (:238-239)
        return err.is_eof() ? Error() : err;
    }

    // Shared body of a single Join / Except over `src`.
    static DataSource probeSource(Fn src, std::shared_ptr<Index> index, std::vector<std::string> columns, bool anti) {
        return DataSource([src, index, columns, anti](const RowFunc& fn) -> Error {
            cph_ctx* ctx = Gpu::Default().ctx();
            return batched(src, columns, [&](std::vector<Row>* batch) { return probeBatch(ctx, index, columns, anti, batch, fn); });
        });
    }

    // upstream.Join(steps[0])...Join(steps[k]) (with the DropColumns between them).  Per batch of stream rows: ONE fused device
    // call — cph_join_chain_ex reporting sorted positions, the subscripts into each index's impl_rows — when every later key
    // has ONE origin for the whole batch: every stream row carries it (the value a later Join sees is then the stream's own:
    // mergeRows :571-583 lets the right operand win), or no stream row does and every row of an earlier index does
    // (cph_chain_step.source: the device reads the key from the row that step matched; the earliest such index wins, as in the
    // nested merges).  Else the steps one after the other over the merged rows.  Either way the rows come out in the reference's
    // nested order: by stream row, then by position in steps[0]'s index, then in steps[1]'s, ...; a step-k row is merged as
    // mergeRows(index_k row, mergeRows(index_k-1 row, ... stream row)): on a shared column name the precedence is
    // stream > steps[0] > steps[1] > ... (csvplus.go:559-560 nested).
    static DataSource chainSource(std::shared_ptr<const ChainSpec> spec) {
        return DataSource([spec](const RowFunc& fn) -> Error {
            cph_ctx* ctx = Gpu::Default().ctx();
            const size_t S = spec->steps.size();
            return batched(spec->upstream, spec->steps[0].columns, [&](std::vector<Row>* batch) -> Error {
                if (batch->empty()) return Error();
                // origin[k]: 0 = step k's key columns come from the stream rows, t + 1 = from the rows of steps[t].index
                std::vector<int> origin(S, 0);
                bool fusable = true;
                for (size_t k = 1; k < S && fusable; k++) {
                    int org = -2;   // not decided
                    for (const auto& col : spec->steps[k].columns) {
                        const int o = columnOrigin(ctx, *spec, k, col, *batch);
                        if (o < 0 || (org != -2 && o != org)) { fusable = false; break; }
                        org = o;
                    }
                    origin[k] = org;
                }
                // the steps one after the other: step k's output rows are step k+1's stream (same order of outputs and of
                // errors as the nested closures: a later step sees the rows in emission order)
                if (!fusable) return runSteps(ctx, *spec, 0, batch, fn);
                // ---- fused: one device call ----
                cph_chain* ch = nullptr;
                if (Error je = fusedJoin(ctx, *spec, origin, *batch, &ch)) return je;
                fused_calls()++;
                Error err;
                for (uint64_t m = 0; m < ch->nrows && !err; m++) {
                    const uint64_t r = ch->stream_row ? ch->stream_row[m] : m;   // NULL: every row joined exactly once, in order
                    Row row = (*batch)[(size_t)r];
                    for (size_t k = 0; k < S; k++) {
                        row = mergeRows(spec->steps[k].index->impl_rows[ch->build_row[k][m]], row);
                        for (const auto& c : spec->steps[k].drop_after) row.erase(c);
                    }
                    err = fn(std::move(row));
                }
                cph_chain_release(ch);
                batch->clear();
                return err;
            });
        });
    }

    // The fused device call of a chain over one batch of stream rows (origin[k] as columnOrigin gives it, none negative): the
    // row-id tuples in host memory, build_row[k][m] = the subscript into steps[k].index->impl_rows.  The caller releases *ch.
    static Error fusedJoin(cph_ctx* ctx, const ChainSpec& spec, const std::vector<int>& origin, const std::vector<Row>& batch, cph_chain** ch) {
        const size_t S = spec.steps.size();
        std::vector<std::unique_ptr<detail::StagedColumns>> staged;
        std::vector<std::vector<cph_strcol>> side(S);
        std::vector<cph_chain_step> steps(S);
        for (size_t k = 0; k < S; k++) {
            const auto& cols = spec.steps[k].columns;
            steps[k] = cph_chain_step{};
            steps[k].index = spec.steps[k].index->device().h;
            steps[k].ncols = (int32_t)cols.size();
            if (origin[k] == 0) {
                std::vector<std::vector<const std::string*>> vals(cols.size());
                for (auto& v : vals) v.resize(batch.size());
                for (size_t i = 0; i < batch.size(); i++)
                    for (size_t c = 0; c < cols.size(); c++) vals[c][i] = &batch[i].at(cols[c]);
                staged.emplace_back(new detail::StagedColumns(ctx, cols.size()));
                staged.back()->stage(vals, batch.size());
                steps[k].cols = staged.back()->cols();
            } else {   // the index's own rows, in sorted order (impl_rows), staged once per index
                const Index& from = *spec.steps[(size_t)origin[k] - 1].index;
                (void)from.device();   // positions must refer to impl_rows as they are now
                for (const auto& c : cols) side[k].push_back(*from.side_column(ctx, c));
                steps[k].cols = side[k].data();
                steps[k].source = -origin[k];
            }
        }
        if (cph_join_chain_ex(ctx, steps.data(), (int32_t)S, 0, CPH_MEM_HOST, CPH_CHAIN_POSITIONS, ch) != CPH_OK)
            return Error(std::string("csvplus_hip: ") + cph_last_error(ctx));
        return Error();
    }

    // Where the value of `col` in the row that step k's Join sees comes from, for a whole batch: 0 = every stream row carries
    // it (and no DropColumns in between removed it), t + 1 = no stream row does and every row of steps[t].index does (the
    // earliest such t < k: mergeRows lets the earlier, right-hand row win), -1 = the rows disagree or the column is gone.
    static int columnOrigin(cph_ctx* ctx, const ChainSpec& spec, size_t k, const std::string& col, const std::vector<Row>& batch) {
        auto dropped_between = [&](size_t from_step) {   // a DropColumns behind steps[from_step .. k-1] names the column
            for (size_t j = from_step; j < k; j++)
                for (const auto& d : spec.steps[j].drop_after)
                    if (d == col) return true;
            return false;
        };
        size_t have = 0;
        for (const Row& r : batch) have += HasColumn(r, col) ? 1 : 0;
        if (have == batch.size()) return dropped_between(0) ? -1 : 0;
        if (have != 0) return -1;
        for (size_t t = 0; t < k; t++) {
            const Index& ix = *spec.steps[t].index;
            const Index::Presence p = ix.column_presence(col);   // cached per (index, column): no walk over the rows per batch
            if (p == Index::kSome) return -1;                    // some rows of this index carry it, some do not
            if (p == Index::kAll) return ix.side_column(ctx, col) && !dropped_between(t) ? (int)t + 1 : -1;
        }
        return -1;
    }

public:
    // number of fused device calls made so far (tests: one call per batch)
    static uint64_t& fused_calls() {
        static uint64_t n = 0;
        return n;
    }

private:
    // steps[from..] one after the other over `rows` (rows of step `from`'s stream that all carry its key columns)
    static Error runSteps(cph_ctx* ctx, const ChainSpec& spec, size_t from, std::vector<Row>* rows, const RowFunc& fn) {
        std::vector<Row> cur = std::move(*rows);
        for (size_t k = from; k < spec.steps.size(); k++) {
            const bool last = k + 1 == spec.steps.size();
            const auto& st = spec.steps[k];
            if (k > from) {
                size_t good = 0;
                Error miss;
                for (; good < cur.size(); good++) {
                    std::vector<const std::string*> tmp;
                    miss = SelectValues(cur[good], st.columns, &tmp);
                    if (miss) break;
                }
                if (miss) {
                    cur.resize(good);
                    Error e = runSteps(ctx, spec, k, &cur, fn);
                    return e ? e : miss;
                }
            }
            std::vector<Row> next;
            const RowFunc sink = last ? fn : RowFunc([&](Row row) { next.push_back(std::move(row)); return Error(); });
            Error e = probeBatch(ctx, st.index, st.columns, false, &cur,
                                 st.drop_after.empty() ? sink : RowFunc([&](Row row) {
                                     for (const auto& c : st.drop_after) row.erase(c);
                                     return sink(std::move(row));
                                 }));
            if (e) return e;
            cur = std::move(next);
        }
        return Error();
    }
};

// iterate (:225-249): clones each row, io.EOF -> nil, other errors -> DataSourceError{Line: i}
inline Error iterate(const std::vector<Row>& rows, const RowFunc& fn) {
    Error err;
    size_t i = 0;
    for (; i < rows.size(); i++) {
        err = fn(rows[i]);   // pass-by-value parameter: the callee gets a copy (Clone, :230)
        if (err) break;
    }
    if (!err) return err;
    if (err.is_eof()) return Error();
    return Error::DataSourceError((uint64_t)i, err);
}

// TakeRows (:218-222).  The rows are captured by value (a Go slice header copy shares the
// backing array; here the DataSource owns a snapshot).
inline DataSource TakeRows(std::vector<Row> rows) {
    auto shared = std::make_shared<std::vector<Row>>(std::move(rows));
    return DataSource([shared](const RowFunc& fn) { return iterate(*shared, fn); });
}

// Take (:252-256): anything with Iterate(fn)
template <class T>
inline DataSource Take(std::shared_ptr<T> src) {
    return DataSource([src](const RowFunc& fn) { return src->Iterate(fn); });
}

inline Error Index::Iterate(const RowFunc& fn) const { return iterate(impl_rows, fn); }

inline DataSource Index::Find(const std::vector<std::string>& values) const {
    auto r = find(values);
    return TakeRows(std::vector<Row>(impl_rows.begin() + (long)r.first, impl_rows.begin() + (long)r.second));
}

inline std::shared_ptr<Index> Index::SubIndex(const std::vector<std::string>& values) const {
    if (values.size() >= impl_columns.size()) throw Panic("too many values in SubIndex()");   // :633-635
    auto r = find(values);
    auto sub = std::make_shared<Index>();
    sub->impl_rows.assign(impl_rows.begin() + (long)r.first, impl_rows.begin() + (long)r.second);
    sub->impl_columns.assign(impl_columns.begin() + (long)values.size(), impl_columns.end());
    return sub;
}

// dedup (:810-867).  The adjacent-equal scans (:815-819, :851-855) and the per-group binary search (:828-830)
// are one GPU pass over the sorted key codes (cph_index_dup_groups); the loop below replays the reference's
// bookkeeping over that list of groups, so the surviving rows — including the reference's habit of not
// copying the final row when the last pack ends before it (:851-859 moves rows[lower-1] only while
// lower < len) — are exactly the reference's.
inline Error Index::ResolveDuplicates(const ResolveFunc& resolve) {
    cph_ctx* ctx = Gpu::Default().ctx();
    cph_groups* g = nullptr;
    if (cph_index_dup_groups(ctx, device().h, &g) != CPH_OK)
        throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
    struct Release { cph_groups* g; ~Release() { cph_groups_release(g); } } rel{g};
    if (g->ngroups == 0) return Error();                                            // :821-823
    const size_t n = impl_rows.size();
    size_t dest = (size_t)g->lower[0];                                              // dest = lower-1 (:825)
    for (uint64_t k = 0; k < g->ngroups; k++) {
        const size_t lo = (size_t)g->lower[k], hi = (size_t)g->upper[k];
        std::vector<Row> pack(impl_rows.begin() + (long)lo, impl_rows.begin() + (long)hi);
        auto res = resolve(pack);                                                   // :835
        if (res.second) {                                                           // :835-837: rows stay as they are now
            invalidate_device();
            return res.second;
        }
        if (res.first.size() >= impl_columns.size()) impl_rows[dest++] = std::move(res.first);   // :842-845
        const size_t stop = k + 1 < g->ngroups ? (size_t)g->lower[k + 1] : n - 1;   // :848-859
        for (size_t i = hi; i < stop; i++, dest++)
            if (dest != i) impl_rows[dest] = impl_rows[i];   // a copy, as the reference's slice assignment: the source slot keeps its row
    }
    impl_rows.resize(dest);                                                         // :862-864
    invalidate_device();   // the device twin is rebuilt from the surviving rows on next use
    return Error();
}

// The named rule as the callback a Go program would write (rows of the pack in index order).
inline Index::ResolveFunc Index::resolver_func(const Resolver& rs) {
    return [rs](const std::vector<Row>& pack) -> std::pair<Row, Error> {
        if (rs.rule == CPH_RESOLVE_FIRST) return {pack.front(), Error()};
        if (rs.rule == CPH_RESOLVE_LAST) return {pack.back(), Error()};
        if (rs.rule == CPH_RESOLVE_DROP) return {Row(), Error()};
        const bool want_min = rs.rule == CPH_RESOLVE_MIN;
        size_t best = SIZE_MAX;
        int64_t bi = 0;
        double bf = 0;
        for (size_t i = 0; i < pack.size(); i++) {
            auto it = pack[i].find(rs.column);
            if (it == pack[i].end()) return {Row(), Error("missing column " + quote(rs.column))};   // :170 / :192
            const std::string& v = it->second;
            if (rs.order_kind == CPH_ORDER_BYTES) {
                const int c = best == SIZE_MAX ? 0 : v.compare(pack[best].at(rs.column));   // char_traits<char>: unsigned bytes
                if (best == SIZE_MAX || (want_min ? c < 0 : c > 0)) best = i;
                continue;
            }
            int64_t vi = 0;
            double vf = 0;
            const int32_t k = rs.order_kind == CPH_NUM_INT64 ? Atoi(v, &vi) : ParseFloat(v, &vf);
            if (k != CPH_NUM_OK) {
                const char* what = k == CPH_NUM_ERR_SYNTAX ? "invalid syntax" : k == CPH_NUM_ERR_RANGE ? "value out of range"
                                                           : "not decided by this library (digit separators, hexadecimal floats)";
                return {Row(), Error("column " + quote(rs.column) + ": cannot convert " + quote(v) + " to " +
                                     (rs.order_kind == CPH_NUM_INT64 ? "integer" : "float") + ": " + what)};
            }
            if (rs.order_kind == CPH_NUM_INT64) {
                if (best == SIZE_MAX || (want_min ? vi < bi : vi > bi)) best = i, bi = vi;
            } else if (vf == vf) {   // a NaN never wins
                if (best == SIZE_MAX || (want_min ? vf < bf : vf > bf)) best = i, bf = vf;
            }
        }
        return {pack[best == SIZE_MAX ? 0 : best], Error()};   // nothing but NaNs: the first row
    };
}

inline Error Index::ResolveDuplicates(const Resolver& rs) {
    const bool ordered = rs.rule == CPH_RESOLVE_MIN || rs.rule == CPH_RESOLVE_MAX;
    if (ordered && column_presence(rs.column) != kAll) return ResolveDuplicates(resolver_func(rs));
    cph_ctx* ctx = Gpu::Default().ctx();
    const cph_resolve_opts opts{rs.rule, rs.order_kind, 0 /* the reference's tail rule */, 0};
    // The order column goes in the row order of the twin's BUILD TABLE: row perm[p] = the value of impl_rows[p].  A twin rebuilt
    // over impl_rows has perm = identity and takes the staged side column; the twin IndexOn leaves behind was built over the
    // unsorted source rows, so the values are put where its perm looks for them.
    const cph_strcol* col = nullptr;
    std::unique_ptr<detail::StagedColumns> scattered;
    if (ordered) {
        const uint32_t* perm = nullptr;
        uint64_t pn = 0;
        if (cph_index_perm(device().h, CPH_MEM_HOST, &perm, &pn) != CPH_OK || pn != impl_rows.size())
            throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
        bool identity = true;
        for (uint64_t p = 0; p < pn && identity; p++) identity = perm[p] == p;
        if (identity) {
            col = side_column(ctx, rs.column);
        } else {
            std::vector<std::vector<const std::string*>> vals(1);
            vals[0].resize(impl_rows.size());
            for (uint64_t p = 0; p < pn; p++) vals[0][perm[p]] = &impl_rows[(size_t)p].at(rs.column);
            scattered = std::make_unique<detail::StagedColumns>(ctx, 1);
            scattered->stage(vals, impl_rows.size());
            col = scattered->cols();
        }
    }
    cph_resolved* res = nullptr;
    if (cph_index_resolve(ctx, device().h, &opts, col, CPH_MEM_HOST, nullptr, &res) != CPH_OK)
        throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
    struct Release { cph_resolved* r; ~Release() { cph_resolved_release(r); } } rel{res};
    if (res->nerrors) {
        const std::string& v = impl_rows[(size_t)res->first_error_position].at(rs.column);   // sorted position = subscript of impl_rows
        const char* what = res->first_error_kind == CPH_NUM_ERR_SYNTAX  ? "invalid syntax"
                           : res->first_error_kind == CPH_NUM_ERR_RANGE ? "value out of range"
                                                                        : "not decided by this library (digit separators, hexadecimal floats)";
        return Error("column " + quote(rs.column) + ": cannot convert " + quote(v) + " to " +
                     (rs.order_kind == CPH_NUM_INT64 ? "integer" : "float") + ": " + what);
    }
    if (res->ngroups == 0) return Error();                                          // :821-823
    for (uint64_t i = 0; i < res->nrows; i++) {   // positions ascend: position[i] >= i, so a slot is read before it is overwritten
        const size_t p = (size_t)res->positions[i];
        if (p != (size_t)i) impl_rows[(size_t)i] = std::move(impl_rows[p]);
    }
    impl_rows.resize((size_t)res->nrows);                                           // :862-864
    invalidate_device();
    return Error();
}

inline std::pair<TotalsResult, Error> Index::Totals(const std::vector<Aggregate>& aggs) const {
    TotalsResult out;
    if (aggs.size() > (size_t)CPH_AGG_MAX_SPECS) return {out, Error("too many aggregates in Index.Totals()")};
    for (const Aggregate& a : aggs) {
        if (impl_rows.empty()) break;
        if (!a.expr) {
            if (column_presence(a.column) != kAll) return {out, Error("missing column " + quote(a.column))};
            continue;
        }
        for (const Col& c : a.expr->cols)
            if (!c.has_default && column_presence(c.name) != kAll) return {out, Error("missing column " + quote(c.name))};
    }
    cph_ctx* ctx = Gpu::Default().ctx();
    // an expression is evaluated over the rows in index order by ONE cph_num_eval call (its lowest failing row is the first in
    // index order) and handed in as numbers, scattered to the build table's row order
    std::vector<std::vector<int64_t>> numbers(aggs.size());
    // value columns in the row order of the twin's BUILD TABLE (see ResolveDuplicates): row perm[p] = the value of impl_rows[p]
    std::vector<cph_agg_spec> specs(aggs.size());
    std::vector<std::unique_ptr<detail::StagedColumns>> scattered;
    if (!aggs.empty() && !impl_rows.empty()) {
        const uint32_t* perm = nullptr;
        uint64_t pn = 0;
        if (cph_index_perm(device().h, CPH_MEM_HOST, &perm, &pn) != CPH_OK || pn != impl_rows.size())
            throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
        bool identity = true;
        for (uint64_t p = 0; p < pn && identity; p++) identity = perm[p] == p;
        for (size_t a = 0; a < aggs.size(); a++) {
            specs[a] = cph_agg_spec{aggs[a].op, aggs[a].kind, nullptr, nullptr, CPH_MEM_HOST, 0};
            if (aggs[a].expr) {
                const Expr& e = *aggs[a].expr;
                std::vector<std::vector<const std::string*>> vals(e.cols.size());
                for (size_t c = 0; c < e.cols.size(); c++) {
                    vals[c].resize(impl_rows.size());
                    for (uint64_t q = 0; q < pn; q++) {
                        auto it = impl_rows[(size_t)q].find(e.cols[c].name);
                        vals[c][(size_t)q] = it == impl_rows[(size_t)q].end() ? &e.cols[c].fallback : &it->second;
                    }
                }
                cph_numcol* nc = nullptr;
                int32_t op = -1;
                if (detail::evalStaged(ctx, e, vals, impl_rows.size(), &nc, &op) != CPH_OK)
                    throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
                struct ReleaseNum { cph_numcol* r; ~ReleaseNum() { cph_numcol_release(r); } } reln{nc};
                if (nc->nerrors) {
                    const size_t row = (size_t)nc->first_error_row;
                    return {TotalsResult(), Error(e.errorText(nc->first_error_kind, op, impl_rows[row]))};
                }
                numbers[a].resize(impl_rows.size());   // 8-byte values of either type
                const int64_t* v = static_cast<const int64_t*>(nc->values);
                for (uint64_t q = 0; q < pn; q++) numbers[a][perm[q]] = v[q];
                specs[a].numbers = numbers[a].data();
                continue;
            }
            if (identity) {
                specs[a].col = side_column(ctx, aggs[a].column);
                continue;
            }
            std::vector<std::vector<const std::string*>> vals(1);
            vals[0].resize(impl_rows.size());
            for (uint64_t p = 0; p < pn; p++) vals[0][perm[p]] = &impl_rows[(size_t)p].at(aggs[a].column);
            scattered.push_back(std::make_unique<detail::StagedColumns>(ctx, 1));
            scattered.back()->stage(vals, impl_rows.size());
            specs[a].col = scattered.back()->cols();
        }
    }
    out.ints.resize(aggs.size());
    out.floats.resize(aggs.size());
    if (impl_rows.empty()) return {out, Error()};
    cph_aggregated* res = nullptr;
    if (cph_index_aggregate(ctx, device().h, specs.data(), (int32_t)specs.size(), CPH_MEM_HOST, &res) != CPH_OK)
        throw std::runtime_error(std::string("csvplus: ") + cph_last_error(ctx));
    struct Release { cph_aggregated* r; ~Release() { cph_aggregated_release(r); } } rel{res};
    if (res->nerrors) {
        const Aggregate& a = aggs[(size_t)res->first_error_spec];
        const std::string& v = impl_rows[(size_t)res->first_error_position].at(a.column);   // sorted position = subscript of impl_rows
        const char* what = res->first_error_kind == CPH_NUM_ERR_SYNTAX  ? "invalid syntax"
                           : res->first_error_kind == CPH_NUM_ERR_RANGE ? "value out of range"
                                                                        : "not decided by this library (digit separators, hexadecimal floats)";
        return {TotalsResult(), Error("column " + quote(a.column) + ": cannot convert " + quote(v) + " to " +
                                      (a.kind == CPH_NUM_INT64 ? "integer" : "float") + ": " + what)};
    }
    const size_t ng = (size_t)res->ngroups;
    out.keys.resize(ng);
    out.counts.assign(res->count, res->count + ng);
    for (size_t g = 0; g < ng; g++) {
        const Row& first = impl_rows[(size_t)res->first_position[g]];
        for (const std::string& c : impl_columns) out.keys[g][c] = first.at(c);
    }
    for (size_t a = 0; a < aggs.size(); a++) {
        if (aggs[a].kind == CPH_NUM_INT64) {
            const int64_t* v = static_cast<const int64_t*>(res->values[a]);
            out.ints[a].assign(v, v + ng);
        } else {
            const double* v = static_cast<const double*>(res->values[a]);
            out.floats[a].assign(v, v + ng);
        }
    }
    return {out, Error()};
}

namespace detail {
inline void put_u64(std::ostream& o, uint64_t v) {
    char b[8];
    for (int i = 0; i < 8; i++) b[i] = (char)(v >> (8 * i));
    o.write(b, 8);
}
inline void put_str(std::ostream& o, const std::string& s) {
    put_u64(o, s.size());
    o.write(s.data(), (std::streamsize)s.size());
}
inline bool get_u64(std::istream& in, uint64_t* v) {
    unsigned char b[8];
    if (!in.read(reinterpret_cast<char*>(b), 8)) return false;
    *v = 0;
    for (int i = 0; i < 8; i++) *v |= (uint64_t)b[i] << (8 * i);
    return true;
}
inline bool get_str(std::istream& in, std::string* s, uint64_t limit) {
    uint64_t n;
    if (!get_u64(in, &n) || n > limit) return false;
    s->resize((size_t)n);
    return n == 0 || (bool)in.read(&(*s)[0], (std::streamsize)n);
}
constexpr char kIndexMagic[8] = {'C', 'S', 'V', 'P', 'I', 'D', 'X', '1'};
}  // namespace detail

inline Error Index::WriteTo(const std::string& fileName) const {
    std::ofstream f(fileName, std::ios::binary | std::ios::trunc);
    if (!f) return Error("open " + fileName + ": cannot create file");
    f.write(detail::kIndexMagic, 8);
    detail::put_u64(f, impl_columns.size());                                        // enc.Encode(columns) :674
    for (const auto& c : impl_columns) detail::put_str(f, c);
    detail::put_u64(f, impl_rows.size());                                           // enc.Encode(rows) :675
    for (const Row& r : impl_rows) {
        detail::put_u64(f, r.size());
        for (const auto& kv : r) {
            detail::put_str(f, kv.first);
            detail::put_str(f, kv.second);
        }
    }
    f.close();
    if (!f) {                                                                       // :663-671: no partial files
        std::remove(fileName.c_str());
        return Error("write " + fileName + ": short write");
    }
    return Error();
}

// LoadIndex (:682-705).  Like the reference it trusts the file: rows are taken to be sorted on `columns`.
inline std::pair<std::shared_ptr<Index>, Error> LoadIndex(const std::string& fileName) {
    std::ifstream f(fileName, std::ios::binary);
    if (!f) return {nullptr, Error("open " + fileName + ": no such file or directory")};
    f.seekg(0, std::ios::end);
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    const Error bad(fileName + ": not a csvplus index file");
    char magic[8];
    if (!f.read(magic, 8) || std::memcmp(magic, detail::kIndexMagic, 8) != 0) return {nullptr, bad};
    auto index = std::make_shared<Index>();
    uint64_t ncols, nrows;
    if (!detail::get_u64(f, &ncols) || ncols > size) return {nullptr, bad};
    index->impl_columns.resize((size_t)ncols);
    for (auto& c : index->impl_columns)
        if (!detail::get_str(f, &c, size)) return {nullptr, bad};
    if (!detail::get_u64(f, &nrows) || nrows > size) return {nullptr, bad};
    index->impl_rows.resize((size_t)nrows);
    for (Row& r : index->impl_rows) {
        uint64_t nf;
        if (!detail::get_u64(f, &nf) || nf > size) return {nullptr, bad};
        for (uint64_t i = 0; i < nf; i++) {
            std::string k, v;
            if (!detail::get_str(f, &k, size) || !detail::get_str(f, &v, size)) return {nullptr, bad};
            r.emplace(std::move(k), std::move(v));
        }
    }
    return {index, Error()};
}

}  // namespace csvplus
