"""The plain-Python models of the time feature (csvplus_amd/timeconv.py), the op and kind codes, and the compile / matches /
render support of predicates.TimeCmp and mapping.Time.  CPU only: nothing here touches the GPU."""
from __future__ import annotations

import calendar
import datetime as dt
import random
import re
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import _native as N, mapping as M, predicates as P, timeconv as T
from tests.time_cases import BASE25, TABLE, mutations

ROOT = Path(__file__).resolve().parent.parent
UTC = dt.timezone.utc


def test_codes_match_the_header():
    text = (ROOT / "include" / "csvplus_hip.h").read_text()

    def const(name):
        return int(re.search(rf"\b{name}\s*=\s*(-?\d+)", text).group(1))

    assert (N.CPH_NUM_TIME_UNIX, N.CPH_NUM_TIME_UNIXNANO) == (const("CPH_NUM_TIME_UNIX"), const("CPH_NUM_TIME_UNIXNANO")) == (4, 5)
    assert N.CPH_MAP_TIME == M.TIME == const("CPH_MAP_TIME") == 10
    names = ["CPH_PRED_TIME_" + r for r in ("LT", "LE", "EQ", "NE", "GE", "GT")]
    assert [const(n) for n in names] == [getattr(N, n) for n in names] == list(range(48, 54))
    assert P.TIME_LT == 48
    assert "timestamp parsing" not in text


def test_days_from_civil_against_datetime_for_every_month_of_years_1_to_9999():
    # every first and last day of every month, and a stride of days in between
    for year in range(1, 10000):
        for month in range(1, 13):
            last = calendar.monthrange(year, month)[1]
            assert T.days_in_month(year, month) == last
            for day in (1, last):
                want = dt.date(year, month, day).toordinal() - 719163
                assert T.days_from_civil(year, month, day) == want
                assert T.civil_from_days(want) == (year, month, day)
    first, end = dt.date(1, 1, 1).toordinal() - 719163, dt.date(9999, 12, 31).toordinal() - 719163
    for days in range(first, end + 1, 97):
        d = dt.date.fromordinal(days + 719163)
        assert T.civil_from_days(days) == (d.year, d.month, d.day)
        assert T.days_from_civil(d.year, d.month, d.day) == days
    # year 0000 is outside datetime: a leap year in front of 0001-01-01
    assert T.days_from_civil(0, 12, 31) == first - 1 and T.days_from_civil(0, 1, 1) == first - 366
    assert T.civil_from_days(first - 1) == (0, 12, 31) and T.civil_from_days(first - 366) == (0, 1, 1)
    assert T.civil_from_days(first - 366 + 59) == (0, 2, 29)
    assert T.MIN_SECONDS == (first - 366) * 86400 and T.MAX_SECONDS == (end + 1) * 86400 - 1


def test_parse_and_format_against_datetime():
    rng = random.Random(5)
    lo = calendar.timegm((1, 1, 2, 0, 0, 0))       # a day inside the ends, so that every zone stays within datetime's range
    hi = calendar.timegm((9999, 12, 30, 23, 59, 59))
    for k in range(20000):
        v = rng.randint(lo, hi) if k % 4 else rng.randint(-10**9, 2 * 10**9)
        zone = rng.choice((0, 60, -330, 1439, -1439, rng.randint(-1439, 1439)))
        tz = dt.timezone(dt.timedelta(minutes=zone))
        local = dt.datetime(1970, 1, 1, tzinfo=UTC) + dt.timedelta(seconds=v)
        local = local.astimezone(tz)
        want = local.strftime("%Y").rjust(4, "0") + local.strftime("-%m-%dT%H:%M:%S")
        want += "Z" if zone == 0 else "%s%02d:%02d" % ("-" if zone < 0 else "+", abs(zone) // 60, abs(zone) % 60)
        got = T.format_model(v, zone)
        assert got == want.encode(), (v, zone)
        assert T.parse_model(got, "s") == (0, v)
        assert calendar.timegm(local.utctimetuple()) == v
        ns = rng.randint(0, 999_999_999)
        nd = rng.randint(1, 9)
        frac = ("%09d" % ns)[:nd]
        text = got[:19] + b"." + frac.encode() + got[19:]
        assert T.parse_model(text, "s") == (0, v)
        st, n = T.parse_model(text, "ns")
        total = v * 10**9 + int(frac.ljust(9, "0"))
        assert (st, n) == ((0, total) if -2**63 <= total < 2**63 else (3, 0))


def test_classification_table_of_the_model():
    for text, st_s, st_ns in TABLE + mutations():
        s, v = T.parse_model(text, "s")
        n, w = T.parse_model(text, "ns")
        assert (s, n) == (st_s, st_ns), text
        assert (s == 0 or v == 0) and (n == 0 or w == 0)
    assert T.parse_model(b"1969-12-31T23:59:59.5Z", "s") == (0, -1)
    assert T.parse_model(b"1969-12-31T23:59:59.5Z", "ns") == (0, -500_000_000)
    assert T.parse_model(b"0000-01-01T00:00:00Z", "s") == (0, -62167219200)
    assert T.parse_model(b"9999-12-31T23:59:59Z", "s") == (0, 253402300799)
    assert T.parse_model(b"2016-09-14T00:30:00+02:00", "s") == T.parse_model(b"2016-09-13T22:30:00Z", "s")
    assert T.parse_model(b"1677-09-21T00:12:43.145224192Z", "ns") == (0, -2**63)
    assert T.parse_model(b"2262-04-11T23:47:16.854775807Z", "ns") == (0, 2**63 - 1)
    assert T.parse_model(BASE25, "s")[0] == 0
    with pytest.raises(ValueError):
        T.parse_model(b"", "ms")


def test_format_model_refuses_what_the_device_refuses():
    assert T.format_model(-62167219200) == b"0000-01-01T00:00:00Z"
    assert T.format_model(253402300799) == b"9999-12-31T23:59:59Z"
    assert T.format_model(-1) == b"1969-12-31T23:59:59Z"
    assert T.format_model(0, -330) == b"1969-12-31T18:30:00-05:30"
    assert T.format_model(0, 1439) == b"1970-01-01T23:59:00+23:59"
    assert T.format_model(253402300799 + 60, -1) == b"9999-12-31T23:59:59-00:01"
    for v, zone in ((253402300799, 1), (-62167219200, -1), (253402300800, 0), (-62167219201, 0)):
        with pytest.raises(ValueError):
            T.format_model(v, zone)
    for zone in (1440, -1440, 0.5, True):
        with pytest.raises(ValueError):
            T.format_model(0, zone)


def test_timecmp_compile_matches_run_ops():
    p = P.TimeCmp("ts", ">=", "2016-09-14T00:00:00Z")
    names, ops = P.compile(p, ["id", "ts"])
    assert names == ["ts"] and ops == [(52, 0, b"2016-09-14T00:00:00Z")]
    assert P.compile(p, ["id"]) == ([], [(52, -1, b"2016-09-14T00:00:00Z")])
    for k, rel in enumerate(P.RELS):
        assert P.compile(P.TimeCmp("ts", rel, "2016-09-14T00:00:00Z"), ["ts"])[1][0][0] == 48 + k
    same = {"ts": "2016-09-14T02:00:00+02:00"}      # the literal's instant in another zone: equal, though its bytes are larger
    before = {"ts": b"2016-09-14T01:59:59.9+02:00"}
    assert p(same) and not p(before)
    assert P.TimeCmp("ts", "==", "2016-09-14T00:00:00Z")(same) and not P.StrCmp("ts", "==", "2016-09-14T00:00:00Z")(same)
    for rel in P.RELS:   # a row that does not convert, or lacks the column, is false under every relation
        q = P.TimeCmp("ts", rel, "2016-09-14T00:00:00Z")
        for bad in ({"ts": ""}, {"ts": "2016-13-14T00:00:00Z"}, {"ts": "2016-09-14T0:00:00Z"}, {"other": "x"}):
            assert not q(bad)
            assert not P.run_ops(P.compile(q, list(bad))[1], list(bad.values()))
    both = P.All(P.TimeCmp("ts", ">=", "2016-09-14T00:00:00Z"), P.Not(P.TimeCmp("ts", ">", "2016-09-14T00:00:00Z")))
    names, ops = P.compile(both, ["ts"])
    assert P.run_ops(ops, [same["ts"]]) and both(same) and not both(before)
    for lit in ("2016-09-14T00:00:00.5Z", "2016-09-14", "2016-13-14T00:00:00Z", "2016-09-14T0:00:00Z", ""):
        with pytest.raises(ValueError):
            P.TimeCmp("ts", "<", lit)
    with pytest.raises(ValueError):
        P.TimeCmp("ts", "~", "2016-09-14T00:00:00Z")
    with pytest.raises(ValueError):   # the term counts against the limit of 32
        P.compile(P.All(*[P.TimeCmp("ts", "<", "2016-09-14T00:00:00Z")] * 33), ["ts"])


def test_time_part_compile_and_render():
    t = M.Time([0, -1, 1473842902], 60)
    names, pieces = M.compile(M.Format("at ", t, "!"), ["id"])
    assert names == [] and [p[0] for p in pieces] == [M.LITERAL, M.TIME, M.LITERAL] and pieces[1][2] is t
    assert M.render(M.Format("at ", t), {}, 2) == b"at 2016-09-14T09:48:22+01:00"
    assert M.render(M.Time(np.array([0], dtype=np.int64)), {}, 0) == b"1970-01-01T00:00:00Z"
    from csvplus_amd import expr as E
    hour = M.Time.of((E.IntCol("t") / 3600) * 3600, -330)
    assert M.columns(M.Format(hour)) == ["t"]
    assert M.render(hour, {"t": "1473842902"}) == T.format_model(1473842902 // 3600 * 3600, -330)
    assert M.compile(hour, ["t"])[1][0][0] == M.TIME
    sw = M.When(P.TimeCmp("ts", "<", "2000-01-01T00:00:00Z"), "old", M.Time([5], 0))
    assert M.columns(sw) == ["ts"]
    assert M.render(sw, {"ts": "1999-12-31T23:59:59-01:00"}) == b"1970-01-01T00:00:05Z"
    assert M.render(sw, {"ts": "1999-12-31T23:59:59+01:00"}) == b"old"
    for zone in (1440, -1440):
        with pytest.raises(ValueError):
            M.Time([0], zone)
    with pytest.raises(ValueError):
        M.render(M.Time([253402300799], 1), {}, 0)
    with pytest.raises(TypeError):
        M.Time.of(E.FloatCol("t"))
    with pytest.raises(ValueError):
        M.render(M.Time.on_device(4096, 1), {}, 0)
