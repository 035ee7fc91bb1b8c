"""RFC 3339 timestamps as the library converts them, in plain Python: the host model of cph_col_to_number's
CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO kinds (`time.Parse(time.RFC3339, s)` then t.Unix() / t.UnixNano()) and of the
CPH_MAP_TIME piece (`time.Unix(v, 0).In(time.FixedZone("", 60 * zone)).Format(time.RFC3339)`).

Written from the rules in include/csvplus_hip.h with integer arithmetic only — no datetime, and not the device's code — so
that it can be checked against datetime / calendar.timegm on one side and the device on the other.  Nothing here touches
the GPU.

The accepted set, with D a byte '0'..'9', the value in full:

    DDDD-DD-DDTDD:DD:DD  [ '.' D{1,9} ]  ( 'Z' | ('+'|'-') DD:DD )

and a value's status is decided in this order: UNSUPPORTED when it matches only with a one-digit hour, ',' for the
fraction's '.', or more than 9 fraction digits; SYNTAX when it does not match at all; RANGE for a month, day (proleptic
Gregorian, year 0000 is a leap year), hour, minute or second (> 59) out of range; UNSUPPORTED for a zone hour > 23 or a zone
minute > 59; UNSUPPORTED, nanoseconds only, when the result does not fit an int64.  The value at an error is 0.
"""
from __future__ import annotations

import re

from .predicates import INT64_MAX, INT64_MIN, NUM_ERR_RANGE, NUM_ERR_SYNTAX, NUM_ERR_UNSUPPORTED, NUM_OK, _bytes

MIN_SECONDS = -62167219200   # 0000-01-01T00:00:00Z
MAX_SECONDS = 253402300799   # 9999-12-31T23:59:59Z
MAX_ZONE = 1439              # minutes east or west of UTC

_STRICT = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})T([0-9]{2}):([0-9]{2}):([0-9]{2})(?:\.([0-9]{1,9}))?(?:Z|([+-])([0-9]{2}):([0-9]{2}))", re.ASCII)
_RELAXED = re.compile(rb"[0-9]{4}-[0-9]{2}-[0-9]{2}T[0-9]{1,2}:[0-9]{2}:[0-9]{2}(?:[.,][0-9]+)?(?:Z|[+-][0-9]{2}:[0-9]{2})", re.ASCII)


def is_leap(year: int) -> bool:
    return (year % 4 == 0 and year % 100 != 0) or year % 400 == 0


def days_in_month(year: int, month: int) -> int:
    if month == 2:
        return 29 if is_leap(year) else 28
    return 30 if month in (4, 6, 9, 11) else 31


def days_from_civil(year: int, month: int, day: int) -> int:
    """Days since 1970-01-01 of a proleptic Gregorian date (any year): whole years, leap days, then the months."""
    y = year - 1   # the years completed in front of this one, counted from year 1
    days = y * 365 + y // 4 - y // 100 + y // 400   # Python's // floors: year 0 and below work too
    days += sum(days_in_month(year, m) for m in range(1, month)) + day - 1
    return days - 719162   # 1970-01-01 is day 719162 of that count


def civil_from_days(days: int) -> tuple:
    """The inverse of days_from_civil: (year, month, day)."""
    n = days + 719162          # days since 0001-01-01
    cycles, n = divmod(n, 146097)
    centuries = min(n // 36524, 3)   # the fourth century of a cycle is a day longer: its last day stays in it
    n -= centuries * 36524
    fours, n = divmod(n, 1461)
    years = min(n // 365, 3)         # likewise the fourth year
    n -= years * 365
    year = 1 + 400 * cycles + 100 * centuries + 4 * fours + years
    month = 1
    while n >= days_in_month(year, month):
        n -= days_in_month(year, month)
        month += 1
    return year, month, n + 1


def parse_model(value, unit: str = "s") -> tuple:
    """(status, value) of one RFC 3339 text: NUM_OK and t.Unix() (unit "s": whole seconds, the floor) or t.UnixNano()
    (unit "ns"); NUM_ERR_* and 0 otherwise."""
    if unit not in ("s", "ns"):
        raise ValueError(f"unit must be 's' or 'ns', not {unit!r}")
    b = _bytes(value)
    m = _STRICT.fullmatch(b)
    if m is None:
        return (NUM_ERR_UNSUPPORTED if _RELAXED.fullmatch(b) else NUM_ERR_SYNTAX), 0
    year, month, day, hour, minute, second = (int(m.group(k)) for k in range(1, 7))
    if not 1 <= month <= 12 or not 1 <= day <= days_in_month(year, month) or hour > 23 or minute > 59 or second > 59:
        return NUM_ERR_RANGE, 0
    offset = 0
    if m.group(8) is not None:
        zh, zm = int(m.group(9)), int(m.group(10))
        if zh > 23 or zm > 59:
            return NUM_ERR_UNSUPPORTED, 0
        offset = (zh * 3600 + zm * 60) * (-1 if m.group(8) == b"-" else 1)
    secs = days_from_civil(year, month, day) * 86400 + hour * 3600 + minute * 60 + second - offset
    if unit == "s":
        return NUM_OK, secs   # the fraction only adds: the floor
    frac = int((m.group(7) or b"0").ljust(9, b"0"))
    ns = secs * 1_000_000_000 + frac
    if not INT64_MIN <= ns <= INT64_MAX:
        return NUM_ERR_UNSUPPORTED, 0
    return NUM_OK, ns


def in_range(seconds: int, zone_minutes: int = 0) -> bool:
    """The local year of `seconds` in the zone lies in 0000..9999: what a Time part formats."""
    return MIN_SECONDS <= int(seconds) + 60 * int(zone_minutes) <= MAX_SECONDS


def check_zone(zone_minutes, who="zone_minutes") -> int:
    if isinstance(zone_minutes, bool) or int(zone_minutes) != zone_minutes or not -MAX_ZONE <= int(zone_minutes) <= MAX_ZONE:
        raise ValueError(f"{who}: the zone must be within -{MAX_ZONE}..{MAX_ZONE} minutes, not {zone_minutes!r}")
    return int(zone_minutes)


def format_model(seconds, zone_minutes: int = 0) -> bytes:
    """time.Unix(seconds, 0).In(time.FixedZone("", 60 * zone_minutes)).Format(time.RFC3339): 20 bytes with 'Z' for zone 0,
    25 bytes with +HH:MM / -HH:MM otherwise.  Raises ValueError where the local year leaves 0000..9999: the model refuses
    what the device refuses."""
    zone = check_zone(zone_minutes, "format_model")
    seconds = int(seconds)
    if not in_range(seconds, zone):
        raise ValueError(f"format_model: the local year of {seconds} in zone {zone} is outside 0000..9999")
    days, sod = divmod(seconds + 60 * zone, 86400)
    year, month, day = civil_from_days(days)
    text = b"%04d-%02d-%02dT%02d:%02d:%02d" % (year, month, day, sod // 3600, sod // 60 % 60, sod % 60)
    if zone == 0:
        return text + b"Z"
    return text + b"%c%02d:%02d" % (b"-" if zone < 0 else b"+", abs(zone) // 60, abs(zone) % 60)
