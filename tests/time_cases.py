"""The classification table of cph_col_to_number's time kinds (include/csvplus_hip.h), shared by test_time_model.py (the
Python model against the table) and test_time.py (the device against the model).  One row per rule:
(text, status of CPH_NUM_TIME_UNIX, status of CPH_NUM_TIME_UNIXNANO); 0 OK, 1 syntax, 2 range, 3 unsupported."""

OK, SYN, RNG, UNS = 0, 1, 2, 3
BASE25 = b"2016-09-14T08:48:22+02:00"

VALID = [
    (b"2016-09-14T08:48:22Z", OK, OK),
    (b"2016-09-14T08:48:22+01:00", OK, OK),
    (b"2016-09-14T08:48:22-00:00", OK, OK),
    (b"2016-09-14T08:48:22+23:59", OK, OK),
    (b"2016-09-14T08:48:22-23:59", OK, OK),
    (b"2016-09-14T08:48:22.5Z", OK, OK),
    (b"2016-09-14T08:48:22.125Z", OK, OK),
    (b"2016-09-14T08:48:22.123456789Z", OK, OK),
    (b"2016-09-14T08:48:22.5+01:00", OK, OK),
    (b"2016-09-14T08:48:22.125-05:30", OK, OK),
    (b"2016-09-14T08:48:22.123456789-05:30", OK, OK),
    (b"2016-09-14T08:48:22.12345678+05:30", OK, OK),
    (b"2016-09-14T08:48:22.1234567+05:30", OK, OK),
    (b"0000-01-01T00:00:00Z", OK, UNS),
    (b"9999-12-31T23:59:59Z", OK, UNS),
    (b"1969-12-31T23:59:59.5Z", OK, OK),
    (b"2000-02-29T12:00:00Z", OK, OK),
    (b"0000-02-29T00:00:00Z", OK, UNS),
    (b"1677-09-21T00:12:44Z", OK, OK),
    (b"2262-04-11T23:47:16Z", OK, OK),
    (b"1677-09-21T00:12:43.145224192Z", OK, OK),
    (b"2262-04-11T23:47:16.854775807Z", OK, OK),
]
RANGE = [
    (b"1900-02-29T00:00:00Z", RNG, RNG),
    (b"2001-02-29T00:00:00Z", RNG, RNG),
    (b"2016-00-14T08:48:22Z", RNG, RNG),
    (b"2016-13-14T08:48:22Z", RNG, RNG),
    (b"2016-09-00T08:48:22Z", RNG, RNG),
    (b"2016-09-32T08:48:22Z", RNG, RNG),
    (b"2016-04-31T08:48:22Z", RNG, RNG),
    (b"2016-09-14T24:00:00Z", RNG, RNG),
    (b"2016-09-14T08:60:22Z", RNG, RNG),
    (b"2016-09-14T23:59:60Z", RNG, RNG),
    (b"2016-13-14T08:48:22+24:00", RNG, RNG),   # decided in front of the zone's rule
]
UNSUPPORTED = [
    (b"2016-09-14T8:48:22Z", UNS, UNS),
    (b"2016-09-14T8:48:22+01:00", UNS, UNS),
    (b"2016-13-14T8:48:22Z", UNS, UNS),          # decided in front of the range rule
    (b"2016-09-14T08:48:22,5Z", UNS, UNS),
    (b"2016-09-14T08:48:22.1234567890Z", UNS, UNS),
    (b"2016-09-14T08:48:22.1234567890+01:00", UNS, UNS),
    (b"2016-09-14T08:48:22." + b"1234567890" * 4 + b"Z", UNS, UNS),   # longer than any valid value
    (b"2016-09-14T08:48:22+24:00", UNS, UNS),
    (b"2016-09-14T08:48:22+01:60", UNS, UNS),
    (b"1677-09-21T00:12:43Z", OK, UNS),
    (b"2262-04-11T23:47:17Z", OK, UNS),
    (b"1677-09-21T00:12:43.145224191Z", OK, UNS),
    (b"2262-04-11T23:47:16.854775808Z", OK, UNS),
]
SYNTAX = [
    (b"", SYN, SYN),
    (b"2016-09-14T08:48:22", SYN, SYN),
    (b"2016-09-14t08:48:22Z", SYN, SYN),
    (b"2016-09-14T08:48:22z", SYN, SYN),
    (b"2016-09-14 08:48:22Z", SYN, SYN),
    (b"2016-09-14T08:48:22.Z", SYN, SYN),
    (b"2016-09-14T08:48:22.+01:00", SYN, SYN),
    (b"2016-09-14T08:48:22+0100", SYN, SYN),
    (b"2016-09-14T08:48:22Z ", SYN, SYN),
    (b"2016-09-14T08:48:22+01:00x", SYN, SYN),
    (b" 2016-09-14T08:48:22Z", SYN, SYN),
    (b"2016-09-14T08:48:22.5", SYN, SYN),
    (b"2016-09-14T08:48:22.12345678x+01:00", SYN, SYN),
    (b"2016-09-14", SYN, SYN),
    (b"Z", SYN, SYN),
    (b"x" * 300, SYN, SYN),
]


def mutations():
    """BASE25 with one wrong byte: a non-digit in each digit position, a wrong byte in each separator position."""
    out = []
    for p, c in enumerate(BASE25):
        for w in (b"x/: -Z" if 0x30 <= c <= 0x39 else b"x0/;tz "):
            if w != c:
                out.append((BASE25[:p] + bytes([w]) + BASE25[p + 1:], SYN, SYN))
    return out


TABLE = VALID + RANGE + UNSUPPORTED + SYNTAX
