"""The full text of every message cph_map_format and cph_map_switch give for a template piece they turn away, and for a row
whose value the FLOAT64 or TIME formatter refuses: each through Format, through a case and through `otherwise`.  The two entry
points share the rules and the report (csrc/map_plan.hpp); only the text in front of a rule's words differs."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P

HOST = N.CPH_MEM_HOST
LITERAL, COLUMN, INT64, FLOAT64, SLICE, TIME = 1, 2, 3, 4, 8, 10
NROWS = 3
OK16 = np.array([0, 4], dtype=np.int64).tobytes()
INTS = np.array([1, 2, 3], dtype=np.int64)
FLOATS = np.array([1.5, 2.5, 3.5], dtype=np.float64)

FORMAT = "cph_map_format: "
CASE = "cph_map_switch: case 0, "
OTHERWISE = "cph_map_switch: otherwise, "


def piece(kind, arg=0, value=None, ints=None, floats=None, prec=0):
    return dict(kind=kind, arg=arg, value=value, ints=ints, floats=floats, prec=prec)


def _pieces(pieces, keep):
    arr = (N.cph_map_piece * len(pieces))()
    for k, p in enumerate(pieces):
        arr[k].kind, arr[k].arg, arr[k].prec = p["kind"], p["arg"], p["prec"]
        if isinstance(p["value"], tuple):   # (pointer or None, len): as given
            arr[k].value.data, arr[k].value.len = p["value"]
        elif p["value"] is not None:
            b = np.frombuffer(p["value"], dtype=np.uint8)
            keep.append(b)
            arr[k].value.data, arr[k].value.len = b.ctypes.data, len(b)
        for field in ("ints", "floats"):
            if p[field] is not None:
                keep.append(p[field])
                setattr(arr[k], field, p[field].ctypes.data)
    keep.append(arr)
    return arr


@pytest.fixture(scope="module")
def column():
    col = StrCol.from_values([b"aa", b"ab", b"ac"], fixed_width=0)
    arr = (N.cph_strcol * 1)()
    arr[0], keep = col.as_c()
    return arr, keep, col


def run_format(ctx, column, pieces):
    keep = []
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_format(ctx.handle, column[0], None, 1, NROWS, _pieces(pieces, keep), len(pieces), HOST, C.byref(out))
    assert not out
    return rc, ctx.last_error()


def run_switch(ctx, column, pieces, in_case):
    """One case over the column: its predicate holds for every row (in_case) or for none, so that every row runs `pieces`."""
    from csvplus_amd.materialize import _pred_program
    keep = []
    carr = (N.cph_map_case * 1)()
    carr[0].prog, carr[0].nops = _pred_program([(P.HAS_PREFIX, 0, b"a" if in_case else b"zz")], keep), 1
    other = [piece(LITERAL, value=b"x")]
    cp, op = (pieces, other) if in_case else (other, pieces)
    carr[0].pieces, carr[0].npieces = _pieces(cp, keep), len(cp)
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_switch(ctx.handle, column[0], None, 1, NROWS, carr, 1, _pieces(op, keep), len(op), HOST, C.byref(out), None)
    assert not out
    return rc, ctx.last_error()


def check_all_three(ctx, column, pieces, format_msg, switch_words):
    """`pieces` through Format, through a case and through `otherwise`: INVALID and exactly these messages."""
    assert run_format(ctx, column, pieces) == (N.CPH_ERR_INVALID, format_msg)
    assert run_switch(ctx, column, pieces, True) == (N.CPH_ERR_INVALID, CASE + switch_words)
    assert run_switch(ctx, column, pieces, False) == (N.CPH_ERR_INVALID, OTHERWISE + switch_words)


RULES = [
    ("literal_no_pointer", piece(LITERAL, value=(None, 3)), "a literal with bytes but no data pointer"),
    ("column_minus_one", piece(COLUMN, arg=-1), "a COLUMN piece outside 0..ncols-1"),
    ("column_ncols", piece(COLUMN, arg=1), "a COLUMN piece outside 0..ncols-1"),
    ("slice_column_minus_one", piece(SLICE, arg=-1, value=OK16), "a SLICE piece's column outside 0..ncols-1"),
    ("slice_column_ncols", piece(SLICE, arg=1, value=OK16), "a SLICE piece's column outside 0..ncols-1"),
    ("slice_8_bytes", piece(SLICE, value=OK16[:8]), "a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer"),
    ("slice_24_bytes", piece(SLICE, value=OK16 + OK16[:8]), "a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer"),
    ("slice_null", piece(SLICE, value=(None, 16)), "a SLICE piece's value is exactly 16 bytes (a cph_map_slice) behind a non-NULL pointer"),
    ("int64_space", piece(INT64, arg=7, ints=INTS), "bad memory space of an INT64 piece"),
    ("int64_no_values", piece(INT64, arg=HOST), "an INT64 piece without values"),
    ("float64_space", piece(FLOAT64, arg=7, floats=FLOATS, prec=2), "bad memory space of a FLOAT64 piece"),
    ("float64_no_values", piece(FLOAT64, arg=HOST, prec=2), "a FLOAT64 piece without values"),
    ("float64_prec_23", piece(FLOAT64, arg=HOST, floats=FLOATS, prec=23), "prec of a FLOAT64 piece outside 0..22"),
    ("float64_prec_minus_one", piece(FLOAT64, arg=HOST, floats=FLOATS, prec=-1), "prec of a FLOAT64 piece outside 0..22"),
    ("time_space", piece(TIME, arg=7, ints=INTS), "bad memory space of a TIME piece"),
    ("time_no_values", piece(TIME, arg=HOST), "a TIME piece without values"),
    ("time_zone_1440", piece(TIME, arg=HOST, ints=INTS, prec=1440), "prec of a TIME piece (the zone in minutes east of UTC) outside -1439..1439"),
    ("time_zone_minus_1440", piece(TIME, arg=HOST, ints=INTS, prec=-1440),
     "prec of a TIME piece (the zone in minutes east of UTC) outside -1439..1439"),
    ("kind_5", piece(5, value=OK16), "unknown piece kind (1..4, 8, 10)"),
    ("kind_9", piece(9, value=OK16), "unknown piece kind (1..4, 8, 10)"),
    ("kind_0", piece(0), "unknown piece kind (1..4, 8, 10)"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("bad,words", [r[1:] for r in RULES], ids=[r[0] for r in RULES])
def test_piece_rule_message(ctx, column, bad, words):
    """The piece stands behind a good literal: cph_map_switch names the alternative and piece 1, cph_map_format neither."""
    check_all_three(ctx, column, [piece(LITERAL, value=b"-"), bad], FORMAT + words, "piece 1: " + words)


@pytest.mark.gpu
def test_refused_float_message(ctx, column):
    """Row 1 holds 2^128; the piece in front of it (piece 1) is a FLOAT64 whose values are all fine."""
    huge = np.array([1.0, 2.0 ** 128, 3.0], dtype=np.float64)
    pieces = [piece(LITERAL, value=b"-"), piece(FLOAT64, arg=HOST, floats=FLOATS, prec=1), piece(FLOAT64, arg=HOST, floats=huge, prec=2)]
    words = "FLOAT64 piece 2, row 1: a finite value of 2^128 or more is not formatted"
    check_all_three(ctx, column, pieces, FORMAT + words, words)


@pytest.mark.gpu
def test_refused_time_message(ctx, column):
    """Row 2 holds the first second of the year 10000 in UTC; row 1's value reaches that year only in a zone east of it."""
    y10k = 253402300800
    secs = np.array([0, y10k - 60, y10k], dtype=np.int64)
    utc = [piece(LITERAL, value=b"-"), piece(TIME, arg=HOST, ints=secs, prec=0)]
    words = "TIME piece 1, row 2: the local year of 253402300800 is outside 0000..9999"
    check_all_three(ctx, column, utc, FORMAT + words, words)
    east = [piece(TIME, arg=HOST, ints=INTS, prec=0), piece(TIME, arg=HOST, ints=secs, prec=1)]
    words = "TIME piece 1, row 1: the local year of 253402300740 is outside 0000..9999"
    check_all_three(ctx, column, east, FORMAT + words, words)
