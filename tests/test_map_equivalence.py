"""cph_map_format and cph_map_switch run the same per-row code (csrc/map_device.hpp) behind the same host plan
(csrc/map_plan.hpp): one template T through cph_map_format against When(p, T, T), whose predicate holds for every other row,
must give the same offsets and the same data, byte for byte — at the wave, the 256-row tile and two tiles plus one, for each
piece set, with 0, 1, 8 and (the generic instantiation) 9 columns."""
import re

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Float, Format, Int, Time, When
from csvplus_amd.materialize import map_column, map_switch

ROW_COUNTS = [1, 64, 65, 255, 256, 257, 513]
NMAX = max(ROW_COUNTS)


def _tables():
    """Nine value columns c0..c8 of 0..13 random bytes and the predicate's column `par`; c0 and `par` begin with b"e" in the
    even rows and b"o" in the odd ones.  Made once, never changed."""
    rng = np.random.default_rng(20)
    parity = [b"e" if i % 2 == 0 else b"o" for i in range(NMAX)]
    t = {f"c{k}": [bytes(rng.integers(0, 256, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(NMAX)] for k in range(9)}
    t["c0"] = [parity[i] + v for i, v in enumerate(t["c0"])]
    t["par"] = parity
    return t


TABLE = _tables()
INTS = (np.arange(NMAX, dtype=np.int64) - 7) * 1_000_000_007 * (np.arange(NMAX, dtype=np.int64) % 5 - 2)
FLOATS = (np.arange(NMAX, dtype=np.float64) - 100.0) * 1234.5678 / 7.0
SECONDS = np.arange(NMAX, dtype=np.int64) * 86_399 * 1000 - 5_000_000_000   # 1811 .. 3374


def template(pieces, ncols, n, floats=FLOATS):
    """Literal + Col + Int; "slice": + a slice of the first column; "float": + Float and Time."""
    parts = ["<"] + [Col(f"c{k}") for k in range(ncols)] + [Int(INTS[:n])]
    if pieces != "base" and ncols:
        parts.append(Col("c0")[1:-2])
    if pieces == "float":
        parts += [Float(floats[:n], 3), Time(SECONDS[:n], 90)]
    return Format(*parts)


def columns(ncols, n, table=TABLE):
    """The template's columns; without any, the column that the predicate alone reads."""
    return {k: StrCol.from_values(table[k][:n], fixed_width=0) for k in ([f"c{j}" for j in range(ncols)] or ["par"])}


def offsets_and_data(cb):
    c = cb.ptr.contents.col
    assert c.offset_bits == 64 and c.nrows == cb.nrows
    return N._ptr_array(c.offsets, cb.nrows + 1, np.uint64).copy(), N._ptr_array(c.data, cb.nbytes, np.uint8).copy()


def both(ctx, cols, t, n):
    """(offsets, data) of T through cph_map_format and of When(every other row, T, T) through cph_map_switch."""
    cb = map_column(ctx, cols, t, nrows=n)
    try:
        one = offsets_and_data(cb)
    finally:
        cb.release()
    cb, which = map_switch(ctx, cols, When(P.HasPrefix(next(iter(cols)), "e"), t, t), nrows=n, want_which=True)
    try:
        assert which.tolist() == [i % 2 for i in range(n)]
        return one, offsets_and_data(cb)
    finally:
        cb.release()


@pytest.mark.gpu
@pytest.mark.parametrize("pieces,ncols", [(p, c) for p in ("base", "slice", "float") for c in (0, 1, 8, 9) if (p, c) != ("slice", 0)])   # a slice reads a column
def test_format_equals_switch_of_the_same_template(ctx, pieces, ncols):
    for n in ROW_COUNTS:
        (offs_f, data_f), (offs_s, data_s) = both(ctx, columns(ncols, n), template(pieces, ncols, n), n)
        assert len(offs_f) == n + 1 and offs_f[0] == 0 and int(offs_f[-1]) == len(data_f) > 0
        np.testing.assert_array_equal(offs_f, offs_s, err_msg=f"offsets, n={n}")
        np.testing.assert_array_equal(data_f, data_s, err_msg=f"data, n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", ["base", "slice", "float"])
def test_a_tile_beyond_the_stage(ctx, pieces):
    """Rows 256..511 carry a 100-byte value: that tile's 25 KB do not fit the 16 KB stage and go to global memory row by row,
    between two tiles that go through the stage."""
    n = 513
    table = dict(TABLE)
    table["c0"] = [v + bytes(range(100, 200)) if 256 <= i < 512 else v for i, v in enumerate(TABLE["c0"])]
    (offs_f, data_f), (offs_s, data_s) = both(ctx, columns(1, n, table), template(pieces, 1, n), n)
    assert int(offs_f[512] - offs_f[256]) > 16 * 1024 and int(offs_f[513] - offs_f[512]) + 48 <= 16 * 1024
    if pieces == "base":
        assert int(offs_f[256]) + 48 <= 16 * 1024
    np.testing.assert_array_equal(offs_f, offs_s)
    np.testing.assert_array_equal(data_f, data_s)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [255, 256])
def test_a_refused_value_at_a_tile_edge(ctx, row):
    """2^128 in the last row of the first tile or the first row of the second: both entry points name that row."""
    n = 513
    floats = FLOATS.copy()
    floats[row] = 2.0 ** 128
    floats[400] = -(2.0 ** 200)   # a later one does not count
    t, cols = template("float", 1, n, floats), columns(1, n)
    rows = []
    for call in (lambda: map_column(ctx, cols, t, nrows=n), lambda: map_switch(ctx, cols, When(P.HasPrefix("c0", "e"), t, t), nrows=n)):
        with pytest.raises(N.CphError) as e:
            call()
        assert e.value.code == N.CPH_ERR_INVALID
        rows.append(int(re.search(r"FLOAT64 piece \d+, row (\d+): a finite value of 2\^128 or more is not formatted$", e.value.msg).group(1)))
    assert rows == [row, row]
