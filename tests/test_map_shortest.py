"""Map with FLOAT64_SHORTEST pieces (mapping.Float.shortest, cph_map_format's CPH_MAP_FLOAT64_SHORTEST):
strconv.FormatFloat(v, 'e' / 'f' / 'g', -1, 64) on the device.  CPU: the power-of-ten table against its formula, the host model
`ftoa_shortest` against pinned answers and against float(), the compiler's rules, the struct layout.  Under `-m gpu`: the
device against `ftoa_shortest` / `render`, byte for byte, never against itself."""
import ctypes as C
import math
import re
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Float, Format, Int, Switch, Time, When
from test_map import device_array, model, run_map
from test_map_switch import model as switch_model
from test_map_switch import run_switch

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "csvplus_amd" / "csrc" / "pow10_table.inc"
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
TILE = 256         # kMatThreads
STAGE = 16 * 1024  # kMatStage
FMTS = "eEfgG"
SHORTEST = M.FLOAT64_SHORTEST


def _bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _next(v, up):
    return math.nextafter(v, math.inf if up else -math.inf)


NAN_PAYLOADS = [_bits(0xFFF8000000001234), _bits(0x7FF0000000000001), _bits(0x7FFFFFFFFFFFFFFF), math.nan]
SUBNORMAL_9_5E_88 = math.ldexp(8511030020275656, -342)   # 9.5e-88: two digits
PINNED = [   # value, {format: text}
    (1.0, {"e": "1e+00", "f": "1", "g": "1"}),
    (100000.0, {"e": "1e+05", "f": "100000", "g": "100000"}),
    (1000000.0, {"g": "1e+06"}),
    (123456.7, {"g": "123456.7"}),
    (1234567.8, {"e": "1.2345678e+06", "f": "1234567.8", "g": "1.2345678e+06"}),
    (0.0001, {"g": "0.0001"}),
    (0.00001, {"f": "0.00001", "g": "1e-05"}),
    (0.3, {"e": "3e-01"}),
    (1e21, {"g": "1e+21"}),
    (1e23, {"e": "1e+23", "f": "100000000000000000000000", "g": "1e+23"}),
    (99999999999999974834176.0, {"e": "9.999999999999997e+22"}),
    (2.0 ** 53, {"f": "9007199254740992", "g": "9.007199254740992e+15"}),
    (2.0 ** 976, {"e": "6.386688990511104e+293"}),
    (SUBNORMAL_9_5E_88, {"e": "9.5e-88"}),
    (5e-324, {"e": "5e-324", "f": "0." + "0" * 323 + "5"}),
    (1.7976931348623157e308, {"e": "1.7976931348623157e+308", "f": "17976931348623157" + "0" * 292}),
    (-0.0, {"e": "-0e+00", "f": "-0", "g": "-0"}),
    (0.0, {"e": "0e+00", "f": "0", "g": "0"}),
    (math.inf, {"e": "+Inf", "f": "+Inf", "g": "+Inf", "E": "+Inf", "G": "+Inf"}),
    (-math.inf, {"e": "-Inf", "f": "-Inf", "g": "-Inf"}),
    (100000.0, {"E": "1E+05"}),
    (1000000.0, {"G": "1E+06"}),
    (-2.2250738585072014e-308, {"e": "-2.2250738585072014e-308", "f": "-0." + "0" * 307 + "22250738585072014"}),
]


def random_finite(seed, count):
    """Random 64-bit patterns read as doubles, the finite ones."""
    v = np.random.default_rng(seed).integers(0, 2 ** 64, count + count // 256 + 64, dtype=np.uint64).view(np.float64)
    v = v[np.isfinite(v)][:count]
    assert len(v) == count
    return v


def powers_of_two_with_neighbours():
    out = []
    for e in range(-1074, 1024):
        v = math.ldexp(1.0, e)
        out += [v, _next(v, True)] + ([_next(v, False)] if e > -1074 else [0.0])
    return out


def powers_of_ten_with_neighbours():
    out = []
    for k in range(-323, 309):
        v = float("1e%d" % k)
        out += [_next(v, False), v, _next(v, True)]
    return out


def subnormals(seed, count):
    rng = np.random.default_rng(seed)
    return [_bits(max(1, int(rng.integers(0, 2 ** 52)) >> int(rng.integers(0, 52)))) for _ in range(count)]


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_pow10_table_entry_by_entry():
    """The committed table against its formula, restated: 10^e scaled by a power of two into [2^127, 2^128) and rounded up."""
    text = TABLE.read_text()
    pairs = re.findall(r"^\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\},$", text, re.M)
    assert len(pairs) == 617
    assert len([ln for ln in text.splitlines() if ln and not ln.startswith("//")]) == 617   # nothing but entries and comments
    for e, (hi, lo) in zip(range(-292, 325), pairs):
        have = (int(hi, 16) << 64) | int(lo, 16)
        if e >= 0:
            p = 10 ** e
            down = p.bit_length() - 128
            want = p << -down if down <= 0 else (p + (1 << down) - 1) >> down
            exact = down <= 0 or p % (1 << down) == 0
        else:
            p = 10 ** -e
            want = ((1 << (127 + p.bit_length())) + p - 1) // p
            exact = False
        assert have == want, e
        assert 1 << 127 <= have < 1 << 128, e
        assert exact == (0 <= e <= 55), e   # rounded up everywhere else
    assert subprocess.run([sys.executable, str(ROOT / "tools" / "gen_pow10_table.py"), "--check"]).returncode == 0


def test_ftoa_shortest_pinned_answers():
    for v, texts in PINNED:
        for fmt, text in texts.items():
            assert M.ftoa_shortest(v, fmt) == text.encode(), (v, fmt)
    for v in NAN_PAYLOADS:
        for fmt in FMTS:
            assert M.ftoa_shortest(v, fmt) == b"NaN"
    assert len(M.ftoa_shortest(-2.2250738585072014e-308, "f")) == 327 and len(M.ftoa_shortest(-2.2250738585072014e-308, "e")) == 24
    for fmt in ("x", "b", "", "ee", None, 2, b"q"):
        with pytest.raises(ValueError):
            M.ftoa_shortest(1.0, fmt)
    assert M.ftoa_shortest(1.5, b"e") == b"1.5e+00"


def test_ftoa_shortest_reads_back_to_the_same_bits():
    vals = np.concatenate([random_finite(3, 20000), powers_of_two_with_neighbours()[::7], subnormals(4, 2000)])
    for i, v in enumerate(vals.tolist()):
        fmt = FMTS[i % 5]
        text = M.ftoa_shortest(v, fmt).decode()
        back = float(text)
        assert struct.pack("<d", back) == struct.pack("<d", v), (v.hex(), fmt, text)
        if fmt in "eE":   # the digits are repr's: 1..17 of them, none shorter reads back (one digit fewer does not)
            digits = text.lstrip("-").split("e" if fmt == "e" else "E")[0].replace(".", "")
            assert 1 <= len(digits) <= 17 and (len(digits) == 1 or digits[-1] != "0")


def test_shortest_parts_compile_and_render():
    f = Float.shortest([0.1, 1e6, -2.5e-7], "g")
    assert f.values.dtype == np.float64 and f.count == 3 and not f.device and f.fmt == "g" and f.prec is None
    assert Float.shortest([1.0]).fmt == "g"
    assert M.compile(Format(f, b"x"), [])[1] == [(SHORTEST, 0, f), (M.LITERAL, 0, b"x")]
    assert M.compile(f, [])[1] == [(SHORTEST, 0, f)]   # a bare part is a template
    assert M.columns(Format(Col("a"), f)) == ["a"]
    t = Format(Col("name"), b"=", f, b"/", Float([1, 2, 3], 1), b"/", Float.shortest([1, 2, 3], "e"))
    assert [M.render(t, {"name": b"n"}, i) for i in range(3)] == [b"n=0.1/1.0/1e+00", b"n=1e+06/2.0/2e+00", b"n=-2.5e-07/3.0/3e+00"]
    d = Float.shortest_on_device(0x1000, 5, "E")
    assert d.device and d.count == 5 and d.fmt == "E" and d.values == 0x1000
    with pytest.raises(ValueError):
        M.render(Format(d), {}, 0)
    for bad in ("x", "", "eg", 1, None):
        with pytest.raises(ValueError):
            Float.shortest([1.0], bad)
        with pytest.raises(ValueError):
            Float.shortest_on_device(0x1000, 1, bad)
        with pytest.raises(ValueError):
            Float.shortest_of(E.FloatCol("p"), bad)
    with pytest.raises(TypeError):
        Float.shortest_of(E.IntCol("q"), "g")
    # an expression's value, and the columns it reads
    e = Float.shortest_of(E.FloatCol("price") * E.ToFloat(E.IntCol("qty")), "g")
    assert M.columns(Format(Col("id"), e)) == ["id", "price", "qty"]
    assert M.render(Format(e), {"price": b"0.1", "qty": b"3"}) == b"0.30000000000000004"
    assert M.compile(Format(e), ["price", "qty"])[1] == [(SHORTEST, 0, e)]
    assert M.render(Format(Float.shortest([1e300, 2.0 ** 128], "f")), {}, 1) == b"3402823669209385" + b"0" * 23   # no value is refused
    # inside a Switch
    sw = Switch((P.Like(k="a"), Format("a:", Float.shortest([1.5, 2.5], "e"))), otherwise=Float.shortest([1e21, 1e-7], "g"))
    names, cases, otherwise = M.compile_switch(sw, ["k"])
    assert names == ["k"] and [p[0] for p in cases[0][1]] == [M.LITERAL, SHORTEST] and [p[0] for p in otherwise] == [SHORTEST]
    assert M.render(sw, {"k": b"a"}, 1) == b"a:2.5e+00" and M.render(sw, {"k": b"b"}, 1) == b"1e-07"
    assert SHORTEST == 12 == N.CPH_MAP_FLOAT64_SHORTEST
    # the fixed-precision part refuses prec -1 as before
    with pytest.raises(ValueError):
        Float([1.0], -1)


def test_map_column_checks_shortest_row_counts():
    """The checks map_column makes in front of the device call (no device is reached: they raise first)."""
    from csvplus_amd.materialize import map_column
    with pytest.raises(ValueError, match="a Float part has 2 values for 3 rows"):
        map_column(None, {}, Format(Float.shortest([1.0, 2.0], "g")), nrows=3)


def test_shortest_piece_layout_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'cph_map_piece four = {CPH_MAP_COLUMN, 1, {NULL, 0}, NULL};'   # the four-field initialiser still compiles
                   'printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(cph_map_piece), offsetof(cph_map_piece, arg), offsetof(cph_map_piece, value),'
                   ' offsetof(cph_map_piece, ints), offsetof(cph_map_piece, floats), offsetof(cph_map_piece, prec), CPH_MAP_FLOAT64_SHORTEST,'
                   ' CPH_MAP_FLOAT64, CPH_MAP_TIME);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [48, 4, 8, 24, 32, 40, 12, 4, 10]
    assert out[:6] == [C.sizeof(N.cph_map_piece), N.cph_map_piece.arg.offset, N.cph_map_piece.value.offset, N.cph_map_piece.ints.offset,
                       N.cph_map_piece.floats.offset, N.cph_map_piece.prec.offset]


def test_map_shortest_binary_builds():
    """CPU: Shortest / Set(name, Shortest) / FormatShortest compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_map_shortest"])
    assert (ROOT / "tests" / "cpp" / "test_map_shortest").exists()


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def check_shortest(ctx, values, fmts, device=False, out_mem=HOST):
    """One call: Format(shortest fmts[0], "|", shortest fmts[1], ...) over the values, against ftoa_shortest."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    keep = []
    ptr = device_array(values, keep) if device else None
    parts = []
    for fmt in fmts:
        parts += [Float.shortest_on_device(ptr, len(values), fmt) if device else Float.shortest(values, fmt), b"|"]
    got = run_map(ctx, {}, Format(*parts[:-1]), nrows=len(values), out_mem=out_mem)
    want = [b"|".join(M.ftoa_shortest(v, fmt) for fmt in fmts) for v in values.tolist()]
    if got != want:
        bad = [(v.hex(), g, w) for v, g, w in zip(values.tolist(), got, want) if g != w]
        raise AssertionError(f"{len(bad)} of {len(want)} values differ, first: {bad[:3]}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700])
def test_shortest_row_counts_around_the_tile(ctx, n):
    vals = random_finite(100 + n, n)
    vals[::9] = [(0.0, -0.0, math.inf, -math.inf, NAN_PAYLOADS[0], 1.0, 1e6, 1e-5)[k % 8] for k in range(len(vals[::9]))]
    for k, fmt in enumerate(FMTS):
        check_shortest(ctx, vals, fmt, device=bool(k & 1), out_mem=DEVICE if k & 2 else HOST)
    check_shortest(ctx, vals, "g", device=False, out_mem=DEVICE)
    check_shortest(ctx, vals, "f", device=True, out_mem=HOST)
    part = Float.shortest(vals, "g")
    assert run_map(ctx, {}, Format(part, b";")) == model(Format(part, b";"), {}, n)   # the row count from the part


@pytest.mark.gpu
def test_shortest_pinned_answers_on_the_device(ctx):
    for fmt in FMTS:
        rows = [(v, texts[fmt]) for v, texts in PINNED if fmt in texts]
        got = run_map(ctx, {}, Format(Float.shortest([v for v, _ in rows], fmt)), nrows=len(rows))
        assert got == [t.encode() for _, t in rows], fmt


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["powers_of_two", "powers_of_ten_subnormals_specials", "random"])
def test_shortest_value_classes(ctx, values):
    """Every power of two with both neighbours (the narrower lower half of the interval), 10^k with both neighbours,
    subnormals, zeros, NaN payloads, infinities; 1e5 random bit patterns.  'e', 'f' and 'g' in one call."""
    if values == "powers_of_two":
        vals = powers_of_two_with_neighbours()
        assert len(vals) == 3 * 2098
    elif values == "random":
        vals = random_finite(7, 100_000)
    else:
        vals = powers_of_ten_with_neighbours() + subnormals(5, 3000) + [0.0, math.inf, SUBNORMAL_9_5E_88, 99999999999999974834176.0] + NAN_PAYLOADS
    vals = np.array(vals, dtype=np.float64)
    vals[1::2] = -vals[1::2]
    check_shortest(ctx, vals, "efg", device=values == "random")


@pytest.mark.gpu
def test_shortest_tiles_beyond_the_stage(ctx):
    """257 rows of 'f' near 1e300 and near 1e-300: about 300 bytes a row, a tile of 77 KB against the 16 KiB stage, written to
    global memory by the rows themselves; then long and short rows interleaved, so that the offsets inside a tile step by 1 to
    about 327 bytes and a tile's rows start at every alignment."""
    rng = np.random.default_rng(9)
    n = TILE + 1
    big = rng.uniform(1.0, 10.0, n) * 1e300
    small = -rng.uniform(1.0, 10.0, n) * 1e-300
    for vals in (big, small):
        got = check_shortest(ctx, vals, "f")
        assert sum(len(g) for g in got[:TILE]) > 4 * STAGE and min(len(g) for g in got) >= 300
    mixed = np.where(np.arange(n) % 2 == 0, small, np.floor(rng.uniform(0, 10, n)))
    mixed[5::6] = -2.2250738585072014e-308
    mixed[7::10] = 5e-324
    got = check_shortest(ctx, mixed, "f", device=True, out_mem=DEVICE)
    assert {len(g) for g in got} >= {1, 326, 327} and sum(len(g) for g in got[:TILE]) > STAGE
    few = np.floor(rng.uniform(0, 10, 700))   # short rows through the stage, three long ones among them
    few[[3, 300, 699]] = [-2.2250738585072014e-308, 1.7976931348623157e308, 5e-324]
    check_shortest(ctx, few, "fg")


@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE])
def test_shortest_in_a_mixed_template(ctx, out_mem):
    """Literal, a column read through row ids, Int, Float at prec 2, a slice, Time and shortest parts in one template."""
    nsrc, n = 40, 300
    rng = np.random.default_rng(21)
    table = {"a": [bytes(rng.integers(0, 256, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(nsrc)],
             "b": [b"%04d-xyz" % i for i in range(nsrc)]}
    sa, sb = rng.integers(0, nsrc, n), rng.integers(0, nsrc, n)
    f2 = Float(rng.integers(-10 ** 7, 10 ** 7, n) / 1000.0, 2)
    wide = random_finite(22, n)
    wide[10] = 2.0 ** 128   # what the fixed-precision piece refuses is a value like any other here
    sg, se = Float.shortest(wide, "g"), Float.shortest(wide * 0.5, "E")
    ints = Int(rng.integers(-10 ** 12, 10 ** 12, n))
    tm = Time(rng.integers(0, 2 * 10 ** 9, n), 90)
    t = Format(b"[", Col("a"), b"|", sg, f2, Col("b")[1:6], ints, b" ~ ", tm, se, b"]")
    cols = {"a": StrCol.from_values(table["a"], fixed_width=0), "b": StrCol.from_values(table["b"])}
    want = model(t, table, n, lambda i: {"a": int(sa[i]), "b": int(sb[i])})
    assert b"|3.402823669209385e+38" in want[10]
    ids = {"a": sa.astype(np.uint32), "b": sb.astype(np.uint64)}
    assert run_map(ctx, cols, t, row_ids=ids, nrows=n, out_mem=out_mem) == want
    keep = []
    dev_ids = {"a": (device_array(ids["a"], keep), 32, n), "b": (device_array(ids["b"], keep), 64, n)}
    assert run_map(ctx, {k: c.to_device() for k, c in cols.items()}, t, row_ids=dev_ids, nrows=n, out_mem=out_mem) == want


@pytest.mark.gpu
def test_refusals_behind_a_shortest_piece(ctx):
    """The FLOAT64 limit and the TIME year limit are still reported, with the right piece and the lowest row, when a shortest
    piece stands in front of them; the shortest piece over the same values succeeds."""
    from csvplus_amd.materialize import map_column
    n = 600
    vals = np.arange(n, dtype=np.float64) + 0.5
    vals[[433, 270]] = 2.0 ** 128, -1e300
    short = Float.shortest(vals, "g")
    with pytest.raises(N.CphError) as ei:
        map_column(ctx, {}, Format(short, b" ", Float(vals, 2)), nrows=n)
    assert ei.value.code == N.CPH_ERR_INVALID and "FLOAT64 piece 2, row 270" in str(ei.value) and "2^128" in str(ei.value)
    with pytest.raises(N.CphError) as ei:
        map_column(ctx, {}, Format(short, Float(np.ones(n), 1), Float(vals, 0)), nrows=n)
    assert "FLOAT64 piece 2, row 270" in str(ei.value)
    secs = np.arange(n, dtype=np.int64)
    secs[[500, 301]] = 253402300800   # the first second of the year 10000
    with pytest.raises(N.CphError) as ei:
        map_column(ctx, {}, Format(short, b" ", Time(secs, 0)), nrows=n)
    assert ei.value.code == N.CPH_ERR_INVALID and "TIME piece 2, row 301" in str(ei.value) and "0000..9999" in str(ei.value)
    got = run_map(ctx, {}, Format(short, b" ", Time(np.arange(n), 0)), nrows=n)
    assert got == model(Format(short, b" ", Time(np.arange(n), 0)), {}, n)
    assert got[433].startswith(b"3.402823669209385e+38 ") and got[270].startswith(b"-1e+300 ")


@pytest.mark.gpu
def test_shortest_in_a_switch(ctx):
    """Shortest pieces in two cases and in `otherwise`, alternatives changing at every row across the tile edges; a value
    in a row that selects another alternative is never interpreted."""
    n = 3 * TILE + 7
    rng = np.random.default_rng(31)
    table = {"k": [b"%d" % (i % 3) for i in range(n)], "v": [b"v%d" % i for i in range(n)]}
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    a, b, c = random_finite(32, n), rng.standard_normal(n) * 1e3, random_finite(33, n)
    limited = np.where(np.arange(n) % 3 == 1, b, 2.0 ** 200)   # prec 2 would refuse the rows that do not select case 1

    def switch(a, b, c, dev=None):
        fa = Float.shortest(a, "e") if dev is None else Float.shortest_on_device(dev, n, "e")
        return Switch((P.Like(k="0"), Format("zero:", fa, Col("v"))),
                      (P.Like(k="1"), Format(Float.shortest(b, "f"), "|", Float(limited, 2))),
                      otherwise=Format(Col("v"), "=", Float.shortest(c, "G"), "/", Float.shortest(a, "g")))

    want = switch_model(switch(a, b, c), table, n)
    assert set(want[1]) == {0, 1, 2}
    assert run_switch(ctx, cols, switch(a, b, c), nrows=n) == want
    keep = []
    assert run_switch(ctx, {k: v.to_device() for k, v in cols.items()}, switch(a, b, c, device_array(a, keep)), nrows=n, out_mem=DEVICE) == want
    # NaN, an infinity and huge values in rows that do not select the piece change nothing
    a2, b2, c2 = a.copy(), b.copy(), c.copy()
    rows = np.arange(n)
    b2[rows % 3 != 1] = np.where(rows[rows % 3 != 1] % 2 == 0, math.nan, 1e308)
    c2[rows % 3 != 2] = -math.inf
    a2[rows % 3 == 1] = NAN_PAYLOADS[0]
    assert run_switch(ctx, cols, switch(a2, b2, c2), nrows=n) == want


@pytest.mark.gpu
def test_text_to_float_to_shortest_text_to_float_round_trip(ctx):
    """to_float on the device, Format(shortest 'g') on the device, to_float (decided on the device) again: identical bits."""
    from csvplus_amd.materialize import map_column, to_float
    n = 100_000
    vals = random_finite(41, n)
    text = StrCol.from_values([repr(v).encode() for v in vals.tolist()], fixed_width=0)
    ctx.set_option("float_device", 1)
    try:
        first = to_float(ctx, text, out_mem=DEVICE)
        assert first.nerrors == 0 and first.values[1] == n
        cb = map_column(ctx, {}, Format(Float.shortest_on_device(first.values[0], n, "g")), nrows=n, out_mem=DEVICE)
        second = to_float(ctx, cb.as_device_strcol(), out_mem=HOST)
        assert second.nerrors == 0 and second.host_rows == 0   # at most 17 digits: nothing is left to the host
        np.testing.assert_array_equal(second.values.view(np.uint64), vals.view(np.uint64))
        cb.release()
        first.release()
    finally:
        ctx.set_option("float_device", 0)


def _piece_call(ctx, n, pieces):
    """cph_map_format over pieces (kind, arg, float array or None, prec): (status, message)."""
    keep = []
    arr = (N.cph_map_piece * len(pieces))()
    for k, (kind, arg, floats, prec) in enumerate(pieces):
        arr[k].kind, arr[k].arg, arr[k].prec = kind, arg, prec
        if floats is not None:
            keep.append(floats)
            arr[k].floats = floats.ctypes.data
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_format(ctx.handle, None, None, 0, n, arr, len(pieces), HOST, C.byref(out))
    msg = ctx.last_error() if rc != N.CPH_OK else ""
    assert bool(out) == (rc == N.CPH_OK)   # nothing is left in *out on failure
    if out:
        ctx.lib.cph_colbuf_release(out)
    return rc, msg


@pytest.mark.gpu
def test_shortest_errors_have_a_status_and_a_message(ctx):
    ten = np.arange(10, dtype=np.float64) + 0.5
    for fmt in FMTS:
        assert _piece_call(ctx, 10, [(SHORTEST, HOST, ten, ord(fmt))])[0] == N.CPH_OK
    assert _piece_call(ctx, 0, [(SHORTEST, HOST, None, ord("g"))])[0] == N.CPH_OK   # floats NULL is fine without rows
    for what, pieces, words in [("format byte 'x'", [(SHORTEST, HOST, ten, ord("x"))], "FLOAT64_SHORTEST"),
                                ("format byte 0", [(SHORTEST, HOST, ten, 0)], "FLOAT64_SHORTEST"),
                                ("format byte -1", [(SHORTEST, HOST, ten, -1)], "FLOAT64_SHORTEST"),
                                ("format byte 2 (a prec)", [(SHORTEST, HOST, ten, 2)], "'e' 'E' 'f' 'g' 'G'"),
                                ("floats NULL", [(SHORTEST, HOST, None, ord("g"))], "a FLOAT64_SHORTEST piece without values"),
                                ("memory space 2", [(SHORTEST, 2, ten, ord("g"))], "bad memory space of a FLOAT64_SHORTEST piece"),
                                ("prec -1 of the fixed piece", [(M.FLOAT64, HOST, ten, -1)], "prec of a FLOAT64 piece outside 0..22")]:
        rc, msg = _piece_call(ctx, 10, pieces)
        assert rc == N.CPH_ERR_INVALID and words in msg, (what, rc, msg)
    for kind in (5, 6, 7, 9, 11, 13):
        rc, msg = _piece_call(ctx, 10, [(kind, HOST, ten, ord("g"))])
        assert rc == N.CPH_ERR_INVALID and "unknown piece kind" in msg, (kind, rc, msg)
