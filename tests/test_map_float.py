"""Map with FLOAT64 pieces (mapping.Float, cph_map_format's CPH_MAP_FLOAT64): strconv.FormatFloat(v, 'f', prec, 64) on the
device.  CPU: the host model `ftoa` against exact decimal arithmetic, the compiler's rules, the struct layout.  Under
`-m gpu`: the device against `ftoa` / `render`, byte for byte, never against itself."""
import ctypes as C
import decimal
import math
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import mapping as M
from csvplus_amd.mapping import Col, Float, Format, Int
from helpers import orders_table, stock_table
from test_map import _csv_text, _hip, device_array, model, run_map

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
TILE = 256        # kMatThreads
STAGE = 16 * 1024  # kMatStage
PRECS = range(M.MAX_PREC + 1)


def _bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _next(v, up):
    return math.nextafter(v, math.inf if up else -math.inf)


BELOW_2_128 = _next(2.0 ** 128, False)
NAN_PAYLOAD = _bits(0xFFF8000000001234)   # the sign bit and a payload
EDGES = [
    0.125, 0.375, 2.5, 3.5, 2.675, 1.005, 9.995, 0.1, 0.5, 1.5,            # ties and near-ties
    9.5, 0.999999, 999999.9999995, 99.5, 0.95,                             # carries that add a digit
    0.0, -0.0, -0.001, 1.0, 123456.789,
    5e-324, 2.2250738585072014e-308,                                       # the smallest subnormal, the smallest normal
    2.0 ** -75, _next(2.0 ** -75, False), _next(2.0 ** -75, True), 2.0 ** -74, 2.0 ** -127, 2.0 ** -128, 2.0 ** -129,
    4503599627370496.5, 4503599627370495.5, 2251799813685248.25, 2251799813685248.75,   # ties at and below 2^52
    2.0 ** 53 + 2, 2.0 ** 53, 2.0 ** 63,
    2.0 ** 64, _next(2.0 ** 64, False), _next(2.0 ** 64, True),
    9999999999999999999.0, 1e19, 1e22, 1e23, 1e38,
    BELOW_2_128, 2.0 ** 127,
    NAN_PAYLOAD, _bits(0x7FF0000000000001), math.inf, -math.inf,
]
EDGES = EDGES + [-v for v in EDGES]


def exact(v, prec):
    """FormatFloat(v, 'f', prec, 64) by exact decimal arithmetic: Decimal(v) is the binary value itself."""
    if math.isnan(v):
        return b"NaN"
    if math.isinf(v):
        return b"-Inf" if v < 0 else b"+Inf"
    with decimal.localcontext() as c:
        c.prec, c.Emax, c.Emin = 1200, 2000, -2000
        q = decimal.Decimal(v).quantize(decimal.Decimal(1).scaleb(-prec), rounding=decimal.ROUND_HALF_EVEN)
        return format(q, "f").encode()


def random_patterns(seed, count):
    """Random 64-bit patterns read as doubles, kept when |v| < 2^128 or not finite."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2 ** 64, count, dtype=np.uint64).view(np.float64)
    return v[~np.isfinite(v) | (np.abs(v) < M.FLOAT_LIMIT)]


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_ftoa_pinned_answers():
    pinned = [(2.675, 2, b"2.67"), (2.5, 0, b"2"), (3.5, 0, b"4"), (0.125, 2, b"0.12"), (0.375, 2, b"0.38"), (1.005, 2, b"1.00"),
              (9.995, 2, b"9.99"), (9.5, 0, b"10"), (0.999999, 2, b"1.00"), (999999.9999995, 6, b"999999.999999"), (999999.9999995, 5, b"1000000.00000"),
              (-0.001, 2, b"-0.00"), (-0.0, 0, b"-0"), (-0.0, 2, b"-0.00"), (0.0, 3, b"0.000"), (0.1, 22, b"0.1000000000000000055511"),
              (4503599627370496.5, 0, b"4503599627370496"), (2.0 ** 64, 0, b"18446744073709551616"), (1e23, 1, b"99999999999999991611392.0"),
              (BELOW_2_128, 0, b"340282366920938425684442744474606501888"), (5e-324, 22, b"0." + b"0" * 22),
              (NAN_PAYLOAD, 5, b"NaN"), (math.nan, 0, b"NaN"), (math.inf, 7, b"+Inf"), (-math.inf, 0, b"-Inf")]
    for v, prec, text in pinned:
        assert M.ftoa(v, prec) == text and exact(v, prec) == text, (v, prec)
    assert len(M.ftoa(-BELOW_2_128, 22)) == 63
    for v in (2.0 ** 128, -(2.0 ** 128), 1e300, 1.7976931348623157e308):
        with pytest.raises(ValueError):
            M.ftoa(v, 2)
    for prec in (-1, 23, 1.5, True):
        with pytest.raises(ValueError):
            M.ftoa(1.0, prec)


def test_ftoa_against_exact_decimal_arithmetic():
    for v in EDGES:
        for prec in PRECS:
            assert M.ftoa(v, prec) == exact(v, prec), (v, prec)
    for i, v in enumerate(random_patterns(1, 9000)[:6000]):
        assert M.ftoa(v, i % 23) == exact(float(v), i % 23), (float(v).hex(), i % 23)
    rng = np.random.default_rng(2)   # magnitudes a table of amounts has
    for i, v in enumerate(rng.integers(0, 10 ** 9, 4000) / rng.choice([1, 10, 100, 1000, 8, 64], 4000)):
        assert M.ftoa(v, i % 7) == exact(float(v), i % 7), (float(v).hex(), i % 7)


def test_float_parts_compile_and_render():
    f = Float([0.125, 2.675, -0.001], 2)
    assert f.values.dtype == np.float64 and f.count == 3 and not f.device and f.prec == 2
    assert Float(np.array([1, 2, 3], dtype=np.int32), 1).values.dtype == np.float64   # float64(qty)
    assert M.compile(Format(f, b"x"), [])[1] == [(M.FLOAT64, 0, f), (M.LITERAL, 0, b"x")]
    assert M.compile(f, [])[1] == [(M.FLOAT64, 0, f)]   # a bare Float is a template
    assert M.columns(Format(Col("a"), f)) == ["a"]
    t = Format(Col("name"), b"=", f, b"/", Float([1, 2, 3], 0), b"/", Int([7, 8, 9]))
    assert [M.render(t, {"name": b"n"}, i) for i in range(3)] == [b"n=0.12/1/7", b"n=2.67/2/8", b"n=-0.00/3/9"]
    assert M.render(f, {}, 1) == b"2.67"
    d = Float.on_device(0x1000, 5, 22)
    assert d.device and d.count == 5 and d.prec == 22 and d.values == 0x1000
    with pytest.raises(ValueError):
        M.render(Format(d), {}, 0)
    for prec in (-1, 23):
        with pytest.raises(ValueError):
            Float([1.0], prec)
        with pytest.raises(ValueError):
            Float.on_device(0x1000, 1, prec)
    with pytest.raises(ValueError):
        Float(["a"], 2)
    with pytest.raises(ValueError):
        M.render(Format(Float([1e300], 2)), {}, 0)   # the model refuses what the device refuses
    assert M.FLOAT64 == 4 == N.CPH_MAP_FLOAT64


def test_map_column_checks_float_row_counts():
    """The checks map_column makes in front of the device call (no device is reached: they raise first)."""
    from csvplus_amd.materialize import map_column
    col = StrCol.from_values([b"a", b"b", b"c"], fixed_width=0)
    with pytest.raises(ValueError, match="a Float part has 2 values for 3 rows"):
        map_column(None, {"a": col}, Format(Col("a"), Float([1.0, 2.0], 2)))
    with pytest.raises(ValueError, match="a Float part has 2 values for 3 rows"):
        map_column(None, {}, Format(Float([1.0, 2.0], 2)), nrows=3)
    with pytest.raises(ValueError, match="an Int part has 1 values for 2 rows"):
        map_column(None, {}, Format(Float([1.0, 2.0], 2), Int([1])), nrows=2)
    with pytest.raises(ValueError, match="needs nrows"):
        map_column(None, {}, Format(b"x"))


def test_float_piece_layout_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'cph_map_piece four = {CPH_MAP_COLUMN, 1, {NULL, 0}, NULL};'   # the four-field initialiser still compiles
                   'printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(cph_map_piece), offsetof(cph_map_piece, ints), offsetof(cph_map_piece, floats),'
                   ' offsetof(cph_map_piece, prec), CPH_MAP_FLOAT64, four.prec, four.floats == NULL);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [C.sizeof(N.cph_map_piece), N.cph_map_piece.ints.offset, N.cph_map_piece.floats.offset, N.cph_map_piece.prec.offset,
                   M.FLOAT64, 0, 1]
    assert N.cph_map_piece.ints.offset == 24 and N.cph_map_piece.floats.offset == 32 and C.sizeof(N.cph_map_piece) == 48


def test_map_float_binary_builds():
    """CPU: Fixed / Set(name, Fixed) / Format::render compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_map_float"])
    assert (ROOT / "tests" / "cpp" / "test_map_float").exists()


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def check_floats(ctx, values, prec, device=False, out_mem=HOST):
    values = np.ascontiguousarray(values, dtype=np.float64)
    keep = []
    part = Float.on_device(device_array(values, keep), len(values), prec) if device else Float(values, prec)
    got = run_map(ctx, {}, Format(part), nrows=len(values), out_mem=out_mem)
    want = [M.ftoa(v, prec) for v in values]
    if got != want:
        bad = [(float(v).hex(), prec, g, w) for v, g, w in zip(values, got, want) if g != w]
        raise AssertionError(f"{len(bad)} of {len(want)} values differ, first: {bad[:5]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_float_row_counts_around_the_tile(ctx, n):
    rng = np.random.default_rng(100 + n)
    vals = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 12, n)
    check_floats(ctx, vals, int(rng.integers(0, 23)))
    part = Float(vals, 3)
    assert run_map(ctx, {}, Format(part, b";")) == model(Format(part, b";"), {}, n)   # the row count from the Float part
    check_floats(ctx, vals, int(rng.integers(0, 23)), device=True, out_mem=DEVICE)


@pytest.mark.gpu
def test_float_edge_table_at_every_prec(ctx):
    """Ties, carries, signed zeros, subnormals, the 2^52 / 2^64 / 2^128 boundaries, NaN and the infinities: prec 19 and 20
    (64-bit / 128-bit fraction digits) are among the 23."""
    for prec in PRECS:
        check_floats(ctx, EDGES, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_float_random_bit_patterns(ctx, device):
    vals = random_patterns(7, 200_000)
    assert len(vals) > 100_000 and not np.isfinite(vals).all()
    for prec, part in zip(PRECS, np.array_split(vals, 23)):
        check_floats(ctx, part, prec, device=device)


@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE])
def test_float_in_a_mixed_template(ctx, out_mem):
    nsrc, n = 40, 300
    rng = np.random.default_rng(21)
    table = {"a": [bytes(rng.integers(0, 256, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(nsrc)],
             "b": [b"%04d" % i for i in range(nsrc)]}
    sa, sb = rng.integers(0, nsrc, n), rng.integers(0, nsrc, n)
    f2 = Float(rng.integers(-10 ** 7, 10 ** 7, n) / 1000.0, 2)
    f9 = Float(np.concatenate([EDGES[:60], rng.standard_normal(n - 60) * 1e18]), 9)
    ints = Int(rng.integers(-10 ** 12, 10 ** 12, n))
    t = Format(b"[", Col("a"), b"|", f2, Col("b"), ints, b" ~ ", f9, b"]")
    cols = {"a": StrCol.from_values(table["a"], fixed_width=0), "b": StrCol.from_values(table["b"])}
    want = model(t, table, n, lambda i: {"a": int(sa[i]), "b": int(sb[i])})
    ids = {"a": sa.astype(np.uint32), "b": sb.astype(np.uint64)}
    assert run_map(ctx, cols, t, row_ids=ids, nrows=n, out_mem=out_mem) == want
    keep = []
    dev_ids = {"a": (device_array(ids["a"], keep), 32, n), "b": (device_array(ids["b"], keep), 64, n)}
    assert run_map(ctx, {k: c.to_device() for k, c in cols.items()}, t, row_ids=dev_ids, nrows=n, out_mem=out_mem) == want


@pytest.mark.gpu
def test_float_tile_beyond_the_stage(ctx):
    """300 rows of 63-character values behind a 10-byte literal: a full tile spans 256 * 73 bytes, more than the stage, and
    goes out through the global sink; the 44 rows behind it fit the stage."""
    assert TILE * 73 > STAGE - 48 >= 44 * 73
    vals = np.full(300, -BELOW_2_128)
    vals[::7] = -_next(BELOW_2_128, False)
    t = Format(b"0123456789", Float(vals, 22))
    got = run_map(ctx, {}, t, nrows=300)
    assert got == model(t, {}, 300) and all(len(g) == 73 for g in got)


def _float_call(ctx, n, pieces, out_mem=HOST):
    """cph_map_format over pieces (kind, arg, float array or None, prec): (status, message, values or None)."""
    keep = []
    arr = (N.cph_map_piece * len(pieces))()
    for k, (kind, arg, floats, prec) in enumerate(pieces):
        arr[k].kind, arr[k].arg, arr[k].prec = kind, arg, prec
        if floats is not None:
            keep.append(floats)
            arr[k].floats = floats if isinstance(floats, int) else floats.ctypes.data
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_format(ctx.handle, None, None, 0, n, arr, len(pieces), out_mem, C.byref(out))
    msg = ctx.last_error() if rc != N.CPH_OK else ""
    assert bool(out) == (rc == N.CPH_OK)   # nothing is left in *out on failure
    if out:
        ctx.lib.cph_colbuf_release(out)
    return rc, msg


@pytest.mark.gpu
def test_float_errors_have_a_status_and_a_message(ctx):
    F = M.FLOAT64
    ten = np.arange(10, dtype=np.float64) + 0.5
    assert _float_call(ctx, 10, [(F, HOST, ten, 2)])[0] == N.CPH_OK
    assert _float_call(ctx, 0, [(F, HOST, None, 2)])[0] == N.CPH_OK   # floats NULL is fine without rows
    for what, pieces in [("prec -1", [(F, HOST, ten, -1)]), ("prec 23", [(F, HOST, ten, 23)]), ("floats NULL", [(F, HOST, None, 2)]),
                         ("memory space 2", [(F, 2, ten, 2)]), ("kind 5", [(5, HOST, ten, 2)])]:
        rc, msg = _float_call(ctx, 10, pieces)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    assert "prec" in _float_call(ctx, 10, [(F, HOST, ten, 23)])[1]
    # finite values of 2^128 or more: refused, the lowest row named, from host and from device memory
    keep = []
    for big in (1e300, 1.7976931348623157e308, 2.0 ** 128, -(2.0 ** 128)):
        bad = ten.copy()
        bad[7] = bad[3] = big
        for arg, ptr in ((HOST, bad), (DEVICE, device_array(bad, keep))):
            rc, msg = _float_call(ctx, 10, [(M.LITERAL, 0, None, 0), (F, arg, ptr, 2)])
            assert rc == N.CPH_ERR_INVALID and "piece 1" in msg and "row 3" in msg, (big, arg, msg)
        bad[3] = 1.0
        rc, msg = _float_call(ctx, 10, [(F, HOST, bad, 2)])
        assert rc == N.CPH_ERR_INVALID and "piece 0" in msg and "row 7" in msg
        bad[7] = BELOW_2_128
        assert _float_call(ctx, 10, [(F, HOST, bad, 2)])[0] == N.CPH_OK   # the same array with those rows replaced
        with pytest.raises(N.CphError):
            run_map(ctx, {}, Format(Float([1.0, big], 2)), nrows=2)
    inf = ten.copy()
    inf[7], inf[3] = math.inf, -math.inf
    check_floats(ctx, inf, 2)   # the infinities in their place are values, not errors
    # a refused value far behind the first tile, beside good pieces
    many = np.full(5000, 1.5)
    many[4321] = 1e200
    rc, msg = _float_call(ctx, 5000, [(F, HOST, many, 0), (F, HOST, np.ones(5000), 1)])
    assert rc == N.CPH_ERR_INVALID and "piece 0" in msg and "row 4321" in msg


@pytest.mark.gpu
def test_amounts_table_through_the_pipeline(ctx):
    """The reference's amounts table (csvplus_test.go:1391-1421) at fixture size: orders.Join(stock), amount =
    FormatFloat(price * float64(qty), 'f', 2, 64), everything on the device up to the CSV text."""
    import torch

    from csvplus_amd import DeviceIndex, join_chain, pipeline
    from csvplus_amd.materialize import to_float, to_int
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    pv, ov = enc(stock_table()), enc(orders_table(n=2000))
    n = 2000
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    try:
        # the joined rows: every order has its product, so they are the orders in order; the build rows by the chain
        ix = DeviceIndex(ctx, [StrCol.from_values(pv["prod_id"])], unique=True)
        ch = join_chain(ctx, [(ix, [StrCol.from_values(ov["prod_id"])])])
        srow, brow = ch.stream_row.copy(), ch.build_row(0).copy()
        ch.release()
        ix.close()
        np.testing.assert_array_equal(srow, np.arange(n))
        np.testing.assert_array_equal(brow, [int(p) for p in ov["prod_id"]])
        keep = []
        price = to_float(ctx, tp["price"], row_ids=(device_array(brow, keep), brow.dtype.itemsize * 8, n), nrows=n, out_mem=DEVICE)
        qty = to_int(ctx, to["qty"], out_mem=DEVICE)
        assert price.nerrors == 0 and qty.nerrors == 0 and price.values[1] == n and qty.values[1] == n
        tprice = torch.empty(n, dtype=torch.float64, device="cuda:0")
        tqty = torch.empty(n, dtype=torch.int64, device="cuda:0")
        for dst, (ptr, cnt) in ((tprice, price.values), (tqty, qty.values)):
            assert _hip().hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(ptr), C.c_size_t(cnt * 8), 3) == 0   # device to device
        amount = tprice * tqty.to(torch.float64)
        torch.cuda.synchronize()
        price.release()
        qty.release()
        outc = [("cust_id", to, "cust_id"), ("product", tp, "product"), ("amount", None, None)]
        got = pipeline.join_to_csv(ctx, to, [(tp, "prod_id", "prod_id")], outc,
                                   computed={"amount": Format(Float.on_device(amount.data_ptr(), n, 2))})
        prices = dict(zip(pv["prod_id"], pv["price"]))
        names = dict(zip(pv["prod_id"], pv["product"]))
        direct = [float(prices[p]) * int(q) for p, q in zip(ov["prod_id"], ov["qty"])]
        want = b"cust_id,product,amount\n" + b"".join(
            b"%s,%s,%s\n" % (c, names[p], b"%.2f" % a) for c, p, a in zip(ov["cust_id"], ov["prod_id"], direct))
        assert got == want
        # the totals per customer from the parsed-back amounts, within the reference's own bound (csvplus_test.go:566)
        sums, direct_sums = {}, {}
        for line, a in zip(got.split(b"\n")[1:-1], direct):
            c, _, text = line.split(b",")
            sums[c] = sums.get(c, 0.0) + float(text)
            direct_sums[c] = direct_sums.get(c, 0.0) + a
        assert sums.keys() == direct_sums.keys() and len(sums) > 100
        for c, s in sums.items():
            assert abs(s - direct_sums[c]) <= 1e-6 * abs(direct_sums[c]), (c, s, direct_sums[c])
    finally:
        tp.release()
        to.release()
