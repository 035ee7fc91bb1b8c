"""Numeric expressions per row (csvplus_amd.expr, cph_num_eval): the reference's `price * float64(qty)`.  CPU: the host model's
known answers, the compiler's typing rules and limits, the header's constants.  Under `-m gpu`: the device against the host
model bit for bit — values, status, error count, first error row and op — never against itself.

NaN results are compared as NaNs: IEEE 754 leaves the sign and payload of a GENERATED NaN open (amd64 produces the negative
quiet NaN, the GPU the positive one); every other value is compared by its 64 bits."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.expr import FloatArr, FloatCol, IntArr, IntCol, Lit, Neg, ToFloat, ToInt
from helpers import orders_table, stock_table

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
MAXI, MINI = P.INT64_MAX, P.INT64_MIN
OK, SYNTAX, RANGE, UNSUP, DIV_ZERO, CONVERT = 0, 1, 2, 3, 4, 5
TILE = 2048   # kExprTile


def ev(e, row=None, i=0):
    return E.evaluate(e, row or {}, i)


# ---- CPU --------------------------------------------------------------------------------------------------------------------
KNOWN = [   # (expression, value, status)
    (Lit(MAXI) + 1, MINI, OK), (Lit(MINI) * -1, MINI, OK), (-Lit(MINI), MINI, OK), (Lit(MINI) / -1, MINI, OK), (Lit(MINI) % -1, 0, OK),
    (Lit(-7) / 2, -3, OK), (Lit(-7) % 2, -1, OK), (Lit(7) / -2, -3, OK), (Lit(7) % -2, 1, OK),
    (Lit(5) / 0, 0, DIV_ZERO), (Lit(5) % 0, 0, DIV_ZERO), (Lit(MINI) / 0, 0, DIV_ZERO),
    (ToFloat(2 ** 53 + 1), 2.0 ** 53, OK), (ToFloat(2 ** 53 + 3), 2.0 ** 53 + 4, OK), (ToFloat(MINI), -(2.0 ** 63), OK),
    (ToInt(-0.9), 0, OK), (ToInt(-(2.0 ** 63)), MINI, OK), (ToInt(2.0 ** 63), 0, CONVERT), (ToInt(math.nan), 0, CONVERT),
    (ToInt(math.inf), 0, CONVERT), (ToInt(math.nextafter(2.0 ** 63, 0.0)), 2 ** 63 - 1024, OK), (ToInt(-7.99), -7, OK),
    (Lit(1.0) / 0.0, math.inf, OK), (Lit(-1.0) / 0.0, -math.inf, OK), (Lit(1.0) / -0.0, -math.inf, OK),
    (Lit(MAXI) - MINI, -1, OK), (Lit(3037000500) * 3037000500, 3037000500 ** 2 - 2 ** 64, OK), (-Lit(0.0), -0.0, OK),
    (Lit(0.1) + 0.2, 0.30000000000000004, OK), (Lit(1e308) * 10.0, math.inf, OK), (Lit(7) - 9, -2, OK), (Lit(7.5) - 9.0, -1.5, OK),
]


def same_value(got, want):
    if isinstance(want, float) or isinstance(got, float):
        if isinstance(got, float) and isinstance(want, float) and math.isnan(want):
            return math.isnan(got)
        return isinstance(got, float) and isinstance(want, float) and np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    return type(got) is int and got == want


def test_host_model_known_answers():
    for e, value, status in KNOWN:
        v, st, op = ev(e)
        assert st == status and same_value(v, value), (e, v, st)
        assert (op == -1) == (status == OK)
    assert math.isnan(ev(Lit(0.0) / 0.0)[0]) and ev(Lit(0.0) / 0.0)[1] == OK
    assert math.isnan(ev(Lit(math.inf) - math.inf)[0])


def test_the_first_failing_op_in_program_order_decides():
    row = {"qty": "x", "price": b"2.5", "zero": "0"}
    e = IntCol("qty") / IntCol("zero")   # ops: COL_INT qty, COL_INT zero, DIV — the leaf fails first
    assert ev(e, row) == (0, SYNTAX, 0)
    assert ev(IntCol("zero") / IntCol("zero") + IntCol("qty"), row) == (0, DIV_ZERO, 2)   # the division precedes the bad leaf
    assert ev(FloatCol("price") * ToFloat(IntCol("qty")), row) == (0.0, SYNTAX, 1)
    assert ev(ToFloat(IntCol("qty")) * FloatCol("price"), row) == (0.0, SYNTAX, 0)
    assert ev(FloatCol("price") * ToFloat(IntCol("zero")), row) == (0.0, OK, -1)
    assert ev(IntCol("qty") + 1, {"qty": "99999999999999999999"}) == (0, RANGE, 0)
    assert ev(FloatCol("p") + 1.0, {b"p": b"1_0"}) == (0.0, UNSUP, 0)
    assert E.error_text(e, row, SYNTAX, 0) == 'column "qty": cannot convert "x" to integer: invalid syntax'
    assert E.error_text(FloatCol("price") * 2.0, {"price": "1.2.3"}, SYNTAX, 0) == 'column "price": cannot convert "1.2.3" to float: invalid syntax'
    with pytest.raises(M.MissingColumn):
        ev(IntCol("nope") + 1, row)
    arr = IntArr([10, 20, 30])
    assert ev(arr * 2, {}, 1) == (40, OK, -1) and ev(FloatArr([1, 2]) / 4.0, {}, 1) == (0.5, OK, -1)


def _chain(leaf, count, right=False):
    e = leaf()
    for _ in range(count - 1):
        e = (leaf() + e) if right else (e + leaf())
    return e


def test_compile_typing_and_limits():
    names, ops = E.compile(FloatCol("price") * ToFloat(IntCol("qty")), ["qty", "x", "price"])
    assert names == ["price", "qty"]
    assert ops == [(E.COL_FLT, 0, None), (E.COL_INT, 1, None), (E.TO_FLT, 0, None), (E.MUL, 0, None)]   # the reference's shape
    assert E.check_ops(ops, 2, 0)[:2] == (E.FLOAT, 2)
    a = IntArr([1, 2])
    assert E.compile(a + a * 3, [])[1] == [(E.NUM_INT, 0, a), (E.NUM_INT, 0, a), (E.LIT_INT, 0, 3), (E.MUL, 0, None), (E.ADD, 0, None)]
    assert E.kind_of(ToInt(FloatCol("a")) % 7) == E.INT and E.kind_of(-FloatCol("a")) == E.FLOAT
    E.compile(_chain(lambda: Lit(1), 16), [])                      # 31 ops
    E.compile(_chain(lambda: Lit(1), 8, right=True), [])           # a stack of 8
    E.compile(_chain(lambda: IntArr([1]), 8), [])                  # 8 arrays
    bad = [_chain(lambda: Lit(1), 17),                             # 33 ops
           _chain(lambda: Lit(1), 9, right=True),                  # a stack of 9
           _chain(lambda: IntArr([1]), 9),                         # 9 arrays
           IntCol("a") + FloatCol("a"), IntCol("a") + 1.5, FloatCol("a") * 2, FloatCol("a") % 2.0, IntCol("a") % 2.0,
           ToFloat(FloatCol("a")), ToInt(IntCol("a")), ToFloat(1.0)]
    for e in bad:
        with pytest.raises(TypeError):
            E.compile(e, ["a"])
    for raw, ncols, nnums in [([(E.LIT_INT, 0, 1), (E.LIT_INT, 0, 2)], 0, 0),              # two values left
                              ([(E.ADD, 0, None)], 0, 0), ([(E.LIT_INT, 0, 1), (E.NEG, 0, None), (E.ADD, 0, None)], 0, 0),
                              ([(7, 0, None)], 0, 0), ([(0, 0, None)], 0, 0), ([(16, 0, None)], 0, 0),
                              ([(E.COL_INT, 1, None)], 1, 0), ([(E.COL_FLT, -1, None)], 1, 0), ([(E.NUM_INT, 0, None)], 0, 0), ([], 0, 0)]:
        with pytest.raises(TypeError):
            E.check_ops(raw, ncols, nnums)
    for v in (True, "1", None, 2 ** 63):
        with pytest.raises((TypeError, ValueError)):
            E.compile(IntCol("a") + v, ["a"])
    with pytest.raises(M.MissingColumn):
        E.compile(IntCol("b") + 1, ["a"])
    with pytest.raises(TypeError):
        M.Float.of(IntCol("a") * 2, 2)
    with pytest.raises(TypeError):
        M.Int.of(FloatCol("a"))
    with pytest.raises(ValueError):
        M.Float.of(FloatCol("a"), 23)


def test_template_parts_from_expressions_render_with_the_host_model():
    amount = M.Float.of(FloatCol("price") * ToFloat(IntCol("qty")), 2)
    t = M.Format(M.Col("product"), b": ", amount, b" #", M.Int.of(IntCol("qty") % 7))
    assert M.columns(t) == ["product", "price", "qty"]
    assert M.render(t, {"product": "bolt", "price": "2.675", "qty": "1"}) == b"bolt: 2.67 #1"   # half-even on the exact binary value
    assert M.render(t, {"product": "nut", "price": b"0.10", "qty": b"30"}) == b"nut: 3.00 #2"
    with pytest.raises(E.ExprError) as err:
        M.render(t, {"product": "nut", "price": b"0.10", "qty": b"3O"}, 12)
    assert err.value.row == 12 and err.value.column == "qty" and err.value.kind == SYNTAX
    assert 'column "qty": cannot convert "3O" to integer: invalid syntax' in str(err.value)
    with pytest.raises(E.ExprError) as err:
        M.render(M.Format(M.Int.of(IntCol("qty") / 0)), {"qty": "1"})
    assert err.value.kind == DIV_ZERO and err.value.column is None


def test_ops_structs_and_enums_against_the_compiled_header(tmp_path):
    names = ["COL_INT", "COL_FLT", "NUM_INT", "NUM_FLT", "LIT_INT", "LIT_FLT", "TO_FLT", "TO_INT", "NEG", "ADD", "SUB", "MUL", "DIV", "MOD"]
    src = tmp_path / "ex.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("ops ' + " %d" * len(names) + '\\n", ' + ", ".join("CPH_EXPR_" + n for n in names) + ");"
                   'printf("max %d %d %d\\n", CPH_EXPR_MAX_OPS, CPH_EXPR_MAX_STACK, CPH_EXPR_MAX_NUMS);'
                   'printf("err %d %d %d %d %d %d\\n", CPH_NUM_OK, CPH_NUM_ERR_SYNTAX, CPH_NUM_ERR_RANGE, CPH_NUM_ERR_UNSUPPORTED, '
                   "CPH_NUM_ERR_DIV_ZERO, CPH_NUM_ERR_CONVERT);"
                   'printf("size %zu %zu %zu %zu\\n", sizeof(cph_expr_op), offsetof(cph_expr_op, lit), sizeof(cph_expr_nums), '
                   "offsetof(cph_expr_nums, mem));return 0;}\n")
    exe = tmp_path / "ex"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert out["ops"] == [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    assert out["ops"] == [getattr(E, n) for n in names] == [getattr(N, "CPH_EXPR_" + n) for n in names]
    assert out["max"] == [32, 8, 8] == [E.MAX_OPS, E.MAX_STACK, E.MAX_NUMS] == [N.CPH_EXPR_MAX_OPS, N.CPH_EXPR_MAX_STACK, N.CPH_EXPR_MAX_NUMS]
    assert out["err"] == [0, 1, 2, 3, 4, 5] == [P.NUM_OK, P.NUM_ERR_SYNTAX, P.NUM_ERR_RANGE, P.NUM_ERR_UNSUPPORTED, E.NUM_ERR_DIV_ZERO, E.NUM_ERR_CONVERT]
    assert (N.CPH_NUM_ERR_DIV_ZERO, N.CPH_NUM_ERR_CONVERT) == (4, 5) and (E.INT, E.FLOAT) == (N.CPH_NUM_INT64, N.CPH_NUM_FLOAT64)
    assert out["size"] == [C.sizeof(N.cph_expr_op), N.cph_expr_op.lit.offset, C.sizeof(N.cph_expr_nums), N.cph_expr_nums.mem.offset] == [16, 8, 16, 8]


def test_symbol_declared_exported_and_bound():
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    assert "CPH_API int32_t cph_num_eval(" in hdr
    assert hasattr(C.CDLL(str(N.LIB_PATH)), "cph_num_eval")
    assert "cph_num_eval" in {p[0] for p in N.PROTOTYPES}


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def run_eval(ctx, cols, e, row_ids=None, nrows=None, out_mem=HOST):
    """cph_num_eval through materialize.eval_number; a device result is read back."""
    from csvplus_amd.materialize import eval_number
    from test_map import _from_device
    nc = eval_number(ctx, cols, e, row_ids=row_ids, nrows=nrows, out_mem=out_mem)
    try:
        assert nc.mem == out_mem
        dt = np.int64 if nc.kind == N.CPH_NUM_INT64 else np.float64
        if out_mem == DEVICE:
            values, status = _from_device(nc.values[0], nc.nrows, dt), _from_device(nc.status[0], nc.nrows, np.uint8)
        else:
            values, status = nc.values, nc.status
        return {"kind": nc.kind, "values": values, "status": status, "nerrors": nc.nerrors, "row": nc.first_error_row,
                "op": nc.first_error_op, "err": nc.first_error_kind if nc.nerrors else 0, "host_rows": nc.host_rows, "n": nc.nrows}
    finally:
        nc.release()


def model(e, table, n, row_of=None):
    """The host model over rows 0..n-1; row_of(i) -> {name: row of that column feeding output row i} (default: i)."""
    kind = E.kind_of(e)
    values = np.zeros(n, np.int64 if kind == E.INT else np.float64)
    status = np.zeros(n, np.uint8)
    first = None
    for i in range(n):
        src = row_of(i) if row_of else {}
        v, st, op = E.evaluate(e, {k: c[src.get(k, i)] for k, c in table.items()}, i)
        values[i], status[i] = v, st
        if st and first is None:
            first = (i, op, st)
    return {"kind": kind, "values": values, "status": status, "nerrors": int(np.count_nonzero(status)), "row": first[0] if first else None,
            "op": first[1] if first else None, "err": first[2] if first else 0, "n": n}


def check(got, want, what=""):
    for k in ("kind", "n", "nerrors", "row", "op", "err"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=str(what))
    g, w = got["values"], want["values"]
    assert g.dtype == w.dtype
    if g.dtype == np.float64:
        nan = np.isnan(w)
        np.testing.assert_array_equal(np.isnan(g), nan, err_msg=str(what))
        g, w = np.where(nan, 0.0, g), np.where(nan, 0.0, w)
    bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
    assert len(bad) == 0, (what, int(bad[0]), g[bad[0]], w[bad[0]])


@pytest.mark.gpu
def test_known_answers_on_the_device(ctx):
    for e, value, status in KNOWN:
        got = run_eval(ctx, {}, e, nrows=3)
        check(got, model(e, {}, 3), e)
        assert got["nerrors"] == (3 if status else 0) and same_value(got["values"][2].item(), value), (e, got)
    # the same operands from arrays: every pair in one call
    ints = [0, 1, -1, 2, -2, 7, -7, MAXI, MINI, MAXI - 1, MINI + 1, 3037000500, -3037000500, 10 ** 18, 5]
    a = IntArr([x for x in ints for _ in ints])
    b = IntArr([y for _ in ints for y in ints])
    for e in (a + b, a - b, a * b, a / b, a % b, -a, ToFloat(a) / ToFloat(b), ToInt(ToFloat(a) * 0.5), ToFloat(a) - ToFloat(b), (a / b) * b + a % b):
        check(run_eval(ctx, {}, e), model(e, {}, len(ints) ** 2), e)
    f = FloatArr([0.0, -0.0, 0.5, -0.9, 1e19, -1e19, 2.0 ** 63, -(2.0 ** 63), math.nextafter(2.0 ** 63, 0.0), math.inf, -math.inf, math.nan, 1e-320, 3.999])
    for e in (ToInt(f), -f, f / 0.0, f * f, f + 1.0, ToFloat(ToInt(f)) - f):
        check(run_eval(ctx, {}, e), model(e, {}, f.count), e)


def _int_text(rng, fixed):
    r = rng.random()
    if r < 0.03:
        v = b"x%d" % rng.integers(0, 99)
    elif r < 0.05:
        v = b"" if not fixed else b"12 45"
    elif r < 0.10:
        v = b"0"
    elif r < 0.14 and not fixed:
        v = [b"9223372036854775807", b"-9223372036854775808", b"9223372036854775808", b"99999999999999999999", b"000000000000000000000123", b"+77"][rng.integers(0, 6)]
    else:
        v = b"%d" % rng.integers(-99999, 100000)
    if fixed:   # leading zeros keep the value: every row is 8 bytes
        sign, digits = (v[:1], v[1:]) if v[:1] == b"-" else (b"", v)
        v = sign + digits.rjust(8 - len(sign), b"0")
    return v


def _float_text(rng, fixed):
    r = rng.random()
    if r < 0.03:
        v = b"1.2.3"
    elif r < 0.05:
        v = b"0x10"
    elif r < 0.07:
        v = b"infinity" if fixed else [b"inf", b"-Inf", b"nan", b"+infinity"][rng.integers(0, 4)]
    elif r < 0.12 and not fixed:
        v = [b"1e3", b"-2.5E-3", b".5", b"7.", b"1_0", b"", b"-0", b"123456789012.125"][rng.integers(0, 8)]
    else:
        v = b"%.2f" % (rng.integers(-999999, 1000000) / 100)
    if fixed:
        sign, digits = (v[:1], v[1:]) if v[:1] == b"-" else (b"", v)
        v = sign + digits.rjust(8 - len(sign), b"0")
    return v


def random_expr(rng, arr, depth, kind):
    """A random tree of depth <= `depth` over IntCol("a"), FloatCol("b") and the int array."""
    if depth == 0 or rng.random() < 0.15:
        if kind == E.INT:
            return [IntCol("a"), arr, Lit(int(rng.integers(-5, 6))), IntCol("a")][rng.integers(0, 4)]
        return [FloatCol("b"), Lit(float(rng.integers(-8, 9)) / 4), FloatCol("b")][rng.integers(0, 3)]
    r = rng.random()
    if r < 0.12:
        return Neg(random_expr(rng, arr, depth - 1, kind))
    if r < 0.27:
        other = E.FLOAT if kind == E.INT else E.INT
        return (ToInt if kind == E.INT else ToFloat)(random_expr(rng, arr, depth - 1, other))
    op = [E.ADD, E.SUB, E.MUL, E.DIV, E.MOD][rng.integers(0, 5 if kind == E.INT else 4)]
    return E.Binary(op, random_expr(rng, arr, depth - 1, kind), random_expr(rng, arr, depth - 1, kind))


LAYOUTS = {   # columns on the device? / fixed width? / offset bits / row ids / out_mem
    "host-offs32-identity": (False, False, 32, None, HOST),
    "device-fixed-ids32+base": (True, True, 32, (32, 1000), DEVICE),
    "device-offs64-ids64": (True, False, 64, (64, 0), HOST),
    "host-fixed-ids32+base": (False, True, 32, (32, 7), DEVICE),
}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_random_programs_against_the_host_model(ctx, n, layout):
    from test_map import device_array
    device, fixed, obits, idspec, out_mem = LAYOUTS[layout]
    rng = np.random.default_rng(1000 * n + len(layout))
    m = n + 5 if idspec else n   # the tables' rows; with row ids the output rows pick among them
    table = {"a": [_int_text(rng, fixed) for _ in range(m)], "b": [_float_text(rng, fixed) for _ in range(m)]}
    cols = {k: StrCol.from_values(v, offset_bits=obits, fixed_width=None if fixed else 0) for k, v in table.items()}
    assert all(bool(c.fixed_width) == (fixed and m > 0) for c in cols.values())
    keep, row_ids, row_of = [], None, None
    if idspec:
        bits, base = idspec
        picks = {k: rng.integers(0, m, n) for k in table}
        row_of = lambda i: {k: int(p[i]) for k, p in picks.items()}   # noqa: E731
        row_ids = {}
        for k, p in picks.items():
            ids = (p + base).astype(np.uint32 if bits == 32 else np.uint64)
            row_ids[k] = (device_array(ids, keep), bits, n, base) if device else (ids, base)
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
    arr = IntArr(rng.integers(-50, 50, n))
    done = 0
    while done < 3:
        kind = E.INT if (done + n) % 2 else E.FLOAT
        e = random_expr(rng, arr, 4, kind)
        try:
            E.compile(e, ["a", "b"])
        except TypeError:   # beyond 32 ops: draw again
            continue
        done += 1
        check(run_eval(ctx, cols, e, row_ids=row_ids, nrows=n, out_mem=out_mem), model(e, table, n, row_of), (layout, n, e))
    e = FloatCol("b") * ToFloat(IntCol("a"))   # the reference's own shape
    check(run_eval(ctx, cols, e, row_ids=row_ids, nrows=n, out_mem=out_mem), model(e, table, n, row_of), (layout, n, e))


@pytest.mark.gpu
def test_a_product_feeding_a_sum_is_never_fused(ctx):
    a = 1.0 + 2.0 ** -30
    c = -(1.0 + 2.0 ** -29)
    assert a * a + c == 0.0   # the exact product is 1 + 2^-29 + 2^-60: rounded first, the sum is 0; fused it is 2^-60
    n = 300
    fa, fb, fc = FloatArr([a] * n), FloatArr([a] * n), FloatArr([c] * n)
    cols = {"a": StrCol.from_values([b"1.000000000931322574615478515625"] * n), "c": StrCol.from_values([b"-1.00000000186264514923095703125"] * n)}
    assert P.parse_float(cols["a"].value(0)) == (a, OK) and P.parse_float(cols["c"].value(0)) == (c, OK)
    for e in (fa * fb + fc, fc + fa * fb, Neg(fc) - fa * fb, fa * fb - Neg(fc), Lit(a) * fb + Lit(c), Neg(fc) - Lit(a) * Lit(a),
              FloatCol("a") * FloatCol("a") + FloatCol("c"), Neg(FloatCol("c")) - FloatCol("a") * fb):
        got = run_eval(ctx, cols, e, nrows=n)
        assert got["nerrors"] == 0
        assert (got["values"] == 0.0).all(), (e, got["values"][0], 2.0 ** -60)
        check(got, model(e, {k: v.values() for k, v in cols.items()}, n), e)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_error_placement(ctx, device):
    n = 2 * TILE + 1
    e = FloatCol("price") * ToFloat(IntCol("qty") / IntCol("per"))   # ops: price 0, qty 1, per 2, DIV 3, TO_FLT 4, MUL 5
    base = {"price": [b"%d.25" % (i % 97) for i in range(n)], "qty": [b"%d" % (i % 1000) for i in range(n)], "per": [b"%d" % (1 + i % 5) for i in range(n)]}

    def run(edits):
        table = {k: list(v) for k, v in base.items()}
        for name, i, v in edits:
            table[name][i] = v
        cols = {k: StrCol.from_values(v) for k, v in table.items()}
        if device:
            cols = {k: c.to_device() for k, c in cols.items()}
        got = run_eval(ctx, cols, e, out_mem=DEVICE if device else HOST)
        check(got, model(e, table, n), edits)
        return got

    assert run([])["nerrors"] == 0
    for r in (TILE - 1, TILE):   # the only error at a tile's last row, then at the next tile's first
        got = run([("per", r, b"0")])
        assert (got["nerrors"], got["row"], got["op"], got["err"]) == (1, r, 3, DIV_ZERO)
    got = run([("qty", TILE, b"abc"), ("price", TILE - 1, b"1e")])   # errors in both: the lower row wins
    assert (got["nerrors"], got["row"], got["op"], got["err"]) == (2, TILE - 1, 0, SYNTAX)
    got = run([("qty", 5, b"99999999999999999999"), ("per", 5, b"0"), ("price", n - 1, b"0x1p3")])   # two failing ops in one row: program order
    assert (got["nerrors"], got["row"], got["op"], got["err"]) == (2, 5, 1, RANGE)   # ... and the row counts once
    got = run([("price", 70, b""), ("qty", 70, b"-"), ("per", 70, b"0"), ("per", 64, b"0")])
    assert (got["nerrors"], got["row"], got["op"], got["err"]) == (2, 64, 3, DIV_ZERO) and got["status"][70] == SYNTAX
    assert got["values"][64] == 0.0 and got["values"][70] == 0.0 and got["values"][71] != 0.0   # error rows hold 0


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_deferred_floats_take_the_plain_route_with_the_same_bits(ctx, device):
    from csvplus_amd.materialize import to_float, to_int
    n = TILE + 77
    hard = [b"0.1234567890123456789", b"1e300", b"-2.5e-300", b"9007199254740993", b"123456789012345678901234567890", b"1e400", b"4.9e-324",
            b"1.7976931348623157e308", b"0.30000000000000004441"]
    price = [b"%d.%02d" % (i % 300, i % 100) for i in range(n)]
    for j, v in enumerate(hard):
        price[11 + 200 * j] = v
    price[1500], price[1501] = b"1.5x", b"1_5"
    qty = [b"%d" % (1 + i % 9) for i in range(n)]
    qty[1400] = b"q"
    table = {"price": price, "qty": qty}
    ndef = sum(P.float_is_deferred(v) for v in price)
    assert ndef == len(hard)
    cols = {k: StrCol.from_values(v) for k, v in table.items()}
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
    out_mem = DEVICE if device else HOST
    for e in (FloatCol("price") * ToFloat(IntCol("qty")), ToFloat(IntCol("qty")) / FloatCol("price") + FloatCol("price")):
        got = run_eval(ctx, cols, e, out_mem=out_mem)
        assert got["host_rows"] == ndef > 0
        want = model(e, table, n)
        check(got, want, e)
        assert want["nerrors"] == 4 and want["status"][11 + 200 * 5] == RANGE   # 1e400
        # the same call with the leaves converted first and passed as arrays
        fp, iq = to_float(ctx, cols["price"]), to_int(ctx, cols["qty"])
        assert fp.host_rows == ndef
        ok = (fp.status == 0) & (iq.status == 0)
        pre = E.Binary(E.MUL, FloatArr(fp.values), ToFloat(IntArr(iq.values))) if e.op == E.MUL else ToFloat(IntArr(iq.values)) / FloatArr(fp.values) + FloatArr(fp.values)
        again = run_eval(ctx, {}, pre, out_mem=out_mem)
        assert again["host_rows"] == 0
        np.testing.assert_array_equal(again["values"].view(np.uint64)[ok], got["values"].view(np.uint64)[ok])
        assert (got["status"][~ok] != 0).all() and (got["values"][~ok] == 0).all()


def _call(ctx, cols=None, sel=None, ncols=0, nrows=4, nums=None, nnums=0, prog=None, nops=None, out_mem=HOST):
    out = C.POINTER(N.cph_numcol)()
    eop = C.c_int32(77)
    rc = ctx.lib.cph_num_eval(ctx.handle, cols, sel, ncols, nrows, nums, nnums, prog, len(prog) if nops is None and prog is not None else (nops or 0),
                              out_mem, C.byref(out), C.byref(eop))
    return rc, out, eop.value


def _prog(*ops):
    arr = (N.cph_expr_op * max(len(ops), 1))()
    for k, o in enumerate(ops):
        arr[k].op, arr[k].arg = o[0], o[1] if len(o) > 1 else 0
        if len(o) > 2:
            if isinstance(o[2], int):
                arr[k].lit.i = o[2]
            else:
                arr[k].lit.f = o[2]
    return arr


@pytest.mark.gpu
def test_argument_errors(ctx):
    col = StrCol.from_values([b"1", b"2", b"3", b"4"], fixed_width=0)
    sc, alive = col.as_c()
    keep = [alive]
    cols = (N.cph_strcol * 1)(sc)
    vals = np.arange(4, dtype=np.int64)
    nums = (N.cph_expr_nums * 9)()
    for k in range(9):
        nums[k].ptr, nums[k].mem = vals.ctypes.data, HOST

    def nums_with(ptr, mem):
        a = (N.cph_expr_nums * 1)()
        a[0].ptr, a[0].mem = ptr, mem
        return a

    def sel_bits(bits):
        ids = np.zeros(4, np.uint32)
        keep.append(ids)
        s = (N.cph_rowsel * 1)()
        s[0].ids, s[0].bits = ids.ctypes.data, bits
        return s

    I, F = (E.LIT_INT, 0, 1), (E.LIT_FLT, 0, 1.0)
    ok = _prog((E.COL_INT, 0), (E.NUM_INT, 0), (E.ADD,))
    rc, out, eop = _call(ctx, cols, None, 1, 4, nums, 1, ok)
    assert rc == N.CPH_OK and eop == -1 and out.contents.nerrors == 0 and out.contents.kind == N.CPH_NUM_INT64
    assert list(N._ptr_array(out.contents.values, 4, np.int64)) == [1, 3, 5, 7]
    ctx.lib.cph_numcol_release(out)
    rc, out, eop = _call(ctx, None, None, 0, 0, None, 0, _prog(I))   # nrows == 0 is legal
    assert rc == N.CPH_OK and out.contents.nrows == 0 and not out.contents.values and not out.contents.status and eop == -1
    ctx.lib.cph_numcol_release(out)
    cases = {
        "int + float": dict(prog=_prog(I, F, (E.ADD,))),
        "MOD on floats": dict(prog=_prog(F, F, (E.MOD,))),
        "TO_FLT of a float": dict(prog=_prog(F, (E.TO_FLT,))),
        "TO_INT of an int": dict(prog=_prog(I, (E.TO_INT,))),
        "a binary op with one operand": dict(prog=_prog(I, (E.ADD,))),
        "a unary op on an empty stack": dict(prog=_prog((E.NEG,))),
        "two values left": dict(prog=_prog(I, I)),
        "op 0": dict(prog=_prog((0,))), "op 7": dict(prog=_prog((7,))), "op 16": dict(prog=_prog((16,))),
        "column outside the table": dict(cols=cols, ncols=1, prog=_prog((E.COL_INT, 1))),
        "column -1": dict(cols=cols, ncols=1, prog=_prog((E.COL_FLT, -1))),
        "array outside the table": dict(nums=nums, nnums=1, prog=_prog((E.NUM_INT, 1))),
        "33 ops": dict(prog=_prog(*([I] + [I, (E.ADD,)] * 16))),
        "0 ops": dict(prog=_prog(I), nops=0),
        "a stack of 9": dict(prog=_prog(*([I] * 9 + [(E.ADD,)] * 8))),
        "9 arrays": dict(nums=nums, nnums=9, prog=_prog((E.NUM_INT, 0))),
        "17 columns": dict(cols=cols, ncols=17, prog=_prog(I)),
        "NULL prog": dict(prog=None, nops=1),
        "NULL cols": dict(cols=None, ncols=1, prog=_prog((E.COL_INT, 0))),
        "NULL nums": dict(nums=None, nnums=1, prog=_prog((E.NUM_INT, 0))),
        "an array without values": dict(nums=nums_with(None, HOST), nnums=1, prog=_prog((E.NUM_INT, 0))),
        "an array in an unknown memory space": dict(nums=nums_with(vals.ctypes.data, 7), nnums=1, prog=_prog((E.NUM_INT, 0))),
        "unknown out_mem": dict(prog=_prog(I), out_mem=9),
        "16-bit row ids": dict(cols=cols, sel=sel_bits(16), ncols=1, prog=_prog((E.COL_INT, 0))),
        "an identity column of another row count": dict(cols=cols, ncols=1, nrows=3, prog=_prog((E.COL_INT, 0))),
    }
    for what, kw in cases.items():
        rc, out, eop = _call(ctx, **kw)
        assert rc == N.CPH_ERR_INVALID, (what, rc)
        assert not out, what               # *out stays NULL
        assert ctx.last_error(), what      # ... and there is a message
    assert ctx.lib.cph_num_eval(ctx.handle, None, None, 0, 1, None, 0, _prog(I), 1, HOST, None, None) == N.CPH_ERR_INVALID   # NULL out
    # the limits themselves pass: 31 ops, a stack of 8, 8 arrays
    for prog, nn in ((_prog(*([I] + [I, (E.ADD,)] * 15)), 0), (_prog(*([I] * 8 + [(E.ADD,)] * 7)), 0), (_prog((E.NUM_INT, 7)), 8)):
        rc, out, _ = _call(ctx, nums=nums, nnums=nn, prog=prog)
        assert rc == N.CPH_OK, ctx.last_error()
        ctx.lib.cph_numcol_release(out)
    del keep


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.fixture(scope="module")
def amounts():
    """The reference's amounts table (csvplus_test.go:1391-1421) at fixture size, computed directly in Python."""
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    pv, ov = enc(stock_table()), enc(orders_table(n=2000))
    prices = dict(zip(pv["prod_id"], pv["price"]))
    names = dict(zip(pv["prod_id"], pv["product"]))
    direct = [float(prices[p]) * int(q) for p, q in zip(ov["prod_id"], ov["qty"])]
    return {"pv": pv, "ov": ov, "prices": prices, "names": names, "direct": direct}


AMOUNT = FloatCol("price") * ToFloat(IntCol("qty"))


@pytest.mark.gpu
@pytest.mark.parametrize("positions", [True, False])
def test_amounts_table_end_to_end_without_torch(ctx, amounts, positions):
    from csvplus_amd import pipeline
    pv, ov = amounts["pv"], amounts["ov"]
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    try:
        outc = [("cust_id", to, "cust_id"), ("product", tp, "product"), ("amount", None, None)]
        got = pipeline.join_to_csv(ctx, to, [(tp, "prod_id", "prod_id")], outc, positions=positions,
                                   computed={"amount": M.Format(M.Float.of(AMOUNT, 2))})
        want = b"cust_id,product,amount\n" + b"".join(
            b"%s,%s,%s\n" % (c, amounts["names"][p], b"%.2f" % a) for c, p, a in zip(ov["cust_id"], ov["prod_id"], amounts["direct"]))
        assert got == want
    finally:
        tp.release()
        to.release()


@pytest.mark.gpu
def test_a_bad_qty_raises_with_its_row_and_column(ctx, amounts):
    from csvplus_amd import pipeline
    pv, ov = amounts["pv"], {k: list(v) for k, v in amounts["ov"].items()}
    ov["qty"][1234] = b"1O"
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    try:
        outc = [("cust_id", to, "cust_id"), ("amount", None, None)]
        with pytest.raises(E.ExprError) as err:
            pipeline.join_to_csv(ctx, to, [(tp, "prod_id", "prod_id")], outc, computed={"amount": M.Format(M.Float.of(AMOUNT, 2))})
        x = err.value
        assert (x.row, x.column, x.kind, x.op, x.nerrors) == (1234, "qty", SYNTAX, 1, 1)
        assert 'row 1234: column "qty": cannot convert "1O" to integer: invalid syntax' in str(x)
    finally:
        tp.release()
        to.release()


@pytest.mark.gpu
def test_totals_of_an_expression_per_customer(ctx, amounts):
    """TestSimpleTotals (csvplus_test.go:516-571): the sum of price * qty per cust_id."""
    from csvplus_amd import DeviceIndex
    from csvplus_amd.aggregate import Max, Sum, totals, totals_model
    ov, direct = amounts["ov"], amounts["direct"]
    price = [amounts["prices"][p] for p in ov["prod_id"]]   # the joined rows' price column
    columns = {"price": StrCol.from_values(price), "qty": StrCol.from_values(ov["qty"]).to_device()}
    ix = DeviceIndex(ctx, [StrCol.from_values(ov["cust_id"])])
    try:
        perm = ix.perm()
        specs = [Sum(AMOUNT), Max(IntCol("qty") * 2)]
        assert (specs[0].kind, specs[1].kind) == (N.CPH_NUM_FLOAT64, N.CPH_NUM_INT64)
        t = totals(ix, specs, columns=columns)
        want = totals_model([ov["cust_id"][r] for r in perm], [[direct[r] for r in perm], [2 * int(ov["qty"][r]) for r in perm]], specs)
        assert t.ngroups == want["ngroups"] > 100
        np.testing.assert_array_equal(t.count, want["count"])
        np.testing.assert_array_equal(t.values[1], want["values"][1])
        sums = {}
        for c, a in zip(ov["cust_id"], direct):
            sums[c] = sums.get(c, 0.0) + a
        for g in range(t.ngroups):
            c = ov["cust_id"][int(t.first_row[g])]
            for ref in (want["values"][0][g], sums[c]):   # the model's order and the reference's: its own 1e-6 bound (:566)
                assert abs(t.values[0][g] - ref) <= 1e-6 * abs(ref), (c, t.values[0][g], ref)
        bad = dict(columns, qty=StrCol.from_values([b"x" if i == 321 else v for i, v in enumerate(ov["qty"])]))
        with pytest.raises(E.ExprError) as err:
            totals(ix, [Sum(AMOUNT)], columns=bad)
        assert (err.value.row, err.value.column) == (321, "qty")
    finally:
        ix.close()
