"""cph_ctx_set_option("float_device", 1): float conversions decide the values outside Clinger's exact cases on the device
(k_num_parse's full float instantiation: the Eisel-Lemire conversion of floatparse_device.hpp) and hand only the undecided
ones to the host.  The values, status bytes and error report are those of option 0 — Python's correctly rounded float(),
test_numeric's model — and host_rows counts what the host really finished.  Every consumer of convert_rows inherits it."""
import math

import numpy as np
import pytest

import test_numeric as TN
from csvplus_amd import DeviceIndex, StrCol
from csvplus_amd import _native as N
from csvplus_amd.predicates import FloatCmp

pytestmark = pytest.mark.gpu

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
OK, RANGE = TN.OK, TN.RANGE
TILE = TN.TILE
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 2 * TILE + 1)

LITERALS = [b"9007199254740993", b"9007199254740992.5", b"1.7976931348623157e308", b"1.7976931348623158e308", b"1.7976931348623159e308",
            b"4.9406564584124654e-324", b"2.4703282292062327e-324", b"2.4703282292062328e-324", b"2.2250738585072011e-308",
            b"2.2250738585072014e-308", b"1e23", b"8.5e22", b"1e-343", b"1e309", b"1e400", b"-1e-400", b"-1e400", b"1e-30",
            b"-122.41941550000001", b"9007199254740993.0000000000000000000001", b"+0.000000000000000000000000000001e-300"]


@pytest.fixture
def float_device(ctx):
    ctx.set_option("float_device", 1)
    yield ctx
    ctx.set_option("float_device", 0)


def digits(rng, k):
    return bytes([0x31 + int(rng.integers(9))]) + bytes(rng.integers(0x30, 0x3A, k - 1).astype(np.uint8))


def deferred_by_default(v):
    """test_numeric's model of option 0: valid, and outside Clinger's exact cases."""
    return TN.m_float_device(v)[0] == "defer"


def repr_doubles(n, seed):
    """repr of random bit patterns over the whole exponent range (at most 17 significant digits), those that option 0
    defers: a short one with a small exponent is one of Clinger's cases and is left out."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        for v in rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64).tolist():
            text = repr(v).encode()
            if math.isfinite(v) and len(out) < n and deferred_by_default(text):
                out.append(text)
    return out


def g17_doubles(n, seed):
    return [b"%.17g" % float(v.decode()) for v in repr_doubles(n, seed)]


def subnormals(n, seed):
    rng = np.random.default_rng(seed)
    return [b"%.17g" % float(np.uint64(max(1, int(rng.integers(0, 2 ** 52)) >> int(rng.integers(0, 52)))).view(np.float64)) for _ in range(n)]


def nineteen_digits(n, seed):
    rng = np.random.default_rng(seed)
    return [digits(rng, 19) + b"e%d" % int(rng.integers(-330, 301)) for _ in range(n)]


def truncated(n, nd, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        d = digits(rng, nd)
        if d[19:].strip(b"0"):
            out.append(d + b"e%d" % (int(rng.integers(-330, 301)) - (nd - 19)))
    return out


def is_truncated(v):
    """Non-zero digits behind the 19th significant one: the only values the device may still leave to the host."""
    m = TN._GRAMMAR.fullmatch(v.decode().lstrip("+-"))
    digs = ((m.group(1) or "") + (m.group(2) or "")).lstrip("0")
    return bool(digs[19:].strip("0"))


def class_pool():
    rng = np.random.default_rng(77)
    return ([v for v, *_ in TN.FLOAT_TABLE] + [TN.random_float_text(rng) for _ in range(300)] + LITERALS + g17_doubles(100, 1) + repr_doubles(60, 2)
            + subnormals(60, 3) + nineteen_digits(100, 4) + truncated(60, 25, 5) + truncated(60, 40, 6))


def check_full(res, values, out_mem=HOST):
    """Values, status bytes and the error report against Python's float() (test_numeric's model); host_rows: no value whose
    digits all fit the 19 kept ones."""
    want = [TN.m_float(v) for v in values]
    n = len(values)
    if out_mem == DEVICE:
        vals, stat = TN.d2h(res.values[0], n, np.float64), TN.d2h(res.status[0], n, np.uint8)
    else:
        vals, stat = res.values, res.status
    assert len(vals) == len(stat) == n == res.nrows
    for i, (v, k, _) in enumerate(want):
        assert stat[i] == k, (i, values[i], stat[i], k)
        assert TN.same_float(float(vals[i]), v), (i, values[i], float(vals[i]), v)
    errs = [i for i, w in enumerate(want) if w[1] != OK]
    assert res.nerrors == len(errs)
    assert res.first_error_row == (errs[0] if errs else None)
    assert res.first_error_kind == (want[errs[0]][1] if errs else 0)
    assert res.host_rows <= sum(1 for v, w in zip(values, want) if w[2] and is_truncated(v))
    res.release()


def to_float(ctx, col, **kw):
    from csvplus_amd.materialize import to_float as f
    return f(ctx, col, **kw)


def test_option_values(ctx):
    """0 and 1 are the values; anything else fails with CPH_ERR_INVALID and leaves the setting as it was."""
    col = TN.make_col(repr_doubles(300, 8) + [b"0.1234567890123456789"], True)
    n = col.nrows

    def host_rows():
        res = to_float(ctx, col)
        res.release()
        return res.host_rows

    try:
        assert host_rows() == n                      # the default: every value outside Clinger's cases
        ctx.set_option("float_device", 1)
        assert host_rows() == 0
        for bad in (2, -1, 1 << 40):
            with pytest.raises(N.CphError) as e:
                ctx.set_option("float_device", bad)
            assert e.value.code == N.CPH_ERR_INVALID and "float_device" in e.value.msg
            assert host_rows() == 0                  # still 1
        ctx.set_option("float_device", 0)
        with pytest.raises(N.CphError):
            ctx.set_option("float_device", 2)
        assert host_rows() == n                      # still 0
    finally:
        ctx.set_option("float_device", 0)


def test_the_model_agrees_with_itself_on_the_literals():
    """1e400 is a range error with +Inf, -1e-400 is fine and -0 (the expectations below lean on the model for them)."""
    v, k, _ = TN.m_float(b"1e400")
    assert (v, k) == (math.inf, RANGE)
    v, k, _ = TN.m_float(b"-1e-400")
    assert k == OK and TN.bits(v) == TN.bits(-0.0)
    assert TN.bits(TN.m_float(b"1.7976931348623158e308")[0]) == TN.bits(1.7976931348623157e308)
    assert TN.m_float(b"1.7976931348623159e308")[:2] == (math.inf, RANGE)
    assert TN.m_float(b"2.4703282292062327e-324")[:2] == (0.0, OK) and TN.m_float(b"2.4703282292062328e-324")[0] == 5e-324


@pytest.mark.parametrize("device,offset_bits", [(False, 32), (False, 64), (True, 32), (True, 64)])
def test_value_parity_at_every_edge_size(float_device, device, offset_bits):
    ctx = float_device
    pool = class_pool()
    rng = np.random.default_rng(99 + offset_bits + device)
    for n in SIZES:
        values = [pool[i] for i in rng.integers(0, len(pool), n)] if n < len(pool) else list(pool) + [pool[i] for i in rng.integers(0, len(pool), n - len(pool))]
        check_full(to_float(ctx, TN.make_col(values, device, offset_bits)), values)
    values = [pool[i] for i in rng.integers(0, len(pool), 2049)]
    check_full(to_float(ctx, TN.make_col(values, device, offset_bits), out_mem=DEVICE), values, out_mem=DEVICE)


def test_the_literals_one_by_one(float_device):
    ctx = float_device
    res = to_float(ctx, TN.make_col(LITERALS, True))
    by = {v: (float(res.values[i]), int(res.status[i])) for i, v in enumerate(LITERALS)}
    assert by[b"1e400"] == (math.inf, RANGE) and by[b"-1e400"] == (-math.inf, RANGE) and by[b"1e309"] == (math.inf, RANGE)
    assert by[b"1.7976931348623159e308"] == (math.inf, RANGE)
    assert by[b"-1e-400"][1] == OK and TN.bits(by[b"-1e-400"][0]) == TN.bits(-0.0)
    assert by[b"1e-343"] == (0.0, OK) and TN.bits(by[b"1e-343"][0]) == TN.bits(0.0)
    assert by[b"9007199254740993"] == (9007199254740992.0, OK)
    assert by[b"2.4703282292062328e-324"] == (5e-324, OK)
    assert res.nerrors == 4 and res.first_error_row == LITERALS.index(b"1.7976931348623159e308") and res.first_error_kind == RANGE
    assert res.host_rows == 1   # the tie that only the dropped digits break
    check_full(res, LITERALS)


@pytest.mark.parametrize("device", [False, True])
def test_through_row_ids(float_device, device):
    ctx = float_device
    pool = class_pool()
    rng = np.random.default_rng(17)
    col = TN.make_col(pool, device)
    for id_bits, base, n in ((32, 7, 2049), (64, 1 << 33, 65)):
        ids = rng.integers(0, len(pool), n).astype(np.uint32 if id_bits == 32 else np.uint64)
        with_base = ids + ids.dtype.type(base)
        keep = []
        row_ids = (TN.device_ids(with_base, keep), id_bits, n, base) if device else (with_base, base)
        check_full(to_float(ctx, col, row_ids=row_ids, nrows=n), [pool[i] for i in ids])
        del keep


def both(ctx, run):
    """run() under option 0, then under option 1 (the caller's fixture restores 0)."""
    ctx.set_option("float_device", 0)
    a = run()
    ctx.set_option("float_device", 1)
    return a, run()


def test_host_rows_against_the_default(float_device):
    ctx = float_device
    for values, most in ((repr_doubles(4097, 21), 0), (truncated(4097, 25, 22), 40)):   # 40 <= 1 % of 4097
        col = TN.make_col(values, True)

        def run():
            res = to_float(ctx, col)
            res.release()
            return res

        off, on = both(ctx, run)
        assert off.host_rows == sum(TN.m_float(v)[2] for v in values)
        if most == 0:
            assert off.host_rows == 4097 and on.host_rows == 0
        assert on.host_rows <= most
        assert on.values.tobytes() == off.values.tobytes() and on.status.tobytes() == off.status.tobytes()
        assert (on.nerrors, on.first_error_row, on.first_error_kind) == (off.nerrors, off.first_error_row, off.first_error_kind)
        assert on.values.tobytes() == np.array([float(v) for v in values]).tobytes()


def test_values_longer_than_a_slot(float_device):
    ctx = float_device
    long_tail = [b"1." + b"0" * 150 + b"1", b"0." + b"0" * 200 + b"17e210", b"1" + b"0" * 310, b"12345678901234567890" * 6]
    assert all(104 < len(v) <= 320 for v in long_tail)   # a slot holds 104 value bytes
    col = TN.make_col(long_tail, True)

    def run():
        res = to_float(ctx, col)
        res.release()
        return res

    off, on = both(ctx, run)
    assert on.values.tobytes() == off.values.tobytes() and on.status.tobytes() == off.status.tobytes()
    assert (on.nerrors, on.first_error_row, on.first_error_kind) == (off.nerrors, off.first_error_row, off.first_error_kind)
    check_full(to_float(ctx, col), long_tail)


def seventeen_digit_values(n=300, seed=31):
    """Measured-looking values: 17 significant digits, magnitudes around 1..1000, both signs ("%.17g" drops trailing zeros:
    the few that fall into Clinger's cases that way are left out, so option 0 defers every row)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        text = b"%.17g" % float(rng.uniform(-1000, 1000))
        if deferred_by_default(text):
            out.append(text)
    return out


def test_filter_with_a_float_term(float_device):
    from csvplus_amd.materialize import filter_rows
    ctx = float_device
    values = seventeen_digit_values()
    cols = {"x": TN.make_col(values, True)}
    pred = FloatCmp("x", ">", 12.5)
    off, on = both(ctx, lambda: filter_rows(ctx, cols, pred).tolist())
    assert on == off == [i for i, v in enumerate(values) if float(v) > 12.5] and 0 < len(on) < len(values)


def test_totals_float_sum(float_device):
    from csvplus_amd.aggregate import Sum, totals
    ctx = float_device
    values = seventeen_digit_values()
    keys = [b"k%d" % (i % 7) for i in range(len(values))]
    ix = DeviceIndex(ctx, [StrCol.from_values(keys)])
    try:
        vcol = TN.make_col(values, False)
        off, on = both(ctx, lambda: totals(ix, [Sum(vcol, "float")]))
        assert off.host_rows == len(values) and on.host_rows == 0
        assert on.ngroups == off.ngroups == 7
        assert on.values[0].tobytes() == off.values[0].tobytes()
        assert on.count.tolist() == off.count.tolist()
    finally:
        ix.close()


def test_expression_with_to_float(float_device):
    from csvplus_amd import expr as E
    from csvplus_amd.materialize import eval_number
    ctx = float_device
    values = seventeen_digit_values()
    qty = [b"%d" % (i % 9 + 1) for i in range(len(values))]
    cols = {"x": TN.make_col(values, True), "q": TN.make_col(qty, True)}
    expr = E.FloatCol("x") * E.ToFloat(E.IntCol("q"))

    def run():
        res = eval_number(ctx, cols, expr)
        res.release()
        return res

    off, on = both(ctx, run)
    assert off.host_rows == len(values) and on.host_rows == 0
    assert on.values.tobytes() == off.values.tobytes() and on.status.tobytes() == off.status.tobytes()
    assert on.values.tobytes() == np.array([float(v) * float(q) for v, q in zip(values, qty)]).tobytes() and on.nerrors == 0


def test_order_by_a_float_key(float_device):
    from csvplus_amd.materialize import order_rows
    from csvplus_amd.ordering import Desc
    ctx = float_device
    values = seventeen_digit_values()
    col = TN.make_col(values, True)

    def run():
        key = to_float(ctx, col, out_mem=DEVICE)
        try:
            got = order_rows(ctx, [Desc(key)], len(values))
            try:
                return key.host_rows, got.to_numpy().tolist()
            finally:
                got.release()
        finally:
            key.release()

    off, on = both(ctx, run)
    assert off[0] == len(values) and on[0] == 0
    assert on[1] == off[1] == sorted(range(len(values)), key=lambda i: -float(values[i]))


def test_the_default_is_back_behind_the_fixture(ctx):
    """Runs behind the tests above: their fixture has restored option 0, and the default call reports the old host_rows."""
    values = repr_doubles(300, 41)
    res = to_float(ctx, TN.make_col(values, True))
    assert res.host_rows == len(values) == sum(TN.m_float(v)[2] for v in values)
    TN.check_numcol(res, values, True)
