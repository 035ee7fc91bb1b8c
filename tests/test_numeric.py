"""Typed column values on the device: Row.ValueAsInt / Row.ValueAsFloat64 (csvplus.go:165-205) for a whole column
(cph_col_to_number through materialize.to_int / to_float) and the numeric compare predicates IntCmp / FloatCmp in
cph_filter_rows — the reference's flagship filter `born > 1970` (csvplus_test.go:272-281).

Go's strconv is restated HERE, independently of the package (m_atoi / m_float below), and the package's host functions
(predicates.atoi / parse_float / float_is_deferred) as well as the device are held against it and against a literal table."""
import ctypes as C
import math
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.predicates import All, Any, FloatCmp, IntCmp, Like, Not

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
OK, SYNTAX, RANGE, UNSUP = 0, 1, 2, 3
MAX, MIN = 2 ** 63 - 1, -2 ** 63
TILE = 2048   # rows per workgroup and tile of the conversion kernel and of k_pred_eval


# ---- the model: strconv.Atoi and strconv.ParseFloat restated --------------------------------------------------------------
def m_atoi(b):
    """(value, kind), decided left to right."""
    neg = b[:1] == b"-"
    body = b[1:] if b[:1] in (b"+", b"-") else b
    if not body:
        return 0, SYNTAX
    n = 0
    for c in body:
        if c < 0x30 or c > 0x39:
            return 0, SYNTAX
        if n * 10 > 2 ** 64 - 1 or n * 10 + (c - 0x30) > 2 ** 64 - 1:
            return (MIN if neg else MAX), RANGE
        n = n * 10 + (c - 0x30)
    if not neg and n >= 2 ** 63:
        return MAX, RANGE
    if neg and n > 2 ** 63:
        return MIN, RANGE
    return (-n if neg else n), OK


P10 = [float(10 ** k) for k in range(23)]
_GRAMMAR = re.compile(r"(\d*)(?:\.(\d*))?(?:[eE]([+-]?)(\d+))?")


def m_float_device(b):
    """What the DEVICE decides: ('ok', f) | ('defer',) | ('syntax',) | ('unsup',)."""
    try:
        s = b.decode("ascii")
    except UnicodeDecodeError:
        return ("unsup",) if b"_" in b else ("syntax",)
    if not s:
        return ("syntax",)
    neg, i = False, 0
    if s[0] in "+-":
        neg, i = s[0] == "-", 1
    rest = s[i:]
    if "_" in s or rest[:2].lower() == "0x":
        return ("unsup",)
    if rest.lower() in ("inf", "infinity"):
        return ("ok", -math.inf if neg else math.inf)
    if s.lower() == "nan":
        return ("ok", math.nan)
    m = _GRAMMAR.fullmatch(rest) if rest.isascii() and all(c in "0123456789.eE+-" for c in rest) else None
    if not m or (not m.group(1) and not m.group(2)):
        return ("syntax",)
    ip, fp = m.group(1), m.group(2) or ""
    digs, dp = ip + fp, len(ip)
    k = len(digs) - len(digs.lstrip("0"))
    digs, dp = digs[k:], dp - k
    trunc = False
    if len(digs) > 19:
        trunc = any(c != "0" for c in digs[19:])
        digs = digs[:19]
    mant = int(digs) if digs else 0
    e = 0
    if m.group(4) is not None:
        e = min(int(m.group(4)), 10000) * (-1 if m.group(3) == "-" else 1)
    if mant == 0:
        return ("ok", -0.0 if neg else 0.0)
    exp = dp - len(digs) + e
    if trunc or mant >= 2 ** 53:
        return ("defer",)
    f = -float(mant) if neg else float(mant)
    if exp == 0:
        return ("ok", f)
    if 0 < exp <= 37:
        if exp > 22:
            f *= P10[exp - 22]
            exp = 22
        if abs(f) > 1e15:
            return ("defer",)
        return ("ok", f * P10[exp])
    if -22 <= exp < 0:
        return ("ok", f / P10[-exp])
    return ("defer",)


def m_float(b):
    """(value, kind, deferred): the library's answer, the deferred rows finished by a correctly rounded conversion."""
    r = m_float_device(b)
    if r[0] == "syntax":
        return 0.0, SYNTAX, False
    if r[0] == "unsup":
        return 0.0, UNSUP, False
    if r[0] == "ok":
        return r[1], OK, False
    v = float(b.decode("ascii"))
    return v, (RANGE if math.isinf(v) else OK), True


def bits(x):
    return struct.pack("<d", x)


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or bits(a) == bits(b)


# ---- the literal table ------------------------------------------------------------------------------------------------------
INT_TABLE = [
    (b"12345", 12345, OK), (b"+7", 7, OK), (b"-0", 0, OK), (b"0000000000000000000000001", 1, OK),
    (b"9223372036854775807", MAX, OK), (b"-9223372036854775808", MIN, OK),
    (b"9223372036854775808", MAX, RANGE), (b"-9223372036854775809", MIN, RANGE), (b"99999999999999999999x", MAX, RANGE),
    (b"9223372036854775808x", 0, SYNTAX),
] + [(v, 0, SYNTAX) for v in (b"xyz", b"", b"+", b"--1", b"1_0", b"0x10", b" 1", b"1 ", b"1.0", b"1e3", b"1\x002", b"\xc3\xa9")]

FLOAT_TABLE = [   # (value, expected, kind, deferred)
    (b"3.1415926", 3.1415926, OK, False), (b"0.3", 0.3, OK, False), (b".5", 0.5, OK, False), (b"5.", 5.0, OK, False),
    (b"+.5e-3", 0.0005, OK, False), (b"-0", -0.0, OK, False), (b"1e22", 1e22, OK, False), (b"1e23", 1e23, OK, False),
    (b"Inf", math.inf, OK, False), (b"-infinity", -math.inf, OK, False), (b"NaN", math.nan, OK, False),
] + [(v, 0.0, SYNTAX, False) for v in (b"+nan", b"infi", b".", b"1e", b"1e+", b"xyz", b"", b" 1")] + [
    (b"1_0", 0.0, UNSUP, False), (b"0x1p-2", 0.0, UNSUP, False),
    (b"9007199254740993", 9007199254740993.0, OK, True), (b"0.1000000000000000055511151231257827", 0.1, OK, True),
    (b"1e-400", 0.0, OK, True), (b"1e400", math.inf, RANGE, True), (b"123456789012345678", 123456789012345678.0, OK, True),
]


def test_atoi_model_and_package_against_the_literal_table():
    for v, want, kind in INT_TABLE:
        assert m_atoi(v) == (want, kind), v
        assert P.atoi(v) == (want, kind), v
    assert P.atoi("12345") == (12345, OK)   # str is its UTF-8 bytes


def test_parse_float_model_and_package_against_the_literal_table():
    for v, want, kind, deferred in FLOAT_TABLE:
        mv, mk, md = m_float(v)
        assert (mk, md) == (kind, deferred) and same_float(mv, want), (v, mv, mk, md)
        pv, pk = P.parse_float(v)
        assert pk == kind and same_float(pv, want), (v, pv, pk)
        assert P.float_is_deferred(v) == deferred, v
    assert bits(m_float(b"-0")[0]) == bits(-0.0) != bits(0.0)   # the sign bit of -0


def random_int_text(rng):
    t = rng.random()
    digits = lambda k: bytes(rng.integers(0x30, 0x3A, k).astype(np.uint8))   # noqa: E731
    if t < 0.5:
        return [b"", b"+", b"-"][rng.integers(3)] + digits(int(rng.integers(0, 24)))
    if t < 0.7:
        return str(int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 9))).encode()
    if t < 0.8:
        return str([2 ** 63, 2 ** 63 - 1, -2 ** 63, -2 ** 63 - 1, 2 ** 64, 2 ** 64 - 1][rng.integers(6)]).encode() + [b"", b"x", b"0"][rng.integers(3)]
    s = bytearray([b"", b"+", b"-"][rng.integers(3)] + digits(int(rng.integers(1, 24))))
    s[rng.integers(len(s))] = b" _.ex+-\x00\xc3/:"[rng.integers(11)]
    return bytes(s)


def random_float_text(rng, depth=0):
    t = rng.random()
    ri = lambda n: int(rng.integers(0, n))   # noqa: E731
    if t < 0.3:
        return b"%d.%02d" % (ri(100000), ri(100))
    if t < 0.45:
        return repr(float(rng.uniform(-1e6, 1e6))).encode()
    if t < 0.6:
        return b"%de%d" % (ri(10 ** ri(19)), ri(75) - 30)
    if t < 0.75:
        return [b"", b"+", b"-"][ri(3)] + b"0" * ri(3) + b"%d.%d" % (ri(10 ** ri(12)), ri(10 ** ri(10)))
    if t < 0.85 or depth:
        return [v for v, *_ in FLOAT_TABLE][ri(len(FLOAT_TABLE))]
    s = bytearray(random_float_text(rng, 1))
    if s:
        s[ri(len(s))] = b" _.eEx+-\x00\xc3in0123456789"[ri(22)]
    return bytes(s)


def test_package_host_functions_agree_with_the_model_on_generated_values():
    rng = np.random.default_rng(20261017)
    for _ in range(20000):
        v = random_int_text(rng)
        assert P.atoi(v) == m_atoi(v), v
    for _ in range(20000):
        v = random_float_text(rng)
        mv, mk, md = m_float(v)
        pv, pk = P.parse_float(v)
        assert pk == mk and same_float(pv, mv), (v, pv, pk, mv, mk)
        assert P.float_is_deferred(v) == md, v


def test_exact_path_is_correctly_rounded_and_price_like_values_never_defer():
    """Every value the model says the device decides equals Python's correctly rounded float() bit for bit; of 100 000
    price-like values ("%d.%02d", integer part < 100 000) none is deferred."""
    rng = np.random.default_rng(7)
    for _ in range(20000):
        v = random_float_text(rng)
        r = m_float_device(v)
        if r[0] == "ok" and not math.isnan(r[1]) and not math.isinf(r[1]):
            assert bits(r[1]) == bits(float(v.decode())), v
    assert sum(m_float_device(v)[0] != "ok" for v in price_values(100000)) == 0


def price_values(n, seed=11):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 100000, n), rng.integers(0, 100, n)
    return [b"%d.%02d" % (int(x), int(y)) for x, y in zip(a, b)]


def test_compile_numeric_terms():
    names, ops = P.compile(IntCmp("born", ">", 1970), ["id", "born"])
    assert names == ["born"] and ops == [(21, 0, struct.pack("<q", 1970))]
    names, ops = P.compile(All(FloatCmp("price", "<=", 9.99), IntCmp("qty", "!=", -3), Like(name="x")), ["name", "qty", "price"])
    assert names == ["price", "qty", "name"]
    assert ops == [(25, 0, struct.pack("<d", 9.99)), (19, 1, struct.pack("<q", -3)), (P.LIKE, 2, b"x"), (P.ALL, 3, None)]
    for i, rel in enumerate(("<", "<=", "==", "!=", ">=", ">")):
        assert P.compile(IntCmp("a", rel, 1), ["a"])[1][0][0] == 16 + i == N.CPH_PRED_INT_LT + i
        assert P.compile(FloatCmp("a", rel, 1), ["a"])[1][0][0] == 24 + i == N.CPH_PRED_FLT_LT + i
    assert P.compile(IntCmp("nope", "<", 5), ["a"]) == ([], [(16, -1, struct.pack("<q", 5))])     # no such column: -1
    assert P.compile(FloatCmp("nope", ">", 0.5), ["a"]) == ([], [(29, -1, struct.pack("<d", 0.5))])
    with pytest.raises(ValueError):
        IntCmp("a", "<>", 1)
    with pytest.raises(ValueError):
        IntCmp("a", "<", 2 ** 63)
    with pytest.raises(ValueError):   # LIKE plus numeric terms share the 32 term bits
        P.compile(All(*[IntCmp("a", "<", i) for i in range(17)], *[Like(a=str(i)) for i in range(16)]), ["a"])
    P.compile(Any(*[IntCmp("a", "<", i) for i in range(16)], *[Like(a=str(i)) for i in range(16)]), ["a"])


NUM_ROWS = [{"a": v, "s": s} for v, s in zip(
    [b"5", b"-5", b"xyz", b"", b"1e3", b"nan", b"0.5", b"9223372036854775808", b"+5", b"5.0", b"1_0", b"inf"],
    [b"x", b"y"] * 6)] + [{"s": b"x"}]   # the last row has no column "a"


def numeric_preds():
    out = []
    for rel in P.RELS:
        out += [IntCmp("a", rel, 5), FloatCmp("a", rel, 5.0), FloatCmp("a", rel, math.nan), Not(IntCmp("a", rel, 5)),
                All(IntCmp("a", rel, 0), Like(s="x")), Any(FloatCmp("a", rel, 0.5), Not(Like(s="x")), IntCmp("zzz", rel, 1)),
                Not(Any(All(FloatCmp("a", rel, 1000.0), Like(s="x")), IntCmp("a", rel, -5)))]
    return out


def test_matches_equals_run_ops_for_numeric_nestings():
    for pred in numeric_preds():
        names, ops = P.compile(pred, ["a", "s"])
        for r in NUM_ROWS[:-1]:
            assert P.run_ops(ops, [r[k] for k in names]) == P.matches(pred, r) == m_eval(pred, r), (pred, r)
    # a row that does not convert, or lacks the column, is false under every relation — "!=" included — and Not of it true
    for rel in P.RELS:
        for row in ({"a": b"xyz"}, {"a": b"9223372036854775808"}, {"b": b"1"}):
            assert not P.matches(IntCmp("a", rel, 1), row) and P.matches(Not(IntCmp("a", rel, 1)), row)
        assert not P.matches(FloatCmp("a", rel, 1.0), {"a": b"1_0"}) and not P.matches(FloatCmp("a", rel, 1.0), {"a": b"1e400"})
        assert P.matches(FloatCmp("a", rel, 1.0), {"a": b"nan"}) == (rel == "!=")       # IEEE: only != holds with a NaN
        assert P.matches(FloatCmp("a", rel, math.nan), {"a": b"1"}) == (rel == "!=")


def m_eval(pred, row):
    """The predicate on one row, numeric terms through this file's model."""
    if isinstance(pred, (IntCmp, FloatCmp)):
        v = row.get(pred.column)
        if v is None:
            return False
        if isinstance(pred, IntCmp):
            x, kind = m_atoi(v)
        else:
            x, kind, _ = m_float(v)
        k = pred.literal
        return kind == OK and {"<": x < k, "<=": x <= k, "==": x == k, "!=": x != k, ">=": x >= k, ">": x > k}[pred.rel]
    if isinstance(pred, Like):
        return all(row.get(name) == value for name, value in pred.items)
    if isinstance(pred, Not):
        return not m_eval(pred.pred, row)
    if isinstance(pred, All):
        return all(m_eval(p, row) for p in pred.preds)
    return any(m_eval(p, row) for p in pred.preds)


def test_conversion_error_strings():
    assert P.conversion_error("string", "xyz", SYNTAX) == 'column "string": cannot convert "xyz" to integer: invalid syntax'    # :932
    assert P.conversion_error("string", "xyz", SYNTAX, as_float=True) == 'column "string": cannot convert "xyz" to float: invalid syntax'   # :954
    assert P.conversion_error("n", b"99999999999999999999", RANGE) == 'column "n": cannot convert "99999999999999999999" to integer: value out of range'
    assert P.conversion_error("n", b'a"b\\c\n\x00\xff\xc3\xa9', SYNTAX).split(": cannot convert ")[1].startswith('"a\\"b\\\\c\\n\\x00\\xffé"')


def test_numeric_struct_sizes_and_enums_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("cph_numcol %zu\\n", sizeof(cph_numcol));'
                   'printf("offs %zu %zu %zu %zu\\n", offsetof(cph_numcol, kind), offsetof(cph_numcol, nerrors), '
                   'offsetof(cph_numcol, first_error_kind), offsetof(cph_numcol, host_rows));'
                   'printf("kinds %d %d %d %d %d %d\\n", CPH_NUM_INT64, CPH_NUM_FLOAT64, CPH_NUM_OK, CPH_NUM_ERR_SYNTAX, CPH_NUM_ERR_RANGE, '
                   "CPH_NUM_ERR_UNSUPPORTED);"
                   'printf("ops %d %d %d %d %d %d %d %d %d %d %d %d\\n", CPH_PRED_INT_LT, CPH_PRED_INT_LE, CPH_PRED_INT_EQ, CPH_PRED_INT_NE, '
                   "CPH_PRED_INT_GE, CPH_PRED_INT_GT, CPH_PRED_FLT_LT, CPH_PRED_FLT_LE, CPH_PRED_FLT_EQ, CPH_PRED_FLT_NE, CPH_PRED_FLT_GE, "
                   "CPH_PRED_FLT_GT);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert C.sizeof(N.cph_numcol) == int(out["cph_numcol"]) == 64
    f = N.cph_numcol
    assert out["offs"].split() == [str(v) for v in (f.kind.offset, f.nerrors.offset, f.first_error_kind.offset, f.host_rows.offset)]
    assert out["kinds"].split() == [str(v) for v in (N.CPH_NUM_INT64, N.CPH_NUM_FLOAT64, N.CPH_NUM_OK, N.CPH_NUM_ERR_SYNTAX,
                                                     N.CPH_NUM_ERR_RANGE, N.CPH_NUM_ERR_UNSUPPORTED)] == ["1", "2", "0", "1", "2", "3"]
    assert [int(v) for v in out["ops"].split()] == list(range(16, 22)) + list(range(24, 30))
    assert (N.CPH_PRED_INT_LT, N.CPH_PRED_INT_GT, N.CPH_PRED_FLT_LT, N.CPH_PRED_FLT_GT) == (16, 21, 24, 29) == (P.INT_LT, P.INT_LT + 5, P.FLT_LT, P.FLT_LT + 5)
    assert (P.NUM_OK, P.NUM_ERR_SYNTAX, P.NUM_ERR_RANGE, P.NUM_ERR_UNSUPPORTED) == (OK, SYNTAX, RANGE, UNSUP)


def test_numeric_symbols_declared_exported_and_bound():
    lib = C.CDLL(str(N.LIB_PATH))
    bound = {p[0] for p in N.PROTOTYPES}
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    for name in ("cph_col_to_number", "cph_numcol_release"):
        assert hasattr(lib, name) and name in bound and re.search(r"CPH_API\s+\w+\s+%s\(" % name, hdr)
    assert "} cph_numcol;" in hdr and hasattr(N, "cph_numcol")
    from csvplus_amd import materialize
    assert callable(materialize.to_int) and callable(materialize.to_float)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _hip():
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def d2h(ptr, count, dtype):
    out = np.empty(count, dtype=dtype)
    if count:
        assert _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def device_ids(ids, keep):
    import torch
    t = torch.from_numpy(ids.view(np.uint8).copy()).to("cuda:0") if len(ids) else torch.empty(8, dtype=torch.uint8, device="cuda:0")
    keep.append(t)
    return t.data_ptr()


def make_col(values, device=False, offset_bits=32, fixed=None):
    sc = StrCol.from_values(values, offset_bits=offset_bits, fixed_width=fixed)
    return sc.to_device() if device else sc


def expect(values, as_float):
    """Per row (value, kind, deferred) by the model."""
    if as_float:
        return [m_float(v) for v in values]
    return [m_atoi(v) + (False,) for v in values]


def check_numcol(res, values, as_float, out_mem=HOST):
    want = expect(values, as_float)
    n = len(values)
    if out_mem == DEVICE:
        vals = d2h(res.values[0], n, np.float64 if as_float else np.int64)
        stat = d2h(res.status[0], n, np.uint8)
        assert res.values[1] == res.status[1] == n
    else:
        vals, stat = res.values, res.status
    assert len(vals) == len(stat) == n == res.nrows
    for i, (v, k, _) in enumerate(want):
        assert stat[i] == k, (i, values[i], stat[i], k)
        if as_float:
            assert same_float(float(vals[i]), v), (i, values[i], float(vals[i]), v)
        else:
            assert int(vals[i]) == v, (i, values[i], int(vals[i]), v)
    errs = [i for i, w in enumerate(want) if w[1] != OK]
    assert res.nerrors == len(errs)
    assert res.first_error_row == (errs[0] if errs else None)
    assert res.first_error_kind == (want[errs[0]][1] if errs else 0)
    assert res.host_rows == sum(w[2] for w in want)
    res.release()


def convert(ctx, col, as_float, **kw):
    from csvplus_amd.materialize import to_float, to_int
    return (to_float if as_float else to_int)(ctx, col, **kw)


def mixed_pool(as_float, count=300, seed=5):
    rng = np.random.default_rng(seed + as_float)
    gen = random_float_text if as_float else random_int_text
    return [gen(rng) for _ in range(count)] + [v for v, *_ in (FLOAT_TABLE if as_float else INT_TABLE)]


SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 2 * TILE + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int", "float"])
@pytest.mark.parametrize("device,offset_bits", [(False, 32), (False, 64), (True, 32), (True, 64)])
def test_columns_of_every_edge_size_against_the_model(ctx, as_float, device, offset_bits):
    pool = mixed_pool(as_float)
    rng = np.random.default_rng(99)
    for n in SIZES:
        values = [pool[i] for i in rng.integers(0, len(pool), n)]
        check_numcol(convert(ctx, make_col(values, device, offset_bits), as_float), values, as_float)
    values = [pool[i] for i in rng.integers(0, len(pool), 2049)]
    check_numcol(convert(ctx, make_col(values, device, offset_bits), as_float, out_mem=DEVICE), values, as_float, out_mem=DEVICE)


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int", "float"])
def test_the_literal_table_as_one_column(ctx, as_float):
    values = [v for v, *_ in (FLOAT_TABLE if as_float else INT_TABLE)]
    for device in (False, True):
        res = convert(ctx, make_col(values, device), as_float)
        if as_float:
            for i, (v, want, kind, _) in enumerate(FLOAT_TABLE):
                assert res.status[i] == kind and same_float(float(res.values[i]), want), v
            assert bits(float(res.values[5])) == bits(-0.0)
            assert res.host_rows == sum(d for *_, d in FLOAT_TABLE) == 5
        else:
            for i, (v, want, kind) in enumerate(INT_TABLE):
                assert (int(res.values[i]), res.status[i]) == (want, kind), v
        check_numcol(res, values, as_float)


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int", "float"])
def test_value_lengths_alignments_and_fixed_widths(ctx, as_float):
    rng = np.random.default_rng(3)
    digits = lambda k: bytes(rng.integers(0x30, 0x3A, k).astype(np.uint8))   # noqa: E731
    by_len = []
    for ln in (0, 1, 7, 8, 9, 15, 16, 17, 19, 20, 25, 40):
        for _ in range(6):
            v = bytearray(digits(ln))
            if ln and rng.random() < 0.5:
                v[0] = b"+-"[rng.integers(2)]
            if as_float and ln > 1 and rng.random() < 0.7:
                v[rng.integers(1 if v[0] in b"+-" else 0, ln)] = 0x2E
            if ln and rng.random() < 0.15:
                v[rng.integers(ln)] = b"x e"[rng.integers(3)]
            by_len.append(bytes(v))
    for shift in range(8):   # the first value moves every later one: each length meets each alignment within a word
        values = [b"7" * shift] + by_len
        for device in (False, True):
            check_numcol(convert(ctx, make_col(values, device), as_float), values, as_float)
    for w in (4, 8, 11):
        pool = [digits(w), b"-" + digits(w - 1), b"+" + digits(w - 1), digits(w - 2) + b". "[rng.integers(2):][:1] + digits(1),
                digits(1) + b"." + digits(w - 2), b"0" * w, b"x" * w, digits(w - 2) + b"e1", b" " * (w - 1) + b"1"]
        assert all(len(p) == w for p in pool)
        values = [pool[i] for i in rng.integers(0, len(pool), 300)]
        for device in (False, True):
            col = make_col(values, device, fixed=w)
            assert col.fixed_width == w
            check_numcol(convert(ctx, col, as_float), values, as_float)


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int", "float"])
def test_first_error_row(ctx, as_float):
    n = 2 * TILE + 1
    good = [b"%d" % i for i in range(n)]
    for at, bad in ((n - 1, b"xyz"), (0, b""), (TILE + 5, b"1_0"), (TILE - 1, b"1e9999" if as_float else b"99999999999999999999")):
        values = list(good)
        values[at] = bad
        res = convert(ctx, make_col(values, True), as_float)
        assert (res.nerrors, res.first_error_row) == (1, at)
        assert res.first_error_kind == (m_float(bad)[1] if as_float else m_atoi(bad)[1])
        check_numcol(res, values, as_float)
    values = list(good)
    values[TILE + 7], values[70], values[n - 1] = b"x", b"99999999999999999999999999", b"-"
    res = convert(ctx, make_col(values, False), as_float)
    assert (res.nerrors, res.first_error_row) == (2 if as_float else 3, TILE + 7 if as_float else 70)
    check_numcol(res, values, as_float)


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int", "float"])
@pytest.mark.parametrize("device", [False, True])
def test_through_row_ids(ctx, as_float, device):
    pool = mixed_pool(as_float, 200)
    rng = np.random.default_rng(17)
    col = make_col(pool, device)
    for id_bits, base, n in ((32, 7, 2049), (64, 1 << 33, 65), (32, 0, 1), (64, 3, 0)):
        ids = rng.integers(0, len(pool), n).astype(np.uint32 if id_bits == 32 else np.uint64)   # repeated ids
        with_base = ids + ids.dtype.type(base)
        keep = []
        row_ids = (device_ids(with_base, keep), id_bits, n, base) if device else (with_base, base)
        check_numcol(convert(ctx, col, as_float, row_ids=row_ids, nrows=n), [pool[i] for i in ids], as_float)
        del keep


@pytest.mark.gpu
def test_over_the_row_ids_of_a_real_join(ctx):
    """orders JOIN people ON cust_id = id: the people's `born` and a price per person convert through the Join's row ids
    without being materialised."""
    rng = np.random.default_rng(23)
    ids = [b"%d" % i for i in range(500)]
    born = [b"%d" % y for y in rng.integers(1900, 2010, 500)]
    born[13] = b"n/a"
    price = price_values(500)
    cust = [b"%d" % i for i in rng.integers(0, 520, 3000)]   # some orders have no customer
    ix = DeviceIndex(ctx, [StrCol.from_values(ids)], unique=True)
    mt = ix.probe([StrCol.from_values(cust)])
    rows = mt.build_row
    assert 0 < len(rows) < 3000
    check_numcol(convert(ctx, StrCol.from_values(born), False, row_ids=rows.astype(np.uint32)), [born[r] for r in rows], False)
    check_numcol(convert(ctx, StrCol.from_values(price), True, row_ids=rows.astype(np.uint64)), [price[r] for r in rows], True)
    ix.close()


@pytest.mark.gpu
def test_host_rows_counts_exactly_the_deferred_values(ctx):
    prices = price_values(100000)
    res = convert(ctx, make_col(prices, True), True)
    assert res.host_rows == 0 and res.nerrors == 0
    want = np.array([float(p) for p in prices])
    assert res.values.tobytes() == want.tobytes()
    res.release()
    pool = mixed_pool(True, 2000, seed=31)
    deferred = sum(m_float(v)[2] for v in pool)
    assert 20 < deferred < len(pool) // 2
    res = convert(ctx, make_col(pool, False), True)
    assert res.host_rows == deferred
    check_numcol(res, pool, True)
    long_tail = [b"1." + b"0" * 150 + b"1", b"0." + b"0" * 200 + b"17e210", b"1" + b"0" * 310, b"12345678901234567890" * 6]   # longer than a slot
    check_numcol(convert(ctx, make_col(long_tail, True), True), long_tail, True)


def people_rows(n=1200, seed=41):
    """A people table with a `born` column, as makePersonsCsvFile writes it (csvplus_test.go:1220-1253)."""
    from helpers import PEOPLE_NAMES, PEOPLE_SURNAMES
    rng = np.random.default_rng(seed)
    return [{"id": b"%d" % i, "name": PEOPLE_NAMES[i % 10].encode(), "surname": PEOPLE_SURNAMES[(i // 10) % 12].encode(),
             "born": b"%d" % (1916 + int(rng.integers(0, 90)))} for i in range(n)]


def cols_from_rows(rows, device):
    return {k: make_col([r[k] for r in rows], device) for k in rows[0]}


def model_select(rows, pred, mode="where", first_row=0, nrows=None, skip=0, limit=None):
    n = len(rows) - first_row if nrows is None else nrows
    out, dropping = [], True
    for i in range(first_row, first_row + n):
        ok = m_eval(pred, rows[i])
        if mode == "where":
            if ok:
                out.append(i)
        elif mode == "take_while":
            if not ok:
                break
            out.append(i)
        else:
            dropping = dropping and ok
            if not dropping:
                out.append(i)
    out = out[skip:]
    return out if limit is None else out[:limit]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_filter_rows_every_relation_and_mode(ctx, device):
    from csvplus_amd.materialize import filter_rows
    rng = np.random.default_rng(53)
    n = 2 * TILE + 1
    texts = [b"%d" % v for v in rng.integers(-50, 50, n)]
    for i in rng.integers(0, n, 40):
        texts[i] = [b"xyz", b"", b"1e3", b"4.5", b"nan", b"99999999999999999999", b"1_0", b"0.1000000000000000055511151231257827",
                    b"1e400", b"+7", b"0000000000000000000000001"][rng.integers(11)]
    rows = [{"v": t, "s": b"xy"[i % 2:][:1]} for i, t in enumerate(texts)]
    cols = cols_from_rows(rows, device)
    for rel in P.RELS:
        for pred in (IntCmp("v", rel, 7), FloatCmp("v", rel, 4.5), FloatCmp("v", rel, 0.1)):
            for mode, kw in (("where", {}), ("where", dict(first_row=70, nrows=TILE, skip=3, limit=50)), ("take_while", dict(first_row=5)),
                             ("drop_while", dict(skip=2, limit=9)), ("take_while", {}), ("drop_while", dict(first_row=TILE + 1))):
                got = filter_rows(ctx, cols, pred, mode=mode, **kw)
                assert got.tolist() == model_select(rows, pred, mode, **kw), (pred, mode, kw)
    # monotone data: the WHILE modes stop in the second tile
    mono = [{"v": b"%d" % i} for i in range(n)]
    mcols = cols_from_rows(mono, device)
    assert filter_rows(ctx, mcols, IntCmp("v", "<", TILE + 9), mode="take_while").tolist() == list(range(TILE + 9))
    assert filter_rows(ctx, mcols, FloatCmp("v", "<=", TILE + 9.5), mode="drop_while").tolist() == list(range(TILE + 10, n))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_filter_rows_nestings_nan_and_unconvertible_rows(ctx, device):
    from csvplus_amd.materialize import filter_rows
    rows = [dict(r) for r in NUM_ROWS[:-1]] * 6
    cols = cols_from_rows(rows, device)
    for pred in numeric_preds():
        for mode in ("where", "take_while", "drop_while"):
            assert filter_rows(ctx, cols, pred, mode=mode).tolist() == model_select(rows, pred, mode), (pred, mode)
    bad = [i for i, r in enumerate(rows) if m_atoi(r["a"])[1] != OK]
    for rel in P.RELS:
        got = set(filter_rows(ctx, cols, IntCmp("a", rel, 5)).tolist())
        assert not got & set(bad)                                                      # false under every relation
        assert set(bad) <= set(filter_rows(ctx, cols, Not(IntCmp("a", rel, 5))).tolist())   # and Not of it true
        nan_rows = [i for i, r in enumerate(rows) if r["a"] == b"nan"]
        got = filter_rows(ctx, cols, FloatCmp("a", rel, 1.0)).tolist()
        assert set(nan_rows) <= set(got) if rel == "!=" else not set(nan_rows) & set(got)
        lit_nan = filter_rows(ctx, cols, FloatCmp("a", rel, math.nan)).tolist()
        assert lit_nan == ([i for i, r in enumerate(rows) if m_float(r["a"])[1] == OK] if rel == "!=" else [])


@pytest.mark.gpu
def test_filter_rows_with_deferred_float_values(ctx):
    """Values the device hands to the host compare as their correctly rounded doubles: the answer does not depend on where
    a value was converted."""
    from csvplus_amd.materialize import filter_rows
    vals = [b"9007199254740993", b"9007199254740992", b"0.1000000000000000055511151231257827", b"0.1", b"1e-400", b"1e400",
            b"123456789012345678", b"0.30000000000000004440892098500626", b"0.3", b"1.7976931348623157e308", b"4.9e-324"] * 200
    rows = [{"x": v} for v in vals]
    assert sum(m_float(v)[2] for v in vals) > 1000
    for device in (False, True):
        cols = cols_from_rows(rows, device)
        for pred in (FloatCmp("x", "==", 0.1), FloatCmp("x", ">", 9007199254740992.0), FloatCmp("x", "<=", 0.3), FloatCmp("x", "!=", 0.0),
                     Any(FloatCmp("x", "==", 9007199254740992.0), FloatCmp("x", "<", 1e-300))):
            for mode in ("where", "take_while", "drop_while"):
                assert filter_rows(ctx, cols, pred, mode=mode).tolist() == model_select(rows, pred, mode), (pred, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_the_reference_flagship_filter(ctx, device):
    """people.Filter(born > 1970).Filter(Like(surname: Smith)).Top(10) (csvplus_test.go:272-293)."""
    from csvplus_amd.materialize import filter_rows
    rows = people_rows()
    cols = cols_from_rows(rows, device)
    pred = All(IntCmp("born", ">", 1970), Like(surname="Smith"))
    got = filter_rows(ctx, cols, pred, limit=10).tolist()
    assert got == model_select(rows, pred, limit=10) and len(got) == 10
    assert all(int(rows[i]["born"]) > 1970 and rows[i]["surname"] == b"Smith" for i in got)
    everyone = filter_rows(ctx, cols, IntCmp("born", ">", 1970)).tolist()
    assert everyone == [i for i, r in enumerate(rows) if int(r["born"]) > 1970] and 0 < len(everyone) < len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_filter_over_joined_rows_through_row_ids(ctx, device):
    from csvplus_amd.materialize import filter_rows
    people = people_rows(300)
    rng = np.random.default_rng(61)
    n = TILE + 77
    who = rng.integers(0, 300, n)
    qty = [b"%d" % q for q in rng.integers(1, 100, n)]
    price = price_values(300, seed=5)
    joined = [{"born": people[w]["born"], "surname": people[w]["surname"], "qty": qty[i], "price": price[w]} for i, w in enumerate(who)]
    cols = {"born": make_col([p["born"] for p in people], device), "surname": make_col([p["surname"] for p in people], device),
            "price": make_col(price, device), "qty": make_col(qty, device)}
    keep = []
    base = 11
    for bits_, dt in ((32, np.uint32), (64, np.uint64)):
        ids = who.astype(dt) + dt(base)
        one = (device_ids(ids, keep), bits_, n, base) if device else (ids, base)
        row_ids = {"born": one, "surname": one, "price": one}
        pred = Any(All(IntCmp("born", ">=", 1970), FloatCmp("price", "<", 50000.0), IntCmp("qty", "!=", 7)), Like(surname="Lewis"))
        for mode, kw in (("where", {}), ("where", dict(first_row=100, nrows=TILE - 100, skip=1, limit=40)), ("drop_while", {})):
            got = filter_rows(ctx, cols, pred, row_ids=row_ids, nrows=kw.get("nrows", n - kw.get("first_row", 0)), mode=mode,
                              **{k: v for k, v in kw.items() if k != "nrows"})
            assert got.tolist() == model_select(joined, pred, mode, **kw), (bits_, mode, kw)
    del keep


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
def test_join_to_csv_where_numeric(ctx):
    """pipeline.join_to_csv(where=IntCmp / FloatCmp) is byte-equal to the unfiltered text filtered line by line on the host."""
    from csvplus_amd import pipeline
    from helpers import orders_table, stock_table
    enc = lambda tab: {k: [v.encode() if isinstance(v, str) else v for v in vs] for k, vs in tab.items()}   # noqa: E731
    people = people_rows(120)
    cv = {k: [r[k] for r in people] for k in ("id", "name", "surname", "born")}
    pv, ov = enc(stock_table()), enc(orders_table(n=3000))
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    steps = [(tc, "id", "cust_id"), (tp, "prod_id", "prod_id")]
    outc = [("order_id", to, "order_id"), ("surname", tc, "surname"), ("born", tc, "born"), ("price", tp, "price"), ("qty", to, "qty")]
    try:
        full = pipeline.join_to_csv(ctx, to, steps, outc)
        lines = full.split(b"\n")
        head, body = lines[0], [ln for ln in lines[1:] if ln]
        assert len(body) == 3000

        def text(keep, skip=0, limit=None):
            kept = [ln for ln in body if keep(ln.split(b","))][skip:]
            return b"".join(ln + b"\n" for ln in [head] + (kept if limit is None else kept[:limit]))

        want = text(lambda f: int(f[2]) > 1970)
        assert 100 < want.count(b"\n") < 2900
        assert pipeline.join_to_csv(ctx, to, steps, outc, where=IntCmp("born", ">", 1970)) == want
        pred = All(IntCmp("born", ">", 1970), Like(surname="Smith"), FloatCmp("price", "<=", 0.05), Not(IntCmp("qty", "<", 10)))
        want = text(lambda f: int(f[2]) > 1970 and f[1] == b"Smith" and float(f[3]) <= 0.05 and not int(f[4]) < 10, skip=1, limit=10)
        assert want.count(b"\n") > 3
        assert pipeline.join_to_csv(ctx, to, steps, outc, where=pred, skip=1, limit=10) == want
        assert pipeline.filter_to_csv(ctx, tc, IntCmp("born", "<", 1916), ["id"]) == b"id\n"
    finally:
        for t in (tc, tp, to):
            t.release()


def _filter_call(ctx, cols, ncols, n, ops, sel=None):
    from csvplus_amd.materialize import _pred_program
    keep = []
    arr = _pred_program(ops, keep)
    o = N.cph_filter_opts(0, 32, 0, 0, N.CPH_NO_LIMIT)
    out = C.POINTER(N.cph_rowlist)()
    rc = ctx.lib.cph_filter_rows(ctx.handle, cols, sel, ncols, n, arr, len(ops), C.byref(o), HOST, C.byref(out))
    assert not out or rc == N.CPH_OK
    if out:
        ctx.lib.cph_rowlist_release(out)
    return rc, ctx.last_error()


@pytest.mark.gpu
def test_argument_errors_have_a_status_and_a_message(ctx):
    a = StrCol.from_values([b"1", b"22", b"1"])
    arr = (N.cph_strcol * 1)()
    arr[0], k0 = a.as_c()
    i8, f8 = struct.pack("<q", 1), struct.pack("<d", 1.0)
    assert _filter_call(ctx, arr, 1, 3, [(16, 0, i8)])[0] == N.CPH_OK and _filter_call(ctx, arr, 1, 3, [(29, 0, f8)])[0] == N.CPH_OK
    assert _filter_call(ctx, arr, 1, 3, [(18, -1, i8)])[0] == N.CPH_OK
    bad = [("literal of 4 bytes", [(16, 0, i8[:4])]), ("float literal of 4 bytes", [(24, 0, f8[:4])]), ("literal of 9 bytes", [(16, 0, i8 + b"\0")]),
           ("NULL literal", [(16, 0, None)]), ("op 6", [(6, 0, i8)]), ("op 15", [(15, 0, i8)]), ("op 22", [(22, 0, i8)]), ("op 23", [(23, 0, i8)]),
           ("op 30", [(30, 0, f8)]), ("column 1 of 1", [(17, 1, i8)]), ("column -2", [(25, -2, f8)]),
           ("33 mixed terms", [(P.LIKE, 0, b"1")] * 16 + [(16, 0, i8)] * 9 + [(24, 0, f8)] * 8 + [(P.ANY, 33, None)])]
    for what, ops in bad:
        rc, msg = _filter_call(ctx, arr, 1, 3, ops)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    assert _filter_call(ctx, arr, 1, 3, [(P.LIKE, 0, b"1")] * 16 + [(16, 0, i8)] * 8 + [(24, 0, f8)] * 8 + [(P.ANY, 32, None)])[0] == N.CPH_OK
    # a numeric literal with a length but no pointer
    prog = (N.cph_pred_op * 1)()
    prog[0].op, prog[0].arg, prog[0].value.len = 16, 0, 8
    o = N.cph_filter_opts(0, 32, 0, 0, N.CPH_NO_LIMIT)
    rl = C.POINTER(N.cph_rowlist)()
    assert ctx.lib.cph_filter_rows(ctx.handle, arr, None, 1, 3, prog, 1, C.byref(o), HOST, C.byref(rl)) == N.CPH_ERR_INVALID
    assert ctx.last_error() and not rl

    def to_number(col=arr, sel=None, n=3, kind=N.CPH_NUM_INT64, out_mem=HOST, out=True):
        res = C.POINTER(N.cph_numcol)()
        rc = ctx.lib.cph_col_to_number(ctx.handle, col, sel, n, kind, out_mem, C.byref(res) if out else None)
        assert not res or rc == N.CPH_OK
        if res:
            ctx.lib.cph_numcol_release(res)
        return rc, ctx.last_error()

    assert to_number()[0] == N.CPH_OK and to_number(kind=N.CPH_NUM_FLOAT64, out_mem=DEVICE)[0] == N.CPH_OK
    for what, kw in (("kind 0", dict(kind=0)), ("kind 3", dict(kind=3)), ("out_mem 2", dict(out_mem=2)), ("NULL col", dict(col=None)),
                     ("short identity column", dict(n=4)), ("long identity column", dict(n=2))):
        rc, msg = to_number(**kw)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    assert to_number(out=False)[0] == N.CPH_ERR_INVALID
    sel = (N.cph_rowsel * 1)()
    ids = np.zeros(3, np.uint32)
    sel[0].ids, sel[0].bits = ids.ctypes.data, 16
    rc, msg = to_number(sel=sel)
    assert rc == N.CPH_ERR_INVALID and "bits" in msg
    sel[0].bits = 32
    assert to_number(sel=sel, n=2)[0] == N.CPH_OK   # through row ids the column's own row count does not matter
    # nrows == 0 is legal: no arrays, no errors
    res = C.POINTER(N.cph_numcol)()
    assert ctx.lib.cph_col_to_number(ctx.handle, arr, sel, 0, N.CPH_NUM_FLOAT64, HOST, C.byref(res)) == N.CPH_OK
    c = res.contents
    assert (c.nrows, c.nerrors, c.first_error_row, c.host_rows, c.kind, c.mem) == (0, 0, N.CPH_NO_ROW, 0, N.CPH_NUM_FLOAT64, HOST)
    ctx.lib.cph_numcol_release(res)
    del k0


@pytest.mark.gpu
def test_programs_without_numeric_terms_launch_the_kernels_they_always_launched(ctx):
    """A numeric program is one k_pred_eval launch too (int terms convert inside it; a float term adds its column's
    conversion in front)."""
    from csvplus_amd.materialize import filter_rows
    rows = people_rows(300)
    cols = cols_from_rows(rows, True)

    def launched(pred):
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            filter_rows(ctx, cols, pred)
            return {k: v["launches"] for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
        finally:
            ctx.profile(False)

    for pred, converts in ((Like(surname="Smith"), 0), (IntCmp("born", ">", 1970), 0), (FloatCmp("born", ">", 1970.5), 1),
                           (All(FloatCmp("born", ">", 1970.5), FloatCmp("born", "<", 1990.0), IntCmp("id", "!=", 5)), 1)):
        st = launched(pred)
        assert st["k_pred_eval"] == 1 and st["k_pred_emit"] == 1, (pred, st)
        assert st.get("k_num_parse_f64", 0) == converts and "k_num_parse_i64" not in st, (pred, st)   # once per float column
