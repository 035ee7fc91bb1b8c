"""Conditions that compare two expressions or two columns, on the host: predicates.ExprCmp / ColCmp, their compiler
(cph_filter_rows ops 56..61 and 72..77) and their host model against hand-written truth tables.  CPU only."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.expr import FloatArr, FloatCol, IntArr, IntCol, ToFloat, ToInt
from csvplus_amd.predicates import All, Any, ColCmp, ExprCmp, Like, Not

RELS = P.RELS   # < <= == != >= >
I64MAX, I64MIN = (1 << 63) - 1, -(1 << 63)


def truth(lt, eq, gt):
    """The six relations' outcomes for a pair that compares as less / equal / greater (all False: unordered or failing,
    where only `ne` says whether "!=" holds)."""
    return {"<": lt, "<=": lt or eq, "==": eq, "!=": lt or gt, ">=": gt or eq, ">": gt}


LESS, EQUAL, GREATER = truth(True, False, False), truth(False, True, False), truth(False, False, True)
NEVER = dict.fromkeys(RELS, False)                       # a failing op, a missing column
ONLY_NE = dict(NEVER, **{"!=": True})                    # a NaN on either side

# (lhs, rhs, row, the expected outcome per relation) — int64
INT_TABLE = [
    (IntCol("a") + 1, IntCol("b"), {"a": str(I64MAX), "b": str(I64MIN)}, EQUAL),                 # lhs wraps to INT64_MIN
    (IntCol("a"), IntCol("b") - 1, {"a": str(I64MAX), "b": str(I64MIN)}, EQUAL),                 # rhs wraps to INT64_MAX
    (IntCol("a") * 2, 0, {"a": str(1 << 62), "b": "0"}, LESS),                                   # 2^63 wraps negative
    (IntCol("a") / 2, -3, {"a": "-7"}, EQUAL),                                                   # toward zero
    (IntCol("a") / 2, -4, {"a": "-7"}, GREATER),
    (IntCol("a") % -2, 1, {"a": "7"}, EQUAL),                                                    # the dividend's sign
    (IntCol("a") % -2, 2, {"a": "7"}, LESS),
    (IntCol("a") / IntCol("b"), 0, {"a": "7", "b": "0"}, NEVER),                                 # zero divisor: false under != too
    (1, IntCol("a") % IntCol("b"), {"a": "7", "b": "0"}, NEVER),
    (IntCol("a"), IntCol("b"), {"a": "12", "b": "x"}, NEVER),                                    # a leaf that does not convert
    (IntCol("a"), IntCol("b"), {"a": "-1", "b": "1"}, LESS),                                     # signed
    (IntCol("a"), IntCol("b"), {"a": "1970", "b": "1969"}, GREATER),
    (ToInt(FloatCol("x")), 0, {"x": "1e19"}, NEVER),                                             # ToInt out of range
    (ToInt(FloatCol("x")), 0, {"x": "NaN"}, NEVER),
    (ToInt(FloatCol("x")), -2, {"x": "-2.9"}, EQUAL),
    (IntCol("a"), 5, {"b": "5"}, NEVER),                                                         # the row lacks the column
]
# float64
FLT_TABLE = [
    (FloatCol("p") * ToFloat(IntCol("q")), 100.0, {"p": "12.5", "q": "8"}, EQUAL),
    (FloatCol("p") * ToFloat(IntCol("q")), 100.0, {"p": "12.5", "q": "7"}, LESS),
    (FloatCol("p") * ToFloat(IntCol("q")), 100.0, {"p": "12.5", "q": "9"}, GREATER),
    (FloatCol("p"), FloatCol("q"), {"p": "NaN", "q": "1"}, ONLY_NE),
    (FloatCol("p"), FloatCol("q"), {"p": "1", "q": "nan"}, ONLY_NE),
    (FloatCol("p") / FloatCol("q"), 0.0, {"p": "0", "q": "0"}, ONLY_NE),                         # 0 / 0 is a NaN, no error
    (FloatCol("p"), FloatCol("q"), {"p": "-0.0", "q": "0.0"}, EQUAL),
    (FloatCol("p") / FloatCol("q"), 1e308, {"p": "1", "q": "0"}, GREATER),                       # +Inf, no error
    (FloatCol("p"), 1.0, {"p": "1e400"}, NEVER),                                                 # out of range: an error
    (FloatCol("p"), 1.0, {"p": ""}, NEVER),
    (FloatCol("p") * 3.0 + FloatCol("q"), 0.30000000000000004, {"p": "0.1", "q": "0"}, EQUAL),   # one rounding per op
]
# (a, b, the expected outcome per relation) — strings
STR_TABLE = [
    (b"10", b"9", LESS), (b"a", b"a\x00", LESS), (b"\x7f", b"\x80", LESS), (b"", b"", EQUAL), (b"", b"\x00", LESS),
    (b"a", b"", GREATER), (b"abc", b"abc", EQUAL), (b"abd", b"abc", GREATER), (b"\xff", b"\x00\xff", GREATER),
    (b"12345678", b"12345678", EQUAL), (b"123456789", b"12345678", GREATER), (b"1234567", b"12345678", LESS),
]


@pytest.mark.parametrize("table", [INT_TABLE, FLT_TABLE], ids=["int64", "float64"])
def test_exprcmp_truth_tables(table):
    for lhs, rhs, row, want in table:
        for rel in RELS:
            assert P.matches(ExprCmp(lhs, rel, rhs), row) is want[rel], (lhs, rel, rhs, row)
            assert ExprCmp(lhs, rel, rhs)(row) is want[rel]
            # the compiled program on the row's values gives the same
            names, ops = P.compile(ExprCmp(lhs, rel, rhs), list(row))
            if all(nm in row for nm in ExprCmp(lhs, rel, rhs).names):
                assert P.run_ops(ops, [row[nm] for nm in names]) is want[rel], (lhs, rel, rhs, row)
            else:
                assert ops == [(P.EXPR_LT + RELS.index(rel), -1, None)] and P.run_ops(ops, []) is False


def test_colcmp_truth_table():
    for a, b, want in STR_TABLE:
        for rel in RELS:
            assert P.matches(ColCmp("a", rel, "b"), {"a": a, "b": b}) is want[rel], (a, rel, b)
            names, ops = P.compile(ColCmp("a", rel, "b"), ["b", "a"])
            assert names == ["a", "b"] and ops == [(P.COLS_LT + RELS.index(rel), 0, 1)]
            assert P.run_ops(ops, [a, b]) is want[rel]
    for rel in RELS:   # either column missing: false, "!=" included
        assert P.matches(ColCmp("a", rel, "b"), {"a": b"x"}) is False and P.matches(ColCmp("a", rel, "b"), {"b": b"x"}) is False
        assert P.compile(ColCmp("a", rel, "b"), ["a"]) == (["a"], [(P.COLS_LT + RELS.index(rel), 0, -1)])
        assert P.compile(ColCmp("a", rel, "b"), ["b"]) == (["b"], [(P.COLS_LT + RELS.index(rel), -1, 0)])
        assert P.run_ops([(P.COLS_LT + RELS.index(rel), 0, -1)], [b"x"]) is False
    assert P.matches(ColCmp("a", "==", "a"), {"a": "same"}) and P.matches(ColCmp("a", "<", "b"), {"a": "10", "b": "9"})   # str values


def test_tables_show_both_outcomes_for_every_relation():
    """A condition on the INPUTS: every table has rows where each relation holds and rows where it fails."""
    for name, outcomes in (("int64", [w for *_, w in INT_TABLE]), ("float64", [w for *_, w in FLT_TABLE]), ("strings", [w for *_, w in STR_TABLE])):
        for rel in RELS:
            seen = {w[rel] for w in outcomes}
            assert seen == {True, False}, (name, rel)


def test_array_leaves_are_indexed_by_position():
    p = ExprCmp(FloatArr([1.0, 2.0, 3.0]), "<", FloatCol("x") + ToFloat(IntArr([0, 10, 0])))
    assert [P.matches(p, {"x": "2.5"}, i) for i in range(3)] == [True, True, False]
    names, ops = P.compile(p, ["x"])
    eops, arrs = ops[0][2]
    assert [a.count for a in arrs] == [3, 3] and [o[0] for o in eops] == [E.NUM_FLT, E.COL_FLT, E.NUM_INT, E.TO_FLT, E.ADD]
    assert [P.run_ops(ops, ["2.5"], i) for i in range(3)] == [True, True, False]
    assert P.matches(All(Not(p), Like(x="2.5")), {"x": "2.5"}, 2)


def test_compile_shapes_and_column_remapping():
    amount = FloatCol("price") * ToFloat(IntCol("qty"))
    pred = All(Like(name="x"), ExprCmp(amount, ">=", 100.0), ColCmp("ship", "!=", "name"), Not(ExprCmp(IntCol("qty"), ">", IntCol("gone"))))
    names, ops = P.compile(pred, ["qty", "ship", "price", "name", "unused"])
    assert names == ["name", "price", "qty", "ship"]   # ONE list, in order of first use; the expression's leaves index it
    assert ops[0] == (P.LIKE, 0, b"x")
    op, arg, (eops, arrs) = ops[1]
    assert (op, arg, arrs) == (P.EXPR_LT + 4, 0, [])
    assert eops == [(E.COL_FLT, 1, None), (E.COL_INT, 2, None), (E.TO_FLT, 0, None), (E.MUL, 0, None), (E.LIT_FLT, 0, 100.0)]
    assert ops[2] == (P.COLS_LT + 3, 3, 0)
    assert ops[3:] == [(P.EXPR_LT + 5, -1, None), (P.NOT, 0, None), (P.ALL, 4, None)]
    assert E.check_ops(eops, len(names), 0, want=2)[:2] == (E.FLOAT, 2)
    # a Python int is an int64 literal, a float a float64 literal
    assert P.compile(ExprCmp(IntCol("a"), "<", 3), ["a"])[1][0][2][0][-1] == (E.LIT_INT, 0, 3)
    assert P.compile(ExprCmp(2.0, "<", FloatCol("a")), ["a"])[1][0][2][0][0] == (E.LIT_FLT, 0, 2.0)
    # a Switch shares one column list among its cases and templates
    sw = M.Switch((ExprCmp(amount, ">=", 1000.0), "gold"), (ColCmp("name", "<", "ship"), M.Col("qty")), otherwise=M.Col("name"))
    shared, cases, _ = M.compile_switch(sw, ["name", "qty", "price", "ship"])
    assert shared == ["price", "qty", "name", "ship"] and M.columns(sw) == shared
    assert [o[:2] for o in cases[0][0][0][2][0][:2]] == [(E.COL_FLT, 0), (E.COL_INT, 1)]
    assert cases[1][0] == [(P.COLS_LT + 0, 2, 3)] and cases[1][1] == [(M.COLUMN, 1, None)]
    assert M.render(sw, {"price": "10", "qty": "100", "name": "b", "ship": "a"}) == b"gold"
    assert M.render(sw, {"price": "10", "qty": "99", "name": "a", "ship": "b"}) == b"99"
    assert M.render(sw, {"price": "x", "qty": "99", "name": "b", "ship": "a"}) == b"b"


def test_typing_errors_and_limits():
    with pytest.raises(TypeError, match="no implicit conversions"):
        ExprCmp(IntCol("a"), "<", 1.0)
    with pytest.raises(TypeError, match="no implicit conversions"):
        ExprCmp(FloatCol("a"), "==", IntCol("b"))
    with pytest.raises(TypeError, match="no implicit conversions"):
        ExprCmp(IntCol("a") + 1.5, "<", 1)          # inside one side
    with pytest.raises(TypeError):
        ExprCmp(FloatCol("a") % 2.0, "<", 1.0)      # % takes ints
    with pytest.raises(ValueError):
        ExprCmp(IntCol("a"), "=", 1)
    with pytest.raises(ValueError):
        ColCmp("a", "<>", "b")
    with pytest.raises(TypeError):
        ExprCmp(lambda r: 1, "<", 1)
    with pytest.raises(TypeError):
        All(ExprCmp(IntCol("a"), "<", 1), lambda r: True)
    # two-value mode of check_ops: exactly two values of one type
    one = [(E.LIT_INT, 0, 1)]
    with pytest.raises(TypeError, match="not exactly two"):
        E.check_ops(one + one + [(E.ADD, 0, None), (E.LIT_INT, 0, 1), (E.LIT_INT, 0, 1)], 0, 0, want=2)
    with pytest.raises(TypeError):
        E.check_ops(one, 0, 0, want=2)
    with pytest.raises(TypeError, match="no implicit conversions"):
        E.check_ops(one + [(E.LIT_FLT, 0, 1.0)], 0, 0, want=2)
    assert E.check_ops(one + one, 0, 0, want=2) == (E.INT, 2, [E.INT, E.INT])
    assert E.check_ops(one, 0, 0) == (E.INT, 1, [E.INT])    # the one-value mode is what it was
    with pytest.raises(TypeError, match="not exactly one"):
        E.check_ops(one + one, 0, 0)
    # 32 expression ops for both sides together, a stack of 8
    chain = IntCol("a")
    for _ in range(14):
        chain = chain + 1                                   # 29 ops
    ExprCmp(chain, "<", IntCol("a") + 1)                    # 32
    with pytest.raises(TypeError):
        ExprCmp(chain, "<", IntCol("a") + 1 + 1)            # 34
    deep = IntCol("a")
    for _ in range(6):
        deep = IntCol("a") + deep                           # a right-leaning tree: stack 7
    ExprCmp(1, "<", deep)                                   # 8 with the lhs below it
    with pytest.raises(TypeError):
        ExprCmp(1, "<", IntCol("a") + deep)                 # 9
    # 32 terms and 64 ops of the predicate program
    t = ExprCmp(IntCol("a"), "<", 1)
    P.compile(All(*[t] * 32), ["a"])
    with pytest.raises(ValueError):
        P.compile(All(*[t] * 33), ["a"])
    c = ColCmp("a", "<", "b")
    P.compile(All(*[Not(c)] * 31, c), ["a", "b"])           # 31 * 2 + 1 + 1 = 64 ops
    with pytest.raises(ValueError):
        P.compile(All(*[Not(c)] * 32), ["a", "b"])          # 65


def test_constants_equal_the_header():
    header = (Path(__file__).resolve().parent.parent / "include" / "csvplus_hip.h").read_text()
    enums = {k: int(v) for k, v in re.findall(r"(CPH_PRED_(?:EXPR|COLS)_[A-Z]{2}) = (\d+)", header)}
    for fam, base in (("EXPR", P.EXPR_LT), ("COLS", P.COLS_LT)):
        for k, rel in enumerate(("LT", "LE", "EQ", "NE", "GE", "GT")):
            assert enums[f"CPH_PRED_{fam}_{rel}"] == base + k == getattr(N, f"CPH_PRED_{fam}_{rel}")
    assert (P.EXPR_LT, P.COLS_LT) == (56, 72)
    assert re.search(r"#define CPH_PRED_MAX_LIKE\s+32", header) and P.MAX_LIKE == 32


def test_pred_expr_struct_against_the_compiled_header(tmp_path):
    import ctypes as C
    import subprocess
    root = Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(cph_pred_expr), offsetof(cph_pred_expr, prog), offsetof(cph_pred_expr, nops),'
                   ' offsetof(cph_pred_expr, nnums), offsetof(cph_pred_expr, nums), CPH_PRED_EXPR_GT, CPH_PRED_COLS_GT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(root / "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    T = N.cph_pred_expr
    assert out == [C.sizeof(T), T.prog.offset, T.nops.offset, T.nnums.offset, T.nums.offset, 61, 77]


def test_float_model_of_the_truth_tables_is_ieee():
    assert math.isnan(E.evaluate(FloatCol("p") / FloatCol("q"), {"p": "0", "q": "0"})[0])
    assert E.evaluate(FloatCol("p") * 3.0, {"p": "0.1"})[0] == 0.30000000000000004
    assert np.float64(-0.0) == np.float64(0.0)
