"""Numeric expressions over the columns of a row, as plain data: the reference's `price * float64(qty)`.

The reference's numeric flows — TestSimpleTotals (csvplus_test.go:516-571) and the amounts table (:1391-1421) — convert two
columns of a joined row with ValueAsInt / ValueAsFloat64 and multiply them in a Go closure.  A closure cannot run on a GPU; an
expression tree is declarative and can:

    IntCol("qty")            strconv.Atoi of the row's value of that column            -> int64
    FloatCol("price")        strconv.ParseFloat(value, 64)                             -> float64
    IntArr(values)           values[i] for OUTPUT row i (host; IntArr.on_device(device_ptr, count) on the device) -> int64
    FloatArr(values)         likewise                                                  -> float64
    a Python int / float     a literal of that type (an int is never a float: Go has no implicit conversions, nor has this)
    ToFloat(x)  ToInt(x)     float64(x) of an int64 (nearest, ties to even); int64(x) of a float64 (toward zero)
    Neg(x)  or  -x
    x + y   x - y   x * y   x / y   x % y      both sides of one type; `/` on ints is Go's `/` (toward zero), not Python's; `%`
                                               takes ints only and has the dividend's sign

Arithmetic is Go's on amd64 (include/csvplus_hip.h, cph_num_eval): int64 wraps in two's complement, INT64_MIN / -1 ==
INT64_MIN and INT64_MIN % -1 == 0; a zero int divisor is DATA (NUM_ERR_DIV_ZERO, value 0), not a panic; every float op is one
correctly rounded IEEE operation and a * b + c is never fused; float division by zero gives +-Inf / NaN and is no error;
ToInt of a NaN or of a value outside [-2^63, 2^63) is NUM_ERR_CONVERT (Go leaves it implementation-defined; this does not
guess).  Within one row the first failing op in program order decides the row's status; an error row holds value 0.

`compile` turns a tree into the postfix program cph_num_eval takes, `check_ops` states the ABI's typing rules and limits
over a raw program, `evaluate` runs the tree on one row held as a dict — the host model, for callers without a GPU and as
the cross-check of the device.  Nothing here touches the GPU.  Comparing two expressions is a predicate (predicates.ExprCmp,
over compile_pair); boolean-valued ops, math functions, rounding helpers and string operands are out of scope.
"""
from __future__ import annotations

import math

import numpy as np

from .predicates import INT64_MAX, INT64_MIN, NUM_OK, _bytes, atoi, conversion_error, parse_float

COL_INT, COL_FLT, NUM_INT, NUM_FLT, LIT_INT, LIT_FLT = 1, 2, 3, 4, 5, 6                 # CPH_EXPR_*
TO_FLT, TO_INT, NEG, ADD, SUB, MUL, DIV, MOD = 8, 9, 10, 11, 12, 13, 14, 15
MAX_OPS, MAX_STACK, MAX_NUMS = 32, 8, 8                                                   # CPH_EXPR_MAX_*
MAX_COLUMNS = 16                                                                          # CPH_MAX_KEY_COLS
NUM_ERR_DIV_ZERO, NUM_ERR_CONVERT = 4, 5                                                  # CPH_NUM_ERR_*, beside predicates' 0..3
INT, FLOAT = 1, 2                                                                         # CPH_NUM_INT64 / CPH_NUM_FLOAT64
_MASK = (1 << 64) - 1
_OP_NAMES = {ADD: "+", SUB: "-", MUL: "*", DIV: "/", MOD: "%"}


def _node(v) -> "Expr":
    if isinstance(v, Expr):
        return v
    if isinstance(v, bool):
        raise TypeError("a bool is no number here")
    if isinstance(v, (int, np.integer)):
        return Lit(int(v))
    if isinstance(v, (float, np.floating)):
        return Lit(float(v))
    raise TypeError(f"not an expression: {v!r} (closures cannot run on the device; use IntCol, FloatCol, IntArr, FloatArr, numbers)")


class Expr:
    """A node of an expression tree.  The operators build Binary / Neg nodes; types are checked by `compile`."""

    def __add__(self, o): return Binary(ADD, self, o)
    def __radd__(self, o): return Binary(ADD, o, self)
    def __sub__(self, o): return Binary(SUB, self, o)
    def __rsub__(self, o): return Binary(SUB, o, self)
    def __mul__(self, o): return Binary(MUL, self, o)
    def __rmul__(self, o): return Binary(MUL, o, self)
    def __truediv__(self, o): return Binary(DIV, self, o)
    def __rtruediv__(self, o): return Binary(DIV, o, self)
    def __mod__(self, o): return Binary(MOD, self, o)
    def __rmod__(self, o): return Binary(MOD, o, self)
    def __neg__(self): return Neg(self)


class IntCol(Expr):
    """Row.ValueAsInt(name) (csvplus.go:165-183)."""

    def __init__(self, name):
        self.name = str(name)

    def __repr__(self):
        return f"IntCol({self.name!r})"


class FloatCol(Expr):
    """Row.ValueAsFloat64(name) (csvplus.go:187-205)."""

    def __init__(self, name):
        self.name = str(name)

    def __repr__(self):
        return f"FloatCol({self.name!r})"


class _Arr(Expr):
    dtype = np.int64

    def __init__(self, values):
        arr = np.asarray(values)
        if self.dtype is np.int64:
            if arr.dtype.kind not in "iu" and arr.size:
                raise ValueError("IntArr: the array does not hold integers")
            if arr.dtype.kind == "u" and arr.size and int(arr.max()) > INT64_MAX:
                raise ValueError("IntArr: a value is not an int64")
        elif arr.dtype.kind not in "fiu" and arr.size:
            raise ValueError("FloatArr: the array does not hold numbers")
        self.device, self.values = False, np.ascontiguousarray(arr.astype(self.dtype, copy=False).reshape(-1))
        self.count = len(self.values)

    @classmethod
    def on_device(cls, device_ptr: int, count: int):
        self = cls.__new__(cls)
        self.device, self.values, self.count = True, int(device_ptr), int(count)
        return self

    def __repr__(self):
        return f"{type(self).__name__}(<{self.count} values{' on the device' if self.device else ''}>)"


class IntArr(_Arr):
    """One int64 per OUTPUT row: anything numpy turns into an int64 array (host), or IntArr.on_device(device_ptr, count)."""
    dtype = np.int64


class FloatArr(_Arr):
    """One float64 per OUTPUT row (an integer array is converted): host, or FloatArr.on_device(device_ptr, count)."""
    dtype = np.float64


class Lit(Expr):
    """A literal: a Python int is an int64 (checked), a Python float a float64."""

    def __init__(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, float)):
            raise TypeError(f"not a numeric literal: {value!r}")
        if isinstance(value, int) and not INT64_MIN <= value <= INT64_MAX:
            raise ValueError(f"the literal {value} is not an int64")
        self.value = value

    def __repr__(self):
        return repr(self.value)


class ToFloat(Expr):
    """float64(x) of an int64."""

    def __init__(self, x):
        self.x = _node(x)

    def __repr__(self):
        return f"ToFloat({self.x!r})"


class ToInt(Expr):
    """int64(x) of a float64."""

    def __init__(self, x):
        self.x = _node(x)

    def __repr__(self):
        return f"ToInt({self.x!r})"


class Neg(Expr):
    def __init__(self, x):
        self.x = _node(x)

    def __repr__(self):
        return f"-({self.x!r})"


class Binary(Expr):
    def __init__(self, op, a, b):
        self.op, self.a, self.b = op, _node(a), _node(b)

    def __repr__(self):
        return f"({self.a!r} {_OP_NAMES[self.op]} {self.b!r})"


def columns(expr) -> list:
    """The names of the expression's IntCol / FloatCol leaves, in order of first use."""
    names: list[str] = []

    def walk(e):
        if isinstance(e, (IntCol, FloatCol)):
            if e.name not in names:
                names.append(e.name)
        elif isinstance(e, (ToFloat, ToInt, Neg)):
            walk(e.x)
        elif isinstance(e, Binary):
            walk(e.a)
            walk(e.b)

    walk(_node(expr))
    return names


def check_ops(ops, ncols: int, nnums: int, want: int = 1) -> tuple:
    """The ABI's rules over a raw program of (op, arg, ...) tuples: (result type, deepest stack, [type each op pushes]).
    Raises TypeError for what cph_num_eval refuses with CPH_ERR_INVALID: an unknown op, an arg outside its table, mixed or
    wrong operand types, a missing operand, more than MAX_OPS ops, a stack deeper than MAX_STACK, more than MAX_NUMS arrays
    or MAX_COLUMNS columns, a program that does not leave exactly one value.  want=2: the program of an expression term of
    cph_filter_rows (predicates.ExprCmp), which leaves exactly two values of one type, lhs below rhs."""
    if not want <= len(ops) <= MAX_OPS:
        raise TypeError(f"a program has {want}..{MAX_OPS} ops, not {len(ops)}")
    if nnums > MAX_NUMS:
        raise TypeError(f"{nnums} number arrays, more than {MAX_NUMS}")
    if ncols > MAX_COLUMNS:
        raise TypeError(f"{ncols} columns, more than {MAX_COLUMNS}")
    stack, pushed, depth = [], [], 0
    for q, o in enumerate(ops):
        op, arg = int(o[0]), int(o[1])
        if op in (COL_INT, COL_FLT):
            if not 0 <= arg < ncols:
                raise TypeError(f"op {q}: column {arg} outside 0..{ncols - 1}")
            t = INT if op == COL_INT else FLOAT
        elif op in (NUM_INT, NUM_FLT):
            if not 0 <= arg < nnums:
                raise TypeError(f"op {q}: number array {arg} outside 0..{nnums - 1}")
            t = INT if op == NUM_INT else FLOAT
        elif op in (LIT_INT, LIT_FLT):
            t = INT if op == LIT_INT else FLOAT
        elif op in (TO_FLT, TO_INT, NEG):
            if not stack:
                raise TypeError(f"op {q}: no operand on the stack")
            x = stack.pop()
            if op == TO_FLT and x != INT:
                raise TypeError(f"op {q}: ToFloat takes an int64 (Go has no implicit conversions)")
            if op == TO_INT and x != FLOAT:
                raise TypeError(f"op {q}: ToInt takes a float64")
            t = FLOAT if op == TO_FLT else INT if op == TO_INT else x
        elif op in (ADD, SUB, MUL, DIV, MOD):
            if len(stack) < 2:
                raise TypeError(f"op {q}: a binary op needs two operands")
            b, a = stack.pop(), stack.pop()
            if a != b:
                raise TypeError(f"op {q}: int64 {_OP_NAMES[op]} float64 mixes types (Go has no implicit conversions: use ToFloat / ToInt)")
            if op == MOD and a != INT:
                raise TypeError(f"op {q}: % takes int64 operands")
            t = a
        else:
            raise TypeError(f"op {q}: unknown op {op}")
        if len(stack) >= MAX_STACK:
            raise TypeError(f"op {q}: a stack deeper than {MAX_STACK}")
        stack.append(t)
        pushed.append(t)
        depth = max(depth, len(stack))
    if len(stack) != want:
        raise TypeError(f"the program leaves {len(stack)} values, not exactly {'one' if want == 1 else 'two'}")
    if want == 2 and stack[0] != stack[1]:
        raise TypeError("int64 REL float64 mixes types (Go has no implicit conversions: use ToFloat / ToInt)")
    return stack[0], depth, pushed


def compile(expr, column_names, also=None):   # noqa: A001 (the name predicates.compile and mapping.compile use)
    """(names of the columns used, ops).  also: a second expression whose ops follow in the same program, which then leaves
    two values of one type (compile_pair).  An op is (opcode, arg, value): COL_* — arg indexes the returned name list; NUM_* —
    arg indexes `arrays(ops)` and value is the IntArr / FloatArr; LIT_* — value is the int / float; others — (op, 0, None).
    A column the rows lack raises mapping.MissingColumn; what the ABI would refuse raises TypeError (see check_ops)."""
    known = [str(c) for c in column_names]
    used: list[str] = []
    arrs: list = []
    ops: list[tuple] = []

    def walk(e):
        if isinstance(e, (IntCol, FloatCol)):
            if e.name not in known:
                from .mapping import MissingColumn
                raise MissingColumn(e.name)
            if e.name not in used:
                used.append(e.name)
            ops.append((COL_INT if isinstance(e, IntCol) else COL_FLT, used.index(e.name), None))
        elif isinstance(e, _Arr):
            k = next((j for j, a in enumerate(arrs) if a is e), len(arrs))
            if k == len(arrs):
                arrs.append(e)
            ops.append((NUM_INT if isinstance(e, IntArr) else NUM_FLT, k, e))
        elif isinstance(e, Lit):
            ops.append((LIT_INT, 0, e.value) if isinstance(e.value, int) else (LIT_FLT, 0, e.value))
        elif isinstance(e, (ToFloat, ToInt, Neg)):
            walk(e.x)
            ops.append((TO_FLT if isinstance(e, ToFloat) else TO_INT if isinstance(e, ToInt) else NEG, 0, None))
        elif isinstance(e, Binary):
            walk(e.a)
            walk(e.b)
            ops.append((e.op, 0, None))
        else:
            raise TypeError(f"not an expression: {e!r}")
        if len(ops) > MAX_OPS:
            raise TypeError(f"the expression compiles to more than {MAX_OPS} ops")

    walk(_node(expr))
    if also is not None:
        walk(_node(also))
    check_ops(ops, len(used), len(arrs), want=1 if also is None else 2)
    return used, ops


def compile_pair(lhs, rhs, column_names):
    """(names of the columns used, ops) of two expressions as ONE program that leaves lhs below rhs, both of one type: what an
    expression term of cph_filter_rows takes (predicates.ExprCmp).  Each side is checked on its own first, so a typing error
    names the side's own op."""
    compile(lhs, column_names)
    compile(rhs, column_names)
    return compile(lhs, column_names, also=rhs)


def arrays(ops) -> list:
    """The IntArr / FloatArr nodes of a compiled program, indexed by the NUM_* ops' arg."""
    out: dict = {}
    for op, arg, value in ops:
        if op in (NUM_INT, NUM_FLT):
            out[arg] = value
    return [out[k] for k in range(len(out))]


def kind_of(expr) -> int:
    """INT or FLOAT: the expression's result type (column names are not looked up)."""
    names = columns(expr)
    _, ops = compile(expr, names)
    return check_ops(ops, len(names), len(arrays(ops)))[0]


# ---- the host model ---------------------------------------------------------------------------------------------------
def _wrap(v: int) -> int:
    v &= _MASK
    return v - (1 << 64) if v >> 63 else v


def _int_binary(op, a, b):
    if op == ADD:
        return _wrap(a + b), NUM_OK
    if op == SUB:
        return _wrap(a - b), NUM_OK
    if op == MUL:
        return _wrap(a * b), NUM_OK
    if b == 0:
        return 0, NUM_ERR_DIV_ZERO
    q = abs(a) // abs(b)   # toward zero
    if (a < 0) != (b < 0):
        q = -q
    return (_wrap(q), NUM_OK) if op == DIV else (_wrap(a - b * q), NUM_OK)   # the remainder has the dividend's sign


def _float_binary(op, a, b):
    if op == DIV:   # IEEE: x / 0 is +-Inf, 0 / 0 is NaN; Python raises instead
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))
    return a + b if op == ADD else a - b if op == SUB else a * b   # Python floats: IEEE doubles, one rounding each, never fused


def run_ops(ops, leaf, want: int = 1) -> tuple:
    """(value, status, op) of a compiled program on one row: leaf(q, op) -> (value, status) of leaf op q.  status is NUM_* /
    NUM_ERR_DIV_ZERO / NUM_ERR_CONVERT, `op` the index of the first failing op (-1 without an error); an error gives value 0.
    want=2 (a two-value program, check_ops): `value` is the pair (lhs, rhs)."""
    stack: list = []
    status, bad = NUM_OK, -1
    for q, o in enumerate(ops):
        op = o[0]
        st = NUM_OK
        if op in (COL_INT, COL_FLT, NUM_INT, NUM_FLT):
            v, st = leaf(q, o)
        elif op in (LIT_INT, LIT_FLT):
            v = o[2]
        elif op == TO_FLT:
            v = float(stack.pop())   # correctly rounded: nearest, ties to even
        elif op == TO_INT:
            x = stack.pop()
            if math.isnan(x) or not -(2.0 ** 63) <= x < 2.0 ** 63:
                v, st = 0, NUM_ERR_CONVERT
            else:
                v = int(x)   # toward zero
        elif op == NEG:
            x = stack.pop()
            v = _wrap(-x) if isinstance(x, int) else -x
        else:
            b, a = stack.pop(), stack.pop()
            v, st = _int_binary(op, a, b) if isinstance(a, int) else (_float_binary(op, a, b), NUM_OK)
        if st != NUM_OK and status == NUM_OK:
            status, bad = st, q
        stack.append(v)
    if want == 2:
        return (stack[0], stack[1]), status, bad
    if status != NUM_OK:
        return (0 if isinstance(stack[0], int) else 0.0), status, bad
    return stack[0], NUM_OK, -1


def _row_value(row, name):
    v = row.get(name)
    if v is None:
        v = row.get(name.encode("utf-8"))
    if v is None:
        from .mapping import MissingColumn
        raise MissingColumn(name)
    return _bytes(v)


def evaluate(expr, row, i: int = 0) -> tuple:
    """The expression on one row (a dict with str or bytes keys and values): (value, status, op), see run_ops.  `i` = the
    row's number, which is what an IntArr / FloatArr leaf is indexed with (host arrays only).  Column leaves go through
    predicates.atoi / parse_float."""
    names = columns(expr)
    _, ops = compile(expr, names)

    def leaf(q, o):
        op, arg, value = o
        if op == COL_INT:
            return atoi(_row_value(row, names[arg]))
        if op == COL_FLT:
            return parse_float(_row_value(row, names[arg]))
        if value.device:
            raise ValueError("evaluate: an array on the device has no host values")
        return (int(value.values[i]) if op == NUM_INT else float(value.values[i])), NUM_OK

    return run_ops(ops, leaf)


def error_text(expr, row, status: int, op: int) -> str:
    """The message for a row whose op `op` failed with `status`: the reference's conversion error for a column leaf
    (predicates.conversion_error: csvplus.go:176, :198), a plain statement for a zero divisor or a ToInt out of range."""
    names = columns(expr)
    _, ops = compile(expr, names)
    code = ops[op][0]
    if code in (COL_INT, COL_FLT):
        name = names[ops[op][1]]
        return conversion_error(name, _row_value(row, name), status, as_float=code == COL_FLT)
    if status == NUM_ERR_DIV_ZERO:
        return "integer divide by zero"
    if status == NUM_ERR_CONVERT:
        return "float64 value does not fit an int64"
    return f"op {op} failed with status {status}"


class ExprError(ValueError):
    """A row of an expression failed (what a Go closure returning row.ValueAsInt's error hands back, or Go's panic on a zero
    divisor): `row` = the lowest failing row, `op` = the index of the op that failed there, `kind` = its status, `column` =
    the leaf's column name (None for an arithmetic error), `nerrors` = the failing rows."""

    def __init__(self, row: int, op: int, kind: int, column, text: str, nerrors: int):
        super().__init__(f"row {row}: {text} ({nerrors} such rows)")
        self.row, self.op, self.kind, self.column, self.nerrors = row, op, kind, column, nerrors
