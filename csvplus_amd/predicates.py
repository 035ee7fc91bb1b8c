"""The reference's named predicates as plain data (csvplus.go:1243-1293): Like, All, Any, Not — and the numeric
conditions its users write as closures over Row.ValueAsInt / ValueAsFloat64 (csvplus.go:165-205, csvplus_test.go:272-281):
IntCmp, FloatCmp — and the conditions that look inside a string (`row["ts"] >= "2016-09"`, strings.HasPrefix / HasSuffix /
Contains): StrCmp, HasPrefix, HasSuffix, Contains.  Those are byte operations in Go; Python's bytes comparison, startswith,
endswith and `in` are their exact host model.  TimeCmp compares a column of RFC 3339 timestamps as INSTANTS
(`t, err := time.Parse(time.RFC3339, row["ts"]); return err == nil && t.Unix() REL u.Unix()`): two stamps of one instant in
different zones are equal, which their bytes are not; csvplus_amd.timeconv is its host model.  ExprCmp compares two numeric
expressions of csvplus_amd.expr (`price(r) * float64(qty(r)) >= 100`, `died(r) > born(r)`) and ColCmp two columns of one row as
strings (`r["ship_city"] != r["bill_city"]`); expr.run_ops and Python's bytes comparison are their host models.

A Go closure cannot run on a GPU; these are declarative and can.  `compile` flattens any nesting of them into the
postfix program cph_filter_rows takes (include/csvplus_hip.h), `matches` evaluates a predicate on one row held as a dict —
the reference's semantics restated on the host, for callers and as the cross-check of the compiler.  `atoi` and
`parse_float` restate strconv.Atoi / strconv.ParseFloat as the header's cph_col_to_number comment does.  Nothing here
touches the GPU.
"""
from __future__ import annotations

import math
import re
import struct

LIKE, NOT, ALL, ANY = 1, 2, 3, 4   # CPH_PRED_*
INT_LT, FLT_LT = 16, 24            # CPH_PRED_INT_LT / CPH_PRED_FLT_LT; + the relation's index in RELS
STR_LT = 32                        # CPH_PRED_STR_LT; + the relation's index in RELS
HAS_PREFIX, HAS_SUFFIX, CONTAINS = 40, 41, 42   # CPH_PRED_*
TIME_LT = 48                       # CPH_PRED_TIME_LT; + the relation's index in RELS
EXPR_LT = 56                       # CPH_PRED_EXPR_LT; + the relation's index in RELS
COLS_LT = 72                       # CPH_PRED_COLS_LT; + the relation's index in RELS
RELS = ("<", "<=", "==", "!=", ">=", ">")
MAX_OPS, MAX_LIKE, MAX_STACK = 64, 32, 32
NUM_OK, NUM_ERR_SYNTAX, NUM_ERR_RANGE, NUM_ERR_UNSUPPORTED = 0, 1, 2, 3   # CPH_NUM_*
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def _bytes(v) -> bytes:
    return v.encode("utf-8") if isinstance(v, str) else bytes(v)


class Pred:
    """Base of the four predicates; `p(row)` evaluates on a dict (str or bytes values)."""

    def __call__(self, row) -> bool:
        return matches(self, row)


class Like(Pred):
    """Like(Row{...}) (:1277-1293): every listed column is present in the row and holds exactly the given value.
    An empty match row raises, as the reference panics (:1280-1282)."""

    def __init__(self, match=None, **more):
        items = dict(match or {})
        items.update(more)
        if not items:
            raise ValueError("Like: empty match row")
        self.items = [(str(k), _bytes(v)) for k, v in items.items()]

    def __repr__(self):
        return f"Like({dict(self.items)!r})"


class All(Pred):
    """All(p...) (:1243-1253): every operand holds; All() is true."""

    def __init__(self, *preds):
        self.preds = _operands(preds)

    def __repr__(self):
        return f"All{tuple(self.preds)!r}"


class Any(Pred):
    """Any(p...) (:1258-1268): some operand holds; Any() is false."""

    def __init__(self, *preds):
        self.preds = _operands(preds)

    def __repr__(self):
        return f"Any{tuple(self.preds)!r}"


class Not(Pred):
    """Not(p) (:1271-1275)."""

    def __init__(self, pred):
        (self.pred,) = _operands((pred,))

    def __repr__(self):
        return f"Not({self.pred!r})"


class _NumCmp(Pred):
    def __init__(self, column, rel, literal):
        if rel not in RELS:
            raise ValueError(f"unknown relation {rel!r}: one of {' '.join(RELS)}")
        self.column, self.rel, self.literal = str(column), rel, literal

    def __repr__(self):
        return f"{type(self).__name__}({self.column!r}, {self.rel!r}, {self.literal!r})"


class IntCmp(_NumCmp):
    """IntCmp("born", ">", 1970): `v, err := row.ValueAsInt(column); return err == nil && v REL k`.  A row whose value
    does not convert (or that lacks the column) is false under every relation, "!=" included."""

    def __init__(self, column, rel, k):
        k = int(k)
        if not INT64_MIN <= k <= INT64_MAX:
            raise ValueError("IntCmp: the literal is not an int64")
        super().__init__(column, rel, k)


class FloatCmp(_NumCmp):
    """FloatCmp("price", "<=", 9.99): the same over ValueAsFloat64.  Comparisons are IEEE: with a NaN on either side
    only "!=" holds."""

    def __init__(self, column, rel, x):
        super().__init__(column, rel, float(x))


class StrCmp(Pred):
    """StrCmp("ts", ">=", "2016-09"): `row[column] REL literal`, Go's string comparison: bytewise and unsigned, the shorter
    of two values that agree on the common prefix is the smaller ("10" < "9", "a" < "a\0").  A row that lacks the column
    is false under every relation, "!=" included."""

    def __init__(self, column, rel, literal):
        if rel not in RELS:
            raise ValueError(f"unknown relation {rel!r}: one of {' '.join(RELS)}")
        self.column, self.rel, self.literal = str(column), rel, _bytes(literal)

    def __repr__(self):
        return f"StrCmp({self.column!r}, {self.rel!r}, {self.literal!r})"


class TimeCmp(Pred):
    """TimeCmp("ts", ">=", "2016-09-14T00:00:00Z"): the column's RFC 3339 stamp REL the literal's, both as Unix seconds
    (t.Unix(): a fraction in the column is floored).  The literal is RFC 3339 text that must convert (timeconv.parse_model)
    and carry no fraction — the term compares whole seconds — else ValueError.  A row whose value does not convert (or that
    lacks the column) is false under every relation, "!=" included."""

    def __init__(self, column, rel, literal):
        from . import timeconv as T
        if rel not in RELS:
            raise ValueError(f"unknown relation {rel!r}: one of {' '.join(RELS)}")
        lit = _bytes(literal)
        status, secs = T.parse_model(lit, "s")
        if status != NUM_OK:
            raise ValueError(f"TimeCmp: the literal {lit!r} is no RFC 3339 timestamp this library converts (status {status})")
        if b"." in lit:
            raise ValueError(f"TimeCmp: the literal {lit!r} has a fraction: the term compares whole seconds")
        self.column, self.rel, self.literal, self.seconds = str(column), rel, lit, secs

    def __repr__(self):
        return f"TimeCmp({self.column!r}, {self.rel!r}, {self.literal!r})"


class ExprCmp(Pred):
    """ExprCmp(FloatCol("price") * ToFloat(IntCol("qty")), ">=", 100.0): `lhs REL rhs` over two expressions of csvplus_amd.expr
    (a Python int is an int64 literal, a float a float64 literal; IntArr / FloatArr leaves are indexed by the row's POSITION in
    the selection).  Both sides have ONE type — Go has no implicit conversions — else TypeError here.  int64 compares signed,
    float64 IEEE (with a NaN on either side only "!=" holds; -0.0 == 0.0).  A row in which any op fails (a leaf that does not
    convert, a zero divisor, a ToInt out of range) or that lacks a column is false under every relation, "!=" included."""

    def __init__(self, lhs, rel, rhs):
        from . import expr as E
        if rel not in RELS:
            raise ValueError(f"unknown relation {rel!r}: one of {' '.join(RELS)}")
        self.lhs, self.rel, self.rhs = E._node(lhs), rel, E._node(rhs)
        self.names = E.columns(self.lhs)
        self.names += [nm for nm in E.columns(self.rhs) if nm not in self.names]
        self.ops = self._compile(self.names)[1]   # typing (both sides, then across the relation) and the limits: TypeError

    def _compile(self, known):
        """(names used, ops) of both sides as ONE program that leaves lhs below rhs; column indices into the names used."""
        from . import expr as E
        return E.compile_pair(self.lhs, self.rhs, known)

    def __repr__(self):
        return f"ExprCmp({self.lhs!r}, {self.rel!r}, {self.rhs!r})"


class ColCmp(Pred):
    """ColCmp("ship_city", "!=", "bill_city"): `row[a] REL row[b]`, Go's string comparison (StrCmp's rules with the second
    column's value in the literal's place).  A row that lacks either column is false under every relation, "!=" included."""

    def __init__(self, a, rel, b):
        if rel not in RELS:
            raise ValueError(f"unknown relation {rel!r}: one of {' '.join(RELS)}")
        self.a, self.rel, self.b = str(a), rel, str(b)

    def __repr__(self):
        return f"ColCmp({self.a!r}, {self.rel!r}, {self.b!r})"


class _StrTest(Pred):
    op = None

    def __init__(self, column, literal):
        self.column, self.literal = str(column), _bytes(literal)

    def __repr__(self):
        return f"{type(self).__name__}({self.column!r}, {self.literal!r})"


class HasPrefix(_StrTest):
    """HasPrefix("ts", "2016-09-14"): strings.HasPrefix(row[column], literal), on bytes.  The empty literal holds for
    every present value; a row that lacks the column is false."""
    op = HAS_PREFIX


class HasSuffix(_StrTest):
    """HasSuffix("ts", "+01:00"): strings.HasSuffix(row[column], literal), on bytes."""
    op = HAS_SUFFIX


class Contains(_StrTest):
    """Contains("surname", "Smith"): strings.Contains(row[column], literal), on bytes."""
    op = CONTAINS


def _operands(preds):
    for p in preds:
        if not isinstance(p, Pred):
            raise TypeError(f"not a predicate: {p!r} (closures cannot run on the device; use Like / All / Any / Not / IntCmp / FloatCmp / StrCmp / HasPrefix / HasSuffix / Contains / TimeCmp / ExprCmp / ColCmp)")
    return list(preds)


# ---- strconv on the host -----------------------------------------------------------------------------------------------

def atoi(value) -> tuple:
    """strconv.Atoi on a 64-bit int: (value, NUM_*).  Decided left to right: a byte that is no digit is a syntax error
    (value 0) unless the unsigned accumulator has overflowed 2^64 in front of it, which is a range error at that byte
    (INT64_MAX, or INT64_MIN after '-')."""
    b = _bytes(value)
    neg = b[:1] == b"-"
    digits = b[1:] if b[:1] in (b"+", b"-") else b
    if not digits:
        return 0, NUM_ERR_SYNTAX
    n = 0
    for c in digits:
        if not 0x30 <= c <= 0x39:
            return 0, NUM_ERR_SYNTAX
        n = n * 10 + (c - 0x30)
        if n >= 1 << 64:
            return (INT64_MIN if neg else INT64_MAX), NUM_ERR_RANGE
    if neg:
        return (-n, NUM_OK) if n <= 1 << 63 else (INT64_MIN, NUM_ERR_RANGE)
    return (n, NUM_OK) if n < 1 << 63 else (INT64_MAX, NUM_ERR_RANGE)


_DECIMAL = re.compile(rb"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?", re.ASCII)
_INF = re.compile(rb"[+-]?(?:inf|infinity)", re.ASCII | re.IGNORECASE)
_DEC_PARTS = re.compile(rb"[+-]?([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]+))?", re.ASCII)


def parse_float(value) -> tuple:
    """strconv.ParseFloat(s, 64): (value, NUM_*).  The grammar is checked BEFORE float() sees the text (Python would
    accept spaces, underscores and a signed nan).  A value with '_' or a 0x / 0X prefix is NUM_ERR_UNSUPPORTED (Go may
    accept it; this library does not decide); a magnitude beyond the largest double is a range error with +-Inf."""
    b = _bytes(value)
    rest = b[1:] if b[:1] in (b"+", b"-") else b
    if not b:
        return 0.0, NUM_ERR_SYNTAX
    if b"_" in b or rest[:2].lower() == b"0x":
        return 0.0, NUM_ERR_UNSUPPORTED
    if _INF.fullmatch(b):
        return (-math.inf if b[:1] == b"-" else math.inf), NUM_OK
    if b.lower() == b"nan":
        return math.nan, NUM_OK
    if not _DECIMAL.fullmatch(b):
        return 0.0, NUM_ERR_SYNTAX
    v = float(b.decode("ascii"))   # correctly rounded; overflow gives inf, underflow 0 or a denormal
    return v, (NUM_ERR_RANGE if math.isinf(v) else NUM_OK)


def float_is_deferred(value) -> bool:
    """True when the device does not decide this (valid, decimal) value itself and the library's host side finishes it:
    a mantissa — the first 19 significant digits — that is truncated or >= 2^53, or a decimal exponent outside Clinger's
    exact cases (-22..37; above 0 only while the mantissa, times 10^(e-22) when e > 22, stays <= 1e15).  This is what cph_numcol.host_rows counts."""
    b = _bytes(value)
    if b"_" in b or not _DECIMAL.fullmatch(b):
        return False
    ip, fp, ex = _DEC_PARTS.fullmatch(b).groups()
    digs = (ip + fp).lstrip(b"0")
    dp = len(ip) - (len(ip + fp) - len(digs))
    if not digs:
        return False
    trunc = any(c != 0x30 for c in digs[19:])
    digs = digs[:19]
    mant = int(digs)
    e = 0
    if ex is not None:
        e = min(int(ex.lstrip(b"+-") or b"0"), 99999) * (-1 if ex[:1] == b"-" else 1)
    exp = dp - len(digs) + e
    if trunc or mant >= 1 << 53:
        return True
    if exp == 0 or -22 <= exp < 0:
        return False
    if 0 < exp <= 37:
        return float(mant) * (10.0 ** (exp - 22) if exp > 22 else 1.0) > 1e15
    return True


def _go_quote(b: bytes) -> str:
    r"""%q of a string: printable ASCII stays, '"' and the backslash get a backslash, the controls Go names become
    \a \b \f \n \r \t \v, other control bytes and invalid UTF-8 become \xNN.  unicode.IsPrint is NOT modelled: every
    validly encoded rune >= U+0080 is copied."""
    out = []
    i = 0
    named = {7: "\\a", 8: "\\b", 12: "\\f", 10: "\\n", 13: "\\r", 9: "\\t", 11: "\\v"}
    while i < len(b):
        c = b[i]
        if c < 0x80:
            if c == 0x22 or c == 0x5C:
                out.append("\\" + chr(c))
            elif c in named:
                out.append(named[c])
            elif c < 0x20 or c == 0x7F:
                out.append("\\x%02x" % c)
            else:
                out.append(chr(c))
            i += 1
            continue
        for k in (2, 3, 4):
            try:
                out.append(b[i:i + k].decode("utf-8"))
                i += k
                break
            except UnicodeDecodeError:
                continue
        else:
            out.append("\\x%02x" % c)
            i += 1
    return '"' + "".join(out) + '"'


def conversion_error(column, value, kind, as_float=False) -> str:
    """The reference's error text (csvplus.go:176, :198):
    `column "<name>": cannot convert "<value>" to integer: invalid syntax` (or `to float`, or `value out of range`);
    column and value are quoted as Go's %q does, see _go_quote."""
    what = {NUM_ERR_SYNTAX: "invalid syntax", NUM_ERR_RANGE: "value out of range",
            NUM_ERR_UNSUPPORTED: "not decided by this library (digit separators, hexadecimal floats)"}[kind]
    return f"column {_go_quote(_bytes(column))}: cannot convert {_go_quote(_bytes(value))} to {'float' if as_float else 'integer'}: {what}"


def _cmp(rel, a, b) -> bool:
    return {"<": a < b, "<=": a <= b, "==": a == b, "!=": a != b, ">=": a >= b, ">": a > b}[rel]


def _str_holds(op, value, literal) -> bool:
    """One string term (STR_LT + relation, HAS_PREFIX, HAS_SUFFIX, CONTAINS) on a present value: Python's bytes operations."""
    v = _bytes(value)
    if op == HAS_PREFIX:
        return v.startswith(literal)
    if op == HAS_SUFFIX:
        return v.endswith(literal)
    if op == CONTAINS:
        return literal in v
    return _cmp(RELS[op - STR_LT], v, literal)


def _is_time_op(op) -> bool:
    return TIME_LT <= op < TIME_LT + len(RELS)


def _time_holds(rel, value, literal) -> bool:
    """One time term on a present value: both sides through timeconv.parse_model, whole seconds."""
    from . import timeconv as T
    status, v = T.parse_model(value, "s")
    return status == NUM_OK and _cmp(rel, v, T.parse_model(literal, "s")[1])


def _is_expr_op(op) -> bool:
    return EXPR_LT <= op < EXPR_LT + len(RELS)


def _is_cols_op(op) -> bool:
    return COLS_LT <= op < COLS_LT + len(RELS)


def _expr_holds(rel, ops, values, i) -> bool:
    """One expression term: `ops` (two values left, lhs below rhs) on the row whose column values are values[k]; i = the
    row's position, which indexes the array leaves.  A failing op makes it false."""
    from . import expr as E

    def leaf(q, o):
        op, arg, value = o
        if op == E.COL_INT:
            return atoi(values[arg])
        if op == E.COL_FLT:
            return parse_float(values[arg])
        if value.device:
            raise ValueError("an array on the device has no host values")
        return (int(value.values[i]) if op == E.NUM_INT else float(value.values[i])), NUM_OK

    (a, b), status, _ = E.run_ops(ops, leaf, want=2)
    return status == NUM_OK and _cmp(rel, a, b)


def remap_columns(ops, index):
    """The ops of `compile` with every column k — a term's own, a ColCmp's second, an expression's COL leaves — replaced by
    index(k): what a caller needs that shares one column list among several programs (mapping.compile_switch)."""
    from . import expr as E
    out = []
    for op, arg, v in ops:
        if _is_expr_op(op):
            if arg >= 0:
                eops, arrs = v
                v = ([(o, index(a), x) if o in (E.COL_INT, E.COL_FLT) else (o, a, x) for o, a, x in eops], arrs)
        elif _is_cols_op(op):
            arg, v = (index(arg) if arg >= 0 else arg), (index(v) if v >= 0 else v)
        elif v is not None and arg >= 0:
            arg = index(arg)
        out.append((op, arg, v))
    return out


def _is_str_op(op) -> bool:
    return STR_LT <= op < STR_LT + len(RELS) or op in (HAS_PREFIX, HAS_SUFFIX, CONTAINS)


def _num_holds(is_float, rel, value, literal) -> bool:
    v, kind = parse_float(value) if is_float else atoi(value)
    return kind == NUM_OK and _cmp(rel, v, literal)


def compile(pred: Pred, column_names):   # noqa: A001 (the name the issue of record uses)
    """(names of the columns used, postfix ops).  An op is (LIKE, column, value bytes) with `column` indexing the returned
    name list, or -1 for a name that is not among `column_names` (the row has no such column: false, :1286); a numeric term
    (INT_LT / FLT_LT + relation, column, 8 literal bytes); a string term (STR_LT + relation / HAS_PREFIX / HAS_SUFFIX /
    CONTAINS, column, literal bytes); a time term (TIME_LT + relation, column, the literal's RFC 3339 text); an expression term
    (EXPR_LT + relation, 0, (expr ops, arrays)) whose expr ops are expr.compile's for both sides in one program (lhs below rhs)
    with COL leaves indexing the returned name list, or (EXPR_LT + relation, -1, None) when a column is missing; a
    column-against-column term (COLS_LT + relation, column a, column b), either -1 when missing; (NOT, 0, None);
    (ALL, k, None); (ANY, k, None).  Raises ValueError beyond the ABI's limits (64 ops, 32 LIKE terms, stack of 32)."""
    known = [str(c) for c in column_names]
    used: list[str] = []
    ops: list[tuple] = []

    def emit(p):
        if isinstance(p, Like):
            for name, value in p.items:
                if name not in known:
                    ops.append((LIKE, -1, value))
                    continue
                if name not in used:
                    used.append(name)
                ops.append((LIKE, used.index(name), value))
            if len(p.items) > 1:
                ops.append((ALL, len(p.items), None))
        elif isinstance(p, _NumCmp):
            flt = isinstance(p, FloatCmp)
            op = (FLT_LT if flt else INT_LT) + RELS.index(p.rel)
            lit = struct.pack("<d" if flt else "<q", p.literal)
            if p.column not in known:
                ops.append((op, -1, lit))
            else:
                if p.column not in used:
                    used.append(p.column)
                ops.append((op, used.index(p.column), lit))
        elif isinstance(p, (StrCmp, _StrTest, TimeCmp)):
            op = TIME_LT + RELS.index(p.rel) if isinstance(p, TimeCmp) else STR_LT + RELS.index(p.rel) if isinstance(p, StrCmp) else p.op
            if p.column not in known:
                ops.append((op, -1, p.literal))
            else:
                if p.column not in used:
                    used.append(p.column)
                ops.append((op, used.index(p.column), p.literal))
        elif isinstance(p, ExprCmp):
            from . import expr as E
            op = EXPR_LT + RELS.index(p.rel)
            if any(nm not in known for nm in p.names):
                ops.append((op, -1, None))
            else:
                for nm in p.names:
                    if nm not in used:
                        used.append(nm)
                own, eops = p._compile(known)
                eops = [(o, used.index(own[a]), x) if o in (E.COL_INT, E.COL_FLT) else (o, a, x) for o, a, x in eops]
                ops.append((op, 0, (eops, E.arrays(eops))))
        elif isinstance(p, ColCmp):
            for nm in (p.a, p.b):
                if nm in known and nm not in used:
                    used.append(nm)
            ops.append((COLS_LT + RELS.index(p.rel), used.index(p.a) if p.a in known else -1, used.index(p.b) if p.b in known else -1))
        elif isinstance(p, Not):
            emit(p.pred)
            ops.append((NOT, 0, None))
        elif isinstance(p, (All, Any)):
            for q in p.preds:
                emit(q)
            ops.append((ALL if isinstance(p, All) else ANY, len(p.preds), None))
        else:
            raise TypeError(f"not a predicate: {p!r}")

    emit(pred)
    depth = likes = 0
    for op, arg, _ in ops:
        if op == LIKE or op >= INT_LT:
            depth += 1
            likes += 1
        elif op in (ALL, ANY):
            depth += 1 - arg
        if depth > MAX_STACK:
            raise ValueError(f"predicate needs a stack deeper than {MAX_STACK}")
    if len(ops) > MAX_OPS:
        raise ValueError(f"predicate compiles to {len(ops)} ops, more than {MAX_OPS}")
    if likes > MAX_LIKE:
        raise ValueError(f"predicate has {likes} Like, numeric and string terms, more than {MAX_LIKE}")
    return used, ops


def _row_get(row, name):
    v = row.get(name)
    return row.get(name.encode("utf-8")) if v is None else v


def matches(pred: Pred, row, i: int = 0) -> bool:
    """The predicate on one row (a dict; str and bytes compare by their UTF-8 bytes); i = the row's position in the
    selection, which is what an ExprCmp's IntArr / FloatArr leaves are indexed with."""
    if isinstance(pred, ExprCmp):
        values = [_row_get(row, nm) for nm in pred.names]
        return all(v is not None for v in values) and _expr_holds(pred.rel, pred.ops, values, i)
    if isinstance(pred, ColCmp):
        a, b = _row_get(row, pred.a), _row_get(row, pred.b)
        return a is not None and b is not None and _cmp(pred.rel, _bytes(a), _bytes(b))
    if isinstance(pred, Like):
        for name, value in pred.items:
            v = row.get(name)
            if v is None and isinstance(name, str):
                v = row.get(name.encode("utf-8"))
            if v is None or _bytes(v) != value:
                return False
        return True
    if isinstance(pred, _NumCmp):
        v = row.get(pred.column)
        if v is None:
            v = row.get(pred.column.encode("utf-8"))
        return v is not None and _num_holds(isinstance(pred, FloatCmp), pred.rel, v, pred.literal)
    if isinstance(pred, (StrCmp, _StrTest)):
        v = row.get(pred.column)
        if v is None:
            v = row.get(pred.column.encode("utf-8"))
        op = STR_LT + RELS.index(pred.rel) if isinstance(pred, StrCmp) else pred.op
        return v is not None and _str_holds(op, v, pred.literal)
    if isinstance(pred, TimeCmp):
        v = row.get(pred.column)
        if v is None:
            v = row.get(pred.column.encode("utf-8"))
        return v is not None and _time_holds(pred.rel, v, pred.literal)
    if isinstance(pred, Not):
        return not matches(pred.pred, row, i)
    if isinstance(pred, All):
        return all(matches(p, row, i) for p in pred.preds)
    if isinstance(pred, Any):
        return any(matches(p, row, i) for p in pred.preds)
    raise TypeError(f"not a predicate: {pred!r}")


def run_ops(ops, values, i: int = 0) -> bool:
    """The postfix program on one row given as the list of its column values (indexed like compile's name list); i = the
    row's position in the selection (an expression term's array leaves)."""
    st: list[bool] = []
    for op, arg, value in ops:
        if _is_expr_op(op):
            st.append(arg >= 0 and _expr_holds(RELS[op - EXPR_LT], value[0], values, i))
        elif _is_cols_op(op):
            st.append(arg >= 0 and value >= 0 and _cmp(RELS[op - COLS_LT], _bytes(values[arg]), _bytes(values[value])))
        elif op == LIKE:
            st.append(arg >= 0 and _bytes(values[arg]) == value)
        elif _is_str_op(op):
            st.append(arg >= 0 and _str_holds(op, values[arg], value))
        elif _is_time_op(op):
            st.append(arg >= 0 and _time_holds(RELS[op - TIME_LT], values[arg], value))
        elif op >= INT_LT:
            flt = op >= FLT_LT
            (lit,) = struct.unpack("<d" if flt else "<q", value)
            st.append(arg >= 0 and _num_holds(flt, RELS[op - (FLT_LT if flt else INT_LT)], values[arg], lit))
        elif op == NOT:
            st.append(not st.pop())
        else:
            k = [st.pop() for _ in range(arg)]
            st.append(all(k) if op == ALL else any(k))
    (res,) = st
    return res


def select_rows(flags, mode="where", first_row=0, nrows=None, skip=0, limit=None):
    """The row-list semantics of cph_filter_rows on the host: `flags[i]` = the predicate on row i of the selection.
    Looks at rows [first_row, first_row + nrows) (Drop / Top in front of the filter), applies the mode — "where" (Filter,
    :276-286), "take_while" (:346-358), "drop_while" (:362-374) — then Drop(skip).Top(limit) behind it.  Returns the
    ascending list of row numbers (positions in the selection, first_row included)."""
    flags = list(flags)
    n = len(flags) - first_row if nrows is None else int(nrows)
    if n < 0 or first_row + n > len(flags):
        raise ValueError("select_rows: the range leaves the selection")
    rows = range(first_row, first_row + n)
    if mode == "where":
        kept = [i for i in rows if flags[i]]
    elif mode in ("take_while", "drop_while"):
        stop = next((i for i in rows if not flags[i]), first_row + n)
        kept = list(range(first_row, stop)) if mode == "take_while" else list(range(stop, first_row + n))
    else:
        raise ValueError(f"unknown mode {mode!r}")
    kept = kept[skip:]
    return kept if limit is None else kept[:limit]
