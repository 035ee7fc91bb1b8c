"""Map (csvplus.go:290-296) as plain data: row templates for computed columns.

The reference's Map takes a closure — `row["name"] = "Julia"`, `row["full"] = row["name"] + " " + row["surname"]`, the
README's Printf over a joined row.  A Go closure cannot run on a GPU; a row template is declarative and can: the value of
the new column in row i is the concatenation of the template's parts —

    bytes / str          a literal (str: its UTF-8 bytes);
    Col("name")          the row's value of that column; Col("name", default=b"x") substitutes the default where the
                         rows have no such column (Row.SafeGetValue, csvplus.go:69-75);
    Col("ts")[0:10]      a Slice: the bytes [from, to) of that value, Go's `row["ts"][:10]` — bytes, not runes.  The ends follow
                         Python's slice rules (negative counts from the end, open ends, both clamped into the value, crossing
                         ends give the empty string); one deviation from Go: an index out of range clamps instead of panicking.
                         No step.  A Col with a default over a missing column slices the default;
    Int(array)           array[i] written as strconv.Itoa writes it ('-' for negatives, no '+', no leading zeros); the array
                         lives on the host, or on the device: Int.on_device(device_ptr, count);
    Float(array, prec)   array[i] written as strconv.FormatFloat(v, 'f', prec, 64) writes it: prec digits behind the point,
                         rounded half-even on the exact binary value — the reference's amounts column,
                         `strconv.FormatFloat(price*float64(qty), 'f', 2, 64)` (csvplus_test.go:1391-1421).  prec is 0..22 and
                         finite values of 2^128 or more are refused, on the device and by the host model alike; host or
                         device array as for Int: Float.on_device(device_ptr, count, prec).
    Float.shortest(array, fmt="g")
                         array[i] written as strconv.FormatFloat(v, fmt, -1, 64) writes it: the SHORTEST digits that read back to
                         the same float64 (Python's repr digits), laid out by fmt = 'e' / 'E' (d.ddde±XX), 'f' (no exponent) or
                         'g' / 'G' ('e' when the exponent is below -4 or at least 6, else 'f').  No value is refused and the
                         text converts back to the same bits.  Float.shortest_on_device(device_ptr, count, fmt) and
                         Float.shortest_of(expr, fmt) as for Float; ftoa_shortest is the host model.
    Time(array, zone)    array[i] = Unix seconds, written as RFC 3339 in the fixed zone `zone_minutes` east of UTC:
                         `time.Unix(v, 0).In(time.FixedZone("", 60*zone)).Format(time.RFC3339)` — "YYYY-MM-DDTHH:MM:SSZ" for
                         zone 0, "...+HH:MM" / "...-HH:MM" otherwise (timeconv.format_model).  The zone is within -1439..1439
                         and a value whose local year leaves 0000..9999 is refused, on the device and by the host model
                         alike; host or device array as for Int: Time.on_device(device_ptr, count, zone_minutes);
                         Time.of(expr, zone_minutes) for an int64 expression, e.g. the hour bucket of a parsed column:
                         Time.of((IntArr(t) / 3600) * 3600).
    Int.of(expr)         the value of an int64 expression of csvplus_amd.expr over the same rows, written as Int writes it;
    Float.of(expr, prec) likewise for a float64 expression: the amounts column is
                         Float.of(FloatCol("price") * ToFloat(IntCol("qty")), 2) — converted, multiplied and formatted on
                         the device (cph_num_eval feeding cph_map_format), evaluated by `render` with expr.evaluate.  A row
                         whose expression fails raises expr.ExprError: the reference's conversion error, row and column named.

`compile` turns a template into the piece list cph_map_format takes (include/csvplus_hip.h), `render` evaluates it on one
row held as a dict — the host model, for callers without a GPU and as the cross-check of the device.  Nothing here
touches the GPU.  Out of scope: FormatFloat's remaining forms ('e' / 'g' with an explicit precision, 'b' / 'x', 32-bit floats); case mapping and
TrimSpace (Go's are Unicode-aware); splitting a value on a delimiter; regular expressions; time layouts other than
RFC 3339, named zones and DST rules.

A value that depends on a condition is a Switch — Go's `if / else if / else` inside the closure, as data:

    Switch((pred, template), ..., otherwise=template)   the template of the FIRST case whose predicate (csvplus_amd.predicates)
                                                        holds for the row, else `otherwise`;
    When(pred, then, otherwise)                         = Switch((pred, then), otherwise=otherwise): the reference's
                                                        `if row["name"] == "Amelia" { row["name"] = "Julia" }` is
                                                        When(Like(name="Amelia"), "Julia", Col("name")).

A Switch stands where a whole template stands (cph_map_switch); it is not a part of a Format and does not nest.  One
deviation from a closure: a Col without default that names a missing column raises MissingColumn when the Switch is
compiled, even if no row would select that alternative — in structure-of-arrays a column exists for all rows or for none.
"""
from __future__ import annotations

import math

import numpy as np

from . import predicates as _P
from . import timeconv as _T
from .predicates import INT64_MAX, INT64_MIN, _bytes, _go_quote

LITERAL, COLUMN, INT64, FLOAT64, SLICE, TIME = 1, 2, 3, 4, 8, 10   # CPH_MAP_*
FLOAT64_SHORTEST = 12              # CPH_MAP_FLOAT64_SHORTEST: prec carries the format byte
SHORTEST_FORMATS = "eEfgG"
MAX_PIECES = 16                    # CPH_MAP_MAX_PIECES
MAX_CASES = 8                      # CPH_MAP_MAX_CASES
SWITCH_MAX_PIECES = 32             # CPH_MAP_SWITCH_MAX_PIECES: the pieces of all alternatives together
MAX_COLUMNS = 16                   # CPH_MAX_KEY_COLS
MAX_PREC = 22                      # a FLOAT64 piece's prec: 0..22
FLOAT_LIMIT = 2.0 ** 128           # finite |v| at or above it is not formatted


class MissingColumn(LookupError):
    """The reference's `missing column "name"` (csvplus.go:129, :145)."""

    def __init__(self, name):
        super().__init__(f"missing column {_go_quote(_bytes(name))}")
        self.column = name


class Col:
    """The row's value of column `name`; with `default`, that literal where the rows lack the column (SafeGetValue)."""

    def __init__(self, name, default=None):
        self.name = str(name)
        self.default = None if default is None else _bytes(default)

    def __repr__(self):
        return f"Col({self.name!r})" if self.default is None else f"Col({self.name!r}, default={self.default!r})"

    def __getitem__(self, key) -> "Slice":
        if not isinstance(key, slice) or key.step is not None:
            raise TypeError(f"Col[...]: only a slice without a step, e.g. Col({self.name!r})[0:10], not {key!r}")
        return Slice(self, key.start, key.stop)


class Slice:
    """Slice(col, start, stop) = col[start:stop]: the bytes [start, stop) of the column's value under Python's slice rules.
    None is an open end; `to` travels as INT64_MAX ("to the end")."""

    def __init__(self, col, start=None, stop=None):
        if not isinstance(col, Col):
            raise TypeError(f"Slice: not a Col: {col!r}")
        for v in (start, stop):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not INT64_MIN <= int(v) <= INT64_MAX):
                raise TypeError(f"Slice: an end is an int64 or None, not {v!r}")
        self.col = col
        self.start = 0 if start is None else int(start)
        self.stop = INT64_MAX if stop is None else int(stop)

    @property
    def name(self):
        return self.col.name

    def apply(self, value: bytes) -> bytes:
        return value[self.start:(None if self.stop == INT64_MAX else self.stop)]

    def __repr__(self):
        return f"{self.col!r}[{self.start or ''}:{'' if self.stop == INT64_MAX else self.stop}]"


class Int:
    """One int64 per OUTPUT row, formatted as strconv.Itoa does.  Int(values): anything numpy turns into an int64 array, in
    host memory; Int.on_device(device_ptr, count): an int64 array on the device, e.g. NumCol.values of
    materialize.to_int / eval_number(..., out_mem=DEVICE); Int.of(expr): an int64 expression of csvplus_amd.expr,
    evaluated over the template's rows."""
    expr = None

    def __init__(self, values):
        if isinstance(values, np.ndarray):
            if values.dtype.kind not in "iu" or (values.dtype.kind == "u" and values.size and int(values.max()) > INT64_MAX):
                raise ValueError("Int: the array does not hold int64 values")
        else:
            values = [int(v) for v in values]
            if any(not INT64_MIN <= v <= INT64_MAX for v in values):
                raise ValueError("Int: a value is not an int64")
        self.device, self.values = False, np.ascontiguousarray(np.asarray(values, dtype=np.int64).reshape(-1))
        self.count = len(self.values)

    @classmethod
    def on_device(cls, device_ptr: int, count: int) -> "Int":
        self = cls.__new__(cls)
        self.device, self.values, self.count = True, int(device_ptr), int(count)
        return self

    @classmethod
    def of(cls, expr) -> "Int":
        from . import expr as E
        if E.kind_of(expr) != E.INT:
            raise TypeError("Int.of: the expression is a float64 (use Float.of, or ToInt)")
        self = cls.__new__(cls)
        self.device, self.values, self.count, self.expr = False, None, None, expr
        return self

    def __repr__(self):
        if self.expr is not None:
            return f"Int.of({self.expr!r})"
        return f"Int(<{self.count} values{' on the device' if self.device else ''}>)"


class Time(Int):
    """One int64 per OUTPUT row, Unix seconds, formatted as RFC 3339 in a fixed zone (timeconv.format_model).
    Time(values, zone_minutes=0): host values as for Int, e.g. NumCol.values of materialize.to_time;
    Time.on_device(device_ptr, count, zone_minutes=0); Time.of(expr, zone_minutes=0): an int64 expression of csvplus_amd.expr."""

    def __init__(self, values, zone_minutes=0):
        self.zone = _T.check_zone(zone_minutes, "Time")
        try:
            super().__init__(values)
        except ValueError as e:
            raise ValueError(str(e).replace("Int:", "Time:")) from None

    @classmethod
    def on_device(cls, device_ptr: int, count: int, zone_minutes=0) -> "Time":
        self = cls.__new__(cls)
        self.zone = _T.check_zone(zone_minutes, "Time.on_device")
        self.device, self.values, self.count = True, int(device_ptr), int(count)
        return self

    @classmethod
    def of(cls, expr, zone_minutes=0) -> "Time":
        from . import expr as E
        if E.kind_of(expr) != E.INT:
            raise TypeError("Time.of: the expression is a float64 (Unix seconds are an int64: use ToInt)")
        self = cls.__new__(cls)
        self.zone = _T.check_zone(zone_minutes, "Time.of")
        self.device, self.values, self.count, self.expr = False, None, None, expr
        return self

    def __repr__(self):
        if self.expr is not None:
            return f"Time.of({self.expr!r}, {self.zone})"
        return f"Time(<{self.count} values{' on the device' if self.device else ''}>, {self.zone})"


def _check_prec(prec, who) -> int:
    if isinstance(prec, bool) or int(prec) != prec or not 0 <= int(prec) <= MAX_PREC:
        raise ValueError(f"{who}: prec must be within 0..{MAX_PREC}, not {prec!r}")
    return int(prec)


def _check_fmt(fmt, who) -> str:
    if isinstance(fmt, (bytes, bytearray)):
        fmt = bytes(fmt).decode("latin-1")
    if not isinstance(fmt, str) or len(fmt) != 1 or fmt not in SHORTEST_FORMATS:
        raise ValueError(f"{who}: fmt must be one of 'e' 'E' 'f' 'g' 'G', not {fmt!r}")
    return fmt


class Float:
    """One float64 per OUTPUT row, formatted as strconv.FormatFloat(v, 'f', prec, 64) does.  Float(values, prec): anything
    numpy turns into a float64 array (an integer array is converted, as Go's float64(qty) would), in host memory;
    Float.on_device(device_ptr, count, prec): a float64 array on the device, e.g. NumCol.values of
    materialize.to_float / eval_number(..., out_mem=DEVICE); Float.of(expr, prec): a float64 expression of csvplus_amd.expr,
    evaluated over the template's rows.  prec: 0..22.
    Float.shortest(values, fmt), Float.shortest_on_device(device_ptr, count, fmt), Float.shortest_of(expr, fmt): the same three
    sources, formatted as strconv.FormatFloat(v, fmt, -1, 64) does (ftoa_shortest); such a part has `fmt` set and prec None."""
    expr = None
    fmt = None

    def __init__(self, values, prec):
        self.prec = _check_prec(prec, "Float")
        arr = np.asarray(values)
        if arr.dtype.kind not in "fiub":
            raise ValueError("Float: the array does not hold numbers")
        self.device, self.values = False, np.ascontiguousarray(arr.astype(np.float64, copy=False).reshape(-1))
        self.count = len(self.values)

    @classmethod
    def on_device(cls, device_ptr: int, count: int, prec: int) -> "Float":
        self = cls.__new__(cls)
        self.prec = _check_prec(prec, "Float.on_device")
        self.device, self.values, self.count = True, int(device_ptr), int(count)
        return self

    @classmethod
    def of(cls, expr, prec: int) -> "Float":
        from . import expr as E
        if E.kind_of(expr) != E.FLOAT:
            raise TypeError("Float.of: the expression is an int64 (use Int.of, or ToFloat)")
        self = cls.__new__(cls)
        self.prec = _check_prec(prec, "Float.of")
        self.device, self.values, self.count, self.expr = False, None, None, expr
        return self

    @classmethod
    def shortest(cls, values, fmt="g") -> "Float":
        fmt = _check_fmt(fmt, "Float.shortest")
        self = cls(values, 0)
        self.prec, self.fmt = None, fmt
        return self

    @classmethod
    def shortest_on_device(cls, device_ptr: int, count: int, fmt="g") -> "Float":
        fmt = _check_fmt(fmt, "Float.shortest_on_device")
        self = cls.on_device(device_ptr, count, 0)
        self.prec, self.fmt = None, fmt
        return self

    @classmethod
    def shortest_of(cls, expr, fmt="g") -> "Float":
        fmt = _check_fmt(fmt, "Float.shortest_of")
        from . import expr as E
        if E.kind_of(expr) != E.FLOAT:
            raise TypeError("Float.shortest_of: the expression is an int64 (use Int.of, or ToFloat)")
        self = cls.of(expr, 0)
        self.prec, self.fmt = None, fmt
        return self

    def text(self, v) -> bytes:
        """What the part writes for the value v: the host model."""
        return ftoa(v, self.prec) if self.fmt is None else ftoa_shortest(v, self.fmt)

    def __repr__(self):
        if self.fmt is not None:
            if self.expr is not None:
                return f"Float.shortest_of({self.expr!r}, {self.fmt!r})"
            return f"Float.shortest(<{self.count} values{' on the device' if self.device else ''}>, {self.fmt!r})"
        if self.expr is not None:
            return f"Float.of({self.expr!r}, {self.prec})"
        return f"Float(<{self.count} values{' on the device' if self.device else ''}>, {self.prec})"


class Format:
    """Format(part, ...): the concatenation of the parts (see the module text)."""

    def __init__(self, *parts):
        if not parts:
            raise ValueError("Format: no parts")
        self.parts = []
        for p in parts:
            if isinstance(p, (Col, Slice, Int, Float)):
                self.parts.append(p)
            elif isinstance(p, (bytes, bytearray, memoryview, str)):
                self.parts.append(_bytes(p))
            else:
                raise TypeError(f"not a template part: {p!r} (closures cannot run on the device; use bytes / str, Col, Col[a:b], Int, Float, Time)")

    def __repr__(self):
        return f"Format{tuple(self.parts)!r}"


def Const(value) -> Format:
    """`row[name] = value` for every row."""
    return Format(value)


class Switch:
    """Switch((pred, template), ..., otherwise=template): the template of the first case whose predicate holds for the row,
    else `otherwise`.  pred: a predicates.Pred; templates: what Format accepts (a Format, or a bare part).  At most 8 cases."""

    def __init__(self, *cases, otherwise):
        if not cases:
            raise ValueError("Switch: no cases")
        self.cases = []
        for c in cases:
            if not isinstance(c, (tuple, list)) or len(c) != 2:
                raise TypeError(f"Switch: a case is a (predicate, template) pair, not {c!r}")
            pred, tmpl = c
            if not isinstance(pred, _P.Pred):
                raise TypeError(f"Switch: not a predicate: {pred!r} (closures cannot run on the device; use csvplus_amd.predicates)")
            self.cases.append((pred, _template(tmpl)))
        self.otherwise = _template(otherwise)

    def alternatives(self) -> list:
        """The templates in selection order: the cases', then `otherwise`."""
        return [t for _, t in self.cases] + [self.otherwise]

    def __repr__(self):
        return f"Switch({', '.join(repr(c) for c in self.cases)}, otherwise={self.otherwise!r})"


def When(pred, then, otherwise) -> Switch:
    """`if pred(row) { then } else { otherwise }`."""
    return Switch((pred, then), otherwise=otherwise)


def _template(t) -> Format:
    if isinstance(t, Format):
        return t
    if isinstance(t, Switch):
        raise TypeError("a Switch stands where a whole template stands: it is no part of a Format and does not nest")
    if isinstance(t, (Col, Slice, Int, Float, bytes, bytearray, memoryview, str)):
        return Format(t)
    raise TypeError(f"not a template: {t!r}")


def _pred_columns(pred) -> list:
    if isinstance(pred, _P.Like):
        return [name for name, _ in pred.items]
    if isinstance(pred, (_P._NumCmp, _P.StrCmp, _P._StrTest, _P.TimeCmp)):
        return [pred.column]
    if isinstance(pred, _P.ExprCmp):
        return list(pred.names)
    if isinstance(pred, _P.ColCmp):
        return [pred.a, pred.b]
    if isinstance(pred, _P.Not):
        return _pred_columns(pred.pred)
    if isinstance(pred, (_P.All, _P.Any)):
        return [name for q in pred.preds for name in _pred_columns(q)]
    raise TypeError(f"not a predicate: {pred!r}")


def columns(template) -> list:
    """The names of the template's Col parts and of the columns its Int.of / Float.of expressions read, in order of first use.
    A Switch: the columns of its predicates and templates, case by case, then those of `otherwise`."""
    names: list[str] = []
    if isinstance(template, Switch):
        for pred, tmpl in template.cases + [(_P.All(), template.otherwise)]:
            for name in _pred_columns(pred) + columns(tmpl):
                if name not in names:
                    names.append(name)
        return names
    for p in _template(template).parts:
        if isinstance(p, (Col, Slice)):
            found = [p.name]
        elif isinstance(p, (Int, Float)) and p.expr is not None:
            from . import expr as E
            found = E.columns(p.expr)
        else:
            continue
        for name in found:
            if name not in names:
                names.append(name)
    return names


def compile(template, column_names):   # noqa: A001 (the name predicates.compile uses)
    """(names of the columns used, pieces).  A piece is (LITERAL, 0, bytes), (COLUMN, k, None) with k indexing the returned
    name list, (SLICE, k, (from, to)), (INT64, 0, Int), (FLOAT64, 0, Float), (FLOAT64_SHORTEST, 0, Float) or (TIME, 0, Time).  A Col (or the Col of a Slice) whose name is not among `column_names` becomes its default as a literal — in
    structure-of-arrays a column is present for all rows or for none — and without a default raises MissingColumn.
    Neighbouring literals are joined.  Raises ValueError beyond the ABI's limits (16 pieces, 16 columns)."""
    known = [str(c) for c in column_names]
    used: list[str] = []
    pieces: list[tuple] = []

    def literal(b):
        if pieces and pieces[-1][0] == LITERAL:
            pieces[-1] = (LITERAL, 0, pieces[-1][2] + b)
        else:
            pieces.append((LITERAL, 0, b))

    for p in _template(template).parts:
        if isinstance(p, bytes):
            literal(p)
        elif isinstance(p, Time):
            pieces.append((TIME, 0, p))
        elif isinstance(p, Int):
            pieces.append((INT64, 0, p))
        elif isinstance(p, Float):
            pieces.append((FLOAT64 if p.fmt is None else FLOAT64_SHORTEST, 0, p))
        elif p.name in known:
            if p.name not in used:
                used.append(p.name)
            if isinstance(p, Slice):
                pieces.append((SLICE, used.index(p.name), (p.start, p.stop)))
            else:
                pieces.append((COLUMN, used.index(p.name), None))
        elif isinstance(p, Slice) and p.col.default is not None:   # the default, sliced on the host
            literal(p.apply(p.col.default))
        elif isinstance(p, Col) and p.default is not None:
            literal(p.default)
        else:
            raise MissingColumn(p.name)
    if len(pieces) > MAX_PIECES:
        raise ValueError(f"template compiles to {len(pieces)} pieces, more than {MAX_PIECES}")
    if len(used) > MAX_COLUMNS:
        raise ValueError(f"template reads {len(used)} columns, more than {MAX_COLUMNS}")
    return used, pieces


def compile_switch(switch, column_names):
    """(names of the columns used, [(predicate ops, pieces) per case], pieces of `otherwise`): what cph_map_switch takes.  The
    ops are predicates.compile's and the pieces `compile`'s, with every column index pointing into the ONE returned name list,
    which the predicates and the templates share.  A predicate column that is not among `column_names` compiles to column -1
    (false); a Col part that is not becomes its default or raises MissingColumn — whether or not a row would select its
    alternative.  Raises ValueError beyond the ABI's limits: 8 cases, 16 pieces per alternative, 32 pieces in all, 16 columns."""
    if not isinstance(switch, Switch):
        raise TypeError(f"not a Switch: {switch!r}")
    if len(switch.cases) > MAX_CASES:
        raise ValueError(f"Switch has {len(switch.cases)} cases, more than {MAX_CASES}")
    known = [str(c) for c in column_names]
    shared: list[str] = []

    def index_of(name):
        if name not in shared:
            shared.append(name)
        return shared.index(name)

    def alternative(tmpl):
        used, pieces = compile(tmpl, known)
        return [(kind, index_of(used[arg]), v) if kind in (COLUMN, SLICE) else (kind, arg, v) for kind, arg, v in pieces]

    cases = []
    for pred, tmpl in switch.cases:
        used, ops = _P.compile(pred, known)
        ops = _P.remap_columns(ops, lambda k: index_of(used[k]))
        cases.append((ops, alternative(tmpl)))
    otherwise = alternative(switch.otherwise)
    total = sum(len(pc) for _, pc in cases) + len(otherwise)
    if total > SWITCH_MAX_PIECES:
        raise ValueError(f"Switch compiles to {total} pieces in all, more than {SWITCH_MAX_PIECES}")
    if len(shared) > MAX_COLUMNS:
        raise ValueError(f"Switch reads {len(shared)} columns, more than {MAX_COLUMNS}")
    return shared, cases, otherwise


def which_of(switch, row, i: int = 0) -> int:
    """The alternative a row selects: the index of the first case whose predicate holds, or the number of cases (`otherwise`);
    i = the row's number (the array leaves of an ExprCmp)."""
    for k, (pred, _) in enumerate(switch.cases):
        if _P.matches(pred, row, i):
            return k
    return len(switch.cases)


def itoa(v) -> bytes:
    """strconv.Itoa / strconv.FormatInt(v, 10) of an int64."""
    v = int(v)
    if not INT64_MIN <= v <= INT64_MAX:
        raise ValueError("itoa: not an int64")
    return b"%d" % v


def ftoa(v, prec) -> bytes:
    """strconv.FormatFloat(v, 'f', prec, 64) of a float64, prec 0..22.  For finite values Python's own %.*f: correctly
    rounded, half-even on the exact binary value, and the sign of a result that rounds to zero stays.  Raises ValueError for
    a finite |v| of 2^128 or more: the model refuses what the device refuses."""
    prec = _check_prec(prec, "ftoa")
    v = float(v)
    if math.isnan(v):
        return b"NaN"
    if math.isinf(v):
        return b"-Inf" if v < 0 else b"+Inf"
    if abs(v) >= FLOAT_LIMIT:
        raise ValueError("ftoa: a finite value of 2^128 or more is not formatted")
    return b"%.*f" % (prec, v)


def ftoa_shortest(v, fmt="g") -> bytes:
    """strconv.FormatFloat(v, fmt, -1, 64) of a float64 for fmt 'e' 'E' 'f' 'g' 'G'.  The digits are repr's — the shortest that
    read back to the same float64, the closest such — taken through decimal.Decimal(repr(v)).as_tuple(); the layouts are
    Go's (strconv/ftoa.go, %e / %f, and for 'g' the exponent test with precision 6).  No value is refused."""
    import decimal
    fmt = _check_fmt(fmt, "ftoa_shortest")
    v = float(v)
    if math.isnan(v):
        return b"NaN"
    if math.isinf(v):
        return b"-Inf" if v < 0 else b"+Inf"
    sign, digits, exponent = decimal.Decimal(repr(v)).as_tuple()
    d = "".join(map(str, digits)).lstrip("0")
    exponent += len(d) - len(d.rstrip("0"))
    d = d.rstrip("0") or "0"
    nd = len(d)
    dp = nd + exponent if d != "0" else 1       # the value is 0.d * 10^dp; zero is the digit 0 with dp 1
    exp = dp - 1
    neg = "-" if sign else ""
    if fmt in "eE" or (fmt in "gG" and (exp < -4 or exp >= 6)):
        e = "E" if fmt in "EG" else "e"
        text = f"{neg}{d[0]}{'.' + d[1:] if nd > 1 else ''}{e}{'-' if exp < 0 else '+'}{abs(exp):02d}"
    elif dp <= 0:
        text = f"{neg}0.{'0' * -dp}{d}"
    elif dp < nd:
        text = f"{neg}{d[:dp]}.{d[dp:]}"
    else:
        text = f"{neg}{d}{'0' * (dp - nd)}"
    return text.encode("ascii")


def _expr_value(p, row, i):
    from . import expr as E
    v, status, op = E.evaluate(p.expr, row, i)
    if status:
        names, ops = E.compile(p.expr, E.columns(p.expr))
        column = names[ops[op][1]] if ops[op][0] in (E.COL_INT, E.COL_FLT) else None
        raise E.ExprError(i, op, status, column, E.error_text(p.expr, row, status, op), 1)
    return v


def render(template, row, i: int = 0) -> bytes:
    """The template on one row (a dict with str or bytes keys and values); `i` = the row's number, which is what an Int
    or Float part is indexed with (host arrays only).  An Int.of / Float.of part is evaluated with expr.evaluate; a row
    where it fails raises expr.ExprError.  A Switch renders the alternative the row selects (which_of): parts of the
    other alternatives are not evaluated."""
    if isinstance(template, Switch):
        return render(template.alternatives()[which_of(template, row, i)], row, i)
    out = []
    for p in _template(template).parts:
        if isinstance(p, bytes):
            out.append(p)
        elif isinstance(p, (Int, Float)) and p.expr is not None:
            v = _expr_value(p, row, i)
            out.append(_T.format_model(v, p.zone) if isinstance(p, Time) else itoa(v) if isinstance(p, Int) else p.text(v))
        elif isinstance(p, Time):
            if p.device:
                raise ValueError("render: a Time part on the device has no host values")
            out.append(_T.format_model(p.values[i], p.zone))
        elif isinstance(p, Int):
            if p.device:
                raise ValueError("render: an Int part on the device has no host values")
            out.append(itoa(p.values[i]))
        elif isinstance(p, Float):
            if p.device:
                raise ValueError("render: a Float part on the device has no host values")
            out.append(p.text(p.values[i]))
        else:
            col = p.col if isinstance(p, Slice) else p
            v = row.get(col.name)
            if v is None:
                v = row.get(col.name.encode("utf-8"))
            if v is None:
                if col.default is None:
                    raise MissingColumn(col.name)
                v = col.default
            out.append(p.apply(_bytes(v)) if isinstance(p, Slice) else _bytes(v))
    return b"".join(out)
