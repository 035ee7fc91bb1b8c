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
    Col("id").trim_space()   a Span: the column's value NARROWED by a short program of span operations — the result is a
                         sub-span of the value, no byte changes.  The methods chain (each returns a new Span, which has the same
                         methods), at most 4 operations per part and 16 per template or Switch:
                           trim_space() / trim_left_space() / trim_right_space()   strings.TrimSpace / TrimLeftFunc / TrimRightFunc(s,
                                                 unicode.IsSpace): Go's 25 space sequences, exact for every byte string;
                           trim(cutset) / trim_left(cutset) / trim_right(cutset)   strings.Trim / TrimLeft / TrimRight with an ASCII
                                                 cutset of at most 32 bytes (a byte of 0x80 or above is refused);
                           trim_prefix(lit) / trim_suffix(lit)                     strings.TrimPrefix / TrimSuffix, at most 255 bytes;
                           field(sep, k, limit=-1)   strings.Split(s, sep)[k] (limit -1) or strings.SplitN(s, sep, limit)[k]; k < 0
                                                 counts from the last part; an index outside the parts gives b"" where Go panics;
                           before(sep) / after(sep)  strings.Cut: field 0 / field 1 of limit 2 (after: b"" without the separator);
                           span[a:b]             a slice of what is left: Col("ts").trim_space()[:10] is one part.
                         Span.apply(value) is the host model.  A Col with a default over a missing column runs the program on
                         the default.  Col("ts")[0:10] stays a Slice;
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
touches the GPU.  Out of scope: FormatFloat's remaining forms ('e' / 'g' with an explicit precision, 'b' / 'x', 32-bit floats); case mapping
(it changes bytes and needs Go's Unicode tables); a cutset with a byte of 0x80 or above; splitting on the empty separator;
regular expressions; time layouts other than RFC 3339, named zones and DST rules.

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
SPAN = 14                          # CPH_MAP_SPAN: value carries the operations
SPAN_TRIM_SPACE, SPAN_TRIM_CUTSET, SPAN_TRIM_PREFIX, SPAN_TRIM_SUFFIX, SPAN_FIELD, SPAN_SLICE = 1, 2, 3, 4, 5, 6   # CPH_SPAN_*
SPAN_LEFT, SPAN_RIGHT, SPAN_BOTH = 1, 2, 3
SPAN_MAX_OPS, SPAN_MAX_TOTAL, SPAN_MAX_CUTSET, SPAN_MAX_LITERAL = 4, 16, 32, 255
# unicode.IsSpace as bytes: the UTF-8 encodings of Go's 25 spaces
SPACE_SEQUENCES = (b"\t", b"\n", b"\v", b"\f", b"\r", b" ", b"\xc2\x85", b"\xc2\xa0", b"\xe1\x9a\x80") + tuple(
    bytes([0xE2, 0x80, c]) for c in range(0x80, 0x8B)) + (b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xe2\x80\xaf", b"\xe2\x81\x9f", b"\xe3\x80\x80")
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


class _SpanMethods:
    """The chainable span operations of Col and Span; each returns a new Span."""

    def _with(self, op):
        raise NotImplementedError

    def trim_space(self) -> "Span":
        return self._with((SPAN_TRIM_SPACE, SPAN_BOTH, 0, 0, b""))

    def trim_left_space(self) -> "Span":
        return self._with((SPAN_TRIM_SPACE, SPAN_LEFT, 0, 0, b""))

    def trim_right_space(self) -> "Span":
        return self._with((SPAN_TRIM_SPACE, SPAN_RIGHT, 0, 0, b""))

    def trim(self, cutset) -> "Span":
        return self._with((SPAN_TRIM_CUTSET, SPAN_BOTH, 0, 0, _cutset(cutset)))

    def trim_left(self, cutset) -> "Span":
        return self._with((SPAN_TRIM_CUTSET, SPAN_LEFT, 0, 0, _cutset(cutset)))

    def trim_right(self, cutset) -> "Span":
        return self._with((SPAN_TRIM_CUTSET, SPAN_RIGHT, 0, 0, _cutset(cutset)))

    def trim_prefix(self, lit) -> "Span":
        return self._with((SPAN_TRIM_PREFIX, 0, 0, 0, _span_literal(lit, "trim_prefix", 0)))

    def trim_suffix(self, lit) -> "Span":
        return self._with((SPAN_TRIM_SUFFIX, 0, 0, 0, _span_literal(lit, "trim_suffix", 0)))

    def field(self, sep, k, limit=-1) -> "Span":
        for v, what in ((k, "k"), (limit, "limit")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"field: {what} is an int, not {v!r}")
        if not INT64_MIN <= int(k) <= INT64_MAX:
            raise ValueError("field: k is not an int64")
        if int(limit) == 0 or not -1 <= int(limit) <= 0x7FFFFFFF:
            raise ValueError(f"field: limit is -1 (all parts) or at least 1, not {limit!r}")
        return self._with((SPAN_FIELD, int(limit), int(k), 0, _span_literal(sep, "field", 1)))

    def before(self, sep) -> "Span":
        return self.field(sep, 0, 2)

    def after(self, sep) -> "Span":
        return self.field(sep, 1, 2)


def _span_literal(lit, who, least) -> bytes:
    b = _bytes(lit)
    if len(b) < least:
        raise ValueError(f"{who}: an empty separator is not supported")
    if len(b) > SPAN_MAX_LITERAL:
        raise ValueError(f"{who}: a literal of {len(b)} bytes, more than {SPAN_MAX_LITERAL}")
    return b


def _cutset(cutset) -> bytes:
    b = _bytes(cutset)
    if len(b) > SPAN_MAX_CUTSET:
        raise ValueError(f"trim: a cutset of {len(b)} bytes, more than {SPAN_MAX_CUTSET}")
    if any(c >= 0x80 for c in b):
        raise ValueError("trim: a cutset byte of 0x80 or above (only an ASCII cutset trims bytewise as Go trims runes)")
    return b


class Col(_SpanMethods):
    """The row's value of column `name`; with `default`, that literal where the rows lack the column (SafeGetValue)."""

    def _with(self, op):
        return Span(self, (op,))

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


def _space_at_head(v: bytes, at: int, end: int) -> int:
    """Bytes of the space sequence that starts at v[at] inside v[:end]: 0, 1, 2 or 3."""
    for seq in SPACE_SEQUENCES:
        if at + len(seq) <= end and v[at:at + len(seq)] == seq:
            return len(seq)
    return 0


def _space_at_tail(v: bytes, at: int, end: int) -> int:
    """Bytes of the space sequence that ends at v[end - 1] inside v[at:end], start byte included: utf8.DecodeLastRune's decision."""
    for seq in SPACE_SEQUENCES:
        if end - len(seq) >= at and v[end - len(seq):end] == seq:
            return len(seq)
    return 0


class Span(_SpanMethods):
    """Span(col, ops): the value of `col` narrowed by the operations, left to right.  An operation is the tuple
    (op, mode, a, b, literal) of a cph_span_op.  Made by the methods of Col and Span, and by Span[a:b]."""

    def __init__(self, col, ops):
        if not isinstance(col, Col):
            raise TypeError(f"Span: not a Col: {col!r}")
        self.col = col
        self.ops = tuple(ops)
        if not 1 <= len(self.ops) <= SPAN_MAX_OPS:
            raise ValueError(f"a Span holds 1..{SPAN_MAX_OPS} operations, not {len(self.ops)}")

    def _with(self, op):
        return Span(self.col, self.ops + (op,))

    def __getitem__(self, key) -> "Span":
        if not isinstance(key, slice) or key.step is not None:
            raise TypeError(f"Span[...]: only a slice without a step, not {key!r}")
        sl = Slice(self.col, key.start, key.stop)   # its checks and its open ends
        return self._with((SPAN_SLICE, 0, sl.start, sl.stop, b""))

    @property
    def name(self):
        return self.col.name

    def apply(self, value: bytes) -> bytes:
        """The host model: the program on one value."""
        v = bytes(value)
        a, e = 0, len(v)
        for op, mode, x, y, lit in self.ops:
            if op == SPAN_TRIM_SPACE:
                if mode & SPAN_LEFT:
                    while True:
                        n = _space_at_head(v, a, e)
                        if not n:
                            break
                        a += n
                if mode & SPAN_RIGHT:
                    while True:
                        n = _space_at_tail(v, a, e)
                        if not n:
                            break
                        e -= n
            elif op == SPAN_TRIM_CUTSET:
                if mode & SPAN_LEFT:
                    while a < e and v[a] in lit:
                        a += 1
                if mode & SPAN_RIGHT:
                    while e > a and v[e - 1] in lit:
                        e -= 1
            elif op == SPAN_TRIM_PREFIX:
                if len(lit) <= e - a and v[a:a + len(lit)] == lit:
                    a += len(lit)
            elif op == SPAN_TRIM_SUFFIX:
                if len(lit) <= e - a and v[e - len(lit):e] == lit:
                    e -= len(lit)
            elif op == SPAN_FIELD:
                starts, ends, at = [], [], a   # strings.SplitN(v[a:e], lit, mode): left to right, no overlap
                while mode < 0 or len(starts) < mode - 1:
                    m = v.find(lit, at, e)
                    if m < 0:
                        break
                    starts.append(at)
                    ends.append(m)
                    at = m + len(lit)
                starts.append(at)
                ends.append(e)
                k = x + len(starts) if x < 0 else x
                a, e = (starts[k], ends[k]) if 0 <= k < len(starts) else (a, a)
            else:   # SPAN_SLICE
                lo, hi, _ = slice(x, None if y == INT64_MAX else y).indices(e - a)
                a, e = (a + lo, a + max(hi, lo))
        return v[a:e]

    def __repr__(self):
        names = {(SPAN_TRIM_SPACE, 3): "trim_space()", (SPAN_TRIM_SPACE, 1): "trim_left_space()", (SPAN_TRIM_SPACE, 2): "trim_right_space()"}
        out = repr(self.col)
        for op, mode, x, y, lit in self.ops:
            if op == SPAN_TRIM_SPACE:
                out += "." + names[(op, mode)]
            elif op == SPAN_TRIM_CUTSET:
                out += f".{('trim_left', 'trim_right', 'trim')[mode - 1]}({lit!r})"
            elif op in (SPAN_TRIM_PREFIX, SPAN_TRIM_SUFFIX):
                out += f".{'trim_prefix' if op == SPAN_TRIM_PREFIX else 'trim_suffix'}({lit!r})"
            elif op == SPAN_FIELD:
                out += f".field({lit!r}, {x}, {mode})"
            else:
                out += f"[{x or ''}:{'' if y == INT64_MAX else y}]"
        return out


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
            if isinstance(p, (Col, Slice, Span, Int, Float)):
                self.parts.append(p)
            elif isinstance(p, (bytes, bytearray, memoryview, str)):
                self.parts.append(_bytes(p))
            else:
                raise TypeError(f"not a template part: {p!r} (closures cannot run on the device; use bytes / str, Col, Col[a:b], Col.trim_space() and its kin, Int, Float, Time)")

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
    if isinstance(t, (Col, Slice, Span, Int, Float, bytes, bytearray, memoryview, str)):
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
        if isinstance(p, (Col, Slice, Span)):
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
    name list, (SLICE, k, (from, to)), (SPAN, k, ((op, mode, a, b, literal), ...)), (INT64, 0, Int), (FLOAT64, 0, Float), (FLOAT64_SHORTEST, 0, Float) or (TIME, 0, Time).  A Col (or the Col of a Slice) whose name is not among `column_names` becomes its default as a literal — in
    structure-of-arrays a column is present for all rows or for none — and without a default raises MissingColumn.
    A Span over such a column runs its program on the default, likewise.
    Neighbouring literals are joined.  Raises ValueError beyond the ABI's limits (16 pieces, 16 columns, 16 span operations)."""
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
            elif isinstance(p, Span):
                pieces.append((SPAN, used.index(p.name), p.ops))
            else:
                pieces.append((COLUMN, used.index(p.name), None))
        elif isinstance(p, (Slice, Span)) and p.col.default is not None:   # the default, sliced or narrowed on the host
            literal(p.apply(p.col.default))
        elif isinstance(p, Col) and p.default is not None:
            literal(p.default)
        else:
            raise MissingColumn(p.name)
    if len(pieces) > MAX_PIECES:
        raise ValueError(f"template compiles to {len(pieces)} pieces, more than {MAX_PIECES}")
    if len(used) > MAX_COLUMNS:
        raise ValueError(f"template reads {len(used)} columns, more than {MAX_COLUMNS}")
    nops = sum(len(v) for kind, _, v in pieces if kind == SPAN)
    if nops > SPAN_MAX_TOTAL:
        raise ValueError(f"template holds {nops} span operations, more than {SPAN_MAX_TOTAL}")
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
        return [(kind, index_of(used[arg]), v) if kind in (COLUMN, SLICE, SPAN) else (kind, arg, v) for kind, arg, v in pieces]

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
    nops = sum(len(v) for pc in [pc for _, pc in cases] + [otherwise] for kind, _, v in pc if kind == SPAN)
    if nops > SPAN_MAX_TOTAL:
        raise ValueError(f"Switch holds {nops} span operations in all, more than {SPAN_MAX_TOTAL}")
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
            col = p.col if isinstance(p, (Slice, Span)) else p
            v = row.get(col.name)
            if v is None:
                v = row.get(col.name.encode("utf-8"))
            if v is None:
                if col.default is None:
                    raise MissingColumn(col.name)
                v = col.default
            out.append(p.apply(_bytes(v)) if isinstance(p, (Slice, Span)) else _bytes(v))
    return b"".join(out)
