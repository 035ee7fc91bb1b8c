"""Map (csvplus.go:290-296) as plain data: row templates for computed columns.

The reference's Map takes a closure — `row["name"] = "Julia"`, `row["full"] = row["name"] + " " + row["surname"]`, the
README's Printf over a joined row.  A Go closure cannot run on a GPU; a row template is declarative and can: the value of
the new column in row i is the concatenation of the template's parts —

    bytes / str          a literal (str: its UTF-8 bytes);
    Col("name")          the row's value of that column; Col("name", default=b"x") substitutes the default where the
                         rows have no such column (Row.SafeGetValue, csvplus.go:69-75);
    Int(array)           array[i] written as strconv.Itoa writes it ('-' for negatives, no '+', no leading zeros); the array
                         lives on the host, or on the device: Int.on_device(device_ptr, count).

`compile` turns a template into the piece list cph_map_format takes (include/csvplus_hip.h), `render` evaluates it on one
row held as a dict — the host model, for callers without a GPU and as the cross-check of the device.  Nothing here
touches the GPU.  Formatting floats, case mapping, trimming, substrings and conditional parts are out of scope.
"""
from __future__ import annotations

import numpy as np

from .predicates import INT64_MAX, INT64_MIN, _bytes, _go_quote

LITERAL, COLUMN, INT64 = 1, 2, 3   # CPH_MAP_*
MAX_PIECES = 16                    # CPH_MAP_MAX_PIECES
MAX_COLUMNS = 16                   # CPH_MAX_KEY_COLS


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


class Int:
    """One int64 per OUTPUT row, formatted as strconv.Itoa does.  Int(values): anything numpy turns into an int64 array, in
    host memory; Int.on_device(device_ptr, count): an int64 array on the device, e.g. NumCol.values of
    materialize.to_int(..., out_mem=DEVICE) after arithmetic on it."""

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

    def __repr__(self):
        return f"Int(<{self.count} values{' on the device' if self.device else ''}>)"


class Format:
    """Format(part, ...): the concatenation of the parts (see the module text)."""

    def __init__(self, *parts):
        if not parts:
            raise ValueError("Format: no parts")
        self.parts = []
        for p in parts:
            if isinstance(p, (Col, Int)):
                self.parts.append(p)
            elif isinstance(p, (bytes, bytearray, memoryview, str)):
                self.parts.append(_bytes(p))
            else:
                raise TypeError(f"not a template part: {p!r} (closures cannot run on the device; use bytes / str, Col, Int)")

    def __repr__(self):
        return f"Format{tuple(self.parts)!r}"


def Const(value) -> Format:
    """`row[name] = value` for every row."""
    return Format(value)


def _template(t) -> Format:
    if isinstance(t, Format):
        return t
    if isinstance(t, (Col, Int, bytes, bytearray, memoryview, str)):
        return Format(t)
    raise TypeError(f"not a template: {t!r}")


def columns(template) -> list:
    """The names of the template's Col parts, in order of first use."""
    names: list[str] = []
    for p in _template(template).parts:
        if isinstance(p, Col) and p.name not in names:
            names.append(p.name)
    return names


def compile(template, column_names):   # noqa: A001 (the name predicates.compile uses)
    """(names of the columns used, pieces).  A piece is (LITERAL, 0, bytes), (COLUMN, k, None) with k indexing the returned
    name list, or (INT64, 0, Int).  A Col whose name is not among `column_names` becomes its default as a literal — in
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
        elif isinstance(p, Int):
            pieces.append((INT64, 0, p))
        elif p.name in known:
            if p.name not in used:
                used.append(p.name)
            pieces.append((COLUMN, used.index(p.name), None))
        elif p.default is not None:
            literal(p.default)
        else:
            raise MissingColumn(p.name)
    if len(pieces) > MAX_PIECES:
        raise ValueError(f"template compiles to {len(pieces)} pieces, more than {MAX_PIECES}")
    if len(used) > MAX_COLUMNS:
        raise ValueError(f"template reads {len(used)} columns, more than {MAX_COLUMNS}")
    return used, pieces


def itoa(v) -> bytes:
    """strconv.Itoa / strconv.FormatInt(v, 10) of an int64."""
    v = int(v)
    if not INT64_MIN <= v <= INT64_MAX:
        raise ValueError("itoa: not an int64")
    return b"%d" % v


def render(template, row, i: int = 0) -> bytes:
    """The template on one row (a dict with str or bytes keys and values); `i` = the row's number, which is what an Int
    part is indexed with (host arrays only)."""
    out = []
    for p in _template(template).parts:
        if isinstance(p, bytes):
            out.append(p)
        elif isinstance(p, Int):
            if p.device:
                raise ValueError("render: an Int part on the device has no host values")
            out.append(itoa(p.values[i]))
        else:
            v = row.get(p.name)
            if v is None:
                v = row.get(p.name.encode("utf-8"))
            if v is None:
                if p.default is None:
                    raise MissingColumn(p.name)
                v = p.default
            out.append(_bytes(v))
    return b"".join(out)
