"""OrderBy: the rows of a selection in the order of typed keys, on the device (cph_order_rows), with Drop / Top behind it.

The reference orders rows only through an Index: by bytes ("10" < "9"), ascending, one comparison for all key columns.  The
order of a report — "the ten customers with the largest amount", "orders by ts descending, then by qty" — is data here:

    Asc(source, kind=None)    Desc(source, kind=None)        kind = "int" | "float" | "bytes"

`source` is a numpy int64 / float64 array with one value per row, a materialize.NumCol (it stays where it lives, status bytes
included), or a DeviceIndex over the table being ordered (kind "bytes": the index's own comparison, strings.Compare per key
column).  `materialize.order_rows(ctx, keys, nrows, skip, limit)` runs it; `order_model` states the same contract in pure
Python — documentation that runs, and what the tests expect.

The statement is Go's slices.SortStableFunc(rows, f): f compares key 0 first, then key 1, ...; a descending key swaps its two
arguments.  Rows equal on every key keep their input order under Asc and Desc alike, so Desc is not the reverse of Asc.
    int     cmp.Compare on int64
    float   cmp.Compare on float64: a NaN is less than every non-NaN, all NaNs are equal, -0 equals +0
    bytes   strings.Compare (a tuple of key columns compares column by column)
"""
from __future__ import annotations

import functools

import numpy as np

from . import _native as N

_KINDS = {"int": N.CPH_NUM_INT64, "float": N.CPH_NUM_FLOAT64, "bytes": N.CPH_ORDER_BYTES}


class OrderKey:
    """One key as data.  `kind` = CPH_NUM_INT64 / CPH_NUM_FLOAT64 / CPH_ORDER_BYTES."""
    descending = False

    def __init__(self, source, kind=None):
        if kind is None:
            if isinstance(source, N.DeviceIndex):
                kind = "bytes"
            elif isinstance(source, np.ndarray):
                kind = "float" if source.dtype.kind == "f" else "int"
            elif hasattr(source, "kind") and hasattr(source, "status"):   # a NumCol
                kind = "float" if source.kind == N.CPH_NUM_FLOAT64 else "int"
        if kind is None and isinstance(source, str):   # a NAME whose kind the consumer knows (pipeline.totals_to_csv)
            self.source, self.kind_name, self.kind = source, None, 0
            return
        if kind not in _KINDS:
            raise ValueError(f'{type(self).__name__}: kind must be "int", "float" or "bytes"')
        self.source, self.kind_name, self.kind = source, kind, _KINDS[kind]

    def __repr__(self):
        return f"{type(self).__name__}(<{type(self.source).__name__}>, {self.kind_name!r})"


class Asc(OrderKey):
    """Ascending: the comparison as it stands."""


class Desc(OrderKey):
    """Descending: the comparison with its arguments swapped; ties still keep their input order."""
    descending = True


class OrderError(ValueError):
    """A key value that did not convert (a status byte other than CPH_NUM_OK): `row` = the lowest such row of the selection,
    `key` = the lowest key that fails there, `kind` = its CPH_NUM_ERR_*, `nerrors` = such values over all keys."""

    def __init__(self, row: int, key: int, kind: int, nerrors: int):
        what = {N.CPH_NUM_ERR_SYNTAX: "invalid syntax", N.CPH_NUM_ERR_RANGE: "value out of range"}.get(kind, "unsupported syntax")
        super().__init__(f"key {key}: the value of row {row} does not convert: {what} ({nerrors} such values)")
        self.row, self.key, self.kind, self.nerrors = row, key, kind, nerrors


# ---- the contract in pure Python ----------------------------------------------------------------------------------------
def compare_int(a, b) -> int:
    """cmp.Compare on int64."""
    a, b = int(a), int(b)
    return (a > b) - (a < b)


def compare_float(a, b) -> int:
    """cmp.Compare on float64: a NaN is less than any non-NaN, a NaN equals a NaN, -0 equals +0."""
    a, b = float(a), float(b)
    a_nan, b_nan = a != a, b != b
    if a_nan:
        return 0 if b_nan else -1
    if b_nan:
        return 1
    return (a > b) - (a < b)   # IEEE comparison: -0.0 == +0.0


def compare_bytes(a, b) -> int:
    """strings.Compare; tuples (several key columns) compare column by column."""
    return (a > b) - (a < b)


_COMPARE = {N.CPH_NUM_INT64: compare_int, N.CPH_NUM_FLOAT64: compare_float, N.CPH_ORDER_BYTES: compare_bytes}


def order_model(keys, skip: int = 0, limit=None) -> list:
    """The host statement of cph_order_rows.  keys: Asc / Desc objects, or (values, kind, descending) triples, whose source
    / values hold one value per row: ints, floats, or bytes / tuples of bytes for kind "bytes".  Returns the row numbers
    order[skip : skip + limit] of slices.SortStableFunc over the keys (`sorted` is stable, as SortStableFunc is)."""
    plan = []
    for k in keys:
        if isinstance(k, OrderKey):
            values, kind, desc = k.source, k.kind, k.descending
        else:
            values, kind, desc = k
            kind = _KINDS.get(kind, kind)
        plan.append((list(values), _COMPARE[kind], bool(desc)))
    if not plan:
        raise ValueError("order_model: at least one key")
    n = len(plan[0][0])
    if any(len(v) != n for v, _, _ in plan):
        raise ValueError("order_model: the keys differ in length")

    def f(a: int, b: int) -> int:
        for values, cmp, desc in plan:
            c = cmp(values[b], values[a]) if desc else cmp(values[a], values[b])
            if c:
                return c
        return 0

    order = sorted(range(n), key=functools.cmp_to_key(f))
    skip = max(int(skip), 0)
    return order[skip:] if limit is None else order[skip:skip + max(int(limit), 0)]
