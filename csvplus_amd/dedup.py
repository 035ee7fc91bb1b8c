"""Index.ResolveDuplicates (csvplus.go:643-653) over the device index.

The device finds every duplicate group in one pass (cph_index_dup_groups); the callback and the compaction
rule of dedup (csvplus.go:810-867) are replayed here on the host over that list, then cph_index_select builds
the compacted index.  The replay keeps the reference's behaviour to the letter, including its tail rule: once
at least one group was resolved, the rows after the LAST group are copied by the loop :851-859, which moves
rows[lower-1] only while lower < len(rows) — the final row of the index is therefore dropped unless it belongs
to the last duplicate group ([A,A,B] -> [A], [A,A,B,C] -> [A,B]).  `keep_last_row=True` opts out of that.

The resolvers people actually write are a handful of fixed rules.  Those are data here — First, Last, DropAll, MinBy,
MaxBy — and resolve_duplicates_device runs them on the device (cph_index_resolve: a segmented arg-min / arg-max over the
sorted index, the same compaction, the same tail rule); rule_pick states the same rule as a callback for the route above.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def dedup_positions(nrows: int, lower, upper, resolve, keep_last_row: bool = False) -> np.ndarray:
    """Sorted positions that survive dedup.  resolve(lo, hi) -> a position in [lo, hi) (the chosen row), or None
    (the reference's "empty row": the whole group is dropped); an exception propagates (the reference returns
    the callback's error, :835-837)."""
    ng = len(lower)
    if ng == 0:                                   # :821-823 no duplicates: nothing changes
        return np.arange(nrows, dtype=np.uint64)
    parts = [np.arange(0, int(lower[0]), dtype=np.uint64)]            # dest = lower-1 (:825)
    for g in range(ng):
        lo, hi = int(lower[g]), int(upper[g])
        choice = resolve(lo, hi)                                       # :835 resolve(rows[lower-1:upper])
        if choice is not None:                                         # :842-845 store the chosen row
            c = int(choice)
            if not lo <= c < hi:
                raise ValueError(f"resolver returned position {c} outside its group [{lo}, {hi})")
            parts.append(np.array([c], dtype=np.uint64))
        # :848-859 copy the non-duplicates up to the next group; rows[lower-1] moves only while lower < len
        stop = int(lower[g + 1]) if g + 1 < ng else (nrows if keep_last_row else nrows - 1)
        if stop > hi:
            parts.append(np.arange(hi, stop, dtype=np.uint64))
    return np.concatenate(parts)


def resolve_duplicates(index: N.DeviceIndex, resolve, keep_last_row: bool = False) -> N.DeviceIndex:
    """Returns the deduplicated index (the input index is left as it was: a failing callback changes nothing,
    where the reference leaves its rows half-compacted)."""
    lower, upper = index.dup_groups()
    pos = dedup_positions(index.nrows, lower, upper, resolve, keep_last_row)
    return index.select(pos)


# ---- named rules: the resolver as data, resolved on the device (cph_index_resolve) -------------------------------------
class Rule:
    """A resolver that is data instead of a closure.  `code` = CPH_RESOLVE_*."""
    code = 0
    ordered = False

    def __repr__(self):
        return type(self).__name__ + "()"


class First(Rule):
    """Keep the first row of every group (the index order is stable: the first in the input)."""
    code = N.CPH_RESOLVE_FIRST


class Last(Rule):
    """Keep the last row of every group."""
    code = N.CPH_RESOLVE_LAST


class DropAll(Rule):
    """Drop every ambiguous key: the reference's resolver returning an empty row."""
    code = N.CPH_RESOLVE_DROP


class MinBy(Rule):
    """Keep the row whose order value is smallest; ties go to the first row.  A NaN loses to every number."""
    code = N.CPH_RESOLVE_MIN
    ordered = True


class MaxBy(Rule):
    """Keep the row whose order value is largest; ties go to the first row.  A NaN loses to every number."""
    code = N.CPH_RESOLVE_MAX
    ordered = True


_KINDS = {"int": N.CPH_NUM_INT64, "float": N.CPH_NUM_FLOAT64, "bytes": N.CPH_ORDER_BYTES}


class ResolveError(ValueError):
    """A row INSIDE a group whose order value does not convert (the error a Go resolver returning row.ValueAsInt's
    error would hand back): `position` = the lowest such sorted position, `row` = perm[position], `kind` = CPH_NUM_ERR_*."""

    def __init__(self, position: int, row: int, kind: int, nerrors: int):
        what = {N.CPH_NUM_ERR_SYNTAX: "invalid syntax", N.CPH_NUM_ERR_RANGE: "value out of range"}.get(kind, "unsupported syntax")
        super().__init__(f"order value of row {row} (sorted position {position}) does not convert: {what} ({nerrors} such rows in groups)")
        self.position, self.row, self.kind, self.nerrors = position, row, kind, nerrors


class Resolved(N.Owned):
    """What resolve_duplicates_device returns: the compacted `index`, the surviving sorted `positions` of the input index
    (a numpy uint64 array, or (device pointer, count) for out_mem = DEVICE, valid until release(); the index lives on),
    and the call's statistics."""
    _release_fn = "cph_resolved_release"

    def __init__(self, ctx, ptr, index, out_mem):
        super().__init__(ctx, ptr)
        r = ptr.contents
        self.index, self.positions = index, N.result_array(r.positions, int(r.nrows), np.uint64, out_mem)
        self.ngroups, self.group_rows, self.host_rows = int(r.ngroups), int(r.group_rows), int(r.host_rows)
        if out_mem == N.CPH_MEM_HOST:
            self.release()   # the array is a copy


def rule_pick(rule: Rule, values_by_sorted_position=None):
    """The resolve(lo, hi) callable that states `rule` on the host, for resolve_duplicates / dedup_positions.
    values_by_sorted_position[p] = the order value of sorted position p as the rule's kind reads it (int, float or
    bytes), needed by MinBy / MaxBy only.  This is the model of cph_index_resolve's choice: floats compare with
    -0 == +0, a NaN loses to every number under both rules, a group of NaNs keeps its first row, bytes compare as
    Python bytes do (unsigned, a proper prefix is smaller), and ties go to the lowest position."""
    if isinstance(rule, First):
        return lambda lo, hi: lo
    if isinstance(rule, Last):
        return lambda lo, hi: hi - 1
    if isinstance(rule, DropAll):
        return lambda lo, hi: None
    if not isinstance(rule, (MinBy, MaxBy)):
        raise TypeError(f"not a resolve rule: {rule!r}")
    if values_by_sorted_position is None:
        raise ValueError("MinBy / MaxBy need the order values")
    vals = values_by_sorted_position
    want_min = isinstance(rule, MinBy)

    def is_nan(v):
        return isinstance(v, float) and v != v

    def pick(lo, hi):
        best = None
        for p in range(lo, hi):
            v = vals[p]
            if is_nan(v):
                continue
            if best is None or (v < vals[best] if want_min else v > vals[best]):
                best = p
        return lo if best is None else best
    return pick


def resolve_duplicates_device(index: N.DeviceIndex, rule: Rule, order=None, kind=None, keep_last_row: bool = False,
                              out_mem: int = N.CPH_MEM_HOST) -> Resolved:
    """Index.ResolveDuplicates with a named rule, on the device (cph_index_resolve): nothing crosses to the host per
    group or per row.  `order` = a StrCol of the index's build table in its original row order (host or device) and
    `kind` = "int" | "float" | "bytes" for MinBy / MaxBy.  The input index is left as it was.  A group row whose order
    value does not convert raises ResolveError."""
    if not isinstance(rule, Rule):
        raise TypeError(f"not a resolve rule: {rule!r}")
    opts = N.cph_resolve_opts(rule.code, 0, 1 if keep_last_row else 0, 0)
    col, keep = None, []
    if rule.ordered:
        if order is None or kind not in _KINDS:
            raise ValueError('MinBy / MaxBy need an order column and kind = "int", "float" or "bytes"')
        opts.order_kind = _KINDS[kind]
        col = N.cols_array([order], keep)
    ctx = index.ctx
    h = N._P()
    out = C.POINTER(N.cph_resolved)()
    rc = ctx.lib.cph_index_resolve(ctx.handle, index.handle, C.byref(opts), col, out_mem, C.byref(h), C.byref(out))
    del keep
    ctx._check(rc)
    r = out.contents
    if r.nerrors:
        err = ResolveError(int(r.first_error_position), int(r.first_error_row), int(r.first_error_kind), int(r.nerrors))
        ctx.lib.cph_resolved_release(out)
        raise err
    return Resolved(ctx, out, N.DeviceIndex._from_handle(ctx, h), out_mem)
