"""Totals: Count and Sum / Min / Max per key of an index, on the device (cph_index_aggregate).

The reference's TestSimpleTotals (csvplus_test.go:516-571) reads the joined rows and accumulates `price * qty` per cust_id in
a Go closure.  A closure cannot run on a GPU; the aggregate is data here, as Like / IntCmp / KeepMaxInt / Format are:

    Sum(source, kind)   Min(source, kind)   Max(source, kind)        kind = "int" | "float"

`source` is a StrCol of the index's build table in its original row order (host or device; converted as to_int / to_float
convert it), or numbers with one entry per row of the build table: a numpy array (host), a (device_ptr, count) pair or an
object with data_ptr() such as a torch tensor (device), or an EXPRESSION of csvplus_amd.expr over the build table's columns —
`Sum(FloatCol("price") * ToFloat(IntCol("qty")))`, the reference's own total: `totals(index, specs, columns={name: StrCol})`
evaluates it on the device over the table's rows (cph_num_eval) and hands the result in as numbers; its kind is the
expression's type.

A group is a maximal run of equal keys in the index, runs of ONE row included.  `totals` returns, per group in key order, the
sorted position and the table row of its first row, its row count and one value per spec; `totals_model` states the same
contract in pure Python over keys and values already in sorted order — documentation that runs, and what the tests expect.

Totals over a Join (`custAmounts[cid] += amount`, csvplus_test.go:754-806) group the JOINED rows by the build row the Join
matched: `join_totals(chain, step, index, specs)` (cph_chain_aggregate) with one value per joined row per spec, and
`join_totals_model` as its contract.  There a group is a row of the index, empty groups included.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from .columns import StrCol

_KINDS = {"int": N.CPH_NUM_INT64, "float": N.CPH_NUM_FLOAT64}
_MASK = (1 << 64) - 1


class Spec:
    """One aggregate as data.  `op` = CPH_AGG_*, `kind` = CPH_NUM_INT64 / CPH_NUM_FLOAT64."""
    op = 0
    name = ""

    def __init__(self, source, kind=None):
        from . import expr as E
        if isinstance(source, E.Expr):
            found = "float" if E.kind_of(source) == E.FLOAT else "int"
            if kind not in (None, found):
                raise ValueError(f"{type(self).__name__}: the expression is {found!r}, not {kind!r}")
            kind = found
        if kind is None and isinstance(source, np.ndarray):
            kind = "float" if source.dtype.kind == "f" else "int"
        if kind not in _KINDS:
            raise ValueError(f'{type(self).__name__}: kind must be "int" or "float"')
        self.source, self.kind_name, self.kind = source, kind, _KINDS[kind]

    def __repr__(self):
        return f"{type(self).__name__}(<{type(self.source).__name__}>, {self.kind_name!r})"


class Sum(Spec):
    """int: wraps around as Go's `+=` on an int does.  float: IEEE addition in a fixed (unspecified) association order."""
    op, name = N.CPH_AGG_SUM, "sum"


class Min(Spec):
    """float: math.Min — a NaN in the run gives NaN, Min(-0, +0) = -0."""
    op, name = N.CPH_AGG_MIN, "min"


class Max(Spec):
    """float: math.Max — a NaN in the run gives NaN, Max(-0, +0) = +0."""
    op, name = N.CPH_AGG_MAX, "max"


class TotalsError(ValueError):
    """A value of a StrCol source that does not convert (what a Go closure returning row.ValueAsInt's error hands back):
    `position` = the lowest such sorted position, `row` = perm[position], `kind` = CPH_NUM_ERR_*, `spec` = the lowest spec
    that fails there, `nerrors` = such values over all specs."""

    def __init__(self, position: int, row: int, kind: int, nerrors: int, spec: int):
        what = {N.CPH_NUM_ERR_SYNTAX: "invalid syntax", N.CPH_NUM_ERR_RANGE: "value out of range"}.get(kind, "unsupported syntax")
        super().__init__(f"spec {spec}: the value of row {row} (sorted position {position}) does not convert: {what} ({nerrors} such values)")
        self.position, self.row, self.kind, self.nerrors, self.spec = position, row, kind, nerrors, spec


class Totals(N.Owned):
    """What `totals` returns.  out_mem = HOST: first_position (uint64), first_row (uint32), count (uint64) and values[i] (int64 /
    float64) are numpy arrays; DEVICE: (device pointer, count) pairs, valid until release()."""
    _release_fn = "cph_aggregated_release"

    def __init__(self, ctx, ptr, specs, out_mem):
        super().__init__(ctx, ptr)
        r = ptr.contents
        self.ngroups, self.host_rows = int(r.ngroups), int(r.host_rows)
        self.first_position = N.result_array(r.first_position, self.ngroups, np.uint64, out_mem)
        self.first_row = N.result_array(r.first_row, self.ngroups, np.uint32, out_mem)
        self.count = N.result_array(r.count, self.ngroups, np.uint64, out_mem)
        self.values = _spec_values(r, self.ngroups, specs, out_mem)
        if out_mem == N.CPH_MEM_HOST:
            self.release()   # the arrays are copies


def _spec_values(r, ngroups, specs, out_mem):
    return [N.result_array(r.values[i], ngroups, np.int64 if sp.kind == N.CPH_NUM_INT64 else np.float64, out_mem)
            for i, sp in enumerate(specs)]


def _numbers(spec, need, rows, keep):
    """(pointer, CPH_MEM_*) of a spec's numbers, one per row of the build table / per joined row (`rows` words the
    message); an empty host array is passed as one zero: the library wants a pointer."""
    return N.number_source(spec.source, spec.kind, need, f"{type(spec).__name__}: {{count}} values for {{need}} {rows}", keep, stand_in=True)


def totals(index: N.DeviceIndex, specs=(), out_mem: int = N.CPH_MEM_HOST, columns=None) -> Totals:
    """Count and the specs' values per key of `index` (cph_index_aggregate); no specs: the distinct keys and their
    frequencies.  A StrCol value that does not convert raises TotalsError.  columns: {name: StrCol} of the build table, in
    its original row order — what a spec whose source is an expression reads; a row where the expression fails raises
    expr.ExprError."""
    from . import expr as E

    specs = list(specs)
    ctx = index.ctx
    arr = (N.cph_agg_spec * max(1, len(specs)))()
    keep, evaluated = [], []
    try:
        for i, sp in enumerate(specs):
            if not isinstance(sp, Spec):
                raise TypeError(f"not an aggregate: {sp!r} (closures cannot run on the device; use Sum, Min, Max)")
            arr[i].op, arr[i].kind = sp.op, sp.kind
            if isinstance(sp.source, E.Expr):
                from .materialize import eval_number, raise_expr_error
                nc = eval_number(ctx, columns or {}, sp.source, out_mem=N.CPH_MEM_DEVICE)   # the identity selection
                evaluated.append(nc)
                if nc.nerrors:
                    raise_expr_error(ctx, columns or {}, sp.source, nc)
                arr[i].numbers, arr[i].numbers_mem = nc.values[0] or None, N.CPH_MEM_DEVICE
            elif isinstance(sp.source, StrCol):
                arr[i].col = N.cols_array([sp.source], keep)
            else:
                arr[i].numbers, arr[i].numbers_mem = _numbers(sp, 0, "rows", keep)
        out = C.POINTER(N.cph_aggregated)()
        rc = ctx.lib.cph_index_aggregate(ctx.handle, index.handle, arr if specs else None, len(specs), out_mem, C.byref(out))
    finally:
        for nc in evaluated:
            nc.release()
    del keep
    ctx._check(rc)
    r = out.contents
    if r.nerrors:
        err = TotalsError(int(r.first_error_position), int(r.first_error_row), int(r.first_error_kind), int(r.nerrors), int(r.first_error_spec))
        ctx.lib.cph_aggregated_release(out)
        raise err
    return Totals(ctx, out, specs, out_mem)


# ---- the contract in pure Python ----------------------------------------------------------------------------------------
def _wrap64(v: int) -> int:
    v &= _MASK
    return v - (1 << 64) if v >> 63 else v


def go_min(x: float, y: float) -> float:
    """math.Min as documented: NaN if either is NaN, Min(-0, +0) = -0."""
    if x != x or y != y:
        return math.nan
    if x == 0 and y == 0:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def go_max(x: float, y: float) -> float:
    """math.Max as documented: NaN if either is NaN, Max(-0, +0) = +0."""
    if x != x or y != y:
        return math.nan
    if x == 0 and y == 0:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def _fold(op: int, is_float: bool, vals):
    if op == N.CPH_AGG_SUM:
        if is_float:
            acc = -0.0   # the identity of IEEE addition
            for v in vals:
                acc = acc + float(v)   # left to right: ONE of the association orders the contract allows
            return acc
        return _wrap64(sum(int(v) for v in vals))
    if not is_float:
        return min(int(v) for v in vals) if op == N.CPH_AGG_MIN else max(int(v) for v in vals)
    f = go_min if op == N.CPH_AGG_MIN else go_max
    acc = float(vals[0])
    for v in vals[1:]:
        acc = f(acc, float(v))
    return acc


def totals_model(keys_in_sorted_order, values_by_sorted_position=(), specs=()):
    """The host statement of cph_index_aggregate.  keys_in_sorted_order[p] = the key at sorted position p (anything comparable
    with ==; equal keys are adjacent); values_by_sorted_position[s][p] = the value spec s reads at position p (int or float);
    specs = Sum / Min / Max objects or (op, kind) pairs of CPH_AGG_* / CPH_NUM_*.  Returns a dict: ngroups, first_position,
    count, and values (one list per spec).  An int sum wraps to int64; a float sum is added left to right (the device's order
    is unspecified: compare bit for bit only where every order is exact); float Min / Max are go_min / go_max."""
    keys = list(keys_in_sorted_order)
    n = len(keys)
    starts = [p for p in range(n) if p == 0 or keys[p] != keys[p - 1]]
    ends = starts[1:] + [n]
    out = {"ngroups": len(starts), "first_position": starts, "count": [e - s for s, e in zip(starts, ends)], "values": []}
    for s, sp in enumerate(specs):
        op, kind = (sp.op, sp.kind) if isinstance(sp, Spec) else sp
        vals = values_by_sorted_position[s]
        out["values"].append([_fold(op, kind == N.CPH_NUM_FLOAT64, vals[lo:hi]) for lo, hi in zip(starts, ends)])
    return out


# ---- Totals over a Join: Count and Sum / Min / Max per BUILD ROW of a chain step (cph_chain_aggregate) --------------------
class JoinTotals(N.Owned):
    """What `join_totals` returns: one group per build row of the step's index (ngroups == index.nrows), empty groups
    included.  `positions`: group g is a sorted position of the index (True) or an original row id of its table (False), as
    in the chain.  out_mem = HOST: count (uint64) and values[i] (int64 / float64) are numpy arrays; DEVICE: (device pointer,
    count) pairs, valid until release()."""
    _release_fn = "cph_chain_aggregated_release"

    def __init__(self, ctx, ptr, specs, out_mem):
        super().__init__(ctx, ptr)
        r = ptr.contents
        self.ngroups, self.positions = int(r.ngroups), bool(r.positions)
        self.count = N.result_array(r.count, self.ngroups, np.uint64, out_mem)
        self.values = _spec_values(r, self.ngroups, specs, out_mem)
        if out_mem == N.CPH_MEM_HOST:
            self.release()   # the arrays are copies


def _chain_row_ids(chain, which):
    """The row ids the writers / eval_number take for a column of the stream table (which None / "stream") or of step
    `which`'s build table, for the joined rows of `chain`."""
    n = chain.nrows
    if chain.mem == N.CPH_MEM_HOST:
        if which in (None, "stream"):
            return None if chain.identity or n == 0 else (chain.stream_row, chain.probe_base)
        return chain.build_row(int(which))
    ptrs = chain.device_ptrs()
    if which in (None, "stream"):
        return None if chain.identity or n == 0 else (ptrs["stream_row"], 64, n, chain.probe_base)
    return (ptrs["build_row"][int(which)], 32, n)


def join_totals(chain: N.Chain, step: int, index: N.DeviceIndex, specs=(), out_mem: int = N.CPH_MEM_HOST, columns=None) -> JoinTotals:
    """Count and the specs' values per build row of `index`, the index of chain step `step`, over the JOINED rows of `chain`
    (cph_chain_aggregate): `qtyMap[id] += qty` of the reference's TestSimpleUniqueJoin without a second index.  specs: Sum /
    Min / Max whose source holds ONE VALUE PER JOINED ROW: a numpy array (host), a (device_ptr, count) pair or a device
    tensor, a materialize.NumCol over the joined rows (its status is handed through: a row that failed raises TotalsError), or
    an expression of csvplus_amd.expr, evaluated over the joined rows on the device (eval_number through the chain's row
    ids; a failing row raises expr.ExprError).  columns: what an expression reads — {name: StrCol} for a column of the
    stream table, {name: (StrCol, k)} for a column of step k's build table: in that table's original row order for a chain
    of row ids, in the index's sorted order (materialize.permute_col) for a chain of positions.  The columns live where the
    chain does (host / device).  A group is a build row, not a key: over a duplicate-key index add the rows of a run."""
    from . import expr as E
    from .materialize import NumCol, eval_number, raise_expr_error

    specs = list(specs)
    ctx = chain.ctx
    n = chain.nrows
    arr = (N.cph_chain_agg_spec * max(1, len(specs)))()
    keep, evaluated = [], []
    try:
        for i, sp in enumerate(specs):
            if not isinstance(sp, Spec):
                raise TypeError(f"not an aggregate: {sp!r} (closures cannot run on the device; use Sum, Min, Max)")
            if isinstance(sp.source, StrCol):
                raise TypeError(f"{type(sp).__name__}: a join total takes one value per JOINED row; read a column with an "
                                'expression (IntCol / FloatCol) and `columns`')
            arr[i].op, arr[i].kind = sp.op, sp.kind
            src = sp.source
            if isinstance(src, E.Expr):
                by_name, rid = {}, {}
                for name in E.columns(src):
                    if name not in (columns or {}):
                        continue   # eval_number raises MissingColumn
                    c = columns[name]
                    col, which = c if isinstance(c, tuple) else (c, None)
                    by_name[name], rid[name] = col, _chain_row_ids(chain, which)
                src = eval_number(ctx, by_name, src, row_ids=rid, nrows=n, out_mem=N.CPH_MEM_DEVICE)
                evaluated.append(src)
                if src.nerrors:
                    raise_expr_error(ctx, by_name, sp.source, src, row_ids=rid)
            if isinstance(src, NumCol):
                if src.kind != sp.kind:
                    raise ValueError(f"{type(sp).__name__}: the NumCol's kind differs from the spec's")
                if src.nrows < n:
                    raise ValueError(f"{type(sp).__name__}: {src.nrows} values for {n} joined rows")
                if src.mem == N.CPH_MEM_DEVICE and n:
                    arr[i].numbers, arr[i].status, arr[i].numbers_mem = src.values[0] or None, src.status[0] or None, N.CPH_MEM_DEVICE
                elif src.mem == N.CPH_MEM_DEVICE:   # no joined rows: a pointer that is never read
                    v = np.zeros(1, np.int64)
                    keep.append(v)
                    arr[i].numbers, arr[i].numbers_mem = v.ctypes.data, N.CPH_MEM_HOST
                else:
                    v, st = np.ascontiguousarray(src.values), np.ascontiguousarray(src.status)
                    if len(v) == 0:
                        v, st = np.zeros(1, v.dtype), np.zeros(1, np.uint8)
                    keep += [v, st]
                    arr[i].numbers, arr[i].status, arr[i].numbers_mem = v.ctypes.data, st.ctypes.data, N.CPH_MEM_HOST
                keep.append(src)
                continue
            arr[i].numbers, arr[i].numbers_mem = _numbers(sp, n, "joined rows", keep)
        out = C.POINTER(N.cph_chain_aggregated)()
        rc = ctx.lib.cph_chain_aggregate(ctx.handle, chain.ptr, int(step), index.handle if index is not None else None,
                                         arr if specs else None, len(specs), out_mem, C.byref(out))
    finally:
        for nc in evaluated:
            nc.release()
    del keep
    ctx._check(rc)
    r = out.contents
    if r.nerrors:
        row = int(r.first_error_row)
        err = TotalsError(row, row, int(r.first_error_kind), int(r.nerrors), int(r.first_error_spec))
        ctx.lib.cph_chain_aggregated_release(out)
        raise err
    return JoinTotals(ctx, out, specs, out_mem)


def join_totals_model(build_rows, ngroups, values=(), specs=()):
    """The host statement of cph_chain_aggregate.  build_rows[m] = the group (build row) of joined row m, below ngroups;
    values[s][m] = the value spec s reads at joined row m; specs = Sum / Min / Max objects or (op, kind) pairs.  Returns a
    dict: ngroups, count, and values (one list per spec; 0 / +0.0 for a group without rows).  An int sum wraps to int64; a
    float sum adds the group's rows in ascending m, left to right from -0.0 (the device's order is fixed but unspecified:
    compare bit for bit only where every order is exact); float Min / Max are go_min / go_max."""
    ngroups = int(ngroups)
    members = [[] for _ in range(ngroups)]
    for m, g in enumerate(build_rows):
        g = int(g)
        if not 0 <= g < ngroups:
            raise ValueError(f"join_totals_model: build row {g} of joined row {m} is not below {ngroups}")
        members[g].append(m)
    out = {"ngroups": ngroups, "count": [len(ms) for ms in members], "values": []}
    for s, sp in enumerate(specs):
        op, kind = (sp.op, sp.kind) if isinstance(sp, Spec) else sp
        is_float = kind == N.CPH_NUM_FLOAT64
        vals = values[s]
        out["values"].append([_fold(op, is_float, [vals[m] for m in ms]) if ms else (0.0 if is_float else 0) for ms in members])
    return out
