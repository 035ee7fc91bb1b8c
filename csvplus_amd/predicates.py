"""The reference's named predicates as plain data (csvplus.go:1243-1293): Like, All, Any, Not.

A Go closure cannot run on a GPU; these four are declarative and can.  `compile` flattens any nesting of them into the
postfix program cph_filter_rows takes (include/csvplus_hip.h), `matches` evaluates a predicate on one row held as a dict —
the reference's semantics restated on the host, for callers and as the cross-check of the compiler.  Nothing here touches
the GPU.
"""
from __future__ import annotations

LIKE, NOT, ALL, ANY = 1, 2, 3, 4   # CPH_PRED_*
MAX_OPS, MAX_LIKE, MAX_STACK = 64, 32, 32


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


def _operands(preds):
    for p in preds:
        if not isinstance(p, Pred):
            raise TypeError(f"not a predicate: {p!r} (closures cannot run on the device; use Like / All / Any / Not)")
    return list(preds)


def compile(pred: Pred, column_names):   # noqa: A001 (the name the issue of record uses)
    """(names of the columns used, postfix ops).  An op is (LIKE, column, value bytes) with `column` indexing the returned
    name list, or -1 for a name that is not among `column_names` (the row has no such column: false, :1286); (NOT, 0, None);
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
        if op == LIKE:
            depth += 1
            likes += 1
        elif op in (ALL, ANY):
            depth += 1 - arg
        if depth > MAX_STACK:
            raise ValueError(f"predicate needs a stack deeper than {MAX_STACK}")
    if len(ops) > MAX_OPS:
        raise ValueError(f"predicate compiles to {len(ops)} ops, more than {MAX_OPS}")
    if likes > MAX_LIKE:
        raise ValueError(f"predicate has {likes} Like terms, more than {MAX_LIKE}")
    return used, ops


def matches(pred: Pred, row) -> bool:
    """The predicate on one row (a dict; str and bytes compare by their UTF-8 bytes)."""
    if isinstance(pred, Like):
        for name, value in pred.items:
            v = row.get(name)
            if v is None and isinstance(name, str):
                v = row.get(name.encode("utf-8"))
            if v is None or _bytes(v) != value:
                return False
        return True
    if isinstance(pred, Not):
        return not matches(pred.pred, row)
    if isinstance(pred, All):
        return all(matches(p, row) for p in pred.preds)
    if isinstance(pred, Any):
        return any(matches(p, row) for p in pred.preds)
    raise TypeError(f"not a predicate: {pred!r}")


def run_ops(ops, values) -> bool:
    """The postfix program on one row given as the list of its column values (indexed like compile's name list)."""
    st: list[bool] = []
    for op, arg, value in ops:
        if op == LIKE:
            st.append(arg >= 0 and _bytes(values[arg]) == value)
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
