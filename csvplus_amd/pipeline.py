"""The reference's README pipeline (README.md:33-66) with every stage on the device:

    customers.csv -> UniqueIndexOn(id)          orders.csv -> SelectColumns(...)
    products.csv  -> UniqueIndexOn(prod_id)        .Join(customers, "cust_id").Join(products, "prod_id").ToCsv(...)

CSV bytes -> columns (cph_csv_parse) -> indices (cph_index_build) -> fused chained join (cph_join_chain) ->
output columns (cph_gather_rows: mergeRows, csvplus.go:571-583, column by column) -> CSV bytes
(cph_csv_write: ToCsv, :379-406; or JSON bytes, cph_json_write_rows: ToJSON, :446-480).  Nothing leaves HBM between
the first and the last step — also not with a Filter(pred).Drop(skip).Top(limit) between the Join and the writer
(`where`, `skip`, `limit`: cph_filter_rows over the joined rows, cph_rowsel_take on every column's row ids) and not with
computed columns behind that (`computed`: Map with row templates, cph_map_format over the joined rows).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import time

from . import _native as N
from . import ingest
from .materialize import gather_rows


class Table:
    """A parsed CSV file: device columns by name."""

    def __init__(self, csv_table: ingest.CsvTable):
        self.t = csv_table
        self.cols = {nm.decode(): col for nm, col in zip(csv_table.names, csv_table.columns)}
        self.nrows = csv_table.nrecords

    def __getitem__(self, name):
        return self.cols[name]

    def release(self):
        self.t.release()


def read_table(ctx: N.Context, text: bytes, select=None, **kw) -> Table:
    """A CSV file as device columns: ingest.read_csv with its keywords (expect_header, assume_header, comma, comment,
    trim_leading_space, num_fields, lazy_quotes).  lazy_quotes=True is Reader.LazyQuotes(): header line and body are read
    by Go's lazy rules (cph_csv_parse_lazy), so a file with `5" nails` or `He said "hi"` in it reaches join_to_csv /
    filter_to_csv / totals_to_csv like any other table.  A parse error of the body raises ingest.CsvParseError
    (one of the header line raises ingest.CsvError, as read_csv does)."""
    t = ingest.read_csv(ctx, text, select=select, out_mem=N.CPH_MEM_DEVICE, **kw)
    if t.error_kind:
        err = ingest.CsvParseError(t.error_kind, t.error_record)
        t.release()
        raise err
    return Table(t)


def join_to_csv(ctx: N.Context, stream: Table, steps, out_columns, timings: dict | None = None, out_mem: int = N.CPH_MEM_HOST,
                fused: bool = True, positions: bool | None = None, where=None, skip: int = 0, limit=None, computed=None):
    """stream and the index tables come from read_table (read_table(..., lazy_quotes=True) for files that need
    Reader.LazyQuotes()).
    steps: [(index_table, index_key_column, stream_key_column), ...] — each index must be unique on its key
    (UniqueIndexOn; a duplicate raises like the reference's error :751).  out_columns: [(output name, table,
    column)] where table is `stream` or one of the index tables; the caller resolves name collisions the way
    mergeRows does (the stream's column wins, :578-580) by naming the table it wants.
    positions: the Join reports SORTED POSITIONS (cph_join_chain_ex CPH_CHAIN_POSITIONS — the
    reference's own row handle, csvplus.go:553-567, and the cheap lookup on the device) and the payload columns of every
    build table are put in index order once (cph_index_permute: the reference's createIndex leaves its rows sorted, :736),
    so a position IS the row subscript; False: original row ids into the tables as they were read (rounds 1-3); None
    (default): whichever is cheaper by the measured costs (profiles/r04_pipeline.txt) — putting a payload column in index
    order costs ~0.3 ms per 1e7 table rows, reporting positions saves ~1.0 ms per 1e8 stream rows, so a one-shot pipeline
    whose stream is only a few times longer than its build tables keeps row ids.
    where / skip / limit: Join(...).Filter(where).Drop(skip).Top(limit) in front of the writer — `where` is a predicate of
    csvplus_amd.predicates (Like, All, Any, Not, IntCmp, FloatCmp, StrCmp, HasPrefix, HasSuffix, Contains, TimeCmp, ExprCmp, ColCmp) over the JOINED row: a name is looked up in the stream first, then in
    steps[0]'s table, steps[1]'s, ... (mergeRows: the stream's value wins); a name none of them has makes its Like false.
    computed: {name: template} — ...Map(row[name] = template(row)) behind the filter, one template of csvplus_amd.mapping
    (Format, Const, Switch; parts may be slices, Col("ts")[0:10]) per new column, applied in dict order over the joined rows that are left: a Col is looked up among the
    columns computed so far, then in the joined row as `where` does.  An out_columns entry whose output name is a computed
    name takes the computed column (its table and column are ignored and may be None): `row[name] = ...` replaces a source
    column of that name.  A Float.of / Int.of part computes its value from an expression of csvplus_amd.expr over the same
    rows on the device — {"amount": Format(Float.of(FloatCol("price") * ToFloat(IntCol("qty")), 2))} is the reference's
    amounts column — and a row where it fails raises expr.ExprError with the row and the column.  None (default): nothing
    is computed.
    Returns the CSV text (header + joined rows, stream order): bytes, or a DeviceBytes handle for out_mem DEVICE."""
    def lap(name, t0):
        if timings is not None:
            ctx.synchronize()
            timings[name] = timings.get(name, 0.0) + (time.perf_counter() - t0) * 1e3

    with _joined(ctx, stream, steps, out_columns, lap, positions, where, skip, limit, computed) as (cols, ids, n, bufs):
        t0 = time.perf_counter()
        from .materialize import csv_write
        if fused:
            # mergeRows inside the writer: fields are read through the row-id tuples, nothing is materialised
            text = csv_write(ctx, cols, [name for name, _, _ in out_columns], out_mem=out_mem, row_ids=ids, nrows=n)
            lap("to_csv_ms", t0)
        else:
            gcols = []
            for c, i in zip(cols, ids):
                if i is None and c.nrows == n:
                    gcols.append(c)
                    continue
                cb = gather_rows(ctx, c, i, out_mem=N.CPH_MEM_DEVICE)
                bufs.append(cb)
                gcols.append(cb.as_device_strcol())
            lap("gather_ms", t0)
            t0 = time.perf_counter()
            text = csv_write(ctx, gcols, [name for name, _, _ in out_columns], out_mem=out_mem)
            lap("to_csv_ms", t0)
        return text


def _compute_columns(ctx: N.Context, computed, source, n, bufs):
    """Map with row templates: computed = {name: template}, applied in dict order over n rows.  source(name) -> (column,
    row ids) of a source column, or None when the rows have no such column; a name computed earlier is read from its
    result.  Returns {name: device column} (identity columns of n rows); their ColBufs are appended to `bufs`."""
    from . import mapping as M
    from .materialize import map_column

    done = {}
    for cname, tmpl in computed.items():
        by_name, rid = {}, {}
        for name in M.columns(tmpl):
            if name in done:
                by_name[name] = done[name]
                continue
            s = source(name)
            if s is not None:
                by_name[name], rid[name] = s
        cb = map_column(ctx, by_name, tmpl, row_ids=rid, nrows=n, out_mem=N.CPH_MEM_DEVICE)
        bufs.append(cb)
        done[str(cname)] = cb.as_device_strcol()
    return done


@contextlib.contextmanager
def _joined(ctx: N.Context, stream: Table, steps, out_columns, lap, positions, where=None, skip=0, limit=None, computed=None):
    """Index, chain and output columns of a Join(...) over `steps`: yields (cols, ids, n, bufs) — per output column the column
    to read and its row ids for the writers (csv_write / json_write row_ids), the joined row count, and a list whose
    ColBufs are released on exit (with the indexes and the chain).  where / skip / limit: see join_to_csv; the rows the
    filter keeps replace the joined rows (every column's row ids narrowed on the device).  computed: see join_to_csv; the
    templates run over the rows that are left and their results stand in for the output columns of their names."""
    filtered = where is not None or skip or limit is not None
    pred_columns = []   # (name, table, name) of the columns the predicate reads, resolved like mergeRows does
    tmpl_columns = []   # the same for the source columns the templates read
    merged = {}
    if filtered or computed:
        for tab in [stream] + [t for t, _, _ in steps]:
            for name in tab.cols:
                merged.setdefault(name, tab)
    if filtered:
        from . import predicates as P
        if where is None:
            where = P.All()   # Drop / Top alone: every row holds
        pred_columns = [(name, merged[name], name) for name in P.compile(where, list(merged))[0]]
    if computed:
        from . import mapping as M
        computed = {str(k): v for k, v in computed.items()}
        earlier = set()
        for cname, tmpl in computed.items():
            for name in M.columns(tmpl):
                if name not in earlier and name in merged and all(name != t[0] for t in tmpl_columns):
                    tmpl_columns.append((name, merged[name], name))
            earlier.add(cname)
        all_out = list(out_columns)
        out_columns = [oc for oc in all_out if oc[0] not in computed] + tmpl_columns
    for name, tab, _ in out_columns:
        if tab is None:
            raise ValueError(f"output column {name!r} names no table and no template computes it")
    if positions is None:
        payload = {}
        for _, tab, col in list(out_columns) + pred_columns:   # (out_columns holds the templates' columns too)
            if tab is not stream:
                payload[(id(tab), col)] = tab.nrows
        positions = 1.0e-8 * stream.nrows > 3.0e-8 * sum(payload.values())
    indices, ch, bufs = [], None, []
    try:   # whatever fails below, the indexes, the chain and the gathered columns go back to the ctx pool
        t0 = time.perf_counter()
        for tab, key, _ in steps:
            ix = N.DeviceIndex(ctx, [tab[key]], unique=True)
            indices.append(ix)
            if ix.status == N.CPH_ERR_DUPLICATE:
                raise ValueError(f"duplicate value while creating unique index on {key!r} (sorted position {ix.first_dup})")
        lap("index_ms", t0)
        t0 = time.perf_counter()
        tabs = [t for t, _, _ in steps]
        sorted_cols = {}   # (table number, column) -> that column in index order
        if positions:
            from .materialize import permute_col
            for _, tab, col in list(out_columns) + pred_columns:
                if tab is not stream and (tabs.index(tab), col) not in sorted_cols:
                    cb = permute_col(ctx, indices[tabs.index(tab)], tab[col])
                    bufs.append(cb)
                    sorted_cols[(tabs.index(tab), col)] = cb.as_device_strcol()
        lap("index_ms", t0)
        t0 = time.perf_counter()
        ch = N.join_chain(ctx, [(ix, [stream[skey]]) for ix, (_, _, skey) in zip(indices, steps)], out_mem=N.CPH_MEM_DEVICE,
                          positions=positions)
        ptrs = ch.device_ptrs()
        n = ch.nrows
        lap("join_ms", t0)
        def resolve(columns):
            cols, ids = [], []
            for _, tab, col in columns:
                cols.append(tab[col] if tab is stream or not positions else sorted_cols[(tabs.index(tab), col)])
                if tab is stream:
                    ids.append(None if ch.identity or n == 0 else (ptrs["stream_row"], 64, n))
                else:
                    ids.append((ptrs["build_row"][tabs.index(tab)], 32, n))
            return cols, ids

        cols, ids = resolve(out_columns)
        if filtered and n:
            t0 = time.perf_counter()
            from .materialize import filter_rows, take_rows
            pcols, pids = resolve(pred_columns)
            names = [name for name, _, _ in pred_columns]
            kept = filter_rows(ctx, dict(zip(names, pcols)), where, row_ids=dict(zip(names, pids)), nrows=n, skip=skip, limit=limit,
                               out_mem=N.CPH_MEM_DEVICE)
            bufs.append(kept)
            narrowed = {}   # the columns of one table share their row ids: one gather per distinct array
            for k, i in enumerate(ids):
                if len(kept) == 0:
                    break
                if i is None:
                    ids[k] = kept.as_row_ids()
                    continue
                if i not in narrowed:
                    narrowed[i] = take_rows(ctx, i, kept, out_mem=N.CPH_MEM_DEVICE)
                    bufs.append(narrowed[i])
                ids[k] = narrowed[i].as_row_ids()
            n = len(kept)
            lap("filter_ms", t0)
        if n == 0:
            cols, ids = [c.head(0) for c in cols], [None] * len(cols)
        if computed:
            t0 = time.perf_counter()
            first = len(cols) - len(tmpl_columns)
            src = {t[0]: (c, i) for t, c, i in zip(tmpl_columns, cols[first:], ids[first:])}
            done = _compute_columns(ctx, computed, src.get, n, bufs)
            real = iter(zip(cols[:first], ids[:first]))
            pairs = [(done[oc[0]], None) if oc[0] in done else next(real) for oc in all_out]
            cols, ids = [c for c, _ in pairs], [i for _, i in pairs]
            lap("map_ms", t0)
        yield cols, ids, n, bufs
    finally:
        for cb in bufs:
            cb.release()
        if ch is not None:
            ch.release()
        for ix in indices:
            ix.close()


def join_to_json(ctx: N.Context, stream: Table, steps, out_columns=None, timings: dict | None = None, out_mem: int = N.CPH_MEM_HOST,
                 positions: bool | None = None, where=None, skip: int = 0, limit=None, computed=None):
    """Join(...).ToJSON() (csvplus.go:446-480) over the steps of join_to_csv, written by cph_json_write_rows with mergeRows
    folded into the writer.  out_columns: [(output name, table, column)] as in join_to_csv, the names all different; None
    (default): what the reference's joined rows hold — every column of the stream and of every index table, a name present
    in several of them taken from the first of stream, steps[0], steps[1], ... (nested mergeRows, :559-560, :571-583).
    where / skip / limit: Filter(where).Drop(skip).Top(limit) in front of the writer, as in join_to_csv.
    computed: {name: template}, as in join_to_csv; with out_columns None every computed name is a key of the objects and
    stands in for a source column of that name.
    Returns the JSON text: bytes, or a DeviceBytes handle for out_mem DEVICE."""
    if out_columns is None:
        out_columns, seen = [], set()
        for tab in [stream] + [t for t, _, _ in steps]:
            for name in tab.cols:
                if name not in seen:
                    seen.add(name)
                    out_columns.append((name, tab, name))
        out_columns += [(str(name), None, None) for name in (computed or {}) if str(name) not in seen]

    def lap(name, t0):
        if timings is not None:
            ctx.synchronize()
            timings[name] = timings.get(name, 0.0) + (time.perf_counter() - t0) * 1e3

    with _joined(ctx, stream, steps, out_columns, lap, positions, where, skip, limit, computed) as (cols, ids, n, _):
        t0 = time.perf_counter()
        from .materialize import json_write
        text = json_write(ctx, cols, [name for name, _, _ in out_columns], out_mem=out_mem, row_ids=ids, nrows=n)
        lap("to_json_ms", t0)
        return text


def filter_to_csv(ctx: N.Context, table: Table, pred, out_columns, mode: str = "where", first_row: int = 0, nrows=None,
                  skip: int = 0, limit=None, out_mem: int = N.CPH_MEM_HOST, computed=None, order_by=None):
    """The reference's headline shape, FromFile(...).Filter(Like(...)).ToCsv(...), on the device: the rows of ONE table
    (read_table; with lazy_quotes=True for FromFile(...).LazyQuotes()) where `pred` holds (mode "where"; "take_while" / "drop_while" for TakeWhile / DropWhile; first_row / nrows: Drop / Top
    in front of the filter, skip / limit: behind it), written as CSV.  out_columns: column names, or (output name, column)
    pairs.  computed: {name: template} — .Map(row[name] = template(row)) behind the filter (csvplus_amd.mapping), in dict
    order over the rows kept; an output column of a computed name takes the computed column.
    order_by: ordering.Asc / ordering.Desc over a column NAME with kind "int" / "float" / "bytes" — .OrderBy(keys) over the
    rows the filter kept, IN FRONT OF skip / limit ("the ten largest"), sorted on the device (materialize.order_rows); a key
    value that does not convert raises ordering.OrderError, its row counted among the rows kept.  None (default): row order.
    Returns the CSV text: bytes, or a DeviceBytes handle for out_mem DEVICE."""
    from . import predicates as P
    from .materialize import csv_write, filter_rows

    pairs = [(c, c) if isinstance(c, str) else tuple(c) for c in out_columns]
    if order_by is not None:
        return _filter_ordered_to_csv(ctx, table, pred, pairs, mode, first_row, nrows, skip, limit, out_mem, computed, list(order_by))
    bufs = []
    kept = filter_rows(ctx, table.cols, pred, nrows=nrows, mode=mode, first_row=first_row, skip=skip, limit=limit,
                       out_mem=N.CPH_MEM_DEVICE)
    try:
        if kept.is_range and len(kept) and kept.first:   # a WHILE mode's answer that does not start at row 0: as an array
            rng = filter_rows(ctx, table.cols, P.All(), nrows=len(kept), first_row=kept.first, out_mem=N.CPH_MEM_DEVICE)
            kept.release()
            kept = rng
        header = [name for name, _ in pairs]
        rows = None if kept.is_range else kept.as_row_ids()   # a range: rows 0 .. len - 1 (or none)
        view = (lambda c: c.head(len(kept))) if kept.is_range else (lambda c: c)
        done = {}
        if computed:
            done = _compute_columns(ctx, {str(k): v for k, v in computed.items()},
                                    lambda name: (view(table[name]), rows) if name in table.cols else None, len(kept), bufs)
        cols = [done[name] if name in done else view(table[c]) for name, c in pairs]
        if kept.is_range:
            return csv_write(ctx, cols, header, out_mem=out_mem)
        return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=[None if name in done else rows for name, _ in pairs],
                         nrows=len(kept))
    finally:
        for cb in bufs:
            cb.release()
        kept.release()


def _filter_ordered_to_csv(ctx, table, pred, pairs, mode, first_row, nrows, skip, limit, out_mem, computed, order_by):
    """filter_to_csv with order_by: Filter | OrderBy | Drop(skip) | Top(limit) | Map | ToCsv, every step on the device."""
    from . import mapping as M
    from . import ordering as O
    from . import predicates as P
    from .materialize import csv_write, filter_rows, gather_rows, order_rows, take_rows, to_float, to_int

    if not order_by:
        raise ValueError("filter_to_csv: order_by needs at least one key")
    for key in order_by:
        if not isinstance(key, O.OrderKey) or not isinstance(key.source, str):
            raise TypeError(f"filter_to_csv: an order key is Asc / Desc over a column name, not {key!r}")
        if key.source not in table.cols:
            raise M.MissingColumn(key.source)
        if not key.kind:
            raise ValueError(f'filter_to_csv: the order key over {key.source!r} needs a kind: "int", "float" or "bytes"')
    bufs, handles = [], []
    kept = filter_rows(ctx, table.cols, pred, nrows=nrows, mode=mode, first_row=first_row, out_mem=N.CPH_MEM_DEVICE)
    handles.append(kept)
    try:
        if kept.is_range and len(kept):   # a WHILE mode's answer: as an array of row numbers
            kept = filter_rows(ctx, table.cols, P.All(), nrows=len(kept), first_row=kept.first, out_mem=N.CPH_MEM_DEVICE)
            handles.append(kept)
        n = len(kept)
        header = [name for name, _ in pairs]
        if n == 0:
            return csv_write(ctx, [table[c].head(0) for _, c in pairs], header, out_mem=out_mem)
        rows = kept.as_row_ids()
        keys = []
        for key in order_by:
            col = table[key.source]
            if key.kind == N.CPH_ORDER_BYTES:   # the index's comparison over the values of the rows kept
                cb = gather_rows(ctx, col, rows, out_mem=N.CPH_MEM_DEVICE)
                bufs.append(cb)
                src = N.DeviceIndex(ctx, [cb.as_device_strcol()])
            else:
                src = (to_int if key.kind == N.CPH_NUM_INT64 else to_float)(ctx, col, row_ids=rows, nrows=n, out_mem=N.CPH_MEM_DEVICE)
            handles.append(src)
            keys.append(type(key)(src, key.kind_name))
        ordered = order_rows(ctx, keys, n, skip=skip, limit=limit, out_mem=N.CPH_MEM_DEVICE)
        handles.append(ordered)
        m = len(ordered)
        if m == 0:
            return csv_write(ctx, [table[c].head(0) for _, c in pairs], header, out_mem=out_mem)
        final = take_rows(ctx, rows, ordered, out_mem=N.CPH_MEM_DEVICE)   # table rows in output order
        handles.append(final)
        ids = final.as_row_ids()
        done = {}
        if computed:
            done = _compute_columns(ctx, {str(k): v for k, v in computed.items()},
                                    lambda name: (table[name], ids) if name in table.cols else None, m, bufs)
        cols = [done[name] if name in done else table[c] for name, c in pairs]
        return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=[None if name in done else ids for name, _ in pairs], nrows=m)
    finally:
        for cb in bufs:
            cb.release()
        for h in reversed(handles):
            h.close()


def totals_to_csv(ctx: N.Context, table: Table, by, specs, names=None, out_mem: int = N.CPH_MEM_HOST, order_by=None, limit=None):
    """IndexOn(by...) over `table`, then Count and the specs per key, written as CSV — the reference's TestSimpleTotals loop
    (csvplus_test.go:516-571) ending in ToCsv, every step in HBM: cph_index_build, cph_index_aggregate, the key columns read
    through the groups' first rows inside the writer, the count and the int64 results as computed columns (mapping.Int).
    by: key column names.  specs: aggregate.Sum / Min / Max whose source is a column NAME of the table, a StrCol, or numbers
    (see csvplus_amd.aggregate).  names: the header of the count column and of every spec's column (default "count",
    "sum0", "min1", ...); the key columns keep their names.  One output row per distinct key, in key order.
    Float results are refused: formatting float64 (Go's shortest round-trip FormatFloat) is out of scope, as for Map.
    order_by: ordering.Asc / ordering.Desc over a NAME — the count column's or a spec's column's name (see `names`), or "by"
    for the key order — .OrderBy(keys).Top(limit) over the groups, sorted on the device (materialize.order_rows): "the ten
    customers with the largest amount".  None (default): key order, every group.
    Returns bytes, or a DeviceBytes handle for out_mem DEVICE."""
    from . import aggregate as A
    from . import mapping as M
    from .materialize import csv_write, map_column

    by = [str(b) for b in by]
    specs = list(specs)
    for sp in specs:
        if not isinstance(sp, A.Spec):
            raise TypeError(f"not an aggregate: {sp!r}")
        if sp.kind == N.CPH_NUM_FLOAT64:
            raise ValueError("totals_to_csv: a float64 result cannot be written (formatting float64 is out of scope); "
                             "use aggregate.totals and format the values on the host")
    if names is None:
        names = ["count"] + [f"{sp.name}{i}" for i, sp in enumerate(specs)]
    if len(names) != 1 + len(specs):
        raise ValueError(f"totals_to_csv: {1 + len(specs)} computed columns but {len(names)} names")
    for b in by:
        if b not in table.cols:
            raise M.MissingColumn(b)
    resolved = []
    for sp in specs:
        if isinstance(sp.source, str):
            if sp.source not in table.cols:
                raise M.MissingColumn(sp.source)
            sp = type(sp)(table.cols[sp.source], sp.kind_name)
        resolved.append(sp)
    index = N.DeviceIndex(ctx, [table.cols[b] for b in by])
    bufs, t = [], None
    try:
        t = A.totals(index, resolved, out_mem=N.CPH_MEM_DEVICE)
        ng = t.ngroups
        cols = [table.cols[b] for b in by]
        ids = [(t.first_row[0], 32, ng) for _ in by]
        for ptr, _ in [t.count] + t.values:   # count[g] < 2^32: the uint64 reads as the same int64
            cb = map_column(ctx, {}, M.Format(M.Int.on_device(ptr, ng)), nrows=ng, out_mem=N.CPH_MEM_DEVICE)
            bufs.append(cb)
            cols.append(cb.as_device_strcol())
            ids.append(None)
        header = by + [str(nm) for nm in names]
        if order_by is None and limit is None:
            return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=ids, nrows=ng)
        return _ordered_groups_to_csv(ctx, t, cols, len(by), header, [str(nm) for nm in names], resolved, order_by, limit, out_mem)
    finally:
        for cb in bufs:
            cb.release()
        if t is not None:
            t.release()
        index.close()


def _ordered_groups_to_csv(ctx, t, cols, nby, header, names, specs, order_by, limit, out_mem):
    """totals_to_csv with order_by / limit: the groups of `t` (device) in the order of the keys, cut to `limit`.  cols = the
    table's key columns (read through the groups' first rows) followed by the computed columns (one row per group)."""
    import numpy as np

    from . import ordering as O
    from .materialize import csv_write, order_rows, take_rows

    ng = t.ngroups
    keys = []
    for key in ([O.Asc("by")] if order_by is None else list(order_by)):
        if not isinstance(key, O.OrderKey) or not isinstance(key.source, str):
            raise TypeError(f"totals_to_csv: an order key is Asc / Desc over a name, not {key!r}")
        if key.source == "by" and "by" not in names:   # the groups are in key order: a group's number is its key's rank
            keys.append(type(key)(np.arange(ng, dtype=np.int64), "int"))
        elif key.source in names:
            j = names.index(key.source)   # 0: the count (below 2^32: the uint64 reads as the same int64)
            keys.append(type(key)(t.count if j == 0 else t.values[j - 1], "int" if j == 0 else specs[j - 1].kind_name))
        else:
            raise ValueError(f"totals_to_csv: order_by names {key.source!r}; the names are {names + ['by']}")
    if not keys:
        raise ValueError("totals_to_csv: order_by needs at least one key")
    if ng == 0:
        return csv_write(ctx, [c.head(0) for c in cols], header, out_mem=out_mem)
    ordered = order_rows(ctx, keys, ng, limit=limit, out_mem=N.CPH_MEM_DEVICE)
    first = None
    try:
        m = len(ordered)
        if m == 0:
            return csv_write(ctx, [c.head(0) for c in cols], header, out_mem=out_mem)
        first = take_rows(ctx, (t.first_row[0], 32, ng), ordered, out_mem=N.CPH_MEM_DEVICE)   # table rows of the groups, in output order
        ids = [first.as_row_ids()] * nby + [ordered.as_row_ids()] * (len(cols) - nby)
        return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=ids, nrows=m)
    finally:
        if first is not None:
            first.release()
        ordered.release()


def join_totals_to_csv(ctx: N.Context, stream_table: Table, build_table: Table, on, specs, names=None, out_mem: int = N.CPH_MEM_HOST,
                       matched_only: bool = False, prec: int = 2):
    """stream.Join(UniqueIndexOn(build, key)) and then Count and the specs per BUILD ROW over the joined rows, written as CSV —
    the reference's TestSimpleUniqueJoin / TestTransformedSource loops (`custAmounts[cid] += amount`, csvplus_test.go:368-452,
    :754-806) ending in ToCsv, every step in HBM: cph_index_build (unique), cph_join_chain_ex with positions,
    cph_chain_aggregate, then the build table's columns read through cph_index_perm inside the writer, the count and the int64
    results as computed columns (mapping.Int), the float64 results through mapping.Float with `prec` digits.
    on: the key column's name in both tables, or (build key, stream key).  specs: aggregate.Sum / Min / Max whose source is an
    expression of csvplus_amd.expr over the JOINED row (a name is looked up in the stream table first, then in the build
    table: mergeRows lets the stream's value win) or one value per joined row (see aggregate.join_totals).  names: the header
    of the count column and of every spec's column (default "count", "sum0", "min1", ...); the build columns keep theirs.
    One output row per build row in key order; matched_only=True drops the build rows no stream row matched (count 0): what
    the reference's inner Join would show.  Returns bytes, or a DeviceBytes handle for out_mem DEVICE."""
    from . import aggregate as A
    from . import expr as E
    from . import mapping as M
    from . import predicates as P
    from .materialize import csv_write, filter_rows, map_column, permute_col, take_rows

    bkey, skey = (on, on) if isinstance(on, str) else (str(on[0]), str(on[1]))
    specs = list(specs)
    for sp in specs:
        if not isinstance(sp, A.Spec):
            raise TypeError(f"not an aggregate: {sp!r}")
    if names is None:
        names = ["count"] + [f"{sp.name}{i}" for i, sp in enumerate(specs)]
    if len(names) != 1 + len(specs):
        raise ValueError(f"join_totals_to_csv: {1 + len(specs)} computed columns but {len(names)} names")
    if bkey not in build_table.cols:
        raise M.MissingColumn(bkey)
    if skey not in stream_table.cols:
        raise M.MissingColumn(skey)
    index = N.DeviceIndex(ctx, [build_table[bkey]], unique=True)
    bufs, t, ch, kept = [], None, None, None
    try:
        if index.status == N.CPH_ERR_DUPLICATE:
            raise ValueError(f"duplicate value while creating unique index on {bkey!r} (sorted position {index.first_dup})")
        ch = N.join_chain(ctx, [(index, [stream_table[skey]])], out_mem=N.CPH_MEM_DEVICE, positions=True)
        columns = {}
        for sp in specs:
            if not isinstance(sp.source, E.Expr):
                continue
            for name in E.columns(sp.source):
                if name in columns:
                    continue
                if name in stream_table.cols:
                    columns[name] = stream_table[name]
                elif name in build_table.cols:   # positions: the build column in index order
                    cb = permute_col(ctx, index, build_table[name])
                    bufs.append(cb)
                    columns[name] = (cb.as_device_strcol(), 0)
        t = A.join_totals(ch, 0, index, specs, out_mem=N.CPH_MEM_DEVICE, columns=columns)
        ng = t.ngroups
        computed = []
        for sp, (ptr, _) in zip([None] + specs, [t.count] + t.values):   # count[g] < 2^32: the uint64 reads as the same int64
            if sp is not None and sp.kind == N.CPH_NUM_FLOAT64:
                part = M.Float.on_device(ptr, ng, prec)
            else:
                part = M.Int.on_device(ptr, ng)
            cb = map_column(ctx, {}, M.Format(part), nrows=ng, out_mem=N.CPH_MEM_DEVICE)
            bufs.append(cb)
            computed.append(cb.as_device_strcol())
        bnames = list(build_table.cols)
        cols = [build_table[b] for b in bnames] + computed
        header = bnames + [str(nm) for nm in names]
        perm_ids = (index.perm_device_ptr(), 32, ng)
        if not matched_only:
            return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=[perm_ids] * len(bnames) + [None] * len(computed), nrows=ng)
        kept = filter_rows(ctx, {"count": computed[0]}, P.IntCmp("count", ">", 0), nrows=ng, out_mem=N.CPH_MEM_DEVICE)
        nk = len(kept)
        if kept.is_range and nk:   # every row kept: as an array, like any other answer
            rng = filter_rows(ctx, {"count": computed[0]}, P.All(), nrows=nk, first_row=kept.first, out_mem=N.CPH_MEM_DEVICE)
            kept.release()
            kept = rng
        if nk == 0:
            return csv_write(ctx, cols, header, out_mem=out_mem, row_ids=[perm_ids] * len(bnames) + [None] * len(computed), nrows=0)
        rows = take_rows(ctx, perm_ids, kept, out_mem=N.CPH_MEM_DEVICE)
        bufs.append(rows)
        return csv_write(ctx, cols, header, out_mem=out_mem,
                         row_ids=[rows.as_row_ids()] * len(bnames) + [kept.as_row_ids()] * len(computed), nrows=nk)
    finally:
        for cb in bufs:
            cb.release()
        if kept is not None:
            kept.release()
        if t is not None:
            t.release()
        if ch is not None:
            ch.release()
        index.close()
