"""The step after the path: gathering columns through the joined row ids and writing the
canonical CSV or JSON (cph_gather_rows / cph_csv_write / cph_json_write_rows; mergeRows csvplus.go:571-583,
ToCsv :379-406, ToJSON :446-480), filtering rows (cph_filter_rows), converting a column to numbers
(cph_col_to_number; ValueAsInt / ValueAsFloat64 :165-205), evaluating a numeric expression per row (cph_num_eval:
`price * float64(qty)`, csvplus_test.go:516-571) and computing a column from a row template (cph_map_format;
Map :290-296, Validate :300-310) or from the template of the first case that holds (cph_map_switch)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .columns import StrCol


def gather_rows(ctx: N.Context, col: StrCol, row_ids=None, id_base: int = 0, out_mem: int = N.CPH_MEM_HOST):
    """out[i] = col[row_ids[i] - id_base].  Host columns take numpy uint32/uint64 ids; device columns take
    (device_ptr, bits, count).  Returns a host StrCol (out_mem HOST) or a ColBuf handle (DEVICE)."""
    sc, keep = N._cols_array([col])
    ptr, bits, n = C.c_void_p(0), 32, 0
    if row_ids is not None:
        if isinstance(row_ids, np.ndarray):
            if row_ids.dtype != np.uint64:
                row_ids = row_ids.astype(np.uint32)
            row_ids = np.ascontiguousarray(row_ids)
            ptr, bits, n = C.c_void_p(row_ids.ctypes.data), row_ids.dtype.itemsize * 8, len(row_ids)
        else:
            ptr, bits, n = C.c_void_p(row_ids[0]), int(row_ids[1]), int(row_ids[2])
    out = C.POINTER(N.cph_colbuf)()
    ctx._check(ctx.lib.cph_gather_rows(ctx.handle, sc, ptr, bits, id_base, n, out_mem, C.byref(out)))
    del keep
    cb = ColBuf(ctx, out)
    return cb.taken(ColBuf.to_strcol) if out_mem == N.CPH_MEM_HOST else cb


def permute_col(ctx: N.Context, index, col: StrCol, out_mem: int = N.CPH_MEM_DEVICE):
    """cph_index_permute: `col` (a column of the table `index` was built over) in index order — out[p] = col[perm[p]] — so
    that the sorted positions a Join reports are row subscripts (csvplus.go:736: the reference keeps its index rows
    sorted).  Returns a ColBuf (DEVICE) or a host StrCol."""
    sc, keep = N._cols_array([col])
    out = C.POINTER(N.cph_colbuf)()
    ctx._check(ctx.lib.cph_index_permute(ctx.handle, index.handle, sc, out_mem, C.byref(out)))
    del keep
    cb = ColBuf(ctx, out)
    return cb.taken(ColBuf.to_strcol) if out_mem == N.CPH_MEM_HOST else cb


class ColBuf(N.Owned):
    _release_fn = "cph_colbuf_release"

    def __init__(self, ctx, ptr):
        super().__init__(ctx, ptr)
        c = ptr.contents
        self.nrows, self.nbytes, self.mem = int(c.col.nrows), int(c.nbytes), int(c.col.mem)

    def to_strcol(self) -> StrCol:
        assert self.mem == N.CPH_MEM_HOST
        c = self.ptr.contents.col
        offs = N._ptr_array(c.offsets, self.nrows + 1, np.uint64).copy()
        data = N._ptr_array(c.data, self.nbytes, np.uint8).copy()
        return StrCol(data, offs, self.nrows, 64)

    def as_device_strcol(self) -> StrCol:
        """Zero-copy device StrCol view (valid until release)."""
        assert self.mem == N.CPH_MEM_DEVICE
        c = self.ptr.contents.col
        return StrCol(N._Raw(c.data), N._Raw(c.offsets), self.nrows, 64, N.CPH_MEM_DEVICE, fixed_width=0)


class DeviceBytes(N.Owned):
    """cph_bytes kept in HBM (valid until release())."""
    _release_fn = "cph_bytes_release"

    def __init__(self, ctx, ptr):
        super().__init__(ctx, ptr)
        self.size, self.data_ptr = int(ptr.contents.size), int(ptr.contents.data or 0)

    def __len__(self):
        return self.size


def _rowsel(cols, row_ids, nrows, keep):
    """cph_strcol array, cph_rowsel array (None without row_ids) and the row count of a writer call (csv_write / json_write)."""
    arr = N.cols_array(cols, keep)
    sel = None
    n = cols[0].nrows if nrows is None else int(nrows)
    if row_ids is not None:
        sel = (N.cph_rowsel * len(cols))()
        for i, ids in enumerate(row_ids):
            if ids is None:
                continue
            cnt = N.fill_rowsel(sel[i], ids, keep)
            if nrows is None:
                n = cnt
    return arr, sel, n


def _strvals(names, size, keep):
    hv = (N.cph_strval * size)()
    for i, h in enumerate(names):
        b = np.frombuffer(h.encode() if isinstance(h, str) else bytes(h), dtype=np.uint8)
        keep.append(b)
        hv[i].data = b.ctypes.data if len(b) else None
        hv[i].len = len(b)
    return hv


def _take_bytes(ctx, out, out_mem):
    db = DeviceBytes(ctx, out)
    if out_mem == N.CPH_MEM_DEVICE:
        return db
    return db.taken(lambda b: N._ptr_array(b.data_ptr, b.size, np.uint8).tobytes())


def csv_write(ctx: N.Context, cols, header=None, out_mem: int = N.CPH_MEM_HOST, row_ids=None, nrows=None):
    """ToCsv: header (list of names or None) + rows of `cols`, Go csv.Writer format.
    row_ids (optional, one entry per column): None = the column's own rows, else the rows of that column feeding
    the output (numpy uint32/uint64 for host columns, (device_ptr, bits, count[, base]) for device columns) —
    Join(...).ToCsv(...) fused: mergeRows happens inside the writer (cph_csv_write_rows).
    Returns bytes (out_mem HOST) or a DeviceBytes handle (DEVICE)."""
    keep = []
    arr, sel, n = _rowsel(cols, row_ids, nrows, keep)
    hv = _strvals(header, len(cols), keep) if header is not None else None
    out = C.POINTER(N.cph_bytes)()
    ctx._check(ctx.lib.cph_csv_write_rows(ctx.handle, arr, sel, len(cols), n, hv, out_mem, C.byref(out)))
    return _take_bytes(ctx, out, out_mem)


def json_write(ctx: N.Context, cols, names, out_mem: int = N.CPH_MEM_HOST, row_ids=None, nrows=None):
    """ToJSON (csvplus.go:446-480): the rows of `cols` as a JSON array of objects keyed by `names` (str or bytes, one per
    column, all different), written as the reference's json.Encoder does — keys in byte order, '\\n' after every object,
    no HTML escaping (cph_json_write_rows).  row_ids and nrows as in csv_write.
    Returns bytes (out_mem HOST) or a DeviceBytes handle (DEVICE)."""
    if len(names) != len(cols):
        raise ValueError(f"json_write: {len(cols)} columns but {len(names)} names")
    keep = []
    arr, sel, n = _rowsel(cols, row_ids, nrows, keep)
    hv = _strvals(names, len(cols), keep)
    out = C.POINTER(N.cph_bytes)()
    ctx._check(ctx.lib.cph_json_write_rows(ctx.handle, arr, sel, hv, len(cols), n, out_mem, C.byref(out)))
    return _take_bytes(ctx, out, out_mem)


# ---- Filter / TakeWhile / DropWhile / Top / Drop (cph_filter_rows, cph_rowsel_take) -----------------------------------

_MODES = {"where": N.CPH_FILTER_WHERE, "take_while": N.CPH_FILTER_TAKE_WHILE, "drop_while": N.CPH_FILTER_DROP_WHILE}


class RowList(N.Owned):
    """cph_rowlist: an ascending list of row numbers (valid until release()).  A range (the WHILE modes, or an empty
    result) has no array behind it: `ids_ptr` is 0 and the rows are first, first + 1, ..."""
    _release_fn = "cph_rowlist_release"

    def __init__(self, ctx, ptr):
        super().__init__(ctx, ptr)
        c = ptr.contents
        self.nrows, self.first, self.bits, self.mem = int(c.nrows), int(c.first), int(c.bits), int(c.mem)
        self.ids_ptr = int(c.ids or 0)
        self.is_range = self.ids_ptr == 0

    def __len__(self):
        return self.nrows

    def to_numpy(self) -> np.ndarray:
        """The row numbers on the host (a copy): only for lists in host memory and ranges."""
        dt = np.uint32 if self.bits == 32 else np.uint64
        if self.is_range:
            return (np.arange(self.nrows, dtype=np.uint64) + np.uint64(self.first)).astype(dt)
        assert self.mem == N.CPH_MEM_HOST, "a device row list has no host view: consume it on the device"
        return N._ptr_array(self.ids_ptr, self.nrows, dt).copy()

    def as_row_ids(self):
        """(device_ptr, bits, count): the tuple csv_write / json_write / gather_rows take as row ids of a device column."""
        assert self.mem == N.CPH_MEM_DEVICE and not self.is_range, "a range has no array: use first / nrows"
        return (self.ids_ptr, self.bits, self.nrows)


def _expr_program(ops, keep):
    """The cph_expr_op array of expr.compile's ops."""
    from . import expr as E

    prog = (N.cph_expr_op * max(len(ops), 1))()
    for k, (op, arg, value) in enumerate(ops):
        prog[k].op, prog[k].arg = op, arg
        if op == E.LIT_INT:
            prog[k].lit.i = value
        elif op == E.LIT_FLT:
            prog[k].lit.f = value
    keep.append(prog)
    return prog


def _expr_nums(arrs, need, who, keep):
    """The cph_expr_nums array of an expression's IntArr / FloatArr leaves (expr.arrays): host arrays are passed as they
    are, device arrays by pointer; every array has at least `need` values."""
    nums = (N.cph_expr_nums * max(len(arrs), 1))()
    for k, a in enumerate(arrs):
        kind = N.CPH_NUM_INT64 if a.dtype is np.int64 else N.CPH_NUM_FLOAT64
        nums[k].ptr, nums[k].mem = N.number_source(a, kind, need, who, keep)
    keep.append(nums)
    return nums if arrs else None


def _pred_expr(eops, arrs, need, keep):
    """One cph_pred_expr for an expression term; its arrays have an entry for each of the `need` positions of the
    selection the call can look at."""
    nums = _expr_nums(arrs, need, "filter_rows: {src!r} has {count} values for positions 0..{last} of the selection", keep)
    pe = N.cph_pred_expr(_expr_program(eops, keep), len(eops), len(arrs), nums)
    keep.append(pe)
    return pe


def _pred_program(ops, keep, need=0):
    """The cph_pred_op array of predicates.compile's ops; need = first_row + nrows of the call (an expression term's arrays)."""
    from . import predicates as P

    arr = (N.cph_pred_op * max(len(ops), 1))()
    for i, (op, arg, value) in enumerate(ops):
        arr[i].op, arr[i].arg = int(op), int(arg)
        if P._is_expr_op(op):
            if arg >= 0:
                pe = _pred_expr(value[0], value[1], need, keep)
                arr[i].value.data, arr[i].value.len = C.addressof(pe), C.sizeof(pe)
        elif P._is_cols_op(op):
            b = np.array([value], dtype=np.int32)
            keep.append(b)
            arr[i].value.data, arr[i].value.len = b.ctypes.data, 4
        elif value is not None:
            b = np.frombuffer(bytes(value), dtype=np.uint8)
            keep.append(b)
            arr[i].value.data = b.ctypes.data if len(b) else None
            arr[i].value.len = len(b)
    return arr


def filter_rows(ctx: N.Context, cols_by_name, pred, row_ids=None, nrows=None, mode: str = "where", first_row: int = 0,
                skip: int = 0, limit=None, out_bits=None, out_mem: int = N.CPH_MEM_HOST, as_handle: bool = False):
    """Filter(pred) / TakeWhile / DropWhile with Drop and Top on either side, evaluated on the device (cph_filter_rows).

    cols_by_name: {column name: StrCol} — the row the predicate sees; a name the predicate uses and the mapping lacks
    makes its Like false (csvplus.go:1286).  row_ids: {name: ids} (numpy uint32 / uint64, or (numpy ids, base), for host
    columns; (device_ptr, bits, count[, base]) for device columns) for columns read through row ids, e.g. a Join's; nrows = the rows of the
    selection to look at, counted from first_row (default: all behind first_row).  mode: "where", "take_while",
    "drop_while"; skip / limit: Drop / Top behind the filter.  out_bits defaults to 32 when the rows fit.

    Returns the row numbers (positions in the selection) as a numpy array (out_mem HOST) or a RowList handle (DEVICE, or
    as_handle=True)."""
    from . import predicates as P

    names, ops = P.compile(pred, list(cols_by_name))
    cols = [cols_by_name[nm] for nm in names]
    ids = None if row_ids is None else [row_ids.get(nm) for nm in names]
    keep = []
    if cols:
        arr, sel, total = _rowsel(cols, ids, None, keep)
    else:
        arr, sel, total = None, None, 0
        if nrows is None and cols_by_name:
            total = min(c.nrows for c in cols_by_name.values())
    n = max(total - first_row, 0) if nrows is None else int(nrows)
    if out_bits is None:
        out_bits = 32 if first_row + n <= 0xFFFFFFFF else 64
    opts = N.cph_filter_opts(_MODES[mode], int(out_bits), int(first_row), int(skip), N.CPH_NO_LIMIT if limit is None else int(limit))
    prog = _pred_program(ops, keep, first_row + n)
    out = C.POINTER(N.cph_rowlist)()
    ctx._check(ctx.lib.cph_filter_rows(ctx.handle, arr, sel, len(cols), n, prog, len(ops), C.byref(opts), out_mem, C.byref(out)))
    del keep
    return _take_rowlist(ctx, out, out_mem, as_handle)


def _take_rowlist(ctx, out, out_mem, as_handle):
    rl = RowList(ctx, out)
    return rl if out_mem == N.CPH_MEM_DEVICE or as_handle else rl.taken(RowList.to_numpy)


def take_rows(ctx: N.Context, row_ids, rows, out_mem: int = N.CPH_MEM_HOST, as_handle: bool = False):
    """out[i] = row_ids[rows[i]] - base (cph_rowsel_take): the row ids of a Join narrowed to the rows a Filter kept.
    row_ids: numpy uint32 / uint64 or (numpy ids, base) (host), (device_ptr, bits, count[, base]) (device), or None
    (identity: a copy of `rows`).  rows: a RowList, an Ordered (order_rows), or a numpy uint32 / uint64 array.  Returns numpy (HOST) or a RowList (DEVICE / as_handle)."""
    keep = []
    sel, sel_mem = None, N.CPH_MEM_HOST
    if row_ids is not None:
        sel = N.cph_rowsel()
        N.fill_rowsel(sel, row_ids, keep)
        sel_mem = N.CPH_MEM_HOST if keep else N.CPH_MEM_DEVICE   # only a host form keeps an array
    if isinstance(rows, RowList):
        lst = rows.ptr
    elif isinstance(rows, Ordered):   # an ordered list is a list of row numbers like any other
        rl = N.cph_rowlist(rows.nrows, 0, rows.ids_ptr or None, 32, rows.mem)
        keep.append(rl)
        lst = C.pointer(rl)
    else:
        a = np.asarray(rows)
        if a.dtype != np.uint64:
            a = a.astype(np.uint32)
        a = np.ascontiguousarray(a)
        keep.append(a)
        rl = N.cph_rowlist(len(a), 0, a.ctypes.data if len(a) else None, a.dtype.itemsize * 8, N.CPH_MEM_HOST)
        keep.append(rl)
        lst = C.pointer(rl)
    out = C.POINTER(N.cph_rowlist)()
    ctx._check(ctx.lib.cph_rowsel_take(ctx.handle, C.byref(sel) if sel is not None else None, sel_mem, lst, out_mem, C.byref(out)))
    del keep
    return _take_rowlist(ctx, out, out_mem, as_handle)


# ---- ValueAsInt / ValueAsFloat64 for a whole column (cph_col_to_number) -------------------------------------------------

class NumCol(N.Owned):
    """cph_numcol: a column as int64 / float64 (valid until release()).  `values` and `status` are numpy arrays (copies)
    for a host result and (device_ptr, count) pairs for a device result; status holds CPH_NUM_* per row, and at an error
    row `values` holds what Go returns beside the error.  first_error_row is None when nerrors == 0."""
    _release_fn = "cph_numcol_release"

    def __init__(self, ctx, ptr):
        super().__init__(ctx, ptr)
        c = ptr.contents
        self.nrows, self.kind, self.mem = int(c.nrows), int(c.kind), int(c.mem)
        self.nerrors, self.host_rows = int(c.nerrors), int(c.host_rows)
        self.first_error_row = None if int(c.first_error_row) == N.CPH_NO_ROW else int(c.first_error_row)
        self.first_error_kind = int(c.first_error_kind)
        dt = np.float64 if self.kind == N.CPH_NUM_FLOAT64 else np.int64   # INT64 and the two TIME kinds
        self.values = N.result_array(c.values, self.nrows, dt, self.mem)
        self.status = N.result_array(c.status, self.nrows, np.uint8, self.mem)
        if self.mem == N.CPH_MEM_HOST:
            self.release()   # the arrays are copies

    def __len__(self):
        return self.nrows


def _to_number(ctx, col, row_ids, nrows, kind, out_mem):
    keep = []
    arr, sel, n = _rowsel([col], None if row_ids is None else [row_ids], nrows, keep)
    out = C.POINTER(N.cph_numcol)()
    ctx._check(ctx.lib.cph_col_to_number(ctx.handle, arr, sel, n, kind, out_mem, C.byref(out)))
    del keep
    return NumCol(ctx, out)


def to_int(ctx: N.Context, col: StrCol, row_ids=None, nrows=None, out_mem: int = N.CPH_MEM_HOST):
    """Row.ValueAsInt (csvplus.go:165-183) for every row of `col`: strconv.Atoi on the device.  row_ids / nrows as in
    csv_write (numpy uint32 / uint64 or (numpy ids, base) for a host column, (device_ptr, bits, count[, base]) for a
    device column).  A conversion error is data: see NumCol (nerrors, first_error_row, first_error_kind, status) and
    predicates.conversion_error for the reference's message."""
    return _to_number(ctx, col, row_ids, nrows, N.CPH_NUM_INT64, out_mem)


def to_float(ctx: N.Context, col: StrCol, row_ids=None, nrows=None, out_mem: int = N.CPH_MEM_HOST):
    """Row.ValueAsFloat64 (csvplus.go:187-205): strconv.ParseFloat(s, 64), correctly rounded.  `host_rows` of the result
    counts the rows the device deferred to the library's host side: by default every valid value outside Clinger's exact
    cases (a mantissa of 2^53 or more — anything with 17 significant digits —, 19+ digits, a decimal exponent outside
    -22..37).  After ctx.set_option("float_device", 1) the device converts those too (Eisel-Lemire) and defers only what
    that cannot decide: a fraction of a per cent of the values with non-zero digits behind the 19th, and no others.  The
    values, status bytes and error report are the same either way."""
    return _to_number(ctx, col, row_ids, nrows, N.CPH_NUM_FLOAT64, out_mem)


def to_time(ctx: N.Context, col: StrCol, row_ids=None, nrows=None, unit: str = "s", out_mem: int = N.CPH_MEM_HOST):
    """`t, err := time.Parse(time.RFC3339, row[col])` for every row, on the device: a NumCol of int64 like to_int's, holding
    t.Unix() (unit "s": whole seconds since 1970-01-01T00:00:00Z, the floor) or t.UnixNano() (unit "ns").  The accepted set
    is the strict RFC 3339 profile stated in include/csvplus_hip.h; csvplus_amd.timeconv.parse_model is the host model.  A row
    that does not convert is data (status, nerrors, first_error_row, first_error_kind), its value 0; host_rows is always 0.
    row_ids / nrows as in to_int."""
    if unit not in ("s", "ns"):
        raise ValueError(f"to_time: unit must be 's' or 'ns', not {unit!r}")
    return _to_number(ctx, col, row_ids, nrows, N.CPH_NUM_TIME_UNIX if unit == "s" else N.CPH_NUM_TIME_UNIXNANO, out_mem)


# ---- numeric expressions per row (cph_num_eval) ---------------------------------------------------------------------------

def eval_number(ctx: N.Context, cols_by_name, expr, row_ids=None, nrows=None, out_mem: int = N.CPH_MEM_HOST) -> NumCol:
    """An expression of csvplus_amd.expr — `FloatCol("price") * ToFloat(IntCol("qty"))` — for every row, on the device
    (cph_num_eval): one kernel parses the string leaves and does the arithmetic with Go's rules.  cols_by_name: {column
    name: StrCol}, the row the expression sees (a name it lacks raises mapping.MissingColumn); row_ids: {name: ids} as in
    filter_rows, for columns read through row ids (a Join's); nrows: the number of rows (default: what the columns, the row
    ids or the arrays give).  An IntArr / FloatArr leaf is indexed by OUTPUT row.

    Returns a NumCol of the expression's type.  A failing row is data — status per row, nerrors, first_error_row,
    first_error_kind and `first_error_op`, the index (into expr.compile's ops) of the op that failed there, None without
    errors; raise_expr_error turns it into the reference's message."""
    from . import expr as E

    names, ops = E.compile(expr, list(cols_by_name))
    cols = [cols_by_name[nm] for nm in names]
    ids = None if row_ids is None else [row_ids.get(nm) for nm in names]
    arrs = E.arrays(ops)
    keep = []
    if cols:
        arr, sel, n = _rowsel(cols, ids, nrows, keep)
    else:
        arr, sel = None, None
        if nrows is not None:
            n = int(nrows)
        elif arrs:
            n = min(a.count for a in arrs)
        else:
            raise ValueError("eval_number: an expression without columns and arrays needs nrows")
    nums = _expr_nums(arrs, n, "eval_number: {src!r} has {count} values for {need} rows", keep)
    prog = _expr_program(ops, keep)
    out = C.POINTER(N.cph_numcol)()
    eop = C.c_int32(-1)
    ctx._check(ctx.lib.cph_num_eval(ctx.handle, arr, sel, len(cols), n, nums, len(arrs), prog, len(ops), out_mem,
                                    C.byref(out), C.byref(eop)))
    del keep
    res = NumCol(ctx, out)
    res.first_error_op = None if eop.value < 0 else int(eop.value)
    return res


def _value_at(ctx, col: StrCol, ids, row: int) -> bytes:
    """The value of `col` that feeds output row `row` (ids: the column's row ids as the writers take them, or None)."""
    one = np.array([row], dtype=np.uint64)
    if col.mem == N.CPH_MEM_HOST:
        src = take_rows(ctx, ids, one)
        return gather_rows(ctx, col, np.asarray(src, dtype=np.uint64)).value(0)
    rl = take_rows(ctx, ids, one, out_mem=N.CPH_MEM_DEVICE)
    try:
        return gather_rows(ctx, col, rl.as_row_ids()).value(0)
    finally:
        rl.release()


def raise_expr_error(ctx, cols_by_name, expr, numcol, row_ids=None):
    """Raises expr.ExprError for the lowest failing row of an eval_number result: the reference's conversion error with the
    column named and the value quoted for a leaf that does not convert (csvplus.go:176, :198), a plain statement for a zero
    divisor or a ToInt out of range."""
    from . import expr as E

    names, ops = E.compile(expr, list(cols_by_name))
    row, op, kind = numcol.first_error_row, numcol.first_error_op, numcol.first_error_kind
    column, values = None, {}
    if ops[op][0] in (E.COL_INT, E.COL_FLT):
        column = names[ops[op][1]]
        values[column] = _value_at(ctx, cols_by_name[column], None if row_ids is None else row_ids.get(column), row)
    # error_text compiles against the expression's own columns: the op index is the same (names are numbered by first use)
    raise E.ExprError(row, op, kind, column, E.error_text(expr, values, kind, op), numcol.nerrors)


# ---- Map with a row template / Validate (cph_map_format; cph_filter_rows in TAKE_WHILE mode) ------------------------------

def map_column(ctx: N.Context, cols_by_name, template, row_ids=None, nrows=None, out_mem: int = N.CPH_MEM_HOST):
    """Map(row[new] = template(row)) for every row, on the device (cph_map_format): returns the NEW column as a ColBuf
    (valid until release(); to_strcol() for a host result, as_device_strcol() for a device one).

    cols_by_name: {column name: StrCol} — the row the template sees; a Col whose name the mapping lacks becomes its default
    or raises mapping.MissingColumn.  template: mapping.Format / Const (or a bare part), or a mapping.Switch / When, which
    goes to map_switch.  row_ids: {name: ids} as in
    filter_rows, for columns read through row ids (a Join's); nrows: the number of rows (default: what the columns, the row
    ids or the Int / Float parts give).  An Int or Float part's array is indexed by OUTPUT row and lives on the host (numpy) or
    on the device (Int.on_device, Float.on_device); an Int.of / Float.of part's expression is evaluated over the same rows
    on the device (eval_number) and a row where it fails raises expr.ExprError."""
    from . import mapping as M

    if isinstance(template, M.Switch):
        return map_switch(ctx, cols_by_name, template, row_ids=row_ids, nrows=nrows, out_mem=out_mem)[0]
    names, pieces = M.compile(template, list(cols_by_name))
    keep = []
    arr, sel, n = _map_rows(cols_by_name, row_ids, nrows, names, pieces, keep, "map_column: a template")
    computed = []   # the expressions' results, on the device until the template has run
    try:
        parr = _fill_pieces(ctx, cols_by_name, row_ids, pieces, n, keep, computed)
        out = C.POINTER(N.cph_colbuf)()
        ctx._check(ctx.lib.cph_map_format(ctx.handle, arr, sel, len(names), n, parr, len(pieces), out_mem, C.byref(out)))
        del keep
        return ColBuf(ctx, out)
    finally:
        for nc in computed:
            nc.release()


def _map_rows(cols_by_name, row_ids, nrows, names, pieces, keep, who):
    """cph_strcol array, cph_rowsel array and row count of a Map call over the columns `names`; without columns the rows
    come from nrows, an expression's columns, the Int / Float arrays or the mapping's columns, in that order."""
    from . import mapping as M

    cols = [cols_by_name[nm] for nm in names]
    ids = None if row_ids is None else [row_ids.get(nm) for nm in names]
    if cols:
        return _rowsel(cols, ids, nrows, keep)
    exprs = [p[2].expr for p in pieces if p[0] in (M.INT64, M.FLOAT64, M.FLOAT64_SHORTEST, M.TIME) and p[2].expr is not None]
    counts = [p[2].count for p in pieces if p[0] in (M.INT64, M.FLOAT64, M.FLOAT64_SHORTEST, M.TIME) and p[2].expr is None]
    from . import expr as E
    ecols = [nm for e in exprs for nm in E.columns(e) if nm in cols_by_name]
    if nrows is not None:
        n = int(nrows)
    elif ecols:   # the rows an expression's columns give
        n = _rowsel([cols_by_name[nm] for nm in ecols], None if row_ids is None else [row_ids.get(nm) for nm in ecols], None, [])[2]
    elif counts:
        n = min(counts)
    elif cols_by_name:
        n = min(c.nrows for c in cols_by_name.values())
    else:
        raise ValueError(f"{who} without columns and Int / Float parts needs nrows")
    return None, None, n


def _fill_pieces(ctx, cols_by_name, row_ids, pieces, n, keep, computed, pending=None, tag=None):
    """The cph_map_piece array of `pieces` (mapping.compile); a SPAN piece's operations become a cph_span_op array.  An Int.of / Float.of part is evaluated over the n rows into a
    device array (cph_num_eval, appended to `computed`).  A failing row raises expr.ExprError at once — or, with a `pending`
    list, the part is evaluated again into host memory and (tag, expression, NumCol with host status) is appended, for a
    caller that decides per row whether the failure counts."""
    from . import mapping as M

    parr = (N.cph_map_piece * len(pieces))()
    for k, (kind, arg, value) in enumerate(pieces):
        parr[k].kind = kind
        if kind == M.LITERAL:
            b = np.frombuffer(value, dtype=np.uint8)
            keep.append(b)
            parr[k].value.data = b.ctypes.data if len(b) else None
            parr[k].value.len = len(b)
        elif kind == M.COLUMN:
            parr[k].arg = arg
        elif kind == M.SLICE:   # value: a cph_map_slice {from, to}, 16 bytes
            b = np.array(value, dtype=np.int64)
            keep.append(b)
            parr[k].arg = arg
            parr[k].value.data = b.ctypes.data
            parr[k].value.len = 16
        elif kind == M.SPAN:   # value: the operations, one cph_span_op each
            ops = (N.cph_span_op * len(value))()
            for q, (op, mode, a, b, lit) in enumerate(value):
                ops[q].op, ops[q].mode, ops[q].a, ops[q].b = op, mode, a, b
                lb = np.frombuffer(lit, dtype=np.uint8)
                keep.append(lb)
                ops[q].lit.data = lb.ctypes.data if len(lb) else None
                ops[q].lit.len = len(lb)
            keep.append(ops)
            parr[k].arg = arg
            parr[k].value.data = C.addressof(ops)
            parr[k].value.len = C.sizeof(ops)
        else:
            src = value
            if value.expr is not None:   # evaluated over the same rows into a device array: cph_num_eval
                nc = eval_number(ctx, cols_by_name, value.expr, row_ids=row_ids, nrows=n, out_mem=N.CPH_MEM_DEVICE)
                computed.append(nc)
                if nc.nerrors and pending is None:
                    raise_expr_error(ctx, cols_by_name, value.expr, nc, row_ids)
                elif nc.nerrors:   # the status bytes on the host; the values travel from there too
                    nc.release()
                    nc = eval_number(ctx, cols_by_name, value.expr, row_ids=row_ids, nrows=n, out_mem=N.CPH_MEM_HOST)
                    pending.append((tag, value.expr, nc))
                src = nc.values
            part = "an Int" if kind == M.INT64 else "a Time" if kind == M.TIME else "a Float"
            ptr, parr[k].arg = N.number_source(src, N.CPH_NUM_INT64 if kind in (M.INT64, M.TIME) else N.CPH_NUM_FLOAT64, n,
                                               f"map_column: {part} part has {{count}} values for {{need}} rows", keep)
            if kind == M.INT64:
                parr[k].ints = ptr
            elif kind == M.TIME:
                parr[k].ints, parr[k].prec = ptr, value.zone
            else:
                parr[k].floats, parr[k].prec = ptr, ord(value.fmt) if kind == M.FLOAT64_SHORTEST else value.prec
    return parr


def map_switch(ctx: N.Context, cols_by_name, switch, row_ids=None, nrows=None, out_mem: int = N.CPH_MEM_HOST, want_which: bool = False):
    """Map with a condition, on the device (cph_map_switch): the value of row i is the template of the first case of
    `switch` (mapping.Switch / When) whose predicate holds for row i, else its `otherwise`.  Arguments as in map_column; a
    column only a predicate names and the mapping lacks makes that term false.

    Returns (ColBuf, which): the new column, and with want_which the alternative every row selected as a numpy uint8 array
    (the case's index, or the number of cases for `otherwise`), else None.

    Int.of / Float.of parts are evaluated over ALL rows; a failing row raises expr.ExprError only if that row selects an
    alternative that contains the part — the lowest such row is reported."""
    from . import mapping as M

    names, cases, otherwise = M.compile_switch(switch, list(cols_by_name))
    alts = [pc for _, pc in cases] + [otherwise]
    keep = []
    arr, sel, n = _map_rows(cols_by_name, row_ids, nrows, names, [p for pc in alts for p in pc], keep, "map_switch: a Switch")
    computed, pending = [], []
    try:
        carr = (N.cph_map_case * len(cases))()
        for a, (ops, pieces) in enumerate(cases):
            prog = _pred_program(ops, keep, n)
            parr = _fill_pieces(ctx, cols_by_name, row_ids, pieces, n, keep, computed, pending, a)
            keep += [prog, parr]
            carr[a].prog, carr[a].nops = prog, len(ops)
            carr[a].pieces, carr[a].npieces = parr, len(pieces)
        oarr = _fill_pieces(ctx, cols_by_name, row_ids, otherwise, n, keep, computed, pending, len(cases))
        which = np.zeros(n, dtype=np.uint8) if want_which or pending else None
        out = C.POINTER(N.cph_colbuf)()
        ctx._check(ctx.lib.cph_map_switch(ctx.handle, arr, sel, len(names), n, carr, len(cases), oarr, len(otherwise), out_mem,
                                          C.byref(out), which.ctypes.data if which is not None and n else None))
        del keep
        cb = ColBuf(ctx, out)
        worst = None   # (row, expression, NumCol, failing rows) of the lowest row whose own alternative holds a failed part
        for a, expr, nc in pending:
            rows = np.flatnonzero((nc.status != N.CPH_NUM_OK) & (which == a))
            if len(rows) and (worst is None or int(rows[0]) < worst[0]):
                worst = (int(rows[0]), expr, nc, len(rows))
        if worst is not None:
            cb.release()
            _raise_expr_error_at(ctx, cols_by_name, worst[1], worst[2], worst[0], worst[3], row_ids)
        return cb, (which if want_which else None)
    finally:
        for nc in computed:
            nc.release()


def _raise_expr_error_at(ctx, cols_by_name, expr, numcol, row, nerrors, row_ids=None):
    """raise_expr_error for a row that need not be the result's first failing one: the failing op is found by evaluating
    the expression on that row's values with the host model."""
    from . import expr as E

    if row == numcol.first_error_row:
        numcol.nerrors = nerrors
        raise_expr_error(ctx, cols_by_name, expr, numcol, row_ids)
    names, ops = E.compile(expr, list(cols_by_name))
    values = {nm: _value_at(ctx, cols_by_name[nm], None if row_ids is None else row_ids.get(nm), row) for nm in names}
    _, status, op = E.evaluate(expr, values, row)
    kind = int(numcol.status[row])
    column = names[ops[op][1]] if ops[op][0] in (E.COL_INT, E.COL_FLT) else None
    raise E.ExprError(row, op, kind, column, E.error_text(expr, values, kind, op), nerrors)


def validate_rows(ctx: N.Context, cols_by_name, pred, row_ids=None, nrows=None, first_row: int = 0):
    """Validate (csvplus.go:300-310) with a declarative predicate: the number of the first row (a position in the selection,
    first_row included) where `pred` FAILS — where the reference's iteration would stop with the validator's error — or None
    when every row of [first_row, first_row + nrows) passes.  cph_filter_rows in TAKE_WHILE mode: the rows in front of the
    first failing one come back as a range, nothing is materialised.  Arguments as in filter_rows."""
    if nrows is None:   # the rows filter_rows would look at
        from . import predicates as P
        names = P.compile(pred, list(cols_by_name))[0]
        if names:
            ids = None if row_ids is None else [row_ids.get(nm) for nm in names]
            total = _rowsel([cols_by_name[nm] for nm in names], ids, None, [])[2]
        else:
            total = min((c.nrows for c in cols_by_name.values()), default=0)
        nrows = max(total - first_row, 0)
    rl = filter_rows(ctx, cols_by_name, pred, row_ids=row_ids, nrows=nrows, mode="take_while", first_row=first_row,
                     out_bits=64, out_mem=N.CPH_MEM_HOST, as_handle=True)
    try:
        passed = len(rl)
    finally:
        rl.release()
    return None if passed >= int(nrows) else first_row + passed


# ---- OrderBy with Drop / Top behind it (cph_order_rows) --------------------------------------------------------------------

class Ordered(N.Owned):
    """cph_ordered: the row numbers (positions in the selection, uint32) of order[skip : skip + limit], valid until
    release().  select_used: the Top-N select ran in front of the sort; candidates: rows that entered the sort."""
    _release_fn = "cph_ordered_release"

    def __init__(self, ctx, ptr):
        super().__init__(ctx, ptr)
        c = ptr.contents
        self.nrows, self.mem, self.bits = int(c.nrows), int(c.mem), 32
        self.ids_ptr = int(c.ids or 0)
        self.select_used, self.candidates = bool(c.select_used), int(c.candidates)

    def __len__(self):
        return self.nrows

    def to_numpy(self) -> np.ndarray:
        """The row numbers on the host (a copy): only for a result in host memory."""
        assert self.mem == N.CPH_MEM_HOST or self.nrows == 0, "a device result has no host view: consume it on the device"
        return N._ptr_array(self.ids_ptr, self.nrows, np.uint32).copy()

    def as_row_ids(self):
        """(device_ptr, bits, count): the tuple csv_write / json_write / map_column / to_int / take_rows take as row ids of
        a device column."""
        assert self.mem == N.CPH_MEM_DEVICE, "a host result is a numpy array: use to_numpy()"
        return (self.ids_ptr, 32, self.nrows)


def order_rows(ctx: N.Context, keys, nrows: int, skip: int = 0, limit=None, out_mem: int = N.CPH_MEM_HOST) -> Ordered:
    """OrderBy(keys) with Drop(skip) / Top(limit) behind it, sorted on the device (cph_order_rows): rows 0..nrows-1 of a
    selection in the order of ordering.Asc / ordering.Desc keys — slices.SortStableFunc, stable for ascending and
    descending keys alike (ordering.order_model is the contract).  A key's source is a numpy int64 / float64 array (host), a
    NumCol (it stays where it lives, its status bytes are handed through: a row that failed raises ordering.OrderError), a
    (device_ptr, count) pair or a device tensor, or a DeviceIndex over the table being ordered (kind "bytes").  With a limit
    that is small against nrows the rows are cut down by a radix select over the first key before anything is sorted
    (Ordered.select_used, Ordered.candidates; ctx.set_option("order_select", 0) turns it off)."""
    from . import ordering as O

    keys = list(keys)
    n = int(nrows)
    arr = (N.cph_order_key * max(1, len(keys)))()
    keep = []
    for i, key in enumerate(keys):
        if not isinstance(key, O.OrderKey):
            raise TypeError(f"not an order key: {key!r} (use ordering.Asc / ordering.Desc)")
        if not key.kind:
            raise TypeError(f"{type(key).__name__}({key.source!r}): a name is a key of pipeline.totals_to_csv / filter_to_csv, not of order_rows")
        ck, src = arr[i], key.source
        ck.kind, ck.descending = key.kind, 1 if key.descending else 0
        if key.kind == N.CPH_ORDER_BYTES:
            if not isinstance(src, N.DeviceIndex):
                raise TypeError(f'{type(key).__name__}: a "bytes" key takes a DeviceIndex over the table being ordered')
            ck.index = src.handle
            keep.append(src)
            continue
        dt = np.int64 if key.kind == N.CPH_NUM_INT64 else np.float64
        if isinstance(src, NumCol):
            if (N.CPH_NUM_FLOAT64 if src.kind == N.CPH_NUM_FLOAT64 else N.CPH_NUM_INT64) != key.kind:   # to_time's kinds hold int64
                raise ValueError(f"{type(key).__name__}: the NumCol's kind differs from the key's")
            if src.nrows < n:
                raise ValueError(f"{type(key).__name__}: {src.nrows} values for {n} rows")
            if src.mem == N.CPH_MEM_DEVICE:
                ck.values, ck.status, ck.values_mem = src.values[0] or None, src.status[0] or None, N.CPH_MEM_DEVICE
            else:
                v, st = np.ascontiguousarray(src.values, dtype=dt), np.ascontiguousarray(src.status, dtype=np.uint8)
                keep += [v, st]
                ck.values, ck.status, ck.values_mem = (v.ctypes.data, st.ctypes.data, N.CPH_MEM_HOST) if n else (None, None, N.CPH_MEM_HOST)
            keep.append(src)
        else:
            ck.values, ck.values_mem = N.number_source(src, key.kind, n, f"{type(key).__name__}: {{count}} values for {{need}} rows", keep)
    out = C.POINTER(N.cph_ordered)()
    ctx._check(ctx.lib.cph_order_rows(ctx.handle, arr if keys else None, len(keys), n, int(skip),
                                      N.CPH_NO_LIMIT if limit is None else int(limit), out_mem, C.byref(out)))
    del keep
    r = out.contents
    if r.nerrors:
        err = O.OrderError(int(r.first_error_row), int(r.first_error_key), int(r.first_error_kind), int(r.nerrors))
        ctx.lib.cph_ordered_release(out)
        raise err
    return Ordered(ctx, out)
