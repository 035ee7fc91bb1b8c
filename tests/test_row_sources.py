"""The host side every row-source entry point shares: staging the columns and their row ids (cph_gather_rows,
cph_csv_write_rows, cph_json_write_rows, cph_filter_rows), checking the arguments, and handing the result over in host or
device memory.  Expected values come from the models the entry points' own tests use (numpy take and orc.csv_write,
test_json_write's restatement of encoding/json, predicates.matches / select_rows)."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.predicates import All, Any, Like, Not
from oracle import orc
from test_filter import device_ids, device_list_to_numpy
from test_json_write import _hip, go_to_json, write as json_write_bytes

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
ENTRIES = ("gather_rows", "csv_write", "json_write", "filter_rows")
ID_KINDS = ("none", "u32", "u64base7")
TABLE_ROWS = 300
VOCAB = [b"", b"x", b"y", b"a,b", b'q"q', b"line\nbreak", b"12345678", b"123456789", b"\xc3\xa9", b"z" * 40]
NAMES = ["a", "b"]
PRED = Any(Like(a=b"x"), All(Like(b=b"y"), Not(Like(a=b""))))


def d2h(ptr, nbytes):
    buf = (C.c_char * (nbytes + 1))()
    if nbytes:
        assert _hip().hipMemcpy(buf, C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return bytes(buf)[:nbytes]


def make_sources(kind, device, n, seed, keep):
    """Two columns and their row ids as the wrappers take them, + the values each output row must show.  kind "none": the
    columns have n rows of their own; else they are tables of TABLE_ROWS rows read through n ids that live where the columns
    live (the two columns through different ids)."""
    rng = np.random.default_rng(seed)
    tables = [[VOCAB[i] for i in rng.integers(0, len(VOCAB), n if kind == "none" else TABLE_ROWS)] for _ in NAMES]
    cols = [StrCol.from_values(t) for t in tables]
    if device:
        cols = [c.to_device() for c in cols]
    if kind == "none":
        return cols, None, tables
    dtype, base = (np.uint32, 0) if kind == "u32" else (np.uint64, 7)
    rows = [rng.integers(0, TABLE_ROWS, n) for _ in NAMES]
    with_base = [(r + base).astype(dtype) for r in rows]
    if device:
        ids = [(device_ids(w, keep), w.dtype.itemsize * 8, n, base) for w in with_base]
    else:
        ids = [(w, base) for w in with_base]
    return cols, ids, [[t[i] for i in r] for t, r in zip(tables, rows)]


def run_gather(ctx, cols, ids, want, n, out_mem):
    from csvplus_amd.materialize import gather_rows
    for c in range(len(cols)):
        if ids is None:
            got = gather_rows(ctx, cols[c], out_mem=out_mem)
        elif isinstance(ids[c][0], np.ndarray):
            got = gather_rows(ctx, cols[c], ids[c][0], id_base=ids[c][1], out_mem=out_mem)
        else:
            got = gather_rows(ctx, cols[c], ids[c][:3], id_base=ids[c][3], out_mem=out_mem)
        if out_mem == DEVICE:
            assert (got.nrows, got.mem) == (n, DEVICE)
            sc = got.ptr.contents.col
            offs = np.frombuffer(d2h(sc.offsets, 8 * (n + 1)), dtype=np.uint64)
            got, cb = StrCol(np.frombuffer(d2h(sc.data, got.nbytes), dtype=np.uint8), offs, n, 64), got
            cb.release()
        assert got.nrows == n and got.values() == want[c]


def run_csv(ctx, cols, ids, want, n, out_mem):
    from csvplus_amd.materialize import csv_write
    out = csv_write(ctx, cols, NAMES, out_mem=out_mem, row_ids=ids, nrows=n)
    if out_mem == DEVICE:
        out, handle = d2h(out.data_ptr, len(out)), out
        handle.release()
    assert out == orc.csv_write([StrCol.from_values(w) for w in want], NAMES)


def run_json(ctx, cols, ids, want, n, out_mem):
    assert json_write_bytes(ctx, cols, NAMES, out_mem=out_mem, row_ids=ids, nrows=n) == go_to_json(NAMES, list(zip(*want)))


def run_filter(ctx, cols, ids, want, n, out_mem):
    from csvplus_amd.materialize import filter_rows
    flags = [P.matches(PRED, dict(zip(NAMES, row))) for row in zip(*want)]
    rl = filter_rows(ctx, dict(zip(NAMES, cols)), PRED, row_ids=None if ids is None else dict(zip(NAMES, ids)), nrows=n,
                     out_mem=out_mem, as_handle=True)
    try:
        assert rl.mem == out_mem
        got = device_list_to_numpy(rl) if out_mem == DEVICE else rl.to_numpy()
    finally:
        rl.release()
    assert got.tolist() == P.select_rows(flags)


RUNNERS = {"gather_rows": run_gather, "csv_write": run_csv, "json_write": run_json, "filter_rows": run_filter}


@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE], ids=["out_host", "out_device"])
@pytest.mark.parametrize("kind", ID_KINDS)
@pytest.mark.parametrize("device", [False, True], ids=["cols_host", "cols_device"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_staging_matrix(ctx, entry, device, kind, out_mem):
    """Column memory x row-id kind x result memory for every entry point; 257 = one 256-thread block and a row, 2049 = one
    2048-row Filter tile and a row."""
    for n in (0, 1, 257) + ((2049,) if entry == "filter_rows" else ()):
        keep = []
        cols, ids, want = make_sources(kind, device, n, 1000 + n, keep)
        RUNNERS[entry](ctx, cols, ids, want, n, out_mem)
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", ["where", "take_while"])
def test_filter_window_reads_its_own_ids(ctx, mode, device):
    """first_row = 3, nrows = 5 over 8 ids: only entries [3, 8) are looked at, each under its own row number.  The ids in
    front of the window differ from those inside it, so a list read from entry 0 gives other rows."""
    from csvplus_amd.materialize import filter_rows
    table = [b"x", b"y"]
    for dtype, base in ((np.uint32, 0), (np.uint64, 7)):
        rows = np.array([0, 0, 0, 1, 0, 1, 1, 0])
        keep = []
        col = StrCol.from_values(table)
        w = (rows + base).astype(dtype)
        ids = (device_ids(w, keep), w.dtype.itemsize * 8, len(w), base) if device else (w, base)
        flags = [P.matches(Like(a=b"y"), {"a": table[i]}) for i in rows]
        want = P.select_rows(flags, mode, first_row=3, nrows=5)
        assert want == ([3, 5, 6] if mode == "where" else [3])
        got = filter_rows(ctx, {"a": col.to_device() if device else col}, Like(a=b"y"), row_ids={"a": ids}, nrows=5, mode=mode,
                          first_row=3)
        assert got.tolist() == want
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_json_ids_follow_their_column_through_the_key_order(ctx, device):
    """Names ["b", "a"]: the writer emits column 1 first.  Column 0 is read through ids, column 1 is not; the two hold
    different values, so ids applied to the other column change the bytes."""
    keep = []
    t0, own = [b"t0", b"t1", b"t2"], [b"r0", b"r1", b"r2", b"r3", b"r4"]
    rows = np.array([2, 0, 1, 1, 0], dtype=np.uint32)
    cols = [StrCol.from_values(t0), StrCol.from_values(own)]
    ids = [rows, None]
    if device:
        cols = [c.to_device() for c in cols]
        ids = [(device_ids(rows, keep), 32, len(rows)), None]
    want = go_to_json(["b", "a"], [[t0[i], own[k]] for k, i in enumerate(rows)])
    assert want.startswith(b'[{"a":"r0","b":"t2"}\n,{"a":"r1","b":"t0"}\n')
    assert json_write_bytes(ctx, cols, ["b", "a"], row_ids=ids, nrows=5) == want
    del keep


# ---- the argument contract, through the C ABI ----------------------------------------------------------------------------
def _strvals(names, keep):
    hv = (N.cph_strval * len(names))()
    for i, nm in enumerate(names):
        b = np.frombuffer(nm, dtype=np.uint8)
        keep.append(b)
        hv[i].data, hv[i].len = b.ctypes.data, len(b)
    return hv


def call_entry(ctx, entry, *, nrows=3, ncols=1, out_mem=HOST, id_bits=None, col_rows=3):
    """One call of `entry` over host column(s) of col_rows rows; id_bits: the width of the row ids of column 0 (None:
    no ids).  Returns (status, whether *out is still NULL, error text)."""
    keep = []
    col = StrCol.from_values([b"1", b"22", b"1", b"4", b"5"][:col_rows])
    arr = (N.cph_strcol * max(ncols, 17))()
    for c in range(len(arr)):
        arr[c], k = col.as_c()
        keep.append(k)
    ids = np.zeros(8, np.uint64)
    sel = None
    if id_bits is not None:
        sel = (N.cph_rowsel * len(arr))()
        sel[0].ids, sel[0].bits = ids.ctypes.data, id_bits
    lib, h = ctx.lib, ctx.handle
    if entry == "gather_rows":
        out = C.POINTER(N.cph_colbuf)()
        rc = lib.cph_gather_rows(h, arr, C.c_void_p(ids.ctypes.data) if id_bits is not None else None, id_bits or 32, 0, nrows,
                                 out_mem, C.byref(out))
        release = lib.cph_colbuf_release
    elif entry == "csv_write":
        out = C.POINTER(N.cph_bytes)()
        rc = lib.cph_csv_write_rows(h, arr, sel, ncols, nrows, None, out_mem, C.byref(out))
        release = lib.cph_bytes_release
    elif entry == "json_write":
        out = C.POINTER(N.cph_bytes)()
        names = _strvals([b"c%02d" % c for c in range(len(arr))], keep)
        rc = lib.cph_json_write_rows(h, arr, sel, names, ncols, nrows, out_mem, C.byref(out))
        release = lib.cph_bytes_release
    else:
        from csvplus_amd.materialize import _pred_program
        out = C.POINTER(N.cph_rowlist)()
        prog = _pred_program([(P.LIKE, 0, b"1")], keep)
        opts = N.cph_filter_opts(N.CPH_FILTER_WHERE, 32, 0, 0, N.CPH_NO_LIMIT)
        rc = lib.cph_filter_rows(h, arr, sel, ncols, nrows, prog, 1, C.byref(opts), out_mem, C.byref(out))
        release = lib.cph_rowlist_release
    null = not out
    if out:
        release(out)
    del keep
    return rc, null, ctx.last_error()


BAD_ARGS = {
    "out_mem 5": dict(out_mem=5),
    "id bits 16": dict(id_bits=16),
    "identity column of the wrong row count": dict(nrows=4),
    "no columns": dict(ncols=0),
    "17 columns": dict(ncols=17),
}


def _applies(entry, what):
    if entry == "gather_rows":   # one column, and a column without ids is copied whole: no column count, no row count to be wrong
        return what in ("out_mem 5", "id bits 16")
    return not (entry == "filter_rows" and what == "no columns")   # a program without LIKE terms needs no column


@pytest.mark.gpu
@pytest.mark.parametrize("entry,what", [(e, w) for e in ENTRIES for w in BAD_ARGS if _applies(e, w)])
def test_bad_arguments_are_refused(ctx, entry, what):
    assert call_entry(ctx, entry)[:2] == (N.CPH_OK, False)
    rc, null, msg = call_entry(ctx, entry, **BAD_ARGS[what])
    assert rc == N.CPH_ERR_INVALID and null and msg, (entry, what, rc, msg)
    if what == "id bits 16":
        assert "bits" in msg


# ---- empty results ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE], ids=["host", "device"])
def test_empty_results_and_their_release(ctx, out_mem):
    """Zero-row and zero-group results are objects like any other: the pointers of the writers', the gather's and the
    parser's are non-NULL, and every one is released through its own release function.  (cph_index_dup_groups has no
    device mode.  cph_groups_release selects the result's device before it frees, like the other release functions; it
    did not before they shared their code, which one GPU cannot show.)"""
    lib, h = ctx.lib, ctx.handle
    keep = []
    empty = StrCol.from_values([])
    arr = (N.cph_strcol * 1)()
    arr[0], k = empty.as_c()
    keep.append(k)

    out = C.POINTER(N.cph_bytes)()
    assert lib.cph_csv_write_rows(h, arr, None, 1, 0, None, out_mem, C.byref(out)) == N.CPH_OK
    assert (out.contents.size, out.contents.mem) == (0, out_mem) and out.contents.data
    lib.cph_bytes_release(out)

    out = C.POINTER(N.cph_bytes)()
    assert lib.cph_json_write_rows(h, arr, None, _strvals([b"a"], keep), 1, 0, out_mem, C.byref(out)) == N.CPH_OK
    assert (out.contents.size, out.contents.mem) == (2, out_mem) and out.contents.data
    got = d2h(out.contents.data, 2) if out_mem == DEVICE else C.string_at(out.contents.data, 2)
    assert got == b"[]"
    lib.cph_bytes_release(out)

    table = StrCol.from_values([b"p", b"q"])
    arr[0], k = table.as_c()
    keep.append(k)
    no_ids = np.zeros(1, np.uint32)
    cb = C.POINTER(N.cph_colbuf)()
    assert lib.cph_gather_rows(h, arr, C.c_void_p(no_ids.ctypes.data), 32, 0, 0, out_mem, C.byref(cb)) == N.CPH_OK
    c = cb.contents
    assert (c.col.nrows, c.nbytes, c.col.mem, c.col.offset_bits) == (0, 0, out_mem, 64) and c.col.offsets and c.col.data
    first = d2h(c.col.offsets, 8) if out_mem == DEVICE else C.string_at(c.col.offsets, 8)
    assert first == bytes(8)
    lib.cph_colbuf_release(cb)

    opt = N.cph_csv_options(ord(","), 0, 0, 0, 0, 0)
    idx = (C.c_int32 * 1)(0)
    tab = C.POINTER(N.cph_csv_table)()
    assert lib.cph_csv_parse(h, None, 0, HOST, C.byref(opt), idx, 1, out_mem, C.byref(tab)) == N.CPH_OK
    t = tab.contents
    assert (t.nrecords, t.ncols, t.cols[0].nrows, t.cols[0].mem) == (0, 1, 0, out_mem) and t.cols[0].offsets and t.cols[0].data
    lib.cph_csv_table_release(tab)

    if out_mem == HOST:
        ix = DeviceIndex(ctx, [StrCol.from_values([b"k%03d" % i for i in range(257)])], unique=True)
        assert ix.status == N.CPH_OK
        g = C.POINTER(N.cph_groups)()
        assert lib.cph_index_dup_groups(h, ix.handle, C.byref(g)) == N.CPH_OK
        assert g.contents.ngroups == 0 and g.contents.lower and g.contents.upper
        lib.cph_groups_release(g)
        ix.close()
    # the ctx goes on working
    from csvplus_amd.materialize import csv_write
    assert csv_write(ctx, [table]) == b"p\nq\n"
    del keep
