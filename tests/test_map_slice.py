"""The Map piece CPH_MAP_SLICE on the device: Col("ts")[0:10] through materialize.map_column / map_switch and
pipeline.join_to_csv, checked byte for byte against Python's bytes slicing (mapping.render).  Value lengths around the
8-byte chunk, values packed back to back (every begin mod 8), slices with negative, open, clamped and crossing ends, rows
whose slice is empty, and calls whose every value is empty."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Format, Int, Switch, When
from helpers import orders_table, people_table

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)
SYMS = np.array([0x00, 0x61, 0x62, 0x80], dtype=np.uint8)
INT64_MAX = (1 << 63) - 1


def values_of_lengths(n, seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(SYMS, LENS[int(k)])) for k in rng.integers(0, len(LENS), n)]


def colbuf_values(cb):
    """The values of a ColBuf and its nbytes: a device result is copied back by the HIP runtime itself."""
    if cb.mem == HOST:
        return cb.to_strcol().values(), cb.nbytes
    c = cb.ptr.contents.col
    offs = np.empty(cb.nrows + 1, dtype=np.uint64)
    data = np.empty(cb.nbytes, dtype=np.uint8)
    hip = _hip()
    assert hip.hipMemcpy(C.c_void_p(offs.ctypes.data), C.c_void_p(c.offsets), C.c_size_t(offs.nbytes), 2) == 0
    if cb.nbytes:
        assert hip.hipMemcpy(C.c_void_p(data.ctypes.data), C.c_void_p(c.data), C.c_size_t(data.nbytes), 2) == 0
    return StrCol(data, offs, cb.nrows, 64, fixed_width=0).values(), cb.nbytes


def _hip():
    import torch  # noqa: F401 (it loads the HIP runtime this process uses)
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def exact_device_col(col: StrCol) -> StrCol:
    """The column on the device in a buffer of exactly its bytes."""
    import torch
    nb = col.data.nbytes
    d = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda:0")
    if nb:
        d[:nb].copy_(torch.from_numpy(np.ascontiguousarray(col.data)))
    o = None
    if not col.fixed_width:
        o = torch.from_numpy(np.ascontiguousarray(col.offsets).view(np.uint8).copy()).to("cuda:0")
    return StrCol(d, o, col.nrows, col.offset_bits, DEVICE, fixed_width=col.fixed_width)


def device_array(a, keep):
    import torch
    t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
    keep.append(t)
    return t.data_ptr()


def check_map(ctx, cols, template, rows, row_ids=None, nrows=None, out_mem=HOST):
    from csvplus_amd.materialize import map_column
    want = [M.render(template, r, i) for i, r in enumerate(rows)]
    cb = map_column(ctx, cols, template, row_ids=row_ids, nrows=nrows, out_mem=out_mem)
    try:
        got, nbytes = colbuf_values(cb)
    finally:
        cb.release()
    assert got == want
    assert nbytes == sum(len(w) for w in want)
    return want


SLICES = [(0, 10), (None, None), (-6, None), (11, 19), (None, -1), (1, None), (8, 9), (7, 17), (-17, -8), (20, 30), (30, 40), (10, 10),
          (12, 3), (-1, -3), (-100, 3), (3, 1000), (-(1 << 63), INT64_MAX), (INT64_MAX, None), (None, -(1 << 63)), (16, 24), (-25, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2049])
@pytest.mark.parametrize("device", [True, False])
def test_slices_over_identity_rows(ctx, n, device):
    """One template per slice (a slice alone, so an empty slice is an empty value), then all of them mixed with a literal, the
    whole column and an Int part; 256 rows are one tile of the copy kernel."""
    a, b = values_of_lengths(n, n), values_of_lengths(n, n + 1000)
    host = {"a": StrCol.from_values(a, fixed_width=0), "b": StrCol.from_values(b, offset_bits=64, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    rows = [{"a": x, "b": y} for x, y in zip(a, b)]
    mem = DEVICE if device else HOST
    for k, (lo, hi) in enumerate(SLICES if n in (65, 2049) else SLICES[::4]):
        want = check_map(ctx, cols, Format(Col("ab"[k % 2])[lo:hi]), rows, out_mem=mem)
        if n >= 63 and (lo, hi) in ((0, 10), (-6, None), (11, 19), (7, 17)):
            assert any(w == b"" for w in want) and any(w for w in want)   # rows whose slice is empty beside rows whose is not
    ints = np.arange(-3, n - 3, dtype=np.int64) * 1_000_003
    mixed = Format("[", Col("a")[:8], "|", Col("a"), "|", Int(ints), "|", Col("b")[-9:], Col("b")[8:17], Col("a")[1:-1], "]")
    check_map(ctx, cols, mixed, rows, out_mem=mem)
    # every value of the call empty: a slice beyond every value, and a crossing one
    assert set(check_map(ctx, cols, Format(Col("a")[26:], Col("b")[5:2]), rows, out_mem=mem)) == {b""}


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("id_bits", [32, 64])
def test_slices_over_joined_rows(ctx, device, id_bits):
    """Columns read through uint32 / uint64 row ids with a base, as a Join hands them over; more than 8 columns takes the
    generic kernels."""
    n, src_rows, base = 2049, 300, 1000
    rng = np.random.default_rng(id_bits * 2 + device)
    a, b = values_of_lengths(src_rows, 1), values_of_lengths(n, 2)
    ids = rng.integers(0, src_rows, n).astype(np.uint32 if id_bits == 32 else np.uint64)
    with_base = ids + ids.dtype.type(base)
    host = {"a": StrCol.from_values(a, fixed_width=0), "b": StrCol.from_values(b, offset_bits=64, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    keep = []
    row_ids = {"a": (device_array(with_base, keep), id_bits, n, base) if device else (with_base, base)}
    rows = [{"a": a[int(ids[i])], "b": b[i]} for i in range(n)]
    t = Format(Col("a")[:10], "/", Col("b")[-6:], "/", Col("a")[9:], Col("a"), Int(np.arange(n)), Col("b")[3:3], Col("a")[-8:-1])
    check_map(ctx, cols, t, rows, row_ids=row_ids, nrows=n, out_mem=DEVICE if device else HOST)
    # nine columns: the kernels without a compile-time column count
    many = {f"c{k}": StrCol.from_values(values_of_lengths(n, 50 + k), fixed_width=0) for k in range(9)}
    mrows = [{nm: c.value(i) for nm, c in many.items()} for i in range(n)]
    mcols = {k: exact_device_col(c) for k, c in many.items()} if device else many
    check_map(ctx, mcols, Format(*[Col(f"c{k}")[k:k + 8] for k in range(9)], Col("c0")), mrows, out_mem=DEVICE if device else HOST)
    del keep


@pytest.mark.gpu
def test_fixed_width_column_and_a_float_part(ctx):
    """A slice of a fixed-width column, and a template that holds a Float part beside a slice (the float instantiations carry
    the slice code too)."""
    n = 300
    ids = [b"%08d" % (i * 7919) for i in range(n)]
    col = StrCol.from_values(ids, fixed_width=8)
    assert col.fixed_width == 8
    cols = {"id": exact_device_col(col)}
    rows = [{"id": v} for v in ids]
    check_map(ctx, cols, Format(Col("id")[-3:], "-", Col("id")[:2]), rows, out_mem=DEVICE)
    fl = np.linspace(-5, 5, n)
    check_map(ctx, cols, Format(Col("id")[2:6], "=", M.Float(fl, 2), Col("id")[6:]), rows, out_mem=DEVICE)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_switch_with_a_prefix_condition_and_slices(ctx, device):
    from csvplus_amd.materialize import map_switch
    n = 2049
    rng = np.random.default_rng(9)
    days = [b"2016-09-13", b"2016-09-14", b"2016-10-01", b"2015-12-31"]
    ts = [days[int(d)] + b"T%02d:%02d:%02d+01:00" % (h, m, s) for d, h, m, s in
          zip(rng.integers(0, 4, n), rng.integers(0, 24, n), rng.integers(0, 60, n), rng.integers(0, 60, n))]
    ts[5], ts[77] = b"", b"2016-09"
    name = values_of_lengths(n, 4)
    host = {"ts": StrCol.from_values(ts, fixed_width=0), "name": StrCol.from_values(name, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    sw = Switch((P.HasPrefix("ts", "2016-09-14"), Format("today ", Col("ts")[11:19])),
                (P.All(P.StrCmp("ts", ">=", "2016-09"), P.Not(P.HasSuffix("name", b"\x80"))), Format(Col("ts")[:10], " ", Col("name")[:3])),
                (P.Contains("name", b"ab"), Col("name")[-4:]),
                otherwise=Format(Col("ts")[:4], Col("gone", default=b"?!")[1:]))
    rows = [{"ts": t, "name": v} for t, v in zip(ts, name)]
    want = [M.render(sw, r) for r in rows]
    want_which = [M.which_of(sw, r) for r in rows]
    assert set(want_which) == {0, 1, 2, 3}
    cb, which = map_switch(ctx, cols, sw, out_mem=DEVICE if device else HOST, want_which=True)
    try:
        got, nbytes = colbuf_values(cb)
    finally:
        cb.release()
    assert which.tolist() == want_which
    assert got == want and nbytes == sum(len(w) for w in want)
    # When: every row selects an empty slice
    cb, which = map_switch(ctx, cols, When(P.HasPrefix("ts", b""), Col("ts")[40:], Col("ts")), out_mem=HOST, want_which=True)
    assert cb.nbytes == 0 and not which.any()
    cb.release()


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
def test_orders_by_day_end_to_end(ctx):
    """The orders text with an RFC3339 `ts`: the orders since a day but not of another one, each with its `day` =
    ts[0:10], as CSV; then totals per day over the day column the Map produced: Count and Sum(qty) against a dict."""
    from csvplus_amd import DeviceIndex, pipeline
    from csvplus_amd.aggregate import Sum, totals
    from csvplus_amd.materialize import map_column
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    cv, ov = enc(people_table()), enc(orders_table(n=3000))
    rng = np.random.default_rng(14)
    ov["ts"] = [b"2016-09-%02dT%02d:%02d:%02d+01:00" % (d, h, m, s) for d, h, m, s in
                zip(rng.integers(10, 20, 3000), rng.integers(0, 24, 3000), rng.integers(0, 60, 3000), rng.integers(0, 60, 3000))]
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    day, other_day = b"2016-09-14", b"2016-09-16"
    where = P.All(P.StrCmp("ts", ">=", day), P.Not(P.HasPrefix("ts", other_day)))
    try:
        outc = [("order_id", to, "order_id"), ("surname", tc, "surname"), ("day", None, None), ("qty", to, "qty")]
        got = pipeline.join_to_csv(ctx, to, [(tc, "id", "cust_id")], outc, where=where, computed={"day": Col("ts")[0:10]})
        lines = [b"order_id,surname,day,qty"]
        for i in range(3000):
            row = {k: v[i] for k, v in ov.items()}
            if P.matches(where, row):
                lines.append(b",".join([row["order_id"], cv["surname"][int(row["cust_id"])], M.render(Col("ts")[0:10], row), row["qty"]]))
        assert 600 < len(lines) < 2400
        assert got == b"".join(ln + b"\n" for ln in lines)
        # totals per day
        cb = map_column(ctx, {"ts": to["ts"]}, Col("ts")[0:10], out_mem=DEVICE)
        ix = DeviceIndex(ctx, [cb.as_device_strcol()])
        try:
            t = totals(ix, [Sum(StrCol.from_values(ov["qty"]), "int")])
            per_day = {}
            for ts, q in zip(ov["ts"], ov["qty"]):
                c, s = per_day.get(ts[:10], (0, 0))
                per_day[ts[:10]] = (c + 1, s + int(q))
            assert t.ngroups == len(per_day) == 10
            got_days = {ov["ts"][int(r)][:10]: (int(c), int(v)) for r, c, v in zip(t.first_row, t.count, t.values[0])}
            assert got_days == per_day
        finally:
            ix.close()
            cb.release()
    finally:
        tc.release()
        to.release()


# ---- argument errors ---------------------------------------------------------------------------------------------------------

def _pieces(pieces, keep):
    arr = (N.cph_map_piece * max(len(pieces), 1))()
    for k, (kind, arg, value) in enumerate(pieces):
        arr[k].kind, arr[k].arg = kind, arg
        if isinstance(value, tuple):   # (pointer or None, len): as given
            arr[k].value.data, arr[k].value.len = value
        elif value is not None:
            b = np.frombuffer(value, dtype=np.uint8)
            keep.append(b)
            arr[k].value.data, arr[k].value.len = (b.ctypes.data if len(b) else None), len(b)
    keep.append(arr)
    return arr


@pytest.mark.gpu
def test_argument_errors(ctx):
    col = StrCol.from_values([b"2016-09-14", b"", b"x"], fixed_width=0)
    arr = (N.cph_strcol * 1)()
    arr[0], k0 = col.as_c()
    ok16 = np.array([0, 4], dtype=np.int64).tobytes()

    def fmt(pieces):
        keep = []
        out = C.POINTER(N.cph_colbuf)()
        rc = ctx.lib.cph_map_format(ctx.handle, arr, None, 1, 3, _pieces(pieces, keep), len(pieces), HOST, C.byref(out))
        vals = None
        if out:
            assert rc == N.CPH_OK
            from csvplus_amd.materialize import ColBuf
            h = ColBuf(ctx, out)
            vals = h.to_strcol().values()
            h.release()
        return rc, ctx.last_error(), vals

    def sw(pieces, in_case):
        from csvplus_amd.materialize import _pred_program
        keep = []
        prog = _pred_program([(P.HAS_PREFIX, 0, b"2016")], keep)
        x = [(M.LITERAL, 0, b"x")]
        carr = (N.cph_map_case * 1)()
        carr[0].prog, carr[0].nops = prog, 1
        cp = pieces if in_case else x
        op = x if in_case else pieces
        carr[0].pieces, carr[0].npieces = _pieces(cp, keep), len(cp)
        out = C.POINTER(N.cph_colbuf)()
        rc = ctx.lib.cph_map_switch(ctx.handle, arr, None, 1, 3, carr, 1, _pieces(op, keep), len(op), HOST, C.byref(out), None)
        if out:
            assert rc == N.CPH_OK
            ctx.lib.cph_colbuf_release(out)
        return rc, ctx.last_error()

    rc, msg, vals = fmt([(M.SLICE, 0, ok16)])
    assert rc == N.CPH_OK and vals == [b"2016", b"", b"x"]
    assert sw([(M.SLICE, 0, ok16)], True)[0] == N.CPH_OK and sw([(M.SLICE, 0, ok16)], False)[0] == N.CPH_OK
    bad = [
        ("a slice value of 8 bytes", (M.SLICE, 0, ok16[:8])), ("a slice value of 24 bytes", (M.SLICE, 0, ok16 + ok16[:8])),
        ("a NULL slice value", (M.SLICE, 0, (None, 16))), ("a slice without a value", (M.SLICE, 0, None)),
        ("a slice column of -1", (M.SLICE, -1, ok16)), ("a slice column of ncols", (M.SLICE, 1, ok16)),
        ("kind 5", (5, 0, ok16)), ("kind 6", (6, 0, ok16)), ("kind 7", (7, 0, ok16)), ("kind 9", (9, 0, ok16)),
    ]
    for what, piece in bad:
        rc, msg, _ = fmt([piece])
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
        for in_case in (True, False):
            rc, msg = sw([(M.LITERAL, 0, b"-"), piece], in_case)
            assert rc == N.CPH_ERR_INVALID and msg and "piece 1" in msg, (what, in_case, rc, msg)
    del k0
