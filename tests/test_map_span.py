"""The Map piece CPH_MAP_SPAN on the device: Col("x").trim_space() and its kin through materialize.map_column / map_switch,
pipeline.filter_to_csv and to_int, checked byte for byte against the host model (mapping.render -> Span.apply) with
nbytes == the sum of the lengths.  Values padded front and back with 0..3 spaces drawn from all 25 sequences around cores of
the lengths at the 8-byte chunk's edges, packed back to back (every begin mod 8), in host columns and in device buffers of
exactly the column's bytes — a routine that read past a value would fault there."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Float, Format, Int, Switch, When
from test_map_slice import check_map, colbuf_values, device_array, exact_device_col

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65)
SYMS = np.frombuffer(b"ab;-: ,\x80\xe2_", dtype=np.uint8)
A, B = Col("a"), Col("b")


def padded_values(n, seed, lens=LENS):
    """pad + core + pad: 0..3 spaces of the 25 kinds on either side, a core of one of `lens` bytes, a third of them behind "id:"."""
    rng = np.random.default_rng(seed)
    out = []
    for k in rng.integers(0, len(lens), n):
        core = bytes(rng.choice(SYMS, lens[int(k)]))
        if rng.integers(0, 3) == 0:
            core = b"id:" + core[3:] if len(core) >= 3 else core
        front = b"".join(M.SPACE_SEQUENCES[int(s)] for s in rng.integers(0, 25, int(rng.integers(0, 4))))
        back = b"".join(M.SPACE_SEQUENCES[int(s)] for s in rng.integers(0, 25, int(rng.integers(0, 4))))
        out.append(front + core + back)
    return out


# one template per operation and mode
OPS = [A.trim_space(), A.trim_left_space(), A.trim_right_space(),
       B.trim(b" ;-"), B.trim_left(b" \t\n_ab"), B.trim_right(b"ab;-: ,_"), A.trim(b""),
       A.trim_prefix(b" "), B.trim_prefix(b"\xe2\x80"), A.trim_suffix(b"\xa0"), B.trim_suffix(b"a"), A.trim_prefix(b"\t\n\x0b\x0c\r \xc2\x85\xc2\xa0x"),
       A.field(b";", 0), B.field(b";", 1), A.field(b";", -1), B.field(b";", -2, 3), A.field(b"a", 2, 3), B.field(b";", 1, 1), A.field(b"ab", 1),
       B.field(b"\x80", -1, 2), A.field(b"-;-;-;-;-", 0), A.before(b":"), B.after(b":"), A.field(b";", 40), B.field(b";", -40)]
PROGRAMS = [A.trim_space().trim_prefix(b"id:").field(b";", -1)[:8],
            B.field(b":", 1, 2).trim_space().trim(b"ab")[-6:],
            A.trim_left_space()[2:].trim_right_space().trim_suffix(b"a"),
            B.trim_right(b" \t")[1:-1].after(b";").before(b"-")]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2049])
@pytest.mark.parametrize("device", [True, False])
def test_spans_over_identity_rows(ctx, n, device):
    """32-bit offsets (a) and 64-bit offsets (b); 256 rows are one tile of the copy kernel."""
    a, b = padded_values(n, n), padded_values(n, n + 1000)
    host = {"a": StrCol.from_values(a, fixed_width=0), "b": StrCol.from_values(b, offset_bits=64, fixed_width=0)}
    assert host["a"].offset_bits == 32 and host["b"].offset_bits == 64
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    rows = [{"a": x, "b": y} for x, y in zip(a, b)]
    mem = DEVICE if device else HOST
    for t in (OPS if n in (65, 2049) else OPS[::3]) + PROGRAMS:
        want = check_map(ctx, cols, Format(t), rows, out_mem=mem)
        if n >= 255 and t in (OPS[0], OPS[12], PROGRAMS[0]):
            assert any(w == b"" for w in want) and any(w for w in want)   # rows whose span is empty beside rows whose is not
    # each piece set composes with SPAN: literal, column, slice, Int, Float, Float.shortest
    ints = np.arange(-3, n - 3, dtype=np.int64) * 1_000_003
    fl = np.linspace(-7.5, 1e6, n)
    check_map(ctx, cols, Format("[", A.trim_space(), "|", A, "|", Int(ints), "|", B.before(b";"), "]"), rows, out_mem=mem)
    check_map(ctx, cols, Format(A[:8], "|", B.trim_space()[:5], B[-3:], A.field(b";", 1)), rows, out_mem=mem)
    check_map(ctx, cols, Format(Float(fl, 2), " ", A.trim_space(), " ", A[1:4], Int(ints)), rows, out_mem=mem)
    check_map(ctx, cols, Format(Float.shortest(fl, "g"), "<", B.trim(b" ;"), ">", Float(fl, 0), A[2:], A, PROGRAMS[0]), rows, out_mem=mem)
    # every span of the call empty
    assert set(check_map(ctx, cols, Format(A.field(b";", 99), B.trim_space()[70:]), rows, out_mem=mem)) == {b""}


@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE])
def test_host_columns_into_device_memory_and_back(ctx, out_mem):
    """out_mem is independent of where the columns live."""
    n = 257
    a = padded_values(n, 5)
    rows = [{"a": x} for x in a]
    host = {"a": StrCol.from_values(a, fixed_width=0)}
    check_map(ctx, host, Format(A.trim_space(), "/", PROGRAMS[0]), rows, out_mem=out_mem)
    check_map(ctx, {"a": exact_device_col(host["a"])}, Format(A.trim_space(), "/", PROGRAMS[0]), rows, out_mem=out_mem)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("id_bits", [32, 64])
def test_spans_over_joined_rows(ctx, device, id_bits):
    """Columns read through uint32 / uint64 row ids with a base, as a Join hands them over; nine columns take the generic kernels."""
    n, src_rows, base = 2049, 300, 1000
    rng = np.random.default_rng(id_bits * 2 + device)
    a, b = padded_values(src_rows, 1), padded_values(n, 2)
    ids = rng.integers(0, src_rows, n).astype(np.uint32 if id_bits == 32 else np.uint64)
    with_base = ids + ids.dtype.type(base)
    host = {"a": StrCol.from_values(a, fixed_width=0), "b": StrCol.from_values(b, offset_bits=64, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    keep = []
    row_ids = {"a": (device_array(with_base, keep), id_bits, n, base) if device else (with_base, base)}
    rows = [{"a": a[int(ids[i])], "b": b[i]} for i in range(n)]
    t = Format(A.trim_space(), "/", B.field(b";", -1), "/", A[:4], PROGRAMS[0], Int(np.arange(n)), B.trim_left(b" a"), A)
    check_map(ctx, cols, t, rows, row_ids=row_ids, nrows=n, out_mem=DEVICE if device else HOST)
    many = {f"c{k}": StrCol.from_values(padded_values(n, 50 + k, LENS[:10]), fixed_width=0) for k in range(9)}
    mrows = [{nm: c.value(i) for nm, c in many.items()} for i in range(n)]
    mcols = {k: exact_device_col(c) for k, c in many.items()} if device else many
    check_map(ctx, mcols, Format(*[Col(f"c{k}").trim_space()[k:k + 8] if k % 2 else Col(f"c{k}").trim_space() for k in range(9)], Col("c0")), mrows, out_mem=DEVICE if device else HOST)
    del keep


@pytest.mark.gpu
def test_fixed_width_column(ctx):
    n = 300
    ids = [(b" " * (i % 3) + b"%d;%d" % (i * 7919, i)).ljust(12)[:12] for i in range(n)]
    col = StrCol.from_values(ids, fixed_width=12)
    assert col.fixed_width == 12
    cols = {"id": exact_device_col(col)}
    rows = [{"id": v} for v in ids]
    check_map(ctx, cols, Format(Col("id").trim_space(), "-", Col("id").after(b";").trim_space(), "-", Col("id")[:2]), rows, out_mem=DEVICE)
    check_map(ctx, {"id": col}, Format(Col("id").before(b";").trim_left_space(), Float(np.linspace(-5, 5, n), 2)), rows, out_mem=HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_tiles_beyond_the_stage_beside_tiles_that_fit(ctx, device):
    """256 rows of about 100 kept bytes are more than the 16 KiB stage: that tile's rows go to global memory themselves."""
    n = 700
    rng = np.random.default_rng(3)
    vals = [b"  \xe2\x80\x83" + bytes(rng.choice(SYMS[:2], 100 if 256 <= i < 512 else int(rng.integers(0, 12)))) + b"\t \xc2\xa0" for i in range(n)]
    col = StrCol.from_values(vals, fixed_width=0)
    cols = {"a": exact_device_col(col) if device else col}
    want = check_map(ctx, cols, Format(A.trim_space()), [{"a": v} for v in vals], out_mem=DEVICE if device else HOST)
    assert sum(len(w) for w in want[256:512]) > 16 * 1024 > sum(len(w) for w in want[:256])
    check_map(ctx, cols, Format("#", A.trim_space()[1:], A.trim_right_space()), [{"a": v} for v in vals], out_mem=HOST)


@pytest.mark.gpu
def test_one_long_value_with_700_separators(ctx):
    rng = np.random.default_rng(8)
    fields = [bytes(rng.choice(SYMS[:2], int(k))) for k in rng.integers(0, 13, 701)]
    long = b";".join(fields)
    long = long + b"x" * (5000 - len(long)) if len(long) < 5000 else long
    assert len(long) >= 5000 and long.count(b";") == 700
    vals = [b" a;b ", long, b"", b"  " + long + b"  "]
    col = StrCol.from_values(vals, fixed_width=0)
    rows = [{"a": v} for v in vals]
    for cols in ({"a": col}, {"a": exact_device_col(col)}):
        for t in (A.field(b";", -1), A.field(b";", 350), A.field(b";", 700), A.field(b";", -701), A.field(b";", 701), A.field(b";", 5, 6),
                  A.trim_space().field(b";", -350).trim(b"a"), A.field(b"b;a", -2)):
            check_map(ctx, cols, Format(t, "|"), rows, out_mem=DEVICE)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_switch_alternatives_with_span_pieces(ctx, device):
    from csvplus_amd.materialize import map_switch
    n = 2049
    a, b = padded_values(n, 21), padded_values(n, 22)
    host = {"a": StrCol.from_values(a, fixed_width=0), "b": StrCol.from_values(b, offset_bits=64, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in host.items()} if device else host
    sw = Switch((P.Contains("a", b"id:"), Format("id ", A.trim_space().trim_prefix(b"id:").before(b";"))),
                (P.HasPrefix("b", b" "), Format(B.trim_space(), "+", A[:3])),
                (P.Contains("b", b";"), B.field(b";", -1).trim_right_space()),
                otherwise=Format(A.trim(b" ab"), Col("gone", default=b" ?! ").trim_space(), Int(np.arange(n))))
    rows = [{"a": x, "b": y} for x, y in zip(a, b)]
    want = [M.render(sw, r, i) for i, r in enumerate(rows)]
    want_which = [M.which_of(sw, r) for r in rows]
    assert set(want_which) == {0, 1, 2, 3}
    cb, which = map_switch(ctx, cols, sw, out_mem=DEVICE if device else HOST, want_which=True)
    try:
        got, nbytes = colbuf_values(cb)
    finally:
        cb.release()
    assert which.tolist() == want_which
    assert got == want and nbytes == sum(len(w) for w in want)
    # SPAN beside a shortest float in another alternative, and a When whose every row selects an empty span
    fl = np.linspace(-3, 3, n)
    sw2 = When(P.HasPrefix("a", b"id:"), Format(Float.shortest(fl), A.after(b":")), Format(B.trim_space(), Float(fl, 1)))
    cb, which = map_switch(ctx, cols, sw2, out_mem=HOST, want_which=True)
    assert cb.to_strcol().values() == [M.render(sw2, r, i) for i, r in enumerate(rows)] and 0 < which.sum() < n
    cb.release()
    cb, which = map_switch(ctx, cols, When(P.HasPrefix("a", b""), A.field(b";", 77), A), out_mem=HOST, want_which=True)
    assert cb.nbytes == 0 and not which.any()
    cb.release()


@pytest.mark.gpu
def test_filter_to_csv_with_computed_spans(ctx):
    from csvplus_amd import pipeline
    n = 500
    ids = ["%s%d%s" % (" " * (i % 3), i, "\t" * (i % 2)) for i in range(n)]
    skus = ["SKU-%04d-%s" % (i * 7, "red blue green".split()[i % 3]) for i in range(n)]
    mails = ["user%d@host%d.example" % (i, i % 7) for i in range(n)]
    text = b"id,sku,email\n" + b"".join(('"%s",%s,%s\n' % r).encode() for r in zip(ids, skus, mails))
    tab = pipeline.read_table(ctx, text)
    try:
        computed = {"key": Col("id").trim_space(), "part": Col("sku").trim_prefix(b"SKU-").field(b"-", 0), "colour": Col("sku").field(b"-", -1),
                    "host": Col("email").after(b"@").before(b".")}
        got = pipeline.filter_to_csv(ctx, tab, P.HasSuffix("sku", b"blue"), ["key", "part", "colour", "host"], computed=computed)
        lines = [b"key,part,colour,host"] + [b"%d,%04d,blue,host%d" % (i, i * 7, i % 7) for i in range(n) if i % 3 == 1]
        assert got == b"".join(ln + b"\n" for ln in lines)
    finally:
        tab.release()


@pytest.mark.gpu
def test_to_int_fails_on_the_raw_column_and_succeeds_on_the_trimmed_one(ctx):
    from csvplus_amd.materialize import map_column, to_int
    n = 1000
    rng = np.random.default_rng(4)
    nums = rng.integers(-10**12, 10**12, n)
    pads = [M.SPACE_SEQUENCES[int(k)] for k in rng.integers(0, 25, 2 * n)]
    vals = [pads[2 * i] + b"%d" % v + pads[2 * i + 1] for i, v in enumerate(nums)]   # " 42 "
    col = exact_device_col(StrCol.from_values(vals, fixed_width=0))
    raw = to_int(ctx, col)
    assert raw.nerrors == n and raw.first_error_row == 0
    raw.release()
    cb = map_column(ctx, {"id": col}, Col("id").trim_space(), out_mem=DEVICE)
    try:
        nc = to_int(ctx, cb.as_device_strcol())
        assert nc.nerrors == 0
        np.testing.assert_array_equal(nc.values, nums)
        nc.release()
    finally:
        cb.release()


# ---- argument errors ---------------------------------------------------------------------------------------------------------

def span_ops(ops, keep):
    """A cph_span_op array of (op, mode, a, b, literal); a literal is bytes, or (pointer or None, len) as given."""
    arr = (N.cph_span_op * max(len(ops), 1))()
    for q, (op, mode, a, b, lit) in enumerate(ops):
        arr[q].op, arr[q].mode, arr[q].a, arr[q].b = op, mode, a, b
        if isinstance(lit, tuple):
            arr[q].lit.data, arr[q].lit.len = lit
        else:
            lb = np.frombuffer(lit, dtype=np.uint8)
            keep.append(lb)
            arr[q].lit.data, arr[q].lit.len = (lb.ctypes.data if len(lb) else None), len(lb)
    keep.append(arr)
    return arr


def span_piece(arr, k, arg, ops, keep, nbytes=None, null=False):
    sa = span_ops(ops, keep)
    arr[k].kind, arr[k].arg = M.SPAN, arg
    arr[k].value.data = None if null else C.addressof(sa)
    arr[k].value.len = len(ops) * C.sizeof(N.cph_span_op) if nbytes is None else nbytes


TS = (M.SPAN_TRIM_SPACE, 3, 0, 0, b"")
BAD_PIECES = [   # what, the piece's keywords, a word of the message
    ("a column of -1", dict(arg=-1, ops=[TS]), "column outside 0..ncols-1"),
    ("a column of ncols", dict(arg=1, ops=[TS]), "column outside 0..ncols-1"),
    ("a NULL value", dict(arg=0, ops=[TS], null=True), "whole number of cph_span_op"),
    ("a value of 39 bytes", dict(arg=0, ops=[TS], nbytes=39), "whole number of cph_span_op"),
    ("a value of 41 bytes", dict(arg=0, ops=[TS, TS], nbytes=41), "whole number of cph_span_op"),
    ("no operations", dict(arg=0, ops=[], nbytes=0), "1..4 operations"),
    ("five operations", dict(arg=0, ops=[TS] * 5), "1..4 operations"),
    ("op 0", dict(arg=0, ops=[(0, 0, 0, 0, b"")]), "unknown span op"),
    ("op 7", dict(arg=0, ops=[TS, (7, 0, 0, 0, b"")]), "SPAN operation 1 (7): unknown span op"),
    ("trim_space mode 0", dict(arg=0, ops=[(M.SPAN_TRIM_SPACE, 0, 0, 0, b"")]), "TRIM_SPACE): unknown mode"),
    ("trim_space mode 4", dict(arg=0, ops=[(M.SPAN_TRIM_SPACE, 4, 0, 0, b"")]), "unknown mode"),
    ("cutset mode 0", dict(arg=0, ops=[(M.SPAN_TRIM_CUTSET, 0, 0, 0, b" ")]), "TRIM_CUTSET): unknown mode"),
    ("prefix mode 1", dict(arg=0, ops=[(M.SPAN_TRIM_PREFIX, 1, 0, 0, b" ")]), "TRIM_PREFIX): unknown mode"),
    ("slice mode 3", dict(arg=0, ops=[(M.SPAN_SLICE, 3, 0, 1, b"")]), "SLICE): unknown mode"),
    ("a cutset byte of 0x80", dict(arg=0, ops=[(M.SPAN_TRIM_CUTSET, 3, 0, 0, b" \x80")]), "0x80 or above"),
    ("a cutset of 33 bytes", dict(arg=0, ops=[(M.SPAN_TRIM_CUTSET, 3, 0, 0, bytes(range(33)))]), "more than 32 bytes"),
    ("a cutset without pointer", dict(arg=0, ops=[(M.SPAN_TRIM_CUTSET, 3, 0, 0, (None, 2))]), "no data pointer"),
    ("a prefix without pointer", dict(arg=0, ops=[(M.SPAN_TRIM_PREFIX, 0, 0, 0, (None, 1))]), "no data pointer"),
    ("a separator without pointer", dict(arg=0, ops=[(M.SPAN_FIELD, -1, 0, 0, (None, 1))]), "no data pointer"),
    ("a prefix of 256 bytes", dict(arg=0, ops=[(M.SPAN_TRIM_PREFIX, 0, 0, 0, b"x" * 256)]), "more than 255 bytes"),
    ("a suffix of 256 bytes", dict(arg=0, ops=[(M.SPAN_TRIM_SUFFIX, 0, 0, 0, b"x" * 256)]), "more than 255 bytes"),
    ("a separator of 256 bytes", dict(arg=0, ops=[(M.SPAN_FIELD, -1, 0, 0, b"x" * 256)]), "separator of more than 255 bytes"),
    ("an empty separator", dict(arg=0, ops=[(M.SPAN_FIELD, -1, 0, 0, b"")]), "empty separator"),
    ("limit 0", dict(arg=0, ops=[(M.SPAN_FIELD, 0, 0, 0, b",")]), "limit"),
    ("limit -2", dict(arg=0, ops=[(M.SPAN_FIELD, -2, 0, 0, b",")]), "limit"),
]


@pytest.mark.gpu
def test_argument_errors(ctx):
    col = StrCol.from_values([b" 2016-09-14 ", b"", b" x;y "], fixed_width=0)
    carr = (N.cph_strcol * 1)()
    carr[0], k0 = col.as_c()

    def fmt(arr, npieces):
        out = C.POINTER(N.cph_colbuf)()
        rc = ctx.lib.cph_map_format(ctx.handle, carr, None, 1, 3, arr, npieces, HOST, C.byref(out))
        vals = None
        if out:
            assert rc == N.CPH_OK
            from csvplus_amd.materialize import ColBuf
            h = ColBuf(ctx, out)
            vals = h.to_strcol().values()
            h.release()
        return rc, ctx.last_error(), vals

    def sw(arr, npieces, in_case, keep):
        from csvplus_amd.materialize import _pred_program
        prog = _pred_program([(P.HAS_PREFIX, 0, b" 2016")], keep)
        x = (N.cph_map_piece * 1)()
        xb = np.frombuffer(b"x", dtype=np.uint8)
        keep.append(xb)
        x[0].kind, x[0].value.data, x[0].value.len = M.LITERAL, xb.ctypes.data, 1
        cases = (N.cph_map_case * 1)()
        cases[0].prog, cases[0].nops = prog, 1
        cases[0].pieces, cases[0].npieces = (arr, npieces) if in_case else (x, 1)
        other, nother = (x, 1) if in_case else (arr, npieces)
        out = C.POINTER(N.cph_colbuf)()
        rc = ctx.lib.cph_map_switch(ctx.handle, carr, None, 1, 3, cases, 1, other, nother, HOST, C.byref(out), None)
        if out:
            assert rc == N.CPH_OK
            ctx.lib.cph_colbuf_release(out)
        return rc, ctx.last_error()

    keep = []
    ok = (N.cph_map_piece * 1)()
    span_piece(ok, 0, 0, [TS, (M.SPAN_FIELD, 2, 1, 0, b";"), (M.SPAN_TRIM_CUTSET, 3, 0, 0, b""), (M.SPAN_TRIM_PREFIX, 0, 0, 0, b"")], keep)
    rc, msg, vals = fmt(ok, 1)
    assert rc == N.CPH_OK and vals == [b"", b"", b"y"], msg
    assert sw(ok, 1, True, keep)[0] == N.CPH_OK and sw(ok, 1, False, keep)[0] == N.CPH_OK
    span_piece(ok, 0, 0, [(M.SPAN_FIELD, 1, 0, 0, b"s" * 255), (M.SPAN_TRIM_CUTSET, 1, 0, 0, bytes(range(1, 33))), (M.SPAN_TRIM_SUFFIX, 0, 0, 0, b"p" * 255)], keep)
    assert fmt(ok, 1)[2] == [b"2016-09-14 ", b"", b"x;y "]   # the limits themselves are fine
    for what, kw, words in BAD_PIECES:
        arr = (N.cph_map_piece * 2)()
        lb = np.frombuffer(b"-", dtype=np.uint8)
        keep.append(lb)
        arr[0].kind, arr[0].value.data, arr[0].value.len = M.LITERAL, lb.ctypes.data, 1
        span_piece(arr, 1, keep=keep, **kw)
        rc, msg, _ = fmt(arr, 2)
        assert rc == N.CPH_ERR_INVALID and words in msg and "cph_map_format" in msg, (what, rc, msg)
        for in_case in (True, False):
            rc, msg = sw(arr, 2, in_case, keep)
            assert rc == N.CPH_ERR_INVALID and words in msg and "piece 1" in msg and ("case 0" if in_case else "otherwise") in msg, (what, in_case, rc, msg)
    # 16 operations in a call are fine, 17 are not: in one template, and over the alternatives of a switch together
    four = [TS, (M.SPAN_TRIM_PREFIX, 0, 0, 0, b" "), (M.SPAN_SLICE, 0, 0, 5, b""), (M.SPAN_TRIM_SPACE, 1, 0, 0, b"")]
    arr = (N.cph_map_piece * 5)()
    for k in range(4):
        span_piece(arr, k, 0, four, keep)
    span_piece(arr, 4, 0, [TS], keep)
    assert fmt(arr, 4)[0] == N.CPH_OK
    rc, msg, _ = fmt(arr, 5)
    assert rc == N.CPH_ERR_INVALID and "more than 16 SPAN operations" in msg
    three = (N.cph_map_piece * 3)()
    for k in range(3):
        span_piece(three, k, 0, four, keep)
    assert sw(three, 3, True, keep)[0] == N.CPH_OK      # 12 + the literal alternative
    from csvplus_amd.materialize import map_switch
    five = Switch((P.HasPrefix("a", b" "), Format(*[A.trim_space().trim_space().trim_space().trim_space()] * 2)),
                  otherwise=Format(*[A.trim_space().trim_space().trim_space().trim_space()] * 2))
    cb, _ = map_switch(ctx, {"a": col}, five)            # 16 over two alternatives
    cb.release()
    both = (N.cph_map_case * 1)()
    from csvplus_amd.materialize import _pred_program
    both[0].prog, both[0].nops = _pred_program([(P.HAS_PREFIX, 0, b" ")], keep), 1
    both[0].pieces, both[0].npieces = three, 3
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_switch(ctx.handle, carr, None, 1, 3, both, 1, arr, 2, HOST, C.byref(out), None)   # 12 + 8
    assert rc == N.CPH_ERR_INVALID and not out and "more than 16 SPAN operations" in ctx.last_error() and "otherwise, piece 1" in ctx.last_error()
    # the neighbours of kind 14 stay unknown
    for kind in (13, 15):
        arr = (N.cph_map_piece * 1)()
        span_piece(arr, 0, 0, [TS], keep)
        arr[0].kind = kind
        rc, msg, _ = fmt(arr, 1)
        assert rc == N.CPH_ERR_INVALID and "unknown piece kind (1..4, 8, 10)" in msg, (kind, rc, msg)
    del k0
