"""Conditional Map (csvplus.go:290-296 with an if inside the closure; csvplus_test.go:283-288): mapping.Switch / When, their
compiler and host model (CPU), and cph_map_switch on the device compared byte for byte — offsets, data and `which` — with
mapping.render / which_of."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Const, Float, Format, Int, Switch, When
from helpers import orders_table, people_table, stock_table

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE


# ---- CPU: the host model and the compiler -----------------------------------------------------------------------------------

def test_render_and_which_of_known_answers():
    julia = When(P.Like(name="Amelia"), "Julia", Col("name"))   # TestLongChain's Map
    assert M.render(julia, {"name": "Amelia", "surname": "Smith"}) == b"Julia" and M.which_of(julia, {"name": "Amelia"}) == 0
    assert M.render(julia, {"name": b"Ava"}) == b"Ava" and M.which_of(julia, {"name": b"Ava"}) == 1
    assert M.columns(julia) == ["name"]
    # the first case that holds wins
    sw = Switch((P.IntCmp("born", "<", 1950), "old"), (P.IntCmp("born", "<", 1980), Format("mid ", Col("born"))), otherwise="young")
    assert [(M.which_of(sw, {"born": b}), M.render(sw, {"born": b})) for b in ("1949", "1950", "1979", "1980")] == \
        [(0, b"old"), (1, b"mid 1950"), (1, b"mid 1979"), (2, b"young")]
    # All() is always true, Any() never
    assert M.which_of(Switch((P.Any(), "a"), (P.All(), "b"), otherwise="c"), {}) == 1
    assert M.render(Switch((P.Any(), "a"), otherwise="c"), {"x": "1"}) == b"c"
    # a value that does not convert, and a row without the predicate's column: false
    assert M.which_of(sw, {"born": "n/a"}) == 2 and M.which_of(sw, {}) == 2
    assert M.which_of(When(P.Not(P.IntCmp("born", "<", 1950)), "x", "y"), {"born": "n/a"}) == 0
    # parts of the alternatives a row does not select are not evaluated
    part = Float.of(E.FloatCol("price") * 2.0, 2)
    priced = When(P.Like(kind="priced"), part, "-")
    assert M.render(priced, {"kind": "free", "price": "none"}) == b"-"
    assert M.render(priced, {"kind": "priced", "price": "1.25"}) == b"2.50"
    with pytest.raises(E.ExprError):
        M.render(priced, {"kind": "priced", "price": "none"})
    assert M.columns(priced) == ["kind", "price"]


def test_compile_switch_rules():
    sw = Switch((P.IntCmp("born", ">", 1970), Format(Col("x"), "a")), (P.Like(name="A", x="1"), "b"), otherwise=Col("name"))
    names, cases, otherwise = M.compile_switch(sw, ["name", "x", "born", "unused"])
    assert names == ["born", "x", "name"]   # one list for predicates and templates, in order of first use
    assert [op[:2] for op in cases[0][0]] == [(P.INT_LT + 5, 0)] and cases[0][1] == [(M.COLUMN, 1, None), (M.LITERAL, 0, b"a")]
    assert [op[:2] for op in cases[1][0]] == [(P.LIKE, 2), (P.LIKE, 1), (P.ALL, 2)] and cases[1][1] == [(M.LITERAL, 0, b"b")]
    assert otherwise == [(M.COLUMN, 2, None)]
    # a predicate column the rows lack is column -1; a Col they lack its default, or MissingColumn whatever the rows select
    names, cases, otherwise = M.compile_switch(When(P.Like(nope="1"), Col("gone", default="d"), "x"), ["name"])
    assert names == [] and cases[0][0] == [(P.LIKE, -1, b"1")] and cases[0][1] == [(M.LITERAL, 0, b"d")]
    with pytest.raises(M.MissingColumn):
        M.compile_switch(When(P.Any(), Col("gone"), "x"), ["name"])
    # 8 cases, 16 pieces per alternative, 32 pieces in all, 16 columns
    case = (P.Like(a="1"), "x")
    M.compile_switch(Switch(*[case] * 8, otherwise="y"), ["a"])
    with pytest.raises(ValueError):
        M.compile_switch(Switch(*[case] * 9, otherwise="y"), ["a"])
    cols = [f"c{k}" for k in range(20)]
    wide = lambda k: Format(*[Col(cols[j % 4]) for j in range(k)])   # noqa: E731 (k column pieces: neighbours do not join)
    M.compile_switch(When(P.All(), wide(16), wide(16)), cols)        # 32 in all
    with pytest.raises(ValueError):
        M.compile_switch(When(P.All(), wide(17), "y"), cols)
    with pytest.raises(ValueError):
        M.compile_switch(Switch((P.All(), wide(16)), (P.All(), wide(16)), otherwise="y"), cols)   # 33
    M.compile_switch(When(P.Like({c: "1" for c in cols[:8]}), Format(*[Col(c) for c in cols[8:16]]), "y"), cols)   # 16 columns
    with pytest.raises(ValueError):
        M.compile_switch(When(P.Like({c: "1" for c in cols[:8]}), Format(*[Col(c) for c in cols[8:17]]), "y"), cols)
    # a Switch stands where a whole template stands
    with pytest.raises(TypeError):
        Switch((P.All(), When(P.All(), "a", "b")), otherwise="c")
    with pytest.raises(TypeError):
        When(P.All(), "a", When(P.All(), "b", "c"))
    with pytest.raises(TypeError):
        Format("a", When(P.All(), "b", "c"))
    with pytest.raises(TypeError):
        Switch((lambda row: True, "a"), otherwise="b")


def test_switch_struct_size_against_the_compiled_header(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(cph_map_case), offsetof(cph_map_case, prog), offsetof(cph_map_case, nops),'
                   ' offsetof(cph_map_case, pieces), offsetof(cph_map_case, npieces), CPH_MAP_MAX_CASES, CPH_MAP_SWITCH_MAX_PIECES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(root / "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    T = N.cph_map_case
    assert out == [C.sizeof(T), T.prog.offset, T.nops.offset, T.pieces.offset, T.npieces.offset, M.MAX_CASES, M.SWITCH_MAX_PIECES]
    assert (N.CPH_MAP_MAX_CASES, N.CPH_MAP_SWITCH_MAX_PIECES) == (M.MAX_CASES, M.SWITCH_MAX_PIECES) == (8, 32)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _hip():
    """The HIP runtime this process already uses (torch loaded it): for reading device results back."""
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def _from_device(ptr, count, dtype):
    out = np.empty(count, dtype=dtype)
    if count:
        assert _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # device to host
    return out


def colbuf_values(cb):
    """The values of a ColBuf (host or device) as a list of bytes; checks the offsets' shape and nbytes on the way."""
    c = cb.ptr.contents.col
    assert c.offset_bits == 64 and c.fixed_width == 0 and c.mem == cb.mem and c.nrows == cb.nrows
    if cb.mem == HOST:
        offs = N._ptr_array(c.offsets, cb.nrows + 1, np.uint64).copy()
        data = N._ptr_array(c.data, cb.nbytes, np.uint8).copy()
    else:
        offs = _from_device(c.offsets, cb.nrows + 1, np.uint64)
        data = _from_device(c.data, cb.nbytes, np.uint8)
    assert offs[0] == 0 and int(offs[-1]) == cb.nbytes and (np.diff(offs.astype(np.int64)) >= 0).all()
    blob = data.tobytes()
    return [blob[int(offs[i]):int(offs[i + 1])] for i in range(cb.nrows)]


def device_array(a, keep):
    import torch
    t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0") if a.nbytes else torch.empty(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    keep.append(t)
    return t.data_ptr()


def run_switch(ctx, cols, sw, row_ids=None, nrows=None, out_mem=HOST):
    """(values, which) of the device."""
    from csvplus_amd.materialize import map_switch
    cb, which = map_switch(ctx, cols, sw, row_ids=row_ids, nrows=nrows, out_mem=out_mem, want_which=True)
    try:
        assert cb.mem == out_mem and which.dtype == np.uint8 and len(which) == cb.nrows
        return colbuf_values(cb), which.tolist()
    finally:
        cb.release()


def model(sw, table, n, row_of=None):
    """(values, which) of the host model over rows 0..n-1; row_of(i) -> {name: row of that column feeding output row i}."""
    vals, which = [], []
    for i in range(n):
        src = row_of(i) if row_of else {}
        row = {k: v[src.get(k, i)] for k, v in table.items()}
        vals.append(M.render(sw, row, i))
        which.append(M.which_of(sw, row))
    return vals, which


def _mod4(n):
    """A key column whose alternative changes at every row, and the 3-case Switch over it that selects every alternative."""
    table = {"k": [b"%d" % (i % 4) for i in range(n)], "v": [b"v%d" % i if i % 7 else b"" for i in range(n)]}
    sw = Switch((P.Like(k="0"), Format("zero:", Col("v"))), (P.Like(k="1"), Col("v")), (P.IntCmp("k", "==", 2), "two"),
                otherwise=Format(Col("k"), "-", Col("v"), "-", Col("k")))
    return table, sw


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_row_counts_around_word_tile_and_predicate_tile(ctx, n):
    """The bitmap word (64), the copy tile (256) and the predicate tile (2048)."""
    table, sw = _mod4(n)
    want = model(sw, table, n)
    if n >= 4:
        assert set(want[1]) == {0, 1, 2, 3}
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    assert run_switch(ctx, cols, sw, nrows=n) == want
    assert run_switch(ctx, {k: c.to_device() for k, c in cols.items()}, sw, nrows=n, out_mem=DEVICE) == want


@pytest.mark.gpu
def test_patterns_all_none_single_rows_and_eight_cases(ctx):
    n = 130
    for hit in (None, 0, 63, 64, 129):
        table = {"k": [b"y" if i == hit else b"x" for i in range(n)]}
        cols = {"k": StrCol.from_values(table["k"], fixed_width=0)}
        for sw in (When(P.Like(k="y"), "hit", Format("<", Col("k"), ">")), When(P.Not(P.Like(k="y")), Col("k"), "miss!")):
            want = model(sw, table, n)
            assert sorted(set(want[1])) == ([0, 1] if hit is not None else [want[1][0]])
            assert run_switch(ctx, cols, sw) == want
    always = When(P.All(), Format(Col("k"), Col("k")), "never")
    never = When(P.Any(), "never", Col("k"))
    assert run_switch(ctx, cols, always) == ([b"xx"] * 129 + [b"yy"], [0] * n)
    assert run_switch(ctx, cols, never) == ([b"x"] * 129 + [b"y"], [1] * n)
    # 8 cases and otherwise, all selected; an earlier case hides a later one that also holds
    n = 700
    table = {"k": [b"%d" % (i * 5 % 9) for i in range(n)]}
    cases = [(P.Any(P.Like(k="5"), P.Like(k="2")) if c == 5 else P.Like(k=str(c)), Format("c%d=" % c, Col("k"))) for c in range(8)]
    sw = Switch(*cases, otherwise=Format("other ", Col("k")))
    want = model(sw, table, n)
    assert set(want[1]) == set(range(9)) and b"c2=2" in want[0] and b"c5=2" not in want[0]
    assert run_switch(ctx, {"k": StrCol.from_values(table["k"], fixed_width=0)}, sw) == want


@pytest.mark.gpu
def test_staged_unstaged_and_empty_tiles(ctx):
    """Tile 0: 256 rows of a 100-byte literal plus a column — beyond the 16 KiB stage, written to global memory; tile 1: every
    row picks the empty value (span 0); tile 2: both alternate, through the stage; then a call whose rows all pick the empty value."""
    n = 3 * 256 + 5
    lit = bytes(range(33, 133))
    kind = lambda i: b"big" if i < 256 or (i >= 512 and i % 2) else b"none"   # noqa: E731
    table = {"k": [kind(i) for i in range(n)], "v": [b"%d" % i for i in range(n)]}
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    sw = When(P.Like(k="big"), Format(lit, Col("v")), Const(b""))
    want = model(sw, table, n)
    assert sum(len(v) for v in want[0][:256]) > 16 * 1024 and not any(want[0][256:512])
    assert run_switch(ctx, cols, sw) == want
    assert run_switch(ctx, {k: c.to_device() for k, c in cols.items()}, sw, out_mem=DEVICE) == want
    from csvplus_amd.materialize import map_switch
    empty = When(P.Like(k="absent"), Format(lit, Col("v")), Const(b""))
    cb, which = map_switch(ctx, cols, empty, want_which=True)
    assert cb.nbytes == 0 and cb.nrows == n and colbuf_values(cb) == [b""] * n and which.tolist() == [1] * n
    cb.release()


ID_KINDS = ["identity", "ids32", "ids64", "ids32_base"]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("id_kind", ID_KINDS)
def test_row_sources_and_a_fixed_width_key(ctx, id_kind, device):
    """Columns read through 32- and 64-bit row ids with a base (joined rows), host and device; the key is a fixed-width
    8-byte column: one aligned load per row in the predicate, and a COLUMN piece."""
    nsrc, n = 40, 300 if id_kind != "identity" else 40
    rng = np.random.default_rng(11)
    keys = [b"%08d" % (i % 3) for i in range(nsrc)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(nsrc)]
    kcol = StrCol.from_values(keys)
    assert kcol.fixed_width == 8
    other = [b"o%d" % i for i in range(n)]   # an identity column beside the ones read through row ids
    cols = {"k": kcol, "v": StrCol.from_values(vals, fixed_width=0), "o": StrCol.from_values(other, fixed_width=0)}
    keep, row_ids, src = [], None, None
    if id_kind != "identity":
        src = np.concatenate([np.arange(nsrc)[::-1], [3, 3, 3], rng.integers(0, nsrc, n - nsrc - 3)])
        base = 1000 if id_kind == "ids32_base" else 0
        ids = (src + base).astype(np.uint64 if id_kind == "ids64" else np.uint32)
        one = (device_array(ids, keep), ids.dtype.itemsize * 8, n, base) if device else (ids, base)
        row_ids = {"k": one, "v": one}
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
    sw = Switch((P.Like(k=b"00000001"), Format(Col("o"), ":", Col("v"))), (P.Like(k=b"00000002"), Format(Col("k"), "/", Col("v"), "/", Col("o"))),
                otherwise=Col("k"))
    want = model(sw, {"k": keys, "v": vals, "o": other}, n, (lambda i: {"k": int(src[i]), "v": int(src[i])}) if src is not None else None)
    assert set(want[1]) == {0, 1, 2}
    assert run_switch(ctx, cols, sw, row_ids=row_ids, nrows=n, out_mem=DEVICE if device else HOST) == want


@pytest.mark.gpu
def test_number_pieces_count_only_where_their_alternative_is_selected(ctx):
    from csvplus_amd.materialize import map_switch
    n = 300
    table = {"k": [b"n" if i % 3 else b"s" for i in range(n)]}
    cols = {"k": StrCol.from_values(table["k"], fixed_width=0)}
    ints = np.arange(n, dtype=np.int64) * 1_000_003 - 77
    flts = np.arange(n, dtype=np.float64) * 0.375 - 9.0
    flts[0] = flts[3] = 2.0 ** 128   # rows that select `otherwise`: never interpreted
    flts[6] = 1e300
    keep = []
    for f in (Float(flts, 2), Float.on_device(device_array(flts, keep), n, 2)):
        sw = When(P.Like(k="n"), Format(Int(ints), "|", f), Format("s", Col("k")))
        got = run_switch(ctx, cols, sw)
        assert got[1] == [1 if i % 3 == 0 else 0 for i in range(n)]
        assert got[0] == [b"ss" if i % 3 == 0 else M.itoa(ints[i]) + b"|" + M.ftoa(flts[i], 2) for i in range(n)]
    # the same value at rows that select the alternative: refused, the alternative, the piece and the lowest row named
    flts[200] = flts[100] = 2.0 ** 128
    for f in (Float(flts, 2), Float.on_device(device_array(flts, keep), n, 2)):
        with pytest.raises(N.CphError) as ei:
            map_switch(ctx, cols, When(P.Like(k="n"), Format(Int(ints), "|", f), Format("s", Col("k"))))
        assert ei.value.code == N.CPH_ERR_INVALID and "case 0" in str(ei.value) and "piece 2" in str(ei.value) and "row 100" in str(ei.value)
        with pytest.raises(N.CphError) as ei:   # ... and in `otherwise`
            map_switch(ctx, cols, When(P.Like(k="s"), "s", Format(f)))
        assert "otherwise" in str(ei.value) and "piece 0" in str(ei.value) and "row 100" in str(ei.value)
    # an expression: a failing row raises only if it selects the alternative that holds the part
    price = [b"%d.25" % i for i in range(n)]
    price[0] = price[9] = b"none"    # rows of `otherwise`
    etable = {"k": table["k"], "price": price}
    ecols = {k: StrCol.from_values(v, fixed_width=0) for k, v in etable.items()}
    sw = When(P.Like(k="n"), Format("$", Float.of(E.FloatCol("price") * 2.0, 2)), "free")
    assert run_switch(ctx, ecols, sw) == model(sw, etable, n)
    etable["price"][20] = etable["price"][10] = b"bad"   # row 10 selects case 0
    ecols = {k: StrCol.from_values(v, fixed_width=0) for k, v in etable.items()}
    with pytest.raises(E.ExprError) as ee:
        map_switch(ctx, ecols, sw)
    assert ee.value.row == 10 and ee.value.column == "price" and '"bad"' in str(ee.value)


@pytest.mark.gpu
def test_float_compare_column_shared_by_cases(ctx):
    """Two cases compare the same float column (converted once); values that do not convert and the rows the device defers
    to the host side are false / exact as in cph_filter_rows."""
    vals = [b"0.5", b"1e3", b"-2", b"x", b"", b"nan", b"3.0000000000000000000001", b"1e400", b"10", b"0.1"] * 30
    n = len(vals)
    table = {"p": vals, "i": [b"%d" % i for i in range(n)]}
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    sw = Switch((P.FloatCmp("p", "<", 1.0), Format("low ", Col("i"))), (P.FloatCmp("p", ">=", 10.0), Format("high ", Col("p"))),
                (P.Not(P.FloatCmp("p", "==", 3.0)), "odd"), otherwise=Col("p"))
    want = model(sw, table, n)
    assert set(want[1]) == {0, 1, 2, 3}
    assert run_switch(ctx, cols, sw) == want
    assert run_switch(ctx, {k: c.to_device() for k, c in cols.items()}, sw, out_mem=DEVICE) == want


def _switch_call(ctx, cols, ncols, n, cases, otherwise, sel=None, out_mem=HOST, ncases=None, notherwise=None, null=()):
    """cases: [(ops, pieces)]; ops / pieces None = a NULL pointer; pieces: [(kind, arg, literal)]."""
    keep = []

    def pieces_of(pieces):
        arr = (N.cph_map_piece * max(len(pieces), 1))()
        for k, (kind, arg, lit) in enumerate(pieces):
            arr[k].kind, arr[k].arg = kind, arg
            if lit is not None:
                b = np.frombuffer(lit, dtype=np.uint8)
                keep.append(b)
                arr[k].value.data, arr[k].value.len = (b.ctypes.data if len(b) else None), len(b)
        keep.append(arr)
        return arr

    from csvplus_amd.materialize import _pred_program
    carr = (N.cph_map_case * max(len(cases), 1))()
    for c, (ops, pieces) in enumerate(cases):
        if ops is not None:
            prog = _pred_program(ops, keep)
            keep.append(prog)
            carr[c].prog, carr[c].nops = prog, len(ops)
        if pieces is not None:
            carr[c].pieces, carr[c].npieces = pieces_of(pieces), len(pieces)
    oarr = pieces_of(otherwise)
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_switch(ctx.handle, cols, sel, ncols, n, None if "cases" in null else carr, len(cases) if ncases is None else ncases,
                                None if "otherwise" in null else oarr, len(otherwise) if notherwise is None else notherwise, out_mem,
                                None if "out" in null else C.byref(out), None)
    assert not out or rc == N.CPH_OK   # nothing is left in *out on failure
    if out:
        ctx.lib.cph_colbuf_release(out)
    return rc, ctx.last_error()


@pytest.mark.gpu
def test_every_error_has_a_status_and_a_message(ctx):
    a = StrCol.from_values([b"1", b"22", b"1"], fixed_width=0)
    arr = (N.cph_strcol * 2)()
    arr[0], k0 = a.as_c()
    arr[1], k1 = a.as_c()
    LIT, COL = M.LITERAL, M.COLUMN
    like = [(P.LIKE, 0, b"1")]
    x = [(LIT, 0, b"x")]
    ok = [(like, [(COL, 0, None), (LIT, 0, b"-")])]
    assert _switch_call(ctx, arr, 1, 3, ok, x)[0] == N.CPH_OK
    assert _switch_call(ctx, arr, 1, 0, ok, x)[0] == N.CPH_OK                               # no rows
    assert _switch_call(ctx, None, 0, 3, [([(P.ALL, 0, None)], x)], x)[0] == N.CPH_OK       # no columns
    assert _switch_call(ctx, arr, 1, 3, [(like, x)] * 8, x)[0] == N.CPH_OK                  # 8 cases
    assert _switch_call(ctx, arr, 1, 3, [(like, [(COL, 0, None)] * 16)], [(COL, 0, None)] * 16)[0] == N.CPH_OK   # 16 + 16 = 32 pieces
    bad_sel = (N.cph_rowsel * 1)()
    ids = np.zeros(3, np.uint32)
    bad_sel[0].ids, bad_sel[0].bits = ids.ctypes.data, 16
    col16 = [(COL, 0, None)] * 16
    bad = [
        ("NULL cases", dict(null=("cases",))), ("NULL otherwise", dict(null=("otherwise",))), ("NULL out", dict(null=("out",))),
        ("no cases", dict(ncases=0)), ("9 cases", dict(cases=[(like, x)] * 9)),
        ("a case without prog", dict(cases=[(None, x)])), ("a case without pieces", dict(cases=[(like, None)])),
        ("a case of 0 pieces", dict(cases=[(like, [])])), ("a case of 17 pieces", dict(cases=[(like, [(COL, 0, None)] * 17)])),
        ("otherwise of 0 pieces", dict(notherwise=0)), ("otherwise of 17 pieces", dict(otherwise=[(COL, 0, None)] * 17)),
        ("33 pieces in all", dict(cases=[(like, col16), (like, x)], otherwise=col16)),
        ("a program that leaves two values", dict(cases=[(like + like, x)])), ("a program without ops", dict(cases=[([], x)])),
        ("LIKE column 1 of 1", dict(cases=[([(P.LIKE, 1, b"1")], x)])), ("a numeric literal of 3 bytes", dict(cases=[([(P.INT_LT, 0, b"123")], x)])),
        ("piece kind 0", dict(otherwise=[(0, 0, None)])), ("COLUMN 1 of 1 in a case", dict(cases=[(like, [(COL, 1, None)])])),
        ("an INT64 piece without values", dict(otherwise=[(M.INT64, HOST, None)])),
        ("a FLOAT64 piece in memory space 2", dict(otherwise=[(M.FLOAT64, 2, None)])),
        ("short identity column", dict(n=4)), ("long identity column", dict(n=2)), ("row-id bits 16", dict(sel=bad_sel)),
        ("out_mem 2", dict(out_mem=2)), ("17 columns", dict(ncols=17)), ("cols NULL", dict(cols=None)),
    ]
    for what, kw in bad:
        kw = dict(kw)
        rc, msg = _switch_call(ctx, kw.pop("cols", arr), kw.pop("ncols", 1), kw.pop("n", 3), kw.pop("cases", ok), kw.pop("otherwise", x), **kw)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    # the message names the case
    assert "case 1" in _switch_call(ctx, arr, 1, 3, [(like, x), (like + like, x)], x)[1]
    assert "case 1" in _switch_call(ctx, arr, 1, 3, [(like, x), (like, [(COL, 5, None)])], x)[1]
    assert "otherwise" in _switch_call(ctx, arr, 1, 3, ok, [(COL, 5, None)])[1]
    # more rows than the predicate evaluator takes (nothing is read: no column, no array)
    rc, msg = _switch_call(ctx, None, 0, 1 << 32, [([(P.ALL, 0, None)], x)], x)
    assert rc == N.CPH_ERR_TOO_MANY_ROWS and msg
    # NULL ctx: the status alone (there is no ctx to keep a message)
    out = C.POINTER(N.cph_colbuf)()
    p = (N.cph_map_piece * 1)()
    cs = (N.cph_map_case * 1)()
    assert ctx.lib.cph_map_switch(None, arr, None, 1, 3, cs, 1, p, 1, HOST, C.byref(out), None) == N.CPH_ERR_INVALID and not out
    del k0, k1


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("positions", [True, False])
def test_pipeline_long_chain_map(ctx, positions):
    """TestLongChain's Join, Join, Map(if name == Amelia: Julia) and Filter, from CSV text to CSV text on the device."""
    from csvplus_amd import pipeline
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    cv, pv, ov = enc(people_table()), enc(stock_table()), enc(orders_table(n=2000))
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    steps = [(tc, "id", "cust_id"), (tp, "prod_id", "prod_id")]
    plain = [("order_id", to, "order_id"), ("name", tc, "name"), ("surname", tc, "surname"), ("product", tp, "product")]
    julia = When(P.Like(name="Amelia"), "Julia", Col("name"))
    try:
        base = pipeline.join_to_csv(ctx, to, steps, plain, positions=positions, where=P.Like(surname="Smith"))
        rows = [dict(zip(["order_id", "name", "surname", "product"], ln.split(b","))) for ln in base.split(b"\n")[1:] if ln]
        assert rows and any(r["name"] == b"Amelia" for r in rows) and any(r["name"] != b"Amelia" for r in rows)
        lines = [b"order_id,name,surname,product"]
        for r in rows:   # the same pipeline with the host models
            assert P.matches(P.Like(surname="Smith"), r)
            lines.append(b",".join([r["order_id"], M.render(julia, r), r["surname"], r["product"]]))
        outc = [("order_id", to, "order_id"), ("name", None, None), ("surname", tc, "surname"), ("product", tp, "product")]
        got = pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, computed={"name": julia}, where=P.Like(surname="Smith"))
        assert got == b"".join(ln + b"\n" for ln in lines)
        assert b"Amelia" not in got and got.count(b",Julia,") == sum(r["name"] == b"Amelia" for r in rows)
        # an earlier computed name feeds a later Switch
        tagged = pipeline.join_to_csv(ctx, to, steps, [("order_id", to, "order_id"), ("tag", None, None)], positions=positions,
                                      computed={"full": Format(Col("name"), " ", Col("surname")),
                                                "tag": When(P.Like(full="Amelia Smith"), Format("*", Col("full")), Col("product"))},
                                      where=P.Like(surname="Smith"))
        want = [b"order_id,tag"] + [r["order_id"] + b"," + (b"*Amelia Smith" if r["name"] == b"Amelia" else r["product"]) for r in rows]
        assert tagged == b"".join(ln + b"\n" for ln in want)
    finally:
        for t in (tc, tp, to):
            t.release()
