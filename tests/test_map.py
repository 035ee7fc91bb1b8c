"""Map with row templates (csvplus_amd.mapping, cph_map_format) and Validate (materialize.validate_rows): the host model
against pinned answers, the compiler's rules, and — under `-m gpu` — the device against the host model, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.mapping import Col, Const, Format, Int
from helpers import PEOPLE_SURNAMES, orders_table, people_table, stock_table

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
TILE = 256   # kMatThreads: records per tile of the copy kernel

# strconv.Itoa, pinned: 0, -1, 9, 10, 99, 100, 10^k - 1 and 10^k for k = 1..18, the two ends of int64
INT_ANSWERS = [
    (0, b"0"), (-1, b"-1"), (9, b"9"), (10, b"10"), (99, b"99"), (100, b"100"),
    (999, b"999"), (1000, b"1000"), (9999, b"9999"), (10000, b"10000"), (99999, b"99999"), (100000, b"100000"),
    (999999, b"999999"), (1000000, b"1000000"), (9999999, b"9999999"), (10000000, b"10000000"),
    (99999999, b"99999999"), (100000000, b"100000000"), (999999999, b"999999999"), (1000000000, b"1000000000"),
    (9999999999, b"9999999999"), (10000000000, b"10000000000"), (99999999999, b"99999999999"), (100000000000, b"100000000000"),
    (999999999999, b"999999999999"), (1000000000000, b"1000000000000"), (9999999999999, b"9999999999999"),
    (10000000000000, b"10000000000000"), (99999999999999, b"99999999999999"), (100000000000000, b"100000000000000"),
    (999999999999999, b"999999999999999"), (1000000000000000, b"1000000000000000"), (9999999999999999, b"9999999999999999"),
    (10000000000000000, b"10000000000000000"), (99999999999999999, b"99999999999999999"),
    (100000000000000000, b"100000000000000000"), (999999999999999999, b"999999999999999999"),
    (1000000000000000000, b"1000000000000000000"),
    (9223372036854775807, b"9223372036854775807"), (-9223372036854775808, b"-9223372036854775808"),
    (-9, b"-9"), (-10, b"-10"), (-99999999, b"-99999999"), (-100000000, b"-100000000"),
    (-999999999999999999, b"-999999999999999999"), (-1000000000000000000, b"-1000000000000000000"),
]


# ---- CPU: the host model and the compiler -----------------------------------------------------------------------------------
def test_render_integers_known_answers():
    vals = [v for v, _ in INT_ANSWERS]
    assert {0, -1, 9, 10, 99, 100, 2**63 - 1, -2**63} <= set(vals)
    for k in range(1, 19):
        assert 10**k in vals and 10**k - 1 in vals
    t = Format(Int(vals))
    for i, (v, text) in enumerate(INT_ANSWERS):
        assert M.render(t, {}, i) == text and M.itoa(v) == text
    assert M.render(Format(b"[", Int(vals), b"|", Int(vals), b"]"), {}, 39) == b"[-9223372036854775808|-9223372036854775808]"
    with pytest.raises(ValueError):
        Int([2**63])
    with pytest.raises(ValueError):
        Int(np.array([2**63], dtype=np.uint64))


def test_render_known_answers():
    row = {"name": b"Amelia", "surname": "Smith", b"raw": bytes(range(0x80, 0x100)), "nul": b"a\x00b", "empty": b""}
    assert M.render(Const(b"Julia"), row) == b"Julia"
    assert M.render(Const("Jülia"), row) == b"J\xc3\xbclia"
    assert M.render(Format(Col("name"), " ", Col("surname")), row) == b"Amelia Smith"
    assert M.render(Format(Col("name"), Col("name"), b"-", Col("name")), row) == b"AmeliaAmelia-Amelia"   # a column used twice
    assert M.render(Format(Col("empty"), b"", Col("empty")), row) == b""
    assert M.render(Format(Col("empty"), b"x"), row) == b"x"
    assert M.render(Format(b"<", Col("raw"), b">"), row) == b"<" + bytes(range(0x80, 0x100)) + b">"   # bytes keys are found too
    assert M.render(Format(Col("nul"), b"\x00", Col("nul")), row) == b"a\x00b\x00a\x00b"
    assert M.render(Format(b"only ", b"literals"), row) == b"only literals"
    assert M.render(Format(Col("nope", default=b"?"), Col("name")), row) == b"?Amelia"
    assert M.render(Col("name"), row) == b"Amelia"   # a bare part is a template
    with pytest.raises(M.MissingColumn) as e:
        M.render(Format(Col("nope")), row)
    assert str(e.value) == 'missing column "nope"'
    for bad in (lambda r: r, 3, None):
        with pytest.raises(TypeError):
            Format(b"x", bad)
    with pytest.raises(ValueError):
        Format()


def test_compile_rules():
    names, pieces = M.compile(Format(Col("name"), " ", Col("surname"), Col("name")), ["id", "name", "surname"])
    assert names == ["name", "surname"]
    assert pieces == [(M.COLUMN, 0, None), (M.LITERAL, 0, b" "), (M.COLUMN, 1, None), (M.COLUMN, 0, None)]
    # a column the rows lack: its default as a literal (joined with its neighbours), or the reference's error
    names, pieces = M.compile(Format(b"a", Col("nope", default=b"?"), b"b", Col("id")), ["id"])
    assert names == ["id"] and pieces == [(M.LITERAL, 0, b"a?b"), (M.COLUMN, 0, None)]
    with pytest.raises(M.MissingColumn) as e:
        M.compile(Format(Col("nope")), ["id"])
    assert str(e.value) == 'missing column "nope"' and e.value.column == "nope"
    names, pieces = M.compile(Const(b""), [])
    assert names == [] and pieces == [(M.LITERAL, 0, b"")]
    ints = Int([1, 2, 3])
    assert M.compile(Format(ints, b"x"), [])[1] == [(M.INT64, 0, ints), (M.LITERAL, 0, b"x")]
    # limits: 16 pieces, 16 columns
    sixteen = [Col(f"c{i}") for i in range(16)]
    assert len(M.compile(Format(*sixteen), [f"c{i}" for i in range(16)])[1]) == 16
    with pytest.raises(ValueError):
        M.compile(Format(*sixteen, Col("c0")), [f"c{i}" for i in range(16)])
    alternating = [p for i in range(9) for p in (Col("a"), b"-")]
    with pytest.raises(ValueError):
        M.compile(Format(*alternating), ["a"])
    assert len(M.compile(Format(*alternating[:16]), ["a"])[1]) == 16
    assert len(M.compile(Format(*[b"x"] * 40), [])[1]) == 1   # literals join: no limit on their number


def test_compile_reads_an_earlier_computed_name():
    """Templates applied in order: the second one's Col names the first one's result once it is among the row's columns."""
    computed = {"full": Format(Col("name"), " ", Col("surname")), "tag": Format(Col("full"), "#", Col("id"))}
    known = ["id", "name", "surname"]
    with pytest.raises(M.MissingColumn):
        M.compile(computed["tag"], known)
    row = {"id": "7", "name": "Ava", "surname": "Jones"}
    for name, t in computed.items():
        M.compile(t, known)
        row[name] = M.render(t, row)
        known.append(name)
    assert row["tag"] == b"Ava Jones#7"
    assert M.columns(computed["tag"]) == ["full", "id"]


def test_validate_model_is_take_while():
    """validate_rows answers "index of the first failing row": select_rows(mode="take_while") stops right in front of it."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, 64):
        for _ in range(20):
            flags = (rng.random(n) < 0.8).tolist()
            for first_row in {0, n // 2, n}:
                kept = P.select_rows(flags, mode="take_while", first_row=first_row)
                fails = [i for i in range(first_row, n) if not flags[i]]
                assert kept == list(range(first_row, fails[0] if fails else n))


def test_map_struct_size_against_the_compiled_header(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %d %d %d %d\\n", sizeof(cph_map_piece), offsetof(cph_map_piece, value), offsetof(cph_map_piece, ints),'
                   ' CPH_MAP_LITERAL, CPH_MAP_COLUMN, CPH_MAP_INT64, CPH_MAP_MAX_PIECES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(root / "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [C.sizeof(N.cph_map_piece), N.cph_map_piece.value.offset, N.cph_map_piece.ints.offset,
                   M.LITERAL, M.COLUMN, M.INT64, M.MAX_PIECES]
    assert (N.CPH_MAP_LITERAL, N.CPH_MAP_COLUMN, N.CPH_MAP_INT64, N.CPH_MAP_MAX_PIECES) == (M.LITERAL, M.COLUMN, M.INT64, M.MAX_PIECES)


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


def run_map(ctx, cols, template, row_ids=None, nrows=None, out_mem=HOST):
    from csvplus_amd.materialize import map_column
    cb = map_column(ctx, cols, template, row_ids=row_ids, nrows=nrows, out_mem=out_mem)
    try:
        assert cb.mem == out_mem
        return colbuf_values(cb)
    finally:
        cb.release()


def model(template, table, n, row_of=None):
    """The template over rows 0..n-1; row_of(i) -> {name: row of that column feeding output row i} (default: i)."""
    out = []
    for i in range(n):
        src = row_of(i) if row_of else {}
        out.append(M.render(template, {k: v[src.get(k, i)] for k, v in table.items()}, i))
    return out


def device_array(a, keep):
    import torch
    t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0") if a.nbytes else torch.empty(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    keep.append(t)
    return t.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("out_mem", [HOST, DEVICE])
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts_around_the_tile(ctx, n, out_mem):
    rng = np.random.default_rng(n)
    table = {"a": [b"v%d" % i for i in range(n)], "b": [bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)) for _ in range(n)]}
    ints = Int(rng.integers(-10**6, 10**6, n))
    t = Format(Col("a"), b"=", Col("b"), b";", ints, Col("a"))
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    assert run_map(ctx, cols, t, nrows=n, out_mem=out_mem) == model(t, table, n)
    assert run_map(ctx, {}, Format(b"#", ints), nrows=n, out_mem=out_mem) == model(Format(b"#", ints), {}, n)   # no columns at all


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_value_lengths_and_alignments(ctx, device):
    """Lengths 0..17 at every alignment 0..7 of the data block, in every column; rows whose output is empty; a column that
    is empty in every row."""
    n = 3000
    rng = np.random.default_rng(17)
    table = {}
    for name in ("a", "b"):
        lens = rng.integers(0, 18, n)
        table[name] = [bytes(rng.integers(0, 256, int(ln), dtype=np.uint8)) for ln in lens]
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        assert len({(int(s) % 8, int(ln)) for s, ln in zip(starts, lens)}) == 8 * 18
    table["c"] = [b""] * n
    cols = {k: StrCol.from_values(v, fixed_width=0) for k, v in table.items()}
    assert cols["c"].fixed_width == 0
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
    t = Format(Col("a"), Col("c"), Col("b"), Col("a"))
    want = model(t, table, n)
    assert sum(1 for w in want if not w) >= 2 and {len(w) % 4 for w in want} == {0, 1, 2, 3}
    assert run_map(ctx, cols, t, out_mem=DEVICE if device else HOST) == want
    assert run_map(ctx, cols, Format(Col("c"), Col("c"))) == [b""] * n   # nothing to copy at all
    assert run_map(ctx, cols, Format(Col("c"), b"", Col("c"), b"xyz")) == [b"xyz"] * n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [TILE, TILE + 44])
def test_a_tile_beyond_the_stage(ctx, n):
    """256 rows of 100-byte values: 25 600 bytes, more than the 16 KB stage — the tile writes to global memory itself; the
    44 rows behind it fit the stage again."""
    rng = np.random.default_rng(3)
    table = {"a": [bytes(rng.integers(0, 256, 100, dtype=np.uint8)) for _ in range(n)]}
    col = StrCol.from_values(table["a"])
    assert col.fixed_width == 100
    t = Format(Col("a"))
    for c in (col, col.as_variable()):
        assert run_map(ctx, {"a": c}, t) == table["a"]
    t2 = Format(b"k=", Col("a"), b"\n")
    assert run_map(ctx, {"a": col.to_device()}, t2, out_mem=DEVICE) == model(t2, table, n)


@pytest.mark.gpu
def test_staged_and_unstaged_tiles_in_one_launch(ctx):
    """One 40 000-byte value among 600 short ones: its tile goes to global memory, the tiles around it through the stage."""
    rng = np.random.default_rng(4)
    table = {"a": [bytes(rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8)) for _ in range(601)]}
    table["a"][300] = bytes(rng.integers(0, 256, 40_000, dtype=np.uint8))
    ints = Int(np.arange(601) - 300)
    t = Format(Col("a"), b"|", ints, b"|", Col("a"))
    assert run_map(ctx, {"a": StrCol.from_values(table["a"])}, t) == model(t, table, 601)


LAYOUTS = ["fixed", "offsets32", "offsets64"]
ID_KINDS = ["identity", "ids32", "ids64", "ids32_base"]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("id_kind", ID_KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_column_layouts_memory_and_row_ids(ctx, layout, id_kind, device):
    nsrc, n = 40, 300 if id_kind != "identity" else 40
    rng = np.random.default_rng(11)
    if layout == "fixed":
        vals = [b"%05d" % (i * 7) for i in range(nsrc)]
        col = StrCol.from_values(vals)
        assert col.fixed_width == 5
    else:
        vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(nsrc)]
        col = StrCol.from_values(vals, offset_bits=32 if layout == "offsets32" else 64, fixed_width=0)
    other = [b"o%d" % i for i in range(n)]   # an identity column beside the one read through row ids
    cols = {"v": col, "o": StrCol.from_values(other, fixed_width=0)}
    keep, row_ids, src = [], None, None
    if id_kind != "identity":
        src = np.concatenate([np.arange(nsrc)[::-1], [3, 3, 3], rng.integers(0, nsrc, n - nsrc - 3)])   # reversed, repeated, random
        base = 1000 if id_kind == "ids32_base" else 0
        ids = (src + base).astype(np.uint64 if id_kind == "ids64" else np.uint32)
        if device:
            row_ids = {"v": (device_array(ids, keep), ids.dtype.itemsize * 8, n, base)}
        else:
            row_ids = {"v": (ids, base)}
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
    t = Format(Col("o"), b":", Col("v"), b"/", Col("v"))
    want = model(t, {"v": vals, "o": other}, n, (lambda i: {"v": int(src[i])}) if src is not None else None)
    assert run_map(ctx, cols, t, row_ids=row_ids, nrows=n, out_mem=DEVICE if device else HOST) == want


@pytest.mark.gpu
def test_int64_pieces_from_host_and_device(ctx):
    from csvplus_amd.materialize import to_int
    vals = np.array([v for v, _ in INT_ANSWERS], dtype=np.int64)
    want = [text for _, text in INT_ANSWERS]
    assert run_map(ctx, {}, Format(Int(vals))) == want
    keep = []
    dev = Int.on_device(device_array(vals, keep), len(vals))
    assert run_map(ctx, {}, Format(dev), out_mem=DEVICE) == want
    t = Format(b"<", Int(vals), b",", dev, b">")
    assert run_map(ctx, {}, t, nrows=len(vals)) == [b"<" + w + b"," + w + b">" for w in want]
    # chained from to_int: convert a column, add 1 on the device, write it back as a column
    import torch
    texts = [b"%d" % v for v in (0, -1, 9, 99, -100, 12345678901234, 9223372036854775806, -9223372036854775808)] * 70
    nc = to_int(ctx, StrCol.from_values(texts).to_device(), out_mem=DEVICE)
    assert nc.nerrors == 0
    ptr, cnt = nc.values
    plus = torch.empty(cnt, dtype=torch.int64, device="cuda:0")
    assert _hip().hipMemcpy(C.c_void_p(plus.data_ptr()), C.c_void_p(ptr), C.c_size_t(cnt * 8), 3) == 0   # device to device
    plus += 1
    torch.cuda.synchronize()
    nc.release()
    host = Int([int(x) + 1 for x in texts])
    assert run_map(ctx, {}, Format(Int.on_device(plus.data_ptr(), cnt), b"!")) == model(Format(host, b"!"), {}, cnt)


def _joined_fixture():
    people, orders = people_table(), orders_table(n=3000)
    orders["cust_id"][7] = "99999"   # orders without a customer: the joined rows are not the stream's rows
    orders["cust_id"][2900] = "-1"
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    return enc(people), enc(orders)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_template_over_joined_rows(ctx, device):
    """orders.Join(people): stream and build columns read through the chain's row ids, against the template rendered over
    the joined rows the oracle reports."""
    from csvplus_amd import DeviceIndex, join_chain
    from oracle import orc
    people, orders = _joined_fixture()
    pc = {k: StrCol.from_values(v, fixed_width=0) for k, v in people.items()}
    oc = {k: StrCol.from_values(v, fixed_width=0) for k, v in orders.items()}
    oj = orc.OracleIndex([pc["id"]]).join([oc["cust_id"]])
    m = int(oj["nmatches"])
    assert m == 2998
    ix = DeviceIndex(ctx, [pc["id"]], unique=True)
    ch = join_chain(ctx, [(ix, [oc["cust_id"]])])
    srow, brow = ch.stream_row, ch.build_row(0)
    ch.release()
    np.testing.assert_array_equal(srow, oj["probe_idx"])
    np.testing.assert_array_equal(brow, oj["build_row"])
    t = Format(Col("name"), b" ", Col("surname"), b" ordered ", Col("qty"), b" of #", Col("prod_id"), b" (", Col("order_id"), b")")
    want = []
    for k in range(m):
        row = {c: v[int(oj["probe_idx"][k])] for c, v in orders.items()}
        row.update({c: v[int(oj["build_row"][k])] for c, v in people.items()})
        want.append(M.render(t, row))
    cols = {"name": pc["name"], "surname": pc["surname"], "qty": oc["qty"], "prod_id": oc["prod_id"], "order_id": oc["order_id"]}
    keep = []
    if device:
        cols = {k: c.to_device() for k, c in cols.items()}
        s, b = (device_array(srow, keep), 64, m), (device_array(brow, keep), 32, m)
    else:
        s, b = srow, brow
    ids = {"name": b, "surname": b, "qty": s, "prod_id": s, "order_id": s}
    assert run_map(ctx, cols, t, row_ids=ids, nrows=m, out_mem=DEVICE if device else HOST) == want
    ix.close()


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("positions", [True, False])
def test_pipeline_computed_columns(ctx, positions):
    import json

    from csvplus_amd import pipeline
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    cv, pv, ov = enc(people_table()), enc(stock_table()), enc(orders_table(n=2000))
    ov["cust_id"][5] = b"99999"
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    steps = [(tc, "id", "cust_id"), (tp, "prod_id", "prod_id")]
    plain = [("order_id", to, "order_id"), ("name", tc, "name"), ("surname", tc, "surname"), ("product", tp, "product"), ("qty", to, "qty")]
    try:
        base = pipeline.join_to_csv(ctx, to, steps, plain, positions=positions)
        assert pipeline.join_to_csv(ctx, to, steps, plain, positions=positions, computed=None) == base   # the default: nothing changes
        body = [ln.split(b",") for ln in base.split(b"\n")[1:] if ln]
        assert len(body) == 1999
        computed = {"full": Format(Col("name"), " ", Col("surname")),
                    "text": Format(Col("full"), " bought ", Col("qty"), " ", Col("product"), "s at ", Col("price"), Col("nope", default="!")),
                    "name": Const("Julia")}   # row["name"] = "Julia" replaces the source column, behind the templates that read it
        outc = [("order_id", to, "order_id"), ("name", None, None), ("text", None, None), ("surname", tc, "surname"), ("full", None, None)]
        price = dict(zip(pv["product"], pv["price"]))

        def expect(rows):
            lines = [b"order_id,name,text,surname,full"]
            for oid, name, surname, product, qty in rows:
                full = name + b" " + surname
                lines.append(b",".join([oid, b"Julia", full + b" bought " + qty + b" " + product + b"s at " + price[product] + b"!", surname, full]))
            return b"".join(ln + b"\n" for ln in lines)

        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, computed=computed) == expect(body)
        smiths = [r for r in body if r[2] == b"Smith"][1:6]
        assert len(smiths) == 5
        got = pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, computed=computed, where=P.Like(surname="Smith"), skip=1, limit=5)
        assert got == expect(smiths)
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, computed=computed, where=P.Like(surname="Nobody")) == expect([])
        js = json.loads(pipeline.join_to_json(ctx, to, steps, positions=positions, computed={"full": computed["full"], "name": Const("Julia")},
                                              where=P.Like(surname="Smith"), limit=3))
        assert [(d["order_id"], d["name"], d["full"]) for d in js] == \
            [(r[0].decode(), "Julia", (r[1] + b" " + r[2]).decode()) for r in body if r[2] == b"Smith"][:3]
        assert "price" in js[0] and "nope" not in js[0]
        # one table: Filter(Like(name: Amelia)).Map(name = Julia).ToCsv(name, surname) — the reference README's first example
        am = pipeline.filter_to_csv(ctx, tc, P.Like(name="Amelia"), ["name", "surname"], computed={"name": Const("Julia")})
        assert am == b"name,surname\n" + b"".join(b"Julia,%s\n" % s.encode() for s in PEOPLE_SURNAMES)
        assert pipeline.filter_to_csv(ctx, tc, P.Like(name="Amelia"), ["name", "surname"], computed=None) == \
            pipeline.filter_to_csv(ctx, tc, P.Like(name="Amelia"), ["name", "surname"])
        tw = pipeline.filter_to_csv(ctx, tc, P.Like(name="Amelia"), ["id", "tag"], mode="take_while", skip=10,
                                    computed={"tag": Format(Col("surname"), "#", Col("id"))})
        assert tw == b"id,tag\n10,Johnson#10\n11,Lewis#11\n"
        with pytest.raises(M.MissingColumn):
            pipeline.join_to_csv(ctx, to, steps, [("order_id", to, "order_id"), ("full", None, None)], positions=positions,
                                 computed={"full": Format(Col("nope"))})
        with pytest.raises(ValueError):   # an output column without a table that no template computes
            pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, computed={"full": computed["full"]})
    finally:
        for t in (tc, tp, to):
            t.release()


@pytest.mark.gpu
def test_computed_column_as_an_index_key(ctx):
    """IndexOn over the computed `name + " " + surname`: the column is an ordinary identity column for cph_index_build."""
    from csvplus_amd import DeviceIndex
    from csvplus_amd.materialize import map_column
    from helpers import assert_join_equal
    from oracle import orc
    people = people_table()
    cols = {k: StrCol.from_values(v).to_device() for k, v in people.items()}
    t = Format(Col("name"), " ", Col("surname"))
    cb = map_column(ctx, cols, t, out_mem=DEVICE)
    full = [M.render(t, {k: v[i] for k, v in people.items()}) for i in range(120)]
    assert colbuf_values(cb) == full
    ix = DeviceIndex(ctx, [cb.as_device_strcol()], unique=True)
    o = orc.OracleIndex([StrCol.from_values(full)])
    assert ix.status == N.CPH_OK
    np.testing.assert_array_equal(ix.perm(), o.perm)
    probe = StrCol.from_values([b"Ava Jones", b"Nobody Here", b"Jack Lewis", b"Ava Jones", b"Ava  Jones", b""])
    assert_join_equal(ix.probe([probe]), o.join([probe]))
    assert ix.find(b"Jack Lewis") == o.find(b"Jack Lewis")
    ix.close()
    cb.release()


def _map_call(ctx, cols, ncols, n, pieces, sel=None, out_mem=HOST, null_pieces=False, null_out=False):
    keep = []
    arr = (N.cph_map_piece * max(len(pieces), 1))()
    for k, (kind, arg, lit, ints) in enumerate(pieces):
        arr[k].kind, arr[k].arg = kind, arg
        if lit is not None:
            b = np.frombuffer(lit, dtype=np.uint8)
            keep.append(b)
            arr[k].value.data, arr[k].value.len = (b.ctypes.data if len(b) else None), len(b)
        if ints is not None:
            keep.append(ints)
            arr[k].ints = ints.ctypes.data
    out = C.POINTER(N.cph_colbuf)()
    rc = ctx.lib.cph_map_format(ctx.handle, cols, sel, ncols, n, None if null_pieces else arr, len(pieces), out_mem,
                                None if null_out else C.byref(out))
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
    LIT, COL, INT = M.LITERAL, M.COLUMN, M.INT64
    three = np.array([1, 2, 3], dtype=np.int64)
    ok = [(COL, 0, None, None), (LIT, 0, b"-", None), (INT, HOST, None, three)]
    assert _map_call(ctx, arr, 1, 3, ok)[0] == N.CPH_OK
    assert _map_call(ctx, None, 0, 3, ok[1:])[0] == N.CPH_OK                        # ncols 0, cols NULL
    assert _map_call(ctx, arr, 1, 0, ok)[0] == N.CPH_OK                             # no rows
    assert _map_call(ctx, None, 0, 0, [(INT, HOST, None, None)])[0] == N.CPH_OK     # ints NULL is fine without rows
    assert _map_call(ctx, arr, 1, 3, [(COL, 0, None, None)] * 16)[0] == N.CPH_OK    # exactly at the limit
    bad_sel = (N.cph_rowsel * 1)()
    ids = np.zeros(3, np.uint32)
    bad_sel[0].ids, bad_sel[0].bits = ids.ctypes.data, 16
    bad = [
        ("NULL pieces", dict(pieces=ok, null_pieces=True)), ("NULL out", dict(pieces=ok, null_out=True)),
        ("no pieces", dict(pieces=[])), ("17 pieces", dict(pieces=[(COL, 0, None, None)] * 17)),
        ("kind 0", dict(pieces=[(0, 0, None, None)])), ("kind 4", dict(pieces=[(4, 0, None, None)])),
        ("column 1 of 1", dict(pieces=[(COL, 1, None, None)])), ("column -1", dict(pieces=[(COL, -1, None, None)])),
        ("column without columns", dict(pieces=[(COL, 0, None, None)], ncols=0)),
        ("ints NULL", dict(pieces=[(INT, HOST, None, None)])), ("ints in memory space 2", dict(pieces=[(INT, 2, None, three)])),
        ("short identity column", dict(pieces=ok, n=4)), ("long identity column", dict(pieces=ok, n=2)),
        ("row-id bits 16", dict(pieces=ok, sel=bad_sel)),
        ("out_mem 2", dict(pieces=ok, out_mem=2)), ("17 columns", dict(pieces=ok, ncols=17)), ("cols NULL", dict(pieces=ok, cols=None)),
    ]
    for what, kw in bad:
        kw = dict(kw)
        rc, msg = _map_call(ctx, kw.pop("cols", arr), kw.pop("ncols", 1), kw.pop("n", 3), kw.pop("pieces"), **kw)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    # a literal with a length but no pointer
    p = (N.cph_map_piece * 1)()
    p[0].kind, p[0].value.len = LIT, 3
    out = C.POINTER(N.cph_colbuf)()
    assert ctx.lib.cph_map_format(ctx.handle, arr, None, 1, 3, p, 1, HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert "pointer" in ctx.last_error() and not out
    # NULL ctx: the status alone (there is no ctx to keep a message)
    assert ctx.lib.cph_map_format(None, arr, None, 1, 3, p, 1, HOST, C.byref(out)) == N.CPH_ERR_INVALID and not out
    del k0, k1


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_validate_rows(ctx, device):
    """All rows pass; the first / the last row fails; the failing row around the predicate kernel's 2048-row tile; the same
    over a first_row window."""
    from csvplus_amd.materialize import validate_rows
    n = 5000
    pred = P.All(P.IntCmp("born", ">", 1800), P.Not(P.Like(name="")))

    def check(bad_rows, first_row=0, nrows=None):
        born = [b"1950"] * n
        for r in bad_rows:
            born[r] = b"1492"
        cols = {"born": StrCol.from_values(born), "name": StrCol.from_values([b"n%d" % i for i in range(n)], fixed_width=0)}
        if device:
            cols = {k: c.to_device() for k, c in cols.items()}
        flags = [b != b"1492" for b in born]
        kept = P.select_rows(flags, mode="take_while", first_row=first_row, nrows=nrows)
        end = first_row + (n - first_row if nrows is None else nrows)
        want = None if len(kept) == end - first_row else first_row + len(kept)
        assert validate_rows(ctx, cols, pred, first_row=first_row, nrows=nrows) == want
        return want

    assert check([]) is None
    assert check([0]) == 0
    assert check([n - 1]) == n - 1
    for r in (2047, 2048, 2049):
        assert check([r, 4000]) == r
        assert check([r], first_row=r + 1) is None          # the window starts behind the bad row
        assert check([5, r], first_row=6) == r              # ... or between two of them
        assert check([r], first_row=100, nrows=r - 100) is None   # ... or ends right in front of it
        assert check([r], first_row=100, nrows=r - 99) == r
    assert check([10], first_row=n) is None                 # an empty window
