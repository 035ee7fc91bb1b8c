"""ToJSON (csvplus.go:446-480) on the device: cph_json_write_rows / materialize.json_write / pipeline.join_to_json against a
byte-level restatement of what the reference writes — json.Encoder.Encode(row) per row (Go >= 1.22 encoding/json,
SetIndent("", ""), SetEscapeHTML(false)), ',' between rows, the whole in '[' ... ']'.

Python's json.dumps is no reference here (it leaves U+2028 / U+2029 alone and takes str), nor is bytes.decode("utf-8",
"replace") (it folds a truncated sequence into one U+FFFD where Go writes one per byte): the restatement below walks the
bytes as Go's appendString and utf8.DecodeRuneInString do, and the known answers pin it."""
import ctypes as C
import functools
import hashlib
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent


# ---- the restatement -------------------------------------------------------------------------------------------------
def _utf8_size(b: bytes, i: int) -> int:
    """utf8.DecodeRuneInString on b[i:] (b[i] >= 0x80): the size of a valid sequence, 0 for RuneError of size 1."""
    c = b[i]
    if c < 0xC2 or c > 0xF4:
        return 0
    sz = 2 if c < 0xE0 else 3 if c < 0xF0 else 4
    if len(b) - i < sz:
        return 0
    lo = 0xA0 if c == 0xE0 else 0x90 if c == 0xF0 else 0x80
    hi = 0x9F if c == 0xED else 0x8F if c == 0xF4 else 0xBF
    if not lo <= b[i + 1] <= hi:
        return 0
    for k in range(2, sz):
        if b[i + k] & 0xC0 != 0x80:
            return 0
    return sz


_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def go_string(b: bytes) -> bytes:
    """encoding/json appendString(b, escapeHTML=false), Go >= 1.22 (\\b and \\f; earlier releases wrote \\u0008, \\u000c)."""
    out = bytearray(b'"')
    i = 0
    while i < len(b):
        c = b[i]
        if c < 0x80:
            i += 1
            if c in _SHORT:
                out += _SHORT[c]
            elif c < 0x20:
                out += b"\\u00%02x" % c
            else:
                out.append(c)
            continue
        sz = _utf8_size(b, i)
        if sz == 0:
            out += b"\\ufffd"
            i += 1
            continue
        seq = b[i:i + sz]
        if seq in (b"\xe2\x80\xa8", b"\xe2\x80\xa9"):
            out += b"\\u202" + (b"8" if seq[2] == 0xA8 else b"9")
        else:
            out += seq
        i += sz
    out.append(0x22)
    return bytes(out)


def go_record(names, row, enc=go_string) -> bytes:
    """json.Encoder.Encode of a map[string]string: keys in byte order, compact, '\\n' after the value."""
    keys = sorted(range(len(names)), key=lambda c: names[c])
    return b"{" + b",".join(enc(names[c]) + b":" + enc(row[c]) for c in keys) + b"}\n"


def go_to_json(names, rows, enc=go_string) -> bytes:
    """DataSource.ToJSON (csvplus.go:446-480): '[', the records with ',' in front of all but the first, ']'."""
    names = [n.encode() if isinstance(n, str) else n for n in names]
    return b"[" + b",".join(go_record(names, r, enc) for r in rows) + b"]"


KNOWN = [   # (input, the encoded string), computed by hand from the rules
    (b'q"\\', b'"q\\"\\\\"'),
    (b"\x01\x08\x0c\x7f", b'"\\u0001\\b\\f\x7f"'),
    (b"\xe2\x80\xa8<&>\xef\xbf\xbd", b'"\\u2028<&>\xef\xbf\xbd"'),
    (b"\xf0\x9f\x98", b'"\\ufffd\\ufffd\\ufffd"'),   # truncated: one per byte
    (b"\xed\xa0\x80", b'"\\ufffd\\ufffd\\ufffd"'),   # surrogate
    (b"\xc0\xaf", b'"\\ufffd\\ufffd"'),              # overlong
    (b"\xe2\x82\xac", b'"\xe2\x82\xac"'),            # the euro sign, as it is
]


# ---- CPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw,enc", KNOWN)
def test_restatement_known_answers(raw, enc):
    assert go_string(raw) == enc


def test_restatement_whole_outputs():
    rows = [[b"x", b"1"], [b'q"\\', b"\x01\x08\x0c\x7f"]]
    assert go_to_json([b"b", b"a"], rows) == b'[{"a":"1","b":"x"}\n,{"a":"\\u0001\\b\\f\x7f","b":"q\\"\\\\"}\n]'
    names = ["B", "a", "é", "_"]
    rec = go_to_json(names, [[b"1", b"2", b"3", b"4"]])
    assert [m.decode() for m in re.findall(rb'"([^"]+)":', rec)] == ["B", "_", "a", "é"]
    assert go_to_json(["a"], []) == b"[]"


def test_restatement_agrees_with_python_json_on_plain_text():
    """Where json.dumps is a valid reference (valid UTF-8 without U+2028 / U+2029, ensure_ascii off) the two agree."""
    vals = ["plain", 'q"uote', "back\\slash", "tab\there", "nl\n", "\x00\x1f", "é€😀", "<&>", "\x7f"]
    for v in vals:
        assert go_string(v.encode()) == json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode()


def test_symbol_declared_exported_and_bound():
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    assert re.search(r"CPH_API int32_t cph_json_write_rows\(", hdr)
    assert any(p[0] == "cph_json_write_rows" for p in N.PROTOTYPES)
    lib = N.load_library()
    assert hasattr(lib, "cph_json_write_rows")
    syms = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT cph_json_write_rows\b", syms)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
SPECIAL = [b'"', b"\\", b"\x00", b"\x08", b"\x0c", b"\n", b"\r", b"\t", b"\x1f", b"\x7f", b"\xe2\x80\xa8", b"\xe2\x80\xa9",
           b"\xef\xbf\xbd", b"\xc3\xa9", b"\xf0\x9f\x98\x80", b"\xff", b"\x80", b"\xed\xa0\x80", b"\xc0\xaf"]
VOCAB = [b"", b"plain", b"1234567", b"12345678", b"123456789", b"x" * 40, b"<a&b>", b"caf\xc3\xa9 \xe2\x82\xac"] + \
        [raw for raw, _ in KNOWN] + SPECIAL + [b"ab" + s + b"cdefghij" for s in SPECIAL]


def _hip():
    """The HIP runtime this process already uses (torch loaded it): for reading a DeviceBytes result back."""
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def write(ctx, cols, names, **kw):
    """materialize.json_write; a DEVICE result is copied back and released."""
    from csvplus_amd.materialize import json_write
    out = json_write(ctx, cols, names, **kw)
    if kw.get("out_mem") != N.CPH_MEM_DEVICE:
        return out
    n = len(out)
    buf = (C.c_char * (n + 1))()
    if n:
        assert _hip().hipMemcpy(buf, C.c_void_p(out.data_ptr), C.c_size_t(n), 2) == 0   # hipMemcpyDeviceToHost
    out.release()
    return bytes(buf)[:n]


def check(ctx, columns, names, **kw):
    cols = [StrCol.from_values(c) for c in columns]
    rows = list(zip(*columns)) if columns and columns[0] else []
    assert write(ctx, cols, names, **kw) == go_to_json(names, rows)


@pytest.mark.gpu
def test_known_answers_one_value_per_row(ctx):
    vals = [raw for raw, _ in KNOWN]
    got = write(ctx, [StrCol.from_values(vals)], ["v"])
    assert got == b"[" + b",".join(b'{"v":' + enc + b"}\n" for _, enc in KNOWN) + b"]"


@pytest.mark.gpu
def test_known_answers_as_records(ctx):
    vals = [raw for raw, _ in KNOWN]
    cols = [vals[k:] + vals[:k] for k in range(len(vals))]
    check(ctx, cols, [f"c{k}" for k in range(len(vals))])
    check(ctx, [[b"x", b'q"\\'], [b"1", b"\x01\x08\x0c\x7f"]], ["b", "a"])
    assert write(ctx, [StrCol.from_values([b"x", b'q"\\']), StrCol.from_values([b"1", b"\x01\x08\x0c\x7f"])], ["b", "a"]) == \
        b'[{"a":"1","b":"x"}\n,{"a":"\\u0001\\b\\f\x7f","b":"q\\"\\\\"}\n]'


@pytest.mark.gpu
def test_every_single_byte(ctx):
    vals = [bytes([b]) for b in range(256)]
    check(ctx, [vals], ["b"])
    check(ctx, [vals, [v * 9 for v in vals]], ["one", "nine"])


@pytest.mark.gpu
def test_special_bytes_at_every_offset(ctx):
    """Each special sequence at offsets 0..17 of a value: across the 8-byte chunks of the classifier and the escape path."""
    vals = [b"a" * k + s + b"z" * (k % 5) for s in SPECIAL for k in range(18)]
    check(ctx, [vals], ["v"])
    check(ctx, [vals, vals[::-1], [b"clean value %d" % i for i in range(len(vals))]], ["v", "w", "x"])


@pytest.mark.gpu
def test_truncated_sequences_at_the_end(ctx):
    heads = [b"\xc3", b"\xe2", b"\xe2\x80", b"\xf0", b"\xf0\x9f", b"\xf0\x9f\x98", b"\xf4\x8f\xbf", b"\xe0\xa0"]
    vals = [b"p" * k + h for h in heads for k in range(17)]
    check(ctx, [vals], ["t"])


@pytest.mark.gpu
def test_empty_values_and_zero_rows(ctx):
    check(ctx, [[b""] * 300, [b"", b"x"] * 150], ["e", "f"])
    assert write(ctx, [StrCol.from_values([])], ["a"]) == b"[]"
    assert write(ctx, [StrCol.from_values([])], ["a"], out_mem=N.CPH_MEM_DEVICE) == b"[]"


@pytest.mark.gpu
def test_names_sorted_and_escaped(ctx):
    names = ["B", "a", "é", "_"]
    got = write(ctx, [StrCol.from_values([b"1"]), StrCol.from_values([b"2"]), StrCol.from_values([b"3"]),
                      StrCol.from_values([b"4"])], names)
    assert got == b'[{"B":"1","_":"4","a":"2","\xc3\xa9":"3"}\n]'
    odd = [b'k"ey', b"\xe2\x80\xa8", b"\x01", b"\xff"]
    check(ctx, [[b"v%d" % c] * 3 for c in range(4)], odd)


def _device_ids(ids, bits):
    import torch
    return torch.tensor(ids.astype(np.int64 if bits == 64 else np.int32), device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", [1, 2, 3, 5, 8, 9, 12, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_random_tables(ctx, ncols, n):
    rng = np.random.default_rng(ncols * 10007 + n)
    names = [f"col{c:02d}" for c in rng.permutation(ncols)]
    tables = [[VOCAB[i] for i in rng.integers(0, len(VOCAB), 300)] for _ in range(ncols)]
    ids = [rng.integers(0, 300, n) for _ in range(ncols)]
    rows = [[tables[c][ids[c][i]] for c in range(ncols)] for i in range(n)]
    want = go_to_json(names, rows)
    hcols = [StrCol.from_values(t) for t in tables]
    # host columns, 32- and 64-bit host row ids, host output
    host_ids = [ids[c].astype(np.uint64 if c % 2 else np.uint32) for c in range(ncols)]
    assert write(ctx, hcols, names, row_ids=host_ids, nrows=n) == want
    base = 1000
    # device columns, device row ids (32 / 64 bits, non-zero base), device and host output
    dcols = [c.to_device() for c in hcols]
    keep = []
    dsel = []
    for c in range(ncols):
        bits = 64 if c % 2 else 32
        t = _device_ids(ids[c] + base, bits)
        keep.append(t)
        dsel.append((t.data_ptr() if n else 0, bits, n, base))
    assert write(ctx, dcols, names, row_ids=dsel, nrows=n) == want
    assert write(ctx, dcols, names, row_ids=dsel, nrows=n, out_mem=N.CPH_MEM_DEVICE) == want
    # identity columns
    if n:
        icols = [StrCol.from_values([r[c] for r in rows]) for c in range(ncols)]
        assert write(ctx, icols, names) == want
        assert write(ctx, [c.to_device() for c in icols], names, out_mem=N.CPH_MEM_DEVICE) == want


@pytest.mark.gpu
def test_more_tiles_than_the_grid(ctx):
    """grid_rows caps the grid at 4096 workgroups of 256 rows: 1.1e6 rows give each workgroup two tiles or more."""
    rng = np.random.default_rng(7)
    vocab = VOCAB[:12]
    idx = rng.integers(0, len(vocab), (1_100_000, 2))
    cols = [[vocab[i] for i in idx[:, c]] for c in range(2)]
    enc = functools.lru_cache(maxsize=None)(go_string)
    got = write(ctx, [StrCol.from_values(c) for c in cols], ["b", "a"])
    assert got == go_to_json(["b", "a"], list(zip(*cols)), enc)


@pytest.mark.gpu
def test_records_beyond_the_stage(ctx):
    """A 20 KB value in a tile of short records (staged), tiles of 2 x 20 KB and of 300 x 200 B (beyond the 32 KB stage:
    the records are written to global memory directly), with bytes to escape in them."""
    big = (b"0123456789abcde\n" * 1280)[:20_000]
    esc = (b"ab\"c\\\x01\xe2\x80\xa8\xf0\x9f\x98\x80\xff" * 1500)[:20_000]
    short = [b"s%d" % i for i in range(600)]
    check(ctx, [short[:100] + [big] + short[:100], short[:201]], ["v", "w"])
    check(ctx, [[big, esc] + short[:300] + [esc, big], short[:304]], ["v", "w"])
    mid = [(b"m%03d" % i) * 50 + (b'"\n' if i % 3 == 0 else b"") for i in range(300)]
    check(ctx, [mid, short[:300]], ["mid", "s"])
    check(ctx, [mid] * 9 + [short[:300]], [f"k{c}" for c in range(10)])


@pytest.mark.gpu
def test_bad_calls(ctx):
    from csvplus_amd.materialize import json_write
    a = StrCol.from_values([b"1", b"2"])
    with pytest.raises(N.CphError) as e:
        json_write(ctx, [a, a], ["x", "x"])
    assert e.value.code == N.CPH_ERR_INVALID
    with pytest.raises(N.CphError) as e:
        json_write(ctx, [a] * 17, [f"c{i}" for i in range(17)])
    assert e.value.code == N.CPH_ERR_INVALID
    with pytest.raises(N.CphError) as e:
        json_write(ctx, [a.to_device()], ["x"], row_ids=[(1, 16, 2)], nrows=2)
    assert e.value.code == N.CPH_ERR_INVALID
    with pytest.raises(N.CphError) as e:
        json_write(ctx, [a, StrCol.from_values([b"1", b"2", b"3"])], ["x", "y"])
    assert e.value.code == N.CPH_ERR_INVALID
    arr = (N.cph_strcol * 1)()
    arr[0], keep = a.as_c()
    names = (N.cph_strval * 1)()
    out = C.POINTER(N.cph_bytes)()
    assert ctx.lib.cph_json_write_rows(ctx.handle, arr, None, names, 0, 2, N.CPH_MEM_HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_json_write_rows(ctx.handle, arr, None, None, 1, 2, N.CPH_MEM_HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert not out


@pytest.mark.gpu
def test_json_struct(ctx):
    """TestJSONStruct (csvplus_test.go:1016): people.csv -> SelectColumns(name, surname, born) -> ToJSON -> back to rows."""
    from csvplus_amd import ingest
    people = [("1", "Amelia", "Pond", "1989"), ("2", "Rory", "Williams", "1987"), ("3", "River", "Song", "1922"),
              ("4", "Clara", "Oswald", "1986"), ("5", "Martha", "Jones", "1987"), ("6", "Rose", "Tyler", "1987")]
    text = "id,name,surname,born\n" + "".join(",".join(p) + "\n" for p in people)
    t = ingest.read_csv(ctx, text.encode(), select=["name", "surname", "born"])
    try:
        cols = dict(zip([n.decode() for n in t.names], t.columns))
        names = ["name", "surname", "born"]
        out = write(ctx, [cols[k] for k in names], names)
    finally:
        t.release()
    data = json.loads(out)
    assert data == [{"name": p[1], "surname": p[2], "born": p[3]} for p in people]
    assert [list(d) for d in data] == [["born", "name", "surname"]] * len(people)


def _csv_text(names, cols):
    q = lambda v: b'"' + v.replace(b'"', b'""') + b'"'   # noqa: E731
    return b",".join(n.encode() for n in names) + b"\n" + b"".join(b",".join(q(c[i]) for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("positions", [True, False])
def test_join_to_json(ctx, positions):
    """The README chain (orders JOIN customers JOIN products) with out_columns=None: every column of the stream and of both
    index tables, the stream's value first on a shared name (nested mergeRows)."""
    from csvplus_amd import datagen as dg
    from csvplus_amd import pipeline
    nc, npd, m = 2000, 40, 12_000
    cust, prod = dg.customers(nc, encoding=dg.ITOA), dg.products(npd)
    ords = dg.orders(m, nc + 50, npd, cust_encoding=dg.ITOA)   # some orders find no customer
    cn = cust["name"].values()
    cn[3], cn[9] = b'Ann "Annie"\tJr', "Zo\u00eb \u2028".encode()
    cv = {"id": cust["id"].values(), "name": cn, "surname": cust["surname"].values(), "prod_id": [b"c%d" % i for i in range(nc)]}
    pv = {k: prod[k].values() for k in ("prod_id", "product", "price")}
    ov = {k: ords[k].values() for k in ("cust_id", "prod_id", "qty")}
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    try:
        got = pipeline.join_to_json(ctx, to, [(tc, "id", "cust_id"), (tp, "prod_id", "prod_id")], positions=positions)
    finally:
        for t in (tc, tp, to):
            t.release()
    crow = {v: i for i, v in enumerate(cv["id"])}
    prow = {v: i for i, v in enumerate(pv["prod_id"])}
    names, rows = None, []
    for i in range(m):
        c, p = crow.get(ov["cust_id"][i]), prow.get(ov["prod_id"][i])
        if c is None or p is None:
            continue
        row = {k: v[i] for k, v in ov.items()}
        for k, v in cv.items():
            row.setdefault(k, v[c])
        for k, v in pv.items():
            row.setdefault(k, v[p])
        names = list(row)
        rows.append([row[k] for k in names])
    assert 0 < len(rows) < m
    assert sorted(names) == ["cust_id", "id", "name", "price", "prod_id", "product", "qty", "surname"]
    assert got == go_to_json(names, rows)


@pytest.mark.gpu
def test_million_rows_by_digest(ctx):
    from csvplus_amd import datagen as dg
    n = 1_200_000
    cust = dg.customers(n, encoding=dg.ITOA)
    vals = {k: cust[k].values() for k in ("id", "name", "surname")}
    vals["name"][::1000] = [b'q"\x01\xe2\x80\xa8\xff'] * len(vals["name"][::1000])
    names = ["surname", "id", "name"]
    cols = [StrCol.from_values(vals[k]).to_device() for k in names]
    got = write(ctx, cols, names, out_mem=N.CPH_MEM_DEVICE)
    cache = {}

    def enc(v):
        e = cache.get(v)
        if e is None:
            e = cache[v] = go_string(v)
        return e
    h = hashlib.sha256(b"[")
    keys = sorted(names)
    ek = [enc(k.encode()) + b":" for k in keys]
    for i in range(n):
        h.update((b"," if i else b"") + b"{" + b",".join(ek[j] + enc(vals[k][i]) for j, k in enumerate(keys)) + b"}\n")
    h.update(b"]")
    assert hashlib.sha256(got).hexdigest() == h.hexdigest()
