"""RFC 3339 timestamps as a typed value on the device: cph_col_to_number's CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO kinds,
the CPH_MAP_TIME piece and the CPH_PRED_TIME_* terms, against the plain-Python model (csvplus_amd/timeconv.py): exact
equality of values, status bytes, nerrors, first_error_row and first_error_kind."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol, _native as N, expr as E, mapping as M, materialize as MZ, predicates as P, timeconv as T
from tests.time_cases import TABLE, VALID, mutations

pytestmark = pytest.mark.gpu

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
SIZES = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)   # the ballot word, the wave's tile, kNumTile = 2048 +- 1
ZONES = (0, 60, -330, 1439, -1439)


def _hip():
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def d2h(ptr, count, dtype):
    out = np.empty(count, dtype=dtype)
    if count:
        assert _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def device_ids(ids, keep):
    import torch
    t = torch.from_numpy(ids.view(np.uint8).copy()).to("cuda:0") if len(ids) else torch.empty(8, dtype=torch.uint8, device="cuda:0")
    keep.append(t)
    return t.data_ptr()


def make_col(values, device=False, offset_bits=32, fixed=None):
    sc = StrCol.from_values(values, offset_bits=offset_bits, fixed_width=fixed)
    return sc.to_device() if device else sc


def stamp(rng, frac=None, zone=None):
    """A valid stamp; frac: fraction digits (0 = none, None = random 0..9); zone: 'Z', 'num' or None (random)."""
    year, month = int(rng.integers(0, 10000)), int(rng.integers(1, 13))
    day = int(rng.integers(1, T.days_in_month(year, month) + 1))
    s = b"%04d-%02d-%02dT%02d:%02d:%02d" % (year, month, day, rng.integers(0, 24), rng.integers(0, 60), rng.integers(0, 60))
    nd = int(rng.integers(0, 10)) if frac is None else frac
    if nd:
        s += b"." + bytes(rng.integers(0x30, 0x3A, nd).astype(np.uint8))
    if zone == "Z" or (zone is None and rng.random() < 0.4):
        return s + b"Z"
    return s + b"%c%02d:%02d" % (b"+-"[int(rng.integers(2))], rng.integers(0, 24), rng.integers(0, 60))


def mixed_pool(seed=7, count=400):
    """Valid stamps of every length 20..35 that exists (all but 21), the classification table and the one-byte mutations."""
    rng = np.random.default_rng(seed)
    pool = [stamp(rng) for _ in range(count)] + [v for v, *_ in TABLE] + [v for v, *_ in mutations()][::3]
    assert {len(v) for v in pool} >= set(range(20, 36)) - {21}
    return pool


def check(res, values, unit, out_mem=HOST):
    want = [T.parse_model(v, unit) for v in values]
    n = len(values)
    assert res.kind == (N.CPH_NUM_TIME_UNIX if unit == "s" else N.CPH_NUM_TIME_UNIXNANO)
    if out_mem == DEVICE:
        vals, stat = d2h(res.values[0], n, np.int64), d2h(res.status[0], n, np.uint8)
        assert res.values[1] == res.status[1] == n
    else:
        vals, stat = res.values, res.status
        assert vals.dtype == np.int64
    assert len(vals) == len(stat) == n == res.nrows
    ws, wv = np.array([w[0] for w in want], dtype=np.uint8), np.array([w[1] for w in want], dtype=np.int64)
    bad = np.flatnonzero((stat != ws) | (vals != wv))
    assert len(bad) == 0, [(int(i), values[i], int(stat[i]), int(vals[i]), want[i]) for i in bad[:5]]
    errs = np.flatnonzero(ws)
    assert res.nerrors == len(errs)
    assert res.first_error_row == (int(errs[0]) if len(errs) else None)
    assert res.first_error_kind == (int(ws[errs[0]]) if len(errs) else 0)
    assert res.host_rows == 0
    res.release()


# ---- parse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", ["s", "ns"])
def test_the_classification_table(ctx, unit):
    rows = TABLE + mutations()
    values = [v for v, *_ in rows]
    for device in (False, True):
        res = MZ.to_time(ctx, make_col(values, device), unit=unit)
        got = [int(s) for s in res.status]
        assert got == [r[1 if unit == "s" else 2] for r in rows], [(values[i], got[i]) for i in range(len(rows)) if got[i] != rows[i][1 if unit == "s" else 2]][:5]
        check(res, values, unit)
    # every row on its own: the first row of a call, every alignment the table's prefix sums give aside
    for v, st_s, st_ns in TABLE:
        res = MZ.to_time(ctx, make_col([v], True), unit=unit)
        assert int(res.status[0]) == (st_s if unit == "s" else st_ns), v
        check(res, [v], unit)


@pytest.mark.parametrize("unit", ["s", "ns"])
@pytest.mark.parametrize("device,offset_bits", [(False, 32), (False, 64), (True, 32), (True, 64)])
def test_row_counts_at_every_edge(ctx, unit, device, offset_bits):
    pool = mixed_pool()
    rng = np.random.default_rng(99)
    for n in SIZES + (0,):
        values = [pool[i] for i in rng.integers(0, len(pool), n)]
        check(MZ.to_time(ctx, make_col(values, device, offset_bits), unit=unit), values, unit)
    values = [pool[i] for i in rng.integers(0, len(pool), 2049)]
    check(MZ.to_time(ctx, make_col(values, device, offset_bits), unit=unit, out_mem=DEVICE), values, unit, out_mem=DEVICE)


@pytest.mark.parametrize("width", [20, 25])
def test_fixed_width_columns(ctx, width):
    rng = np.random.default_rng(width)
    if width == 20:
        pool = [stamp(rng, 0, "Z") for _ in range(60)] + [b"2016-09-14T08:48:22+", b"2016-02-30T08:48:22Z", b"2016-09-14t08:48:22Z", b"x" * 20]
    else:
        pool = [stamp(rng, 0, "num") for _ in range(40)] + [stamp(rng, 4, "Z") for _ in range(20)]
        pool += [b"2016-09-14T8:48:22.12345Z", b"2016-09-14T08:48:22,1234Z", b"2016-09-14T08:48:22+24:00", b"2016-09-14T08:48:22.12345", b" " * 25]
    assert all(len(p) == width for p in pool)
    for n in (1, 65, 2049):
        values = [pool[i] for i in rng.integers(0, len(pool), n)]
        for device in (False, True):
            col = make_col(values, device, fixed=width)
            assert col.fixed_width == width
            for unit in ("s", "ns"):
                check(MZ.to_time(ctx, col, unit=unit), values, unit)


def test_every_length_at_every_alignment(ctx):
    rng = np.random.default_rng(3)
    by_len = [stamp(rng, nd, z) for nd in range(10) for z in ("Z", "num") for _ in range(3)]
    assert {len(v) for v in by_len} == set(range(20, 36)) - {21}
    for shift in range(8):   # the first value moves every later one: each length meets each alignment within a word
        values = [b"7" * shift] + by_len
        for device in (False, True):
            check(MZ.to_time(ctx, make_col(values, device), unit="ns"), values, "ns")


@pytest.mark.parametrize("device", [False, True])
def test_through_row_ids(ctx, device):
    pool = mixed_pool(count=200)
    rng = np.random.default_rng(17)
    col = make_col(pool, device)
    for id_bits, base, n in ((32, 7, 2049), (64, 1 << 33, 65), (32, 0, 1), (64, 3, 0)):
        ids = rng.integers(0, len(pool), n).astype(np.uint32 if id_bits == 32 else np.uint64)   # repeated ids
        with_base = ids + ids.dtype.type(base)
        keep = []
        row_ids = (device_ids(with_base, keep), id_bits, n, base) if device else (with_base, base)
        check(MZ.to_time(ctx, col, row_ids=row_ids, nrows=n, unit="s"), [pool[i] for i in ids], "s")
        del keep


def test_first_and_last_row_errors(ctx):
    rng = np.random.default_rng(5)
    n = 2 * 2048 + 1
    good = [stamp(rng) for _ in range(n)]
    for at, bad in ((n - 1, b"2016-09-14T08:48:22"), (0, b""), (2048 + 5, b"2016-09-14T8:48:22Z"), (2047, b"2016-02-30T00:00:00Z")):
        values = list(good)
        values[at] = bad
        res = MZ.to_time(ctx, make_col(values, True), unit="s")
        assert (res.nerrors, res.first_error_row, res.first_error_kind) == (1, at, T.parse_model(bad, "s")[0])
        check(res, values, "s")
    values = list(good)
    values[2048 + 7], values[70], values[n - 1] = b"x", b"2016-13-01T00:00:00Z", b"2016-09-14T08:48:22,5Z"
    res = MZ.to_time(ctx, make_col(values, False), unit="s")
    assert (res.nerrors, res.first_error_row, res.first_error_kind) == (3, 70, N.CPH_NUM_ERR_RANGE)
    check(res, values, "s")


def test_a_device_column_that_ends_at_its_buffers_end(ctx):
    """The column's bytes fill their allocation exactly (no slack word behind them) and end on a word boundary; the last value
    is 20 bytes, so the loads of bytes 16.. must stay inside the value's own words.  Run with the pool's canaries on."""
    import torch
    rng = np.random.default_rng(11)
    values = [stamp(rng) for _ in range(300)] + [b"2016-09-14T08:48:22Z"]
    values[0] = b"x" * ((8 - sum(len(v) for v in values[1:]) % 8) % 8 + 8)
    host = StrCol.from_values(values)
    assert host.data.nbytes % 8 == 0 and len(values[-1]) == 20
    data = torch.from_numpy(host.data.copy()).to("cuda:0")            # exactly nbytes: nothing behind the last value
    offs = torch.from_numpy(host.offsets.view(np.uint8).copy()).to("cuda:0")
    col = StrCol(data, offs, len(values), 32, DEVICE, fixed_width=0)
    ctx.set_option("pool_guard", 1)
    try:
        for unit in ("s", "ns"):
            check(MZ.to_time(ctx, col, unit=unit), values, unit)
        check(MZ.to_time(ctx, host, unit="s"), values, "s")             # the library's own staged copy, canary behind it
        ctx.set_option("pool_guard_check", 0)
    finally:
        ctx.set_option("pool_guard", 0)


def test_kinds_0_and_3_stay_refused(ctx):
    arr = (N.cph_strcol * 1)()
    arr[0], keep = StrCol.from_values([b"2016-09-14T08:48:22Z"]).as_c()
    for kind, rc in ((0, N.CPH_ERR_INVALID), (3, N.CPH_ERR_INVALID), (6, N.CPH_ERR_INVALID), (4, N.CPH_OK), (5, N.CPH_OK)):
        out = C.POINTER(N.cph_numcol)()
        assert ctx.lib.cph_col_to_number(ctx.handle, arr, None, 1, kind, HOST, C.byref(out)) == rc, kind
        if out:
            ctx.lib.cph_numcol_release(out)
    with pytest.raises(ValueError):
        MZ.to_time(ctx, StrCol.from_values([b"x"]), unit="ms")


# ---- format -----------------------------------------------------------------------------------------------------------------
def column_values(cb):
    vals = cb.to_strcol().values()
    cb.release()
    return vals


EDGE_SECONDS = [-62167219200, 0, -1, 253402300799]


@pytest.mark.parametrize("zone", ZONES)
def test_time_piece_against_the_model(ctx, zone):
    rng = np.random.default_rng(2000 + zone)
    lo, hi = T.MIN_SECONDS + 86400, T.MAX_SECONDS - 86400
    for n in (1, 255, 256, 257, 1500):   # both sides of the copy pass's tile of 256 rows
        vals = rng.integers(lo, hi, n).astype(np.int64)
        edges = [v for v in EDGE_SECONDS if T.in_range(v, zone)]
        vals[:len(edges)][:n] = edges[:n]
        want = [T.format_model(v, zone) for v in vals]
        assert column_values(MZ.map_column(ctx, {}, M.Format(M.Time(vals, zone)), nrows=n)) == want
    import torch
    dev = torch.from_numpy(vals).to("cuda:0")
    tmpl = M.Format("[", M.Time.on_device(dev.data_ptr(), n, zone), "] ", M.Int(vals))
    assert column_values(MZ.map_column(ctx, {}, tmpl, nrows=n)) == [b"[" + w + b"] %d" % v for w, v in zip(want, vals)]


def test_round_trip_of_the_valid_table_rows(ctx):
    texts = [v for v, st, _ in VALID if st == 0]
    secs = MZ.to_time(ctx, make_col(texts, True), unit="s")
    assert secs.nerrors == 0
    for zone in ZONES:
        ok = np.array([T.in_range(v, zone) for v in secs.values])
        vals = secs.values[ok]
        out = column_values(MZ.map_column(ctx, {}, M.Format(M.Time(vals, zone)), nrows=len(vals)))
        assert out == [T.format_model(v, zone) for v in vals]
        again = MZ.to_time(ctx, StrCol.from_values(out), unit="s")
        assert again.nerrors == 0 and np.array_equal(again.values, vals)


def test_a_year_outside_0000_9999_fails_the_call_and_names_the_lowest_row(ctx):
    vals = np.zeros(3000, dtype=np.int64)
    for bad, zone, at in ((253402300799, 1, (2900, 700, 2999)), (-62167219200, -1, (257,)), (253402300800, 0, (0,)), (1 << 62, 0, (2999,)), (-(1 << 63), -1439, (5,))):
        v = vals.copy()
        v[list(at)] = bad
        for part in (M.Time(v, zone), None):
            if part is None:
                import torch
                dev = torch.from_numpy(v).to("cuda:0")
                part = M.Time.on_device(dev.data_ptr(), len(v), zone)
            with pytest.raises(N.CphError) as e:
                MZ.map_column(ctx, {}, M.Format("t=", part), nrows=len(v))
            assert e.value.code == N.CPH_ERR_INVALID and f"TIME piece 1, row {min(at)}:" in e.value.msg, e.value.msg
    v = vals.copy()
    v[9] = 253402300799 + 60
    assert column_values(MZ.map_column(ctx, {}, M.Format(M.Time(v, -1)), nrows=10))[9] == b"9999-12-31T23:59:59-00:01"


def test_a_zone_of_1440_minutes_is_refused(ctx):
    for zone in (1440, -1440, 1 << 20):
        part = M.Time([0, 1], 0)
        part.zone = zone   # past the Python check: the C ABI's own
        with pytest.raises(N.CphError) as e:
            MZ.map_column(ctx, {}, M.Format(part), nrows=2)
        assert e.value.code == N.CPH_ERR_INVALID and "-1439..1439" in e.value.msg
        with pytest.raises(N.CphError) as e:
            MZ.map_switch(ctx, {"k": StrCol.from_values([b"a", b"b"])}, M.When(P.Like(k="a"), part, "x"))
        assert e.value.code == N.CPH_ERR_INVALID and "-1439..1439" in e.value.msg
    for kind in (5, 6, 7, 9, 11):   # the neighbours of CPH_MAP_TIME = 10 stay unknown
        parr = (N.cph_map_piece * 1)()
        parr[0].kind = kind
        out = C.POINTER(N.cph_colbuf)()
        assert ctx.lib.cph_map_format(ctx.handle, None, None, 0, 1, parr, 1, HOST, C.byref(out)) == N.CPH_ERR_INVALID and not out


def test_inside_a_switch_only_selecting_rows_can_fail(ctx):
    n = 700
    rng = np.random.default_rng(8)
    keys = [b"ab"[int(i)::2][:1] for i in rng.integers(0, 2, n)]
    vals = rng.integers(0, 2_000_000_000, n).astype(np.int64)
    a_rows = [i for i, k in enumerate(keys) if k == b"a"]
    b_rows = [i for i, k in enumerate(keys) if k == b"b"]
    vals[b_rows[3]] = 1 << 60          # never formatted: its row selects the other alternative
    vals[b_rows[-1]] = -(1 << 62)
    cols = {"k": StrCol.from_values(keys)}
    sw = M.When(P.Like(k="a"), M.Format("at ", M.Time(vals, 60)), M.Format("no ", M.Col("k")))
    cb, which = MZ.map_switch(ctx, cols, sw, want_which=True)
    got = column_values(cb)
    assert got == [b"at " + T.format_model(vals[i], 60) if keys[i] == b"a" else b"no b" for i in range(n)]
    assert which.tolist() == [0 if k == b"a" else 1 for k in keys]
    vals[a_rows[40]] = vals[a_rows[9]] = 1 << 60
    with pytest.raises(N.CphError) as e:
        MZ.map_switch(ctx, cols, M.When(P.Like(k="a"), M.Format("at ", M.Time(vals, 60)), "no"))
    assert e.value.code == N.CPH_ERR_INVALID and f"case 0, TIME piece 1, row {a_rows[9]}:" in e.value.msg, e.value.msg


# ---- predicate --------------------------------------------------------------------------------------------------------------
def zoned_rows(n=1300, seed=21):
    """Stamps within a day of the literal in three zone offsets (a few with fractions) and rows of every error status: the
    byte order and the instant order disagree."""
    rng = np.random.default_rng(seed)
    base = T.parse_model(b"2016-09-14T00:00:00Z")[1]
    rows = []
    for i in range(n):
        v = base + int(rng.integers(-86400, 86400)) if i % 9 else base   # every ninth row IS the literal's instant
        text = T.format_model(v, (0, 120, -300)[i % 3])
        if i % 7 == 0:
            text = text[:19] + b".%03d" % rng.integers(0, 1000) + text[19:]
        rows.append(text)
    for i, bad in ((5, b""), (77, b"2016-09-14T0:00:00Z"), (300, b"2016-09-31T00:00:00Z"), (n - 1, b"2016-09-14T00:00:00+24:00"), (640, b"2016-09-14 00:00:00Z")):
        rows[i] = bad
    return rows


LITERAL = b"2016-09-14T00:00:00Z"


@pytest.mark.parametrize("device", [False, True])
def test_the_six_relations_compare_instants_not_bytes(ctx, device):
    rows = zoned_rows()
    cols = {"ts": make_col(rows, device)}
    differs = 0
    for rel in P.RELS:
        pred = P.TimeCmp("ts", rel, LITERAL)
        want = [i for i, v in enumerate(rows) if pred({"ts": v})]
        got = MZ.filter_rows(ctx, cols, pred).tolist()
        assert got == want, rel
        assert 0 < len(want) < len(rows)
        by_bytes = MZ.filter_rows(ctx, cols, P.StrCmp("ts", rel, LITERAL)).tolist()
        differs += by_bytes != want
        for i in (5, 77, 300, 640, len(rows) - 1):   # a row of each error status is false under all six
            assert i not in got
    assert differs == 6   # the byte comparison gives another row set under every relation
    other_zone = P.TimeCmp("ts", "==", "2016-09-14T02:00:00+02:00")   # the same instant, written in another zone
    assert MZ.filter_rows(ctx, cols, other_zone).tolist() == [i for i, v in enumerate(rows) if T.parse_model(v) == (0, T.parse_model(LITERAL)[1])]


def test_time_terms_nest_and_run_in_every_mode(ctx):
    rows = zoned_rows(5000, 4)
    kinds = [(b"1", b"2", b"a")[i % 3] for i in range(len(rows))]
    cols = {"ts": make_col(rows, True), "k": make_col(kinds, True)}
    preds = [P.All(P.TimeCmp("ts", ">=", LITERAL), P.TimeCmp("ts", "<", "2016-09-14T12:00:00+00:00")),
             P.Any(P.Not(P.TimeCmp("ts", ">", "2016-09-13T20:00:00-02:00")), P.Like(k="a")),
             P.All(P.TimeCmp("ts", "!=", LITERAL), P.StrCmp("ts", ">=", "2016-09-14"), P.IntCmp("k", "<", 2)),
             P.Any(P.TimeCmp("missing", "<", LITERAL), P.All(P.TimeCmp("ts", "<=", LITERAL), P.HasSuffix("ts", "Z")))]
    for pred in preds:
        flags = [P.matches(pred, {"ts": t, "k": k}) for t, k in zip(rows, kinds)]
        for mode in ("where", "take_while", "drop_while"):
            for kw in ({}, {"first_row": 2049, "nrows": 2100, "skip": 3, "limit": 500}):
                got = MZ.filter_rows(ctx, cols, pred, mode=mode, **kw)
                want = P.select_rows(flags, mode, kw.get("first_row", 0), kw.get("nrows"), kw.get("skip", 0), kw.get("limit"))
                assert got.tolist() == want, (pred, mode, kw)
    # a WHILE mode that runs long before it stops: ascending stamps
    asc = [T.format_model(1473811200 + 30 * i, (0, 120, -300)[i % 3]) for i in range(5000)]
    pred = P.TimeCmp("ts", "<", "2016-09-15T12:00:00+02:00")
    stop = next(i for i, v in enumerate(asc) if not pred({"ts": v}))
    assert 2048 < stop < 5000
    assert MZ.filter_rows(ctx, {"ts": make_col(asc, True)}, pred, mode="take_while").tolist() == list(range(stop))
    assert MZ.filter_rows(ctx, {"ts": make_col(asc)}, pred, mode="drop_while").tolist() == list(range(stop, 5000))


def _filter_call(ctx, cols, ncols, n, ops):
    keep = []
    arr = MZ._pred_program(ops, keep)
    o = N.cph_filter_opts(0, 32, 0, 0, N.CPH_NO_LIMIT)
    out = C.POINTER(N.cph_rowlist)()
    rc = ctx.lib.cph_filter_rows(ctx.handle, cols, None, ncols, n, arr, len(ops), C.byref(o), HOST, C.byref(out))
    rows = None
    if out:
        rows = N._ptr_array(out.contents.ids, int(out.contents.nrows), np.uint32).tolist() if out.contents.ids else list(range(int(out.contents.nrows)))
        ctx.lib.cph_rowlist_release(out)
    return rc, ctx.last_error(), rows


def test_literals_columns_and_op_codes_at_the_c_abi(ctx):
    arr = (N.cph_strcol * 1)()
    arr[0], keep = StrCol.from_values([b"2016-09-14T00:00:00Z", b"2016-09-14T02:00:00+02:00", b"2016-09-14T00:00:01Z"]).as_c()
    for op, want in zip(range(48, 54), ([], [0, 1], [0, 1], [2], [0, 1, 2], [2])):
        rc, _, rows = _filter_call(ctx, arr, 1, 3, [(op, 0, LITERAL)])
        assert (rc, rows) == (N.CPH_OK, want), op
        rc, _, rows = _filter_call(ctx, arr, 1, 3, [(op, -1, LITERAL)])   # no such column: false, NE included
        assert (rc, rows) == (N.CPH_OK, []), op
    bad = [("a fraction", [(48, 0, b"2016-09-14T00:00:00.5Z")]), ("a fraction and a zone", [(52, 0, b"2016-09-14T00:00:00.000+01:00")]),
           ("no stamp", [(48, 0, b"2016-09")]), ("empty", [(48, 0, b"")]), ("NULL", [(48, 0, None)]), ("range", [(53, 0, b"2016-02-30T00:00:00Z")]),
           ("one-digit hour", [(50, 0, b"2016-09-14T0:00:00Z")]), ("zone hour 24", [(50, 0, b"2016-09-14T00:00:00+24:00")]),
           ("a long literal", [(50, 0, b"2016-09-14T00:00:00Z" * 5)]), ("a bad literal on column -1", [(50, -1, b"x")]),
           ("column 1 of 1", [(49, 1, LITERAL)]), ("column -2", [(49, -2, LITERAL)]),
           ("op 31", [(31, 0, LITERAL)]), ("op 38", [(38, 0, LITERAL)]), ("op 39", [(39, 0, LITERAL)]), ("op 43", [(43, 0, LITERAL)]),
           ("op 44", [(44, 0, LITERAL)]), ("op 47", [(47, 0, LITERAL)]), ("op 54", [(54, 0, LITERAL)]), ("op 64", [(64, 0, LITERAL)]),
           ("33 terms", [(48, 0, LITERAL)] * 33 + [(P.ANY, 33, None)])]
    for what, ops in bad:
        rc, msg, rows = _filter_call(ctx, arr, 1, 3, ops)
        assert rc == N.CPH_ERR_INVALID and msg and rows is None, (what, rc, msg)
    assert _filter_call(ctx, arr, 1, 3, [(48, 0, LITERAL)] * 32 + [(P.ANY, 32, None)])[0] == N.CPH_OK


def test_a_time_term_as_a_switch_condition(ctx):
    rows = zoned_rows(900, 9)
    cols = {"ts": make_col(rows, True)}
    sw = M.Switch((P.TimeCmp("ts", "<", LITERAL), "before"), (P.TimeCmp("ts", "==", LITERAL), M.Format("at ", M.Col("ts")[11:19])),
                  otherwise=M.Format("after/", M.Col("ts")))
    cb, which = MZ.map_switch(ctx, cols, sw, want_which=True)
    assert column_values(cb) == [M.render(sw, {"ts": v}) for v in rows]
    assert which.tolist() == [M.which_of(sw, {"ts": v}) for v in rows] and set(which.tolist()) == {0, 1, 2}


# ---- end to end -------------------------------------------------------------------------------------------------------------
def orders_csv(n=5000, seed=31):
    rng = np.random.default_rng(seed)
    base = 1473811200   # 2016-09-14T00:00:00Z
    lines, stamps = [b"order_id,cust_id,ts"], []
    for i in range(n):
        v = base + int(rng.integers(0, 40 * 3600))
        ts = T.format_model(v, (0, 120, -330)[i % 3])
        if i % 11 == 0:
            ts = ts[:19] + b".%d" % rng.integers(1, 1000) + ts[19:]
        stamps.append(ts)
        lines.append(b"%d,c%d,%s" % (i, rng.integers(0, 50), ts))
    return b"\n".join(lines) + b"\n", stamps


def test_orders_per_hour_across_zones_from_csv_text_to_the_top_five(ctx):
    from csvplus_amd import DeviceIndex, aggregate as A, ordering as O, pipeline as PL
    text, stamps = orders_csv()
    n = len(stamps)
    table = PL.read_table(ctx, text)
    try:
        t = MZ.to_time(ctx, table["ts"], unit="s", out_mem=DEVICE)
        assert t.nerrors == 0 and t.nrows == n
        hour = M.Time.of((E.IntArr.on_device(t.values[0], n) / 3600) * 3600)
        hours = MZ.map_column(ctx, {}, M.Format(hour), nrows=n, out_mem=DEVICE)
        ix = DeviceIndex(ctx, [hours.as_device_strcol()])
        tot = A.totals(ix, [A.Max((t.values[0], n), "int")])
        top = MZ.order_rows(ctx, [O.Desc(tot.count.astype(np.int64))], tot.ngroups, limit=5).to_numpy().tolist()
        keep = []
        first = np.ascontiguousarray(tot.first_row[top].astype(np.uint32))
        keys = MZ.gather_rows(ctx, hours.as_device_strcol(), (device_ids(first, keep), 32, len(first))).values()
        got = [(keys[k], int(tot.count[g]), int(tot.values[0][g])) for k, g in enumerate(top)]
        # the same in plain Python over the model
        secs = [T.parse_model(s)[1] for s in stamps]
        groups = {}
        for v in secs:
            key = T.format_model(v // 3600 * 3600, 0)
            c, m = groups.get(key, (0, v))
            groups[key] = (c + 1, max(m, v))
        ordered = sorted(sorted(groups), key=lambda k: -groups[k][0])[:5]   # stable: ties keep the key order
        assert got == [(k,) + groups[k] for k in ordered]
        assert len({T.format_model(v, 0)[:13] for v in secs}) == len(groups) < len({s[:13] for s in stamps})   # the bytes would bucket differently
        # a time window through the pipeline's own compile path
        window = P.All(P.TimeCmp("ts", ">=", "2016-09-14T10:00:00+02:00"), P.TimeCmp("ts", "<", "2016-09-14T09:00:00Z"))
        out = PL.filter_to_csv(ctx, table, window, ["order_id", "ts"])
        want = [i for i, s in enumerate(stamps) if window({"ts": s})]
        assert 0 < len(want) < n
        assert out == b"order_id,ts\n" + b"".join(b"%d,%s\n" % (i, stamps[i]) for i in want)
        ix.close()
        hours.release()
        t.release()
    finally:
        table.release()
