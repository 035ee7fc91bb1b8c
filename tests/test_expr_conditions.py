"""Conditions that compare two expressions or two columns, on the device: cph_filter_rows ops 56..61 (k_expr_cmp) and 72..77
(k_pred_eval's column-against-column term) through materialize.filter_rows, validate_rows, map_switch and pipeline.filter_to_csv,
row by row against the host model predicates.matches.  Results are equal, not close.

Shapes: row counts at the wave (64) and at the 2048-row tile T; first_row in front of a word and inside one; the three index
spaces of k_expr_cmp (a column leaf at first_row + i through the row ids, a caller's array at first_row + i, a converted leaf of the
plain route at i) in one call; values whose float conversion the device defers; an error row in the last word of a tile."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd import predicates as P
from csvplus_amd.expr import FloatArr, FloatCol, IntArr, IntCol, ToFloat, ToInt
from csvplus_amd.predicates import All, ColCmp, ExprCmp, HasPrefix, IntCmp, Like, Not

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
T = 2048
ROWS = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
RELS = P.RELS
# outside Clinger's exact cases: the device defers them.  ("1e23" is NOT: 1 x 10^(23 - 22) still fits the exact multiplication, so it
# stays an ordinary value below; predicates.float_is_deferred is asserted wherever the route matters.)
DEFERRED = ("1e38", "123456789012345678901e-5")


# ---- columns, row ids and the model's rows ---------------------------------------------------------------------------------

def make_col(values, kind="o32", device=False):
    """kind: "o32" / "o64" (offsets) or "fix" (fixed width: every value is padded by the caller to one length)."""
    vals = [v.encode() if isinstance(v, str) else bytes(v) for v in values]
    if kind == "fix":
        w = len(vals[0])
        assert w and all(len(v) == w for v in vals)
        col = StrCol.from_values(vals, fixed_width=w)
        assert col.fixed_width == w
    else:
        col = StrCol.from_values(vals, offset_bits=64 if kind == "o64" else 32, fixed_width=0)
    if not device:
        return col
    import torch
    nb = col.data.nbytes
    d = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda:0")   # exactly the bytes: the last value ends with the buffer
    if nb:
        d[:nb].copy_(torch.from_numpy(np.ascontiguousarray(col.data)))
    o = None if col.fixed_width else torch.from_numpy(np.ascontiguousarray(col.offsets).view(np.uint8).copy()).to("cuda:0")
    return StrCol(d, o, col.nrows, col.offset_bits, DEVICE, fixed_width=col.fixed_width)


_KEEP = []   # device row-id tensors live as long as the module


def make_ids(src_rows, bits, base, device):
    """Row ids as filter_rows takes them: entry p = the source row of position p, plus `base`."""
    a = (np.asarray(src_rows, dtype=np.uint64) + np.uint64(base)).astype(np.uint32 if bits == 32 else np.uint64)
    if not device:
        return (a, base)
    import torch
    t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
    _KEEP.append(t)
    return (t.data_ptr(), bits, len(a), base)


def model_flags(pred, rows):
    return np.array([P.matches(pred, r, i) for i, r in enumerate(rows)], dtype=bool)


def check_modes(ctx, cols, pred, flags, first_row=0, nrows=None, skip=0, limit=None, row_ids=None, modes=("where",), bits=(None,), what=None):
    """filter_rows against predicates.select_rows over the model's flags (flags[p] = position p of the selection)."""
    from csvplus_amd.materialize import filter_rows
    for mode in modes:
        for ob in bits:
            got = filter_rows(ctx, cols, pred, row_ids=row_ids, nrows=nrows, mode=mode, first_row=first_row, skip=skip, limit=limit, out_bits=ob)
            want = P.select_rows(flags, mode, first_row, nrows, skip, limit)
            assert got.dtype == (np.uint64 if ob == 64 else np.uint32)
            assert np.array_equal(got.astype(np.int64), np.asarray(want, dtype=np.int64)), (what, mode, ob, first_row, nrows, skip, limit)


# ---- the reference's shape: price * float64(qty) REL x ------------------------------------------------------------------------

PRICES = ["12.5", "0.5", "100", "99.99", "1e2", "-3.25", "0.1", "33.333", "", "abc", "0x10", "NaN", "25", "4"]
QTYS = ["8", "1", "0", "200", "-4", "3", "25", "x7", "99999999999999999999", "4", "1000"]
NMAX = 2 * T + 1 + 70


def _amount_data():
    rng = np.random.default_rng(20261021)
    price = [PRICES[k] for k in rng.integers(0, len(PRICES), NMAX)]
    qty = [QTYS[k] for k in rng.integers(0, len(QTYS), NMAX)]
    price[0], qty[0] = "12.5", "8"        # == 100
    price[1], qty[1] = "12.5", "7"        # <
    slow = list(price)                    # the same with values the device defers (and a range error among them) at one row in ten
    for i in np.flatnonzero(rng.integers(0, 10, NMAX) == 0):
        slow[i] = (DEFERRED + ("1e400",))[i % 3]
    slow[0] = DEFERRED[0]
    return price, qty, slow


PRICE, QTY, PRICE_SLOW = _amount_data()
AMOUNT = FloatCol("price") * ToFloat(IntCol("qty"))
MIRROR = {"<": ">", "<=": ">=", "==": "==", "!=": "!=", ">=": "<=", ">": "<"}   # x REL a  ==  a MIRROR[REL] x
_FLAGS = {}


def amount_flags(rel):
    """The model over all NMAX rows, once per relation; every row count below is a prefix of it."""
    if rel not in _FLAGS:
        f = model_flags(ExprCmp(AMOUNT, rel, 100.0), [{"price": p, "qty": q} for p, q in zip(PRICE, QTY)])
        assert f.any() and not f.all(), rel
        f.setflags(write=False)
        _FLAGS[rel] = f
    return _FLAGS[rel]


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_reference_program_all_relations(ctx, n):
    """FloatCol(price) * ToFloat(IntCol(qty)) REL 100.0 at every row count of the wave and tile edges, host and device columns,
    32- and 64-bit offsets.  No value here is deferred: the fast route."""
    assert not any(P.float_is_deferred(p) for p in PRICES)
    device = ROWS.index(n) % 2 == 0
    cols = {"price": make_col(PRICE[:max(n, 1)], "o32", device), "qty": make_col(QTY[:max(n, 1)], "o64", device)}
    for rel in RELS:
        check_modes(ctx, cols, ExprCmp(AMOUNT, rel, 100.0), amount_flags(rel)[:n], nrows=n, what=(rel, n))
        check_modes(ctx, cols, ExprCmp(100.0, MIRROR[rel], AMOUNT), amount_flags(rel)[:n], nrows=n, what=("mirrored", rel, n))
    # the same rows with deferred values among them: the plain route, row for row
    assert P.float_is_deferred(PRICE_SLOW[0]) and P.float_is_deferred("1e400")
    cols["price"] = make_col(PRICE_SLOW[:max(n, 1)], "o32", device)
    for rel in (">=", "!="):
        pred = ExprCmp(AMOUNT, rel, 100.0)
        check_modes(ctx, cols, pred, model_flags(pred, [{"price": p, "qty": q} for p, q in zip(PRICE_SLOW[:n], QTY[:n])]), nrows=n, what=("slow", rel, n))


@pytest.mark.gpu
@pytest.mark.parametrize("first_row", [0, 5, 70])
def test_first_row_modes_bits_skip_limit(ctx, first_row):
    """Drop / Top on either side of the filter, the three modes, 32- and 64-bit row numbers: T + 1 rows behind first_row."""
    n = T + 1
    total = first_row + n
    device = first_row != 5
    cols = {"price": make_col(PRICE[:total], "o64", device), "qty": make_col(QTY[:total], "o32", device)}
    for rel in (">=", "!="):
        pred = ExprCmp(AMOUNT, rel, 100.0)
        flags = amount_flags(rel)[:total]
        check_modes(ctx, cols, pred, flags, first_row, n, modes=("where", "take_while", "drop_while"), bits=(32, 64), what=rel)
        check_modes(ctx, cols, pred, flags, first_row, n, skip=3, limit=1000, modes=("where", "take_while", "drop_while"), what=rel)
        check_modes(ctx, cols, pred, flags, first_row, 65, skip=1, limit=2, what=rel)
    # the WHILE modes with the first failing row in the last word of the first tile and in the second tile
    for stop in (first_row + T - 3, first_row + T):
        p2, q2 = ["12.5"] * total, ["9"] * total
        p2[stop], q2[stop] = "abc", "9"
        cols2 = {"price": make_col(p2, "o32", device), "qty": make_col(q2, "o32", device)}
        f2 = np.ones(total, dtype=bool)
        f2[stop] = False
        check_modes(ctx, cols2, ExprCmp(AMOUNT, ">", 100.0), f2, first_row, n, modes=("take_while", "drop_while", "where"), what=stop)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_int_columns_layouts_and_row_ids(ctx, device):
    """IntCol(a) REL IntCol(b) over a fixed-width and an offsets column read through row ids of different widths and bases."""
    rng = np.random.default_rng(7)
    n, first_row = T + 70, 5
    born = ["%04d" % v for v in rng.integers(1900, 1910, 300)] + ["19x0"]          # fixed width 4; the last does not convert
    died = [str(v) for v in rng.integers(1895, 1915, 500)] + ["", "-0", "+1905"]   # variable
    ia, ib = rng.integers(0, len(born), first_row + n), rng.integers(0, len(died), first_row + n)
    rows = [{"born": born[a], "died": died[b]} for a, b in zip(ia, ib)]
    for ka, kb, bits_a, bits_b in (("fix", "o32", 32, 64), ("fix", "o64", 64, 32)):
        cols = {"born": make_col(born, ka, device), "died": make_col(died, kb, device)}
        ids = {"born": make_ids(ia, bits_a, 3, device), "died": make_ids(ib, bits_b, 1000, device)}
        for rel in RELS:
            pred = ExprCmp(IntCol("died"), rel, IntCol("born"))
            flags = model_flags(pred, rows)
            assert flags[first_row:].any() and not flags[first_row:].all()
            check_modes(ctx, cols, pred, flags, first_row, n, row_ids=ids, what=(ka, kb, rel))
        check_modes(ctx, cols, ExprCmp(IntCol("died") - IntCol("born"), ">=", 5), model_flags(ExprCmp(IntCol("died") - IntCol("born"), ">=", 5), rows),
                    first_row, n, row_ids=ids, modes=("where", "take_while", "drop_while"), bits=(32, 64))


# ---- the three index spaces in one call -----------------------------------------------------------------------------------------

def _index_space_case(deferred):
    rng = np.random.default_rng(99 if deferred else 98)
    first_row, n = 70, T
    total = first_row + n
    pool = ["0.5", "2", "12.5", "3e0", "1e2", "7", "1e23"] + (list(DEFERRED) if deferred else [])
    src = [pool[k] for k in rng.integers(0, len(pool), 400)]
    if deferred:
        src[17], src[18] = DEFERRED
    ids = rng.integers(0, len(src), total)
    ids[first_row + 3], ids[first_row + T - 1] = 17, 18 if deferred else 5
    weight = rng.choice([0.25, 1.0, 4.0, 1e21], total)     # one per POSITION of the selection
    qty = [str(v) for v in rng.integers(1, 40, total)]
    qty[first_row + T - 5] = "n/a"                          # an error row in the last word of the call's (only) tile
    qty[first_row - 1] = "n/a"                              # ... and one in front of first_row that the call must not see
    rows = [{"price": src[ids[p]], "qty": qty[p]} for p in range(total)]
    return first_row, n, src, ids, weight, qty, rows


@pytest.mark.gpu
@pytest.mark.parametrize("float_device", [0, 1])
@pytest.mark.parametrize("deferred", [True, False])
def test_three_index_spaces_at_first_row_70(ctx, deferred, float_device):
    """first_row = 70 with a FloatArr leaf (entry first_row + i), a column leaf through row ids (source_row(rid, first_row + i))
    and, when a value is deferred, every string leaf converted first (entry i) — with an error row in the tile's last word."""
    import torch
    first_row, n, src, ids, weight, qty, rows = _index_space_case(deferred)
    if deferred:
        assert all(P.float_is_deferred(v) for v in DEFERRED)
        assert any(P.float_is_deferred(r["price"]) for r in rows[first_row:])
    else:
        assert not any(P.float_is_deferred(r["price"]) for r in rows)
    wdev = torch.from_numpy(weight.copy()).to("cuda:0")
    ctx.set_option("float_device", float_device)
    try:
        for device in (False, True):
            cols = {"price": make_col(src, "o32", device), "qty": make_col(qty, "o64", device)}
            rid = {"price": make_ids(ids, 32, 7, device)}
            for arr in (FloatArr(weight), FloatArr.on_device(wdev.data_ptr(), len(weight))):
                for rel in (">=", "!=", "<"):
                    pred = ExprCmp(FloatCol("price") * arr, rel, ToFloat(IntCol("qty")))
                    flags = model_flags(ExprCmp(FloatCol("price") * FloatArr(weight), rel, ToFloat(IntCol("qty"))), rows)
                    assert flags[first_row:].any() and not flags[first_row:].all()
                    assert not flags[first_row + T - 5] and not flags[first_row - 1]            # the error rows: false under != too
                    check_modes(ctx, cols, pred, flags, first_row, n, row_ids=rid, modes=("where", "take_while", "drop_while"), bits=(32, 64),
                                what=(deferred, float_device, device, arr.device, rel))
                    check_modes(ctx, cols, All(pred, Not(Like(qty="1"))), flags & np.array([r["qty"] != "1" for r in rows]), first_row, n, row_ids=rid,
                                what=("in All", deferred, device, rel))
    finally:
        ctx.set_option("float_device", 0)


# ---- deeper programs, int arrays, ToInt -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_depth_4_and_depth_8_programs(ctx):
    rng = np.random.default_rng(5)
    n = T + 65
    a = [str(v) for v in rng.integers(-50, 50, n)]
    b = [str(v) for v in rng.integers(-3, 4, n)]            # zero divisors among them
    x = [rng.choice(["1.5", "-2.25", "1e19", "NaN", "0", "3"]) for _ in range(n)]
    bonus = rng.integers(-5, 6, n)
    a[1], b[1] = str((1 << 63) - 1), "1"                    # a + b wraps
    rows = [{"a": a[i], "b": b[i], "x": x[i]} for i in range(n)]
    cols = {"a": make_col(a, "o32", True), "b": make_col(b, "o32", True), "x": make_col(x, "o64", True)}
    A, B, X = IntCol("a"), IntCol("b"), FloatCol("x")
    d4_l, d4_r = (A + B) * (A - B), (A - B * 3) % (A + 7)                                         # stack 4 with the lhs below
    assert E.check_ops(P.compile(ExprCmp(d4_l, "<", d4_r), ["a", "b"])[1][0][2][0], 2, 0, want=2)[1] == 4
    d8 = A
    for k in range(6):
        d8 = B + d8 if k % 2 else A - d8                    # right-leaning: the stack grows to 7
    d8_pred_ops = P.compile(ExprCmp(IntArr(bonus), ">=", d8), ["a", "b"])[1][0][2][0]
    assert E.check_ops(d8_pred_ops, 2, 1, want=2)[1] == 8
    progs = [(d4_l, d4_r), (IntArr(bonus), d8), (A / B, A % B), (ToInt(X * 2.0) + A, B), (ToFloat(A) / ToFloat(B), X), (-A, ToInt(-X))]
    for lhs, rhs in progs:
        for rel in RELS:
            pred = ExprCmp(lhs, rel, rhs)
            flags = model_flags(pred, rows)
            check_modes(ctx, cols, pred, flags, nrows=n, what=(lhs, rel, rhs))
        both = model_flags(ExprCmp(lhs, "<=", rhs), rows)
        assert both.any() and not both.all(), (lhs, rhs)


# ---- the bits meet every other term kind ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_expression_term_among_the_other_terms(ctx, device):
    rng = np.random.default_rng(11)
    n = 2 * T + 1
    names = ["Amelia", "Ava", "Oliver", "Olivia", "Isla"]
    rows = [{"price": PRICE[i], "qty": QTY[i], "name": names[rng.integers(0, 5)], "ship": names[rng.integers(0, 5)],
             "ts": rng.choice(["2016-09-14T10:00:00Z", "2016-10-01T00:00:00+01:00", "bad"])} for i in range(n)]
    cols = {k: make_col([r[k] for r in rows], "o64" if k == "name" else "o32", device) for k in rows[0]}
    amount = ExprCmp(AMOUNT, ">=", 100.0)
    preds = [
        All(Not(amount), Like(name="Olivia"), HasPrefix("ship", "O")),                                   # BITS + STR, lean
        All(Not(amount), Like(name="Olivia")),                                                           # BITS alone, lean
        P.Any(All(amount, ColCmp("name", "<", "ship")), ExprCmp(IntCol("qty"), "==", 25)),               # two expression terms + COLS
        All(amount, IntCmp("qty", ">", 3), P.FloatCmp("price", "<", 50.0), P.TimeCmp("ts", ">=", "2016-09-20T00:00:00Z"),
            P.Contains("name", "li"), ColCmp("ship", "!=", "name")),                                     # every kind in one kernel
        Not(All(ColCmp("name", "==", "ship"), P.StrCmp("name", ">", "B"))),                              # COLS + STR, lean
        All(amount, ExprCmp(IntCol("nope"), "<", 1)),                                                    # a missing column: false
        P.Any(amount, ExprCmp(IntCol("nope"), "!=", 1)),
    ]
    for k, pred in enumerate(preds):
        flags = model_flags(pred, rows)
        if k < 5:
            assert flags.any() and not flags.all(), k
        check_modes(ctx, cols, pred, flags, nrows=n, modes=("where", "take_while", "drop_while"), what=k)
        check_modes(ctx, cols, pred, flags, 70, n - 70, skip=2, limit=500, what=k)


@pytest.mark.gpu
def test_single_term_runs_k_expr_cmp_alone(ctx):
    """A WHERE program of exactly one expression term: k_expr_cmp's bitmap is the answer, no k_pred_eval is launched."""
    n = T + 1
    cols = {"price": make_col(PRICE[:n], "o32", True), "qty": make_col(QTY[:n], "o32", True)}
    ctx.profile(True)
    try:
        ctx.profile_read()
        check_modes(ctx, cols, ExprCmp(AMOUNT, ">=", 100.0), amount_flags(">=")[:n], nrows=n)
        stats = ctx.profile_read()
        assert stats["k_expr_cmp"]["launches"] == 1 and stats["k_expr_cmp"]["algo_bytes"] > n / 8
        assert not any(name.startswith("k_pred_eval") for name in stats), sorted(stats)
        assert "k_pred_emit" in stats
        # beside another term the bits go through k_pred_eval; a WHILE mode always does
        check_modes(ctx, cols, All(ExprCmp(AMOUNT, ">=", 100.0), Not(Like(qty="8"))),
                    amount_flags(">=")[:n] & np.array([q != "8" for q in QTY[:n]]), nrows=n)
        stats = ctx.profile_read()
        assert stats["k_expr_cmp"]["launches"] == 1 and stats["k_pred_eval"]["launches"] == 1
        check_modes(ctx, cols, ExprCmp(AMOUNT, ">=", 100.0), amount_flags(">=")[:n], nrows=n, modes=("take_while",))
        stats = ctx.profile_read()
        assert stats["k_expr_cmp"]["launches"] == 1 and stats["k_pred_eval"]["launches"] == 1
    finally:
        ctx.profile(False)


# ---- ColCmp -------------------------------------------------------------------------------------------------------------------

def _colcmp_pool():
    master = bytes([0x61, 0x00, 0x80, 0x62, 0xFF, 0x61, 0x7F, 0x80, 0x00, 0x62, 0x61, 0x61, 0xFE, 0x01, 0x62, 0x80, 0x61]) + bytes(range(0x30, 0x30 + 23))
    assert len(master) == 40
    pool = [master[:k] for k in (0, 1, 7, 8, 9, 16, 17, 40)]
    for k in range(0, 18):                                   # equal prefixes of every length up to 17, then a smaller / larger byte
        pool.append(master[:k] + b"\x00")
        pool.append(master[:k] + b"\xff" + master[k + 1:k + 3])
    out = []
    for v in pool:
        if v not in out:
            out.append(v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_colcmp_all_relations(ctx, device):
    pool = _colcmp_pool()
    assert {0, 1, 7, 8, 9, 16, 17, 40} <= {len(v) for v in pool}
    rng = np.random.default_rng(3)
    n, first_row = T + 65, 5
    total = first_row + n
    ia, ib = rng.integers(0, len(pool), total), rng.integers(0, len(pool), total)
    pairs = [(i, j) for i in range(len(pool)) for j in range(len(pool))]
    for p, (i, j) in enumerate(pairs[:total - first_row]):   # every pair of the pool, both orders, behind first_row
        ia[first_row + p], ib[first_row + p] = i, j
    assert len(pairs) <= n
    rows = [{"a": pool[i], "b": pool[j]} for i, j in zip(ia, ib)]
    fix = [v.ljust(8, b"\x00")[:8] for v in pool]            # a fixed-width column of 8 bytes
    layouts = [(make_col(pool, "o32", device), make_col(pool, "o64", device), rows),
               (make_col(fix, "fix", device), make_col(pool, "o32", device), [{"a": fix[i], "b": pool[j]} for i, j in zip(ia, ib)])]
    for ca, cb, rws in layouts:
        cols = {"a": ca, "b": cb}
        ids = {"a": make_ids(ia, 64, 11, device), "b": make_ids(ib, 32, 0, device)}
        for rel in RELS:
            pred = ColCmp("a", rel, "b")
            flags = model_flags(pred, rws)
            assert flags[first_row:].any() and not flags[first_row:].all()
            check_modes(ctx, cols, pred, flags, first_row, n, row_ids=ids, modes=("where", "take_while", "drop_while"), what=rel)
            # a column the rows lack, on either side: false under every relation
            for pred in (ColCmp("a", rel, "nope"), ColCmp("nope", rel, "b")):
                check_modes(ctx, cols, pred, np.zeros(total, dtype=bool), first_row, n, row_ids=ids, what=("missing", rel))
            check_modes(ctx, cols, Not(ColCmp("nope", rel, "b")), np.ones(total, dtype=bool), first_row, 70, row_ids=ids)
        check_modes(ctx, cols, ColCmp("a", "==", "a"), np.ones(total, dtype=bool), first_row, n, row_ids=ids)


# ---- CPH_ERR_INVALID ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_argument_errors(ctx):
    from csvplus_amd.materialize import _pred_program
    col = StrCol.from_values([b"1", b"22", b"1"], fixed_width=0)
    arr = (N.cph_strcol * 2)()
    arr[0], k0 = col.as_c()
    arr[1], k1 = col.as_c()
    one, flt = (E.LIT_INT, 0, 1), (E.LIT_FLT, 0, 1.0)

    def call(ops, patch=None):
        keep = []
        prog = _pred_program(ops, keep, 3)
        if patch:
            patch(prog, keep)
        opts = N.cph_filter_opts(N.CPH_FILTER_WHERE, 32, 0, 0, N.CPH_NO_LIMIT)
        out = C.POINTER(N.cph_rowlist)()
        rc = ctx.lib.cph_filter_rows(ctx.handle, arr, None, 2, 3, prog, len(ops), C.byref(opts), HOST, C.byref(out))
        if out:
            assert rc == N.CPH_OK
            ctx.lib.cph_rowlist_release(out)
        return rc, ctx.last_error()

    def pexpr(prog):
        return C.cast(prog[0].value.data, C.POINTER(N.cph_pred_expr)).contents

    ex = lambda eops, arrs=(): [(P.EXPR_LT, 0, (list(eops), list(arrs)))]   # noqa: E731
    assert call(ex([(E.COL_INT, 1, None), one]))[0] == N.CPH_OK
    assert call([(P.EXPR_LT + 3, -1, None)])[0] == N.CPH_OK                 # a missing column: the value is ignored
    assert call([(P.COLS_LT, 0, 1)])[0] == N.CPH_OK and call([(P.COLS_LT, -1, 1)])[0] == N.CPH_OK and call([(P.COLS_LT, 0, -1)])[0] == N.CPH_OK
    bad = {
        "one value left": ex([one, one, (E.ADD, 0, None)]),
        "three values left": ex([one, one, one]),
        "mixed types": ex([one, flt]),
        "mixed types inside": ex([one, flt, (E.ADD, 0, None), one]),
        "a COL arg out of range": ex([(E.COL_INT, 2, None), one]),
        "a negative COL arg": ex([(E.COL_INT, -1, None), one]),
        "a NUM arg out of range": ex([(E.NUM_INT, 0, None), one]),
        "arg 1": [(P.EXPR_LT, 1, ([one, one], []))],
        "COLS column out of range": [(P.COLS_LT, 2, 0)],
        "COLS second column out of range": [(P.COLS_LT, 0, 2)],
        "COLS second column below -1": [(P.COLS_LT, 0, -2)],
    }
    for what, ops in bad.items():
        rc, msg = call(ops)
        assert rc == N.CPH_ERR_INVALID and msg, what
    assert "no implicit conversions" in call(bad["mixed types"])[1]
    assert "not exactly two" in call(bad["one value left"])[1] and "not exactly two" in call(bad["three values left"])[1]

    def patched(fn):
        return call(ex([one, one]), lambda prog, keep: fn(prog, keep))

    def len_wrong(prog, keep):
        prog[0].value.len = C.sizeof(N.cph_pred_expr) - 1

    def data_null(prog, keep):
        prog[0].value.data = None

    def prog_null(prog, keep):
        pexpr(prog).prog = None

    def nnums_9(prog, keep):
        nums = (N.cph_expr_nums * 9)()
        keep.append(nums)
        pexpr(prog).nnums, pexpr(prog).nums = 9, nums

    def nums_null(prog, keep):
        pexpr(prog).nnums = 1

    def nops_1(prog, keep):
        pexpr(prog).nops = 1

    def nops_33(prog, keep):
        pexpr(prog).nops = 33

    for fn in (len_wrong, data_null, prog_null, nnums_9, nums_null, nops_1, nops_33):
        rc, msg = patched(fn)
        assert rc == N.CPH_ERR_INVALID and msg, fn.__name__

    def cols_len(prog, keep):
        prog[0].value.len = 8

    def cols_null(prog, keep):
        prog[0].value.data = None

    for fn in (cols_len, cols_null):
        rc, msg = call([(P.COLS_LT + 2, 0, 1)], fn)
        assert rc == N.CPH_ERR_INVALID and msg, fn.__name__
    for op in (55, 62, 63, 64, 71, 78):                                     # still unknown
        rc, msg = call([(op, 0, b"1")])
        assert rc == N.CPH_ERR_INVALID and "unknown op" in msg, op
    # 32 terms in all: expression and column terms count
    t = (P.COLS_LT, 0, 1)
    assert call([t] * 32 + [(P.ALL, 32, None)])[0] == N.CPH_OK
    rc, msg = call([t] * 32 + ex([one, one]) + [(P.ALL, 33, None)])
    assert rc == N.CPH_ERR_INVALID and "32" in msg
    del k0, k1


# ---- Switch, Validate, the pipeline ---------------------------------------------------------------------------------------------

def _values(cb):
    sc = cb.to_strcol()
    data, offs = sc.data.tobytes(), sc.offsets
    return [data[int(offs[i]):int(offs[i + 1])] for i in range(sc.nrows)]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_switch_tiers_over_joined_rows(ctx, device):
    """When(amount >= 1000, gold, When(amount >= 100, silver, std)) with price read through a Join's row ids."""
    from csvplus_amd.materialize import map_switch
    rng = np.random.default_rng(21)
    n = T + 70
    stock = ["0.5", "12.5", "100", "250.75", "n/a", "1e23", "1e38"]   # the last: a deferred float leaf
    sid = rng.integers(0, len(stock), n)
    qty = [str(v) for v in rng.choice([1, 4, 8, 10, 80, 2000], n)]
    amount = FloatCol("price") * ToFloat(IntCol("qty"))
    sw = M.Switch((ExprCmp(amount, ">=", 1000.0), "gold"), (ExprCmp(amount, ">=", 100.0), M.Format("silver ", M.Col("qty"))),
                  (ColCmp("qty", "==", "price"), "same"), otherwise=M.Format("std ", M.Col("price")))
    rows = [{"price": stock[sid[i]], "qty": qty[i]} for i in range(n)]
    cols = {"price": make_col(stock, "o32", device), "qty": make_col(qty, "o64", device)}
    cb, which = map_switch(ctx, cols, sw, row_ids={"price": make_ids(sid, 32, 2, device)}, nrows=n, want_which=True)
    try:
        want_which = [M.which_of(sw, r, i) for i, r in enumerate(rows)]
        assert {0, 1, 3} <= set(want_which)
        assert which.tolist() == want_which
        assert _values(cb) == [M.render(sw, r, i) for i, r in enumerate(rows)]
    finally:
        cb.release()


@pytest.mark.gpu
def test_validate_first_failing_row(ctx):
    from csvplus_amd.materialize import validate_rows
    n = T + 70
    price, qty, amount = ["2.5"] * n, ["4"] * n, ["10"] * n
    ok = All(ExprCmp(IntCol("qty"), ">", 0), ExprCmp(FloatCol("price") * ToFloat(IntCol("qty")), "==", FloatCol("amount")))
    cols = lambda: {"price": make_col(price, "o32", True), "qty": make_col(qty, "o32", True), "amount": make_col(amount, "o32", True)}   # noqa: E731
    assert validate_rows(ctx, cols(), ok) is None
    for bad, behind in ((T + 69, None), (T - 1, T + 69), (64, T - 1)):   # the lowest failing row decides
        amount[bad] = "10.5"
        assert validate_rows(ctx, cols(), ok) == bad
        assert validate_rows(ctx, cols(), ok, first_row=bad + 1) == behind
    qty[3] = "zero"
    assert validate_rows(ctx, cols(), ok) == 3
    single = ExprCmp(FloatCol("price") * ToFloat(IntCol("qty")), "==", FloatCol("amount"))
    assert validate_rows(ctx, cols(), single, first_row=4) == 64


@pytest.mark.gpu
def test_filter_to_csv_where_exprcmp(ctx):
    from csvplus_amd import pipeline as PL
    n = 3000
    rng = np.random.default_rng(8)
    price = [rng.choice(["12.5", "0.75", "100", "bad", "1e23"]) for _ in range(n)]
    qty = [str(v) for v in rng.integers(0, 30, n)]
    ship = [rng.choice(["Leeds", "York", "Hull"]) for _ in range(n)]
    bill = [rng.choice(["Leeds", "York", "Hull"]) for _ in range(n)]
    text = b"id,price,qty,ship,bill\n" + b"".join(f"{i},{price[i]},{qty[i]},{ship[i]},{bill[i]}\n".encode() for i in range(n))
    table = PL.read_table(ctx, text)
    try:
        for pred in (ExprCmp(FloatCol("price") * ToFloat(IntCol("qty")), ">=", 100.0),
                     All(ExprCmp(FloatCol("price") * ToFloat(IntCol("qty")), "<", 100.0), ColCmp("ship", "!=", "bill"))):
            rows = [{"price": price[i], "qty": qty[i], "ship": ship[i], "bill": bill[i]} for i in range(n)]
            kept = [i for i in range(n) if P.matches(pred, rows[i], i)]
            assert 0 < len(kept) < n
            want = b"id,qty\n" + b"".join(f"{i},{qty[i]}\n".encode() for i in kept[2:2 + 500])
            assert PL.filter_to_csv(ctx, table, pred, ["id", "qty"], skip=2, limit=500) == want
            tier = M.When(ExprCmp(IntCol("qty"), ">=", 20), "bulk", "few")
            got = PL.filter_to_csv(ctx, table, pred, ["id", "tier"], computed={"tier": tier}, limit=100)
            assert got == b"id,tier\n" + b"".join(f"{i},{'bulk' if int(qty[i]) >= 20 else 'few'}\n".encode() for i in kept[:100])
    finally:
        table.release()


@pytest.mark.gpu
def test_join_to_csv_where_and_computed(ctx):
    """pipeline.join_to_csv(where=ExprCmp over a stream column and a build column, computed=a Switch keyed on the expression) is
    byte-equal to the unfiltered text filtered and extended line by line on the host."""
    from csvplus_amd import pipeline as PL
    from helpers import orders_table, stock_table
    stock, orders = stock_table(), orders_table(n=3000)
    stock["price"] = ["0.5", "2.25", "10", "12.5", "n/a", "1e38", "40", "99.99"]
    text = lambda tab: (",".join(tab) + "\n" + "".join(",".join(tab[k][i] for k in tab) + "\n" for i in range(len(next(iter(tab.values())))))).encode()   # noqa: E731
    tp, to = PL.read_table(ctx, text(stock)), PL.read_table(ctx, text(orders))
    steps = [(tp, "prod_id", "prod_id")]
    outc = [("order_id", to, "order_id"), ("product", tp, "product"), ("price", tp, "price"), ("qty", to, "qty")]
    amount = FloatCol("price") * ToFloat(IntCol("qty"))
    pred = All(ExprCmp(amount, ">=", 100.0), Not(ColCmp("product", "<", "order_id")))
    tier = M.When(ExprCmp(amount, ">=", 1000.0), "gold", M.Format("silver ", M.Col("product")))
    try:
        body = [ln for ln in PL.join_to_csv(ctx, to, steps, outc).split(b"\n")[1:] if ln]
        assert len(body) == 3000
        rows = [dict(zip(("order_id", "product", "price", "qty"), ln.split(b","))) for ln in body]
        kept = [i for i, r in enumerate(rows) if P.matches(pred, r)]
        assert 100 < len(kept) < 2900
        head = b"order_id,product,price,qty\n"
        assert PL.join_to_csv(ctx, to, steps, outc, where=pred, skip=1, limit=700) == head + b"".join(body[i] + b"\n" for i in kept[1:701])
        got = PL.join_to_csv(ctx, to, steps, [("order_id", to, "order_id"), ("tier", None, None)], where=pred, computed={"tier": tier})
        want = b"order_id,tier\n" + b"".join(rows[i]["order_id"] + b"," + M.render(tier, rows[i]) + b"\n" for i in kept)
        assert got == want and b"gold" in got and b"silver" in got
    finally:
        tp.release()
        to.release()
