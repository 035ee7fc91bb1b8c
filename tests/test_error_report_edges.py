"""The error report of the typed-value passes at the edges the other tests only touch at small n: the LOWEST (row, tag) wins
across lanes, waves, tiles and grid-stride rounds, its kind comes with it, and nerrors is the full count.

Through the Python facade: to_int / to_float (k_num_parse: 2048-row tiles, 8 groups of 64 rows per wave), eval_number
(k_expr_eval, the same geometry; tag = the failing op), order_rows (k_order_key_num: at most 8192 x 256 rows per grid-stride
round; tag = the key), join_totals (k_jt_errors: 2048 x 256 rows per round; tag = the spec), resolve_duplicates_device
(k_resolve_tile) and totals (the merge of several columns' reports; tag = the spec).  Every expected value is computed here from
the inputs with numpy / plain Python."""
import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import aggregate as A
from csvplus_amd import datagen as dg
from csvplus_amd import dedup as D
from csvplus_amd import expr as E
from csvplus_amd.materialize import NumCol, eval_number, order_rows, to_float, to_int
from csvplus_amd.ordering import Asc, OrderError

pytestmark = pytest.mark.gpu

OK, SYNTAX, RANGE = N.CPH_NUM_OK, N.CPH_NUM_ERR_SYNTAX, N.CPH_NUM_ERR_RANGE
TILE = 2048
TEXT = {"int": {OK: b"17", SYNTAX: b"1x", RANGE: b"99999999999999999999"},
        "float": {OK: b"2.5", SYNTAX: b"2.5.", RANGE: b"1e999"}}


def first_and_count(kinds):
    """(lowest bad row, its kind, number of bad rows) of one status-per-row array."""
    bad = np.flatnonzero(kinds)
    return int(bad[0]), int(kinds[bad[0]]), len(bad)


def text_col(kinds, what):
    return StrCol.from_values([TEXT[what][int(k)] for k in kinds])


def host_numcol(values, status):
    """What order_rows / join_totals take as a number source with status bytes: a NumCol in host memory."""
    nc = NumCol.__new__(NumCol)
    nc.ctx, nc.ptr = None, None
    nc.nrows, nc.mem = len(values), N.CPH_MEM_HOST
    nc.kind = N.CPH_NUM_FLOAT64 if values.dtype == np.float64 else N.CPH_NUM_INT64
    nc.values, nc.status = values, status
    nc.nerrors, nc.host_rows, nc.first_error_row, nc.first_error_kind = int(np.count_nonzero(status)), 0, None, 0
    return nc


# ---- to_int / to_float ------------------------------------------------------------------------------------------------------
def numparse_cases():
    cases = []
    for rows in ([TILE], [63, 64], [TILE - 1, TILE], [0, TILE]):
        k = np.zeros(TILE + 1, np.uint8)
        k[rows] = SYNTAX
        cases.append(("rows " + "+".join(map(str, rows)), k))
    k = np.zeros(2 * TILE + 1, np.uint8)
    k[1000:] = SYNTAX
    cases.append(("every row from 1000 on", k))
    k = np.zeros(TILE + 1, np.uint8)
    k[TILE - 1], k[TILE] = RANGE, SYNTAX     # the lower row's kind is the one reported
    cases.append(("range below syntax", k))
    k = np.zeros(TILE + 1, np.uint8)
    k[70], k[TILE] = SYNTAX, RANGE
    cases.append(("syntax below range", k))
    return cases


@pytest.mark.parametrize("what", ["int", "float"])
@pytest.mark.parametrize("reverse", [False, True], ids=["identity", "reversed row ids"])
def test_numparse_first_error_across_groups_waves_and_tiles(ctx, what, reverse):
    conv = to_int if what == "int" else to_float
    for name, kinds in numparse_cases():
        n = len(kinds)
        ids = np.arange(n - 1, -1, -1, dtype=np.uint32) if reverse else None
        seen = kinds[ids] if reverse else kinds            # status by row of the SELECTION
        got = conv(ctx, text_col(kinds, what), row_ids=ids)
        row, kind, count = first_and_count(seen)
        assert (got.nerrors, got.first_error_row, got.first_error_kind) == (count, row, kind), (name, what, reverse)
        np.testing.assert_array_equal(got.status, seen, err_msg=name)
    assert first_and_count(numparse_cases()[4][1]) == (1000, SYNTAX, 3097)


# ---- eval_number ------------------------------------------------------------------------------------------------------------
def test_expr_first_error_row_kind_and_op(ctx):
    n = TILE + 1
    expr = E.IntCol("a") / E.IntCol("b")
    names, ops = E.compile(expr, ["a", "b"])
    div = [q for q, o in enumerate(ops) if o[0] == E.DIV][0]
    col_a = [q for q, o in enumerate(ops) if o[0] == E.COL_INT and names[o[1]] == "a"][0]
    assert col_a < div
    a, b = [b"12"] * n, [b"3"] * n
    a[TILE] = b"1x"                                        # row 2048: the leaf fails (op col_a), and 0 / 0 would fail too
    b[TILE - 1] = b[TILE] = b"0"
    got = eval_number(ctx, {"a": StrCol.from_values(a), "b": StrCol.from_values(b)}, expr)
    assert (got.nerrors, got.first_error_row, got.first_error_kind, got.first_error_op) == (2, TILE - 1, N.CPH_NUM_ERR_DIV_ZERO, div)
    assert got.status[TILE - 1] == N.CPH_NUM_ERR_DIV_ZERO and got.status[TILE] == SYNTAX   # the first failing op decides a row
    assert not got.status[: TILE - 1].any()
    b[TILE - 1] = b"3"                                     # only the row where two ops fail
    got = eval_number(ctx, {"a": StrCol.from_values(a), "b": StrCol.from_values(b)}, expr)
    assert (got.nerrors, got.first_error_row, got.first_error_kind, got.first_error_op) == (1, TILE, SYNTAX, col_a)


# ---- order_rows -------------------------------------------------------------------------------------------------------------
ROUND_ORDER = 8192 * 256   # rows one grid-stride round of k_order_key_num covers


@pytest.mark.parametrize("rows", [[ROUND_ORDER], [5, ROUND_ORDER]], ids=["second round only", "first round wins"])
def test_order_first_error_across_grid_stride_rounds(ctx, rows):
    n = ROUND_ORDER + 1
    st = np.zeros(n, np.uint8)
    st[rows[-1]] = SYNTAX
    st[rows[0]] = RANGE
    with pytest.raises(OrderError) as ei:
        order_rows(ctx, [Asc(host_numcol(np.zeros(n, np.int64), st))], n)
    row, kind, count = first_and_count(st)
    assert (ei.value.row, ei.value.key, ei.value.kind, ei.value.nerrors) == (row, 0, kind, count)


def test_order_lowest_row_then_lowest_key(ctx):
    n = 300
    v = np.arange(n, dtype=np.int64)
    st0, st1 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    st0[7], st1[7], st1[3] = SYNTAX, RANGE, SYNTAX
    with pytest.raises(OrderError) as ei:
        order_rows(ctx, [Asc(host_numcol(v, st0)), Asc(host_numcol(v, st1))], n)
    assert (ei.value.row, ei.value.key, ei.value.kind, ei.value.nerrors) == (3, 1, SYNTAX, 3)
    st1[3] = OK                                            # both keys fail at row 7 and nowhere else: key 0 is named
    with pytest.raises(OrderError) as ei:
        order_rows(ctx, [Asc(host_numcol(v, st0)), Asc(host_numcol(v, st1))], n)
    assert (ei.value.row, ei.value.key, ei.value.kind, ei.value.nerrors) == (7, 0, SYNTAX, 2)


# ---- join_totals ------------------------------------------------------------------------------------------------------------
ROUND_JT = 2048 * 256      # rows one round of k_jt_errors covers


@pytest.fixture(scope="module")
def joined(ctx):
    """ROUND_JT + 1 joined rows onto a 4-row unique index."""
    n = ROUND_JT + 1
    ix = N.DeviceIndex(ctx, [dg.customers(4)["id"]], unique=True)
    assert ix.status == N.CPH_OK
    ch = N.join_chain(ctx, [(ix, [dg.orders(n, 4, 4)["cust_id"]])], out_mem=N.CPH_MEM_DEVICE)
    assert ch.nrows == n
    yield ch, ix, n
    ch.release()
    ix.close()


def jt_error(joined, statuses):
    ch, ix, n = joined
    v = np.ones(n, np.int64)
    with pytest.raises(A.TotalsError) as ei:
        A.join_totals(ch, 0, ix, [A.Sum(host_numcol(v, st), "int") for st in statuses])
    e = ei.value
    return e.row, e.spec, e.kind, e.nerrors


def test_join_totals_first_error_across_rounds(joined):
    n = joined[2]
    st = np.zeros(n, np.uint8)
    st[ROUND_JT] = SYNTAX
    assert jt_error(joined, [st]) == (ROUND_JT, 0, SYNTAX, 1)
    st[9] = RANGE
    assert jt_error(joined, [st]) == (9, 0, RANGE, 2)


def test_join_totals_lowest_row_then_lowest_spec(joined):
    n = joined[2]
    st0, st1 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    st0[9], st1[9] = SYNTAX, RANGE
    st0[ROUND_JT] = RANGE
    assert jt_error(joined, [st0, st1]) == (9, 0, SYNTAX, 3)          # both at row 9: spec 0; nerrors adds up over the specs
    st1[9], st1[4] = OK, RANGE
    assert jt_error(joined, [st0, st1]) == (4, 1, RANGE, 3)           # spec 1 fails lower down


# ---- resolve with MIN over an int order column -------------------------------------------------------------------------------
def shuffled_keys(n, per_key, seed):
    """n fixed-width keys, sorted position p holding key p // per_key, in a shuffled table order; perm[p] = its table row."""
    rng = np.random.default_rng(seed)
    table_of = rng.permutation(n)                      # sorted position -> table row, were the sort unstable ...
    key_of_row = np.empty(n, np.int64)
    key_of_row[table_of] = np.arange(n) // per_key
    perm = np.argsort(key_of_row, kind="stable")       # ... the index is stable: equal keys keep their table order
    return [b"%07d" % int(k) for k in key_of_row], perm


def test_resolve_first_error_position_and_row_across_tiles(ctx):
    n = TILE + 1
    # every sorted position inside a group of 3 (an order value outside a group is never looked at); the last group spans the tile edge
    keys, perm = shuffled_keys(n, 3, seed=5)
    order = [b"5"] * n
    order[perm[TILE - 1]] = TEXT["int"][RANGE]
    order[perm[TILE]] = TEXT["int"][SYNTAX]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    with pytest.raises(D.ResolveError) as ei:
        D.resolve_duplicates_device(ix, D.MinBy(), order=StrCol.from_values(order), kind="int")
    e = ei.value
    assert (e.position, e.row, e.kind, e.nerrors) == (TILE - 1, int(perm[TILE - 1]), RANGE, 2)
    ix.close()


def test_resolve_distinct_keys_have_no_group_to_fail_in(ctx):
    """All keys distinct: positions equal runs, no row lies inside a group, so bad order values at positions 2047 and 2048 are not
    read as errors (ResolveError is about rows INSIDE a group) and every row survives."""
    n = TILE + 1
    keys, perm = shuffled_keys(n, 1, seed=6)
    order = [b"5"] * n
    order[perm[TILE - 1]] = order[perm[TILE]] = TEXT["int"][SYNTAX]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    got = D.resolve_duplicates_device(ix, D.MinBy(), order=StrCol.from_values(order), kind="int")
    assert (got.ngroups, got.group_rows) == (0, 0)
    np.testing.assert_array_equal(got.positions, np.arange(n, dtype=np.uint64))
    got.index.close()
    ix.close()


# ---- totals with two StrCol specs ---------------------------------------------------------------------------------------------
def test_totals_lowest_position_then_lowest_spec(ctx):
    n = 64
    keys, perm = shuffled_keys(n, 2, seed=7)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])

    def run(bad0, bad1):
        c0, c1 = [b"1"] * n, [b"2"] * n
        for p, k in bad0:
            c0[perm[p]] = TEXT["int"][k]
        for p, k in bad1:
            c1[perm[p]] = TEXT["int"][k]
        with pytest.raises(A.TotalsError) as ei:
            A.totals(ix, [A.Sum(StrCol.from_values(c0), "int"), A.Sum(StrCol.from_values(c1), "int")])
        e = ei.value
        return e.position, e.row, e.spec, e.kind, e.nerrors

    assert run([(20, SYNTAX)], [(10, RANGE)]) == (10, int(perm[10]), 1, RANGE, 2)
    assert run([(10, SYNTAX)], [(10, RANGE)]) == (10, int(perm[10]), 0, SYNTAX, 2)
    ix.close()
