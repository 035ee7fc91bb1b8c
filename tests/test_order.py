"""OrderBy on the device (cph_order_rows, materialize.order_rows, pipeline.totals_to_csv / filter_to_csv with order_by) against
ordering.order_model — slices.SortStableFunc over cmp.Compare per key, in pure Python — for EQUALITY: a stable sort has one
right answer.  The large cases arrange their rows in a few ascending stretches of random 64-bit values, which Python's merge
sort orders in a few passes; the device sort does not look at the arrangement."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import aggregate as A
from csvplus_amd import materialize as MZ
from csvplus_amd import ordering as O
from csvplus_amd import pipeline as PL
from tests.helpers import orders_table

pytestmark = pytest.mark.gpu

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
TILE = 4096       # keys per sort tile: radix_plan (csvplus_amd/csrc/radix_sort.hip) — 256 threads x kSortItems = 16, below 2^22 rows of 64-bit keys
GATE = 4          # kSelectGate in csvplus_amd/csrc/order.hip: skip + limit <= nrows / 4 takes the select
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
SIZES = [0, 1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]   # around a wave, a workgroup and a sort tile


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


def ids_of(r):
    """The ids of an Ordered as a list, from wherever they live."""
    if r.mem == HOST or len(r) == 0:
        return r.to_numpy().tolist()
    ptr, bits, cnt = r.as_row_ids()
    assert bits == 32 and cnt == len(r)
    return d2h(ptr, cnt, np.uint32).tolist()


def run(ctx, keys, n, skip=0, limit=None, out_mem=HOST):
    r = MZ.order_rows(ctx, keys, n, skip=skip, limit=limit, out_mem=out_mem)
    try:
        return ids_of(r), r.select_used, r.candidates
    finally:
        r.release()


def model_keys(keys):
    """The same keys for order_model: arrays as lists."""
    return [type(k)(k.source.tolist() if isinstance(k.source, np.ndarray) else k.source, k.kind_name) for k in keys]


def stretches(rng, n, r, lo=INT64_MIN, hi=INT64_MAX):
    """n distinct random int64 in r ascending stretches (stretch c holds the values of rank c, c + r, ...)."""
    vals = np.unique(rng.integers(lo, hi, n + n // 8 + 16, dtype=np.int64))
    vals = vals[np.sort(rng.choice(len(vals), n, replace=False))]
    return np.ascontiguousarray(np.concatenate([vals[c::r] for c in range(r)]))


# ---- one key -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_one_int_key(ctx, n):
    rng = np.random.default_rng(100 + n)
    few = rng.integers(-3, 4, n, dtype=np.int64)                       # a range of 7: many ties
    full = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    if n >= 2:
        full[rng.integers(0, n)] = INT64_MIN
        full[(int(np.argmin(full)) + 1) % n] = INT64_MAX
        assert INT64_MIN in full and INT64_MAX in full
    for v in (few, full):
        for kind in (O.Asc, O.Desc):
            got, sel, cand = run(ctx, [kind(v)], n)
            assert got == O.order_model([kind(v.tolist(), "int")]), (n, kind.__name__)
            assert not sel and cand == n


FLOAT_EDGES = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.7976931348623157e308,
               -1.7976931348623157e308, math.inf, -math.inf]
NAN_BITS = [0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF]


def float_mix(rng, n):
    """Random doubles (random bit patterns: every exponent) with the edge values, several NaNs of different bits and both
    zeros written over them at distinct positions, each several times."""
    v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    pos = rng.permutation(n)[:4 * (len(FLOAT_EDGES) + len(NAN_BITS))]
    pats = [int(np.float64(x).view(np.uint64)) for x in FLOAT_EDGES] + NAN_BITS
    for i, p in enumerate(pos):
        v[p] = pats[i % len(pats)]
    return v.view(np.float64)


@pytest.mark.parametrize("n", [257, TILE + 1, 3 * TILE + 1])
def test_one_float_key(ctx, n):
    v = float_mix(np.random.default_rng(200 + n), n)
    assert np.isnan(v).sum() >= 4 * len(NAN_BITS) and (v == 0).sum() >= 8 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    for kind in (O.Asc, O.Desc):
        got, _, _ = run(ctx, [kind(v)], n)
        want = O.order_model([kind(v.tolist(), "float")])
        assert got == want, kind.__name__
    # stability is visible: the NaNs come out in input order, first under Asc and last under Desc; so do the zeros
    nans = np.flatnonzero(np.isnan(v)).tolist()
    assert run(ctx, [O.Asc(v)], n)[0][:len(nans)] == nans and run(ctx, [O.Desc(v)], n)[0][-len(nans):] == nans


# ---- three keys ------------------------------------------------------------------------------------------------------------
def three_key_table(seed, n=5000):
    rng = np.random.default_rng(seed)
    names = [b"pear", b"apple", b"fig", b"apple pie", b"10"]            # 5 distinct keys; "10" sorts first, "apple" < "apple pie"
    a = [names[i] for i in rng.integers(0, 5, n)]
    b = [[b"x", b"", b"xy"][i] for i in rng.integers(0, 3, n)]
    qty = rng.integers(7, 11, n, dtype=np.int64)                        # 4 distinct values
    price = rng.integers(0, 40, n).astype(np.float64) / 4.0             # 40 values: the input order decides the rest
    return a, b, qty, price


@pytest.mark.parametrize("shape", ["one_column", "two_columns", "selected"])
def test_three_keys_bytes_int_float(ctx, shape):
    n = 5000
    a, b, qty, price = three_key_table(31)
    if shape == "two_columns":
        ix = N.DeviceIndex(ctx, [StrCol.from_values(a), StrCol.from_values(b)])
        first = list(zip(a, b))
    else:
        ix = N.DeviceIndex(ctx, [StrCol.from_values(a)])
        first = a
        if shape == "selected":   # the same rows through cph_index_select: every sorted position
            whole, ix = ix, ix.select(np.arange(n, dtype=np.uint64))
            whole.close()
    assert ix.nrows == n
    try:
        for k0, k1, k2 in ((O.Asc, O.Desc, O.Asc), (O.Desc, O.Asc, O.Desc)):
            got, _, _ = run(ctx, [k0(ix), k1(qty), k2(price)], n)
            want = O.order_model([k0(first, "bytes"), k1(qty.tolist(), "int"), k2(price.tolist(), "float")])
            assert got == want, (shape, k0.__name__)
        # the BYTES key last: ranks sorted first, the number keys on top
        got, _, _ = run(ctx, [O.Desc(qty), O.Asc(ix)], n)
        assert got == O.order_model([O.Desc(qty.tolist(), "int"), O.Asc(first, "bytes")])
        # ... and through the select: the rank key is the first key, 32-bit
        got, sel, cand = run(ctx, [O.Asc(ix), O.Desc(qty), O.Asc(price)], n, skip=5, limit=100)
        assert got == O.order_model([O.Asc(first, "bytes"), O.Desc(qty.tolist(), "int"), O.Asc(price.tolist(), "float")], 5, 100)
        assert sel and cand == sum(1 for x in first if x == min(first))   # 105 rows lie inside the smallest key's run (~1000 rows)
    finally:
        ix.close()


# ---- skip x limit ------------------------------------------------------------------------------------------------------------
def test_skip_and_limit(ctx):
    n = 1000
    rng = np.random.default_rng(7)
    v = rng.integers(0, 300, n, dtype=np.int64)
    w = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    for keys in ([O.Desc(v)], [O.Asc(v), O.Desc(w)]):
        mk = model_keys(keys)
        for skip in (0, 1, n - 1, n, n + 5):
            for limit in (0, 1, 10, n, None):
                got, sel, cand = run(ctx, keys, n, skip=skip, limit=limit)
                assert got == O.order_model(mk, skip, limit), (skip, limit)
                if limit is not None and 0 < limit and skip + limit <= n // GATE:
                    assert sel and skip + limit <= cand <= n
                elif got:
                    assert not sel and cand == n
    r = MZ.order_rows(ctx, [O.Asc(v)], n, skip=n + 5)
    assert len(r) == 0 and r.to_numpy().tolist() == [] and r.candidates == 0
    r.release()


# ---- the select route ----------------------------------------------------------------------------------------------------------
def sort_bytes(prof):
    return sum(st["algo_bytes"] for name, st in prof.items() if name.startswith("k_radix_"))


@pytest.mark.parametrize("skip", [0, 3])
def test_select_route_distinct_keys(ctx, skip):
    n, limit = 200_000, 10
    v = stretches(np.random.default_rng(11), n, 4)
    for kind in (O.Asc, O.Desc):
        want = O.order_model([kind(v.tolist(), "int")], skip, limit)
        ctx.profile(True)
        try:
            ctx.profile_read()
            got, sel, cand = run(ctx, [kind(v)], n, skip=skip, limit=limit)
            prof_on = ctx.profile_read()
            ctx.set_option("order_select", 0)
            try:
                got_off, sel_off, cand_off = run(ctx, [kind(v)], n, skip=skip, limit=limit)
            finally:
                ctx.set_option("order_select", 1)
            prof_off = ctx.profile_read()
        finally:
            ctx.profile(False)
        assert got == want and got_off == want
        assert sel and cand == skip + limit and not sel_off and cand_off == n
        select_kernels = {name for name in prof_on if name.startswith("k_order_select_")}
        assert {"k_order_select_hist_u64", "k_order_select_pick", "k_order_select_flag_u64", "k_order_select_emit"} <= select_kernels
        assert prof_on["k_order_select_hist_u64"]["launches"] == 8 and not any(name.startswith("k_order_select_") for name in prof_off)
        assert 0 < sort_bytes(prof_on) < sort_bytes(prof_off)


def test_select_route_ties_at_the_threshold(ctx):
    n = 200_000
    rng = np.random.default_rng(12)
    sizes = [2500, 50_000, 47_500, 2500, 50_000, 47_500]                # first key 0, 1, 2, 0, 1, 2
    first = np.concatenate([np.full(s, i % 3, dtype=np.int64) for i, s in enumerate(sizes)])
    second = np.concatenate([np.sort(rng.integers(INT64_MIN, INT64_MAX, s, dtype=np.int64)) for s in sizes])
    skip, limit = 4990, 20                                               # rows 4990 .. 5009 of the order: the cut lies inside the run of 1s
    got, sel, cand = run(ctx, [O.Asc(first), O.Asc(second)], n, skip=skip, limit=limit)
    want = O.order_model([O.Asc(first.tolist(), "int"), O.Asc(second.tolist(), "int")], skip, limit)
    assert got == want and sel and cand == int((first <= 1).sum()) == 105_000
    assert set(first[got].tolist()) == {0, 1}                            # the second key decided on both sides of the boundary
    got, sel, cand = run(ctx, [O.Asc(first), O.Desc(second)], n, skip=skip, limit=limit)
    assert got == O.order_model([O.Asc(first.tolist(), "int"), O.Desc(second.tolist(), "int")], skip, limit) and cand == 105_000
    # an all-equal first key: every row is a candidate
    same = np.full(n, 5, dtype=np.int64)
    got, sel, cand = run(ctx, [O.Desc(same), O.Asc(second)], n, limit=10)
    assert got == O.order_model([O.Desc(same.tolist(), "int"), O.Asc(second.tolist(), "int")], 0, 10) and cand == n


def test_select_threshold_at_the_extreme_keys(ctx):
    n = 5000
    rng = np.random.default_rng(13)
    # the all-zero digits: NaN under Asc.  20 NaNs of different bits, the 13th smallest row is one of them
    v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    v[np.isnan(v.view(np.float64))] = 0
    nan_at = np.sort(rng.permutation(n)[:20])
    v[nan_at] = [NAN_BITS[i % len(NAN_BITS)] for i in range(20)]
    f = v.view(np.float64)
    got, sel, cand = run(ctx, [O.Asc(f)], n, skip=3, limit=10)
    assert got == O.order_model([O.Asc(f.tolist(), "float")], 3, 10) == nan_at[3:13].tolist() and sel and cand == 20
    # ... the largest skip + limit the gate lets through, descending
    got, sel, cand = run(ctx, [O.Desc(f)], n, skip=n // GATE - 10, limit=10)
    assert got == O.order_model([O.Desc(f.tolist(), "float")], n // GATE - 10, 10) and sel
    # NaN under Desc is the all-one key: NaNs everywhere but at 5 rows, every row is at or below the threshold
    g = np.full(n, NAN_BITS[1], dtype=np.uint64)
    g[[9, 10, 3000, 4095, 4096]] = np.array([1.5, -0.0, math.inf, 0.0, -math.inf]).view(np.uint64)
    g[[0, 4999]] = [NAN_BITS[3], NAN_BITS[4]]
    got, sel, cand = run(ctx, [O.Desc(g.view(np.float64))], n, limit=10)
    assert got == O.order_model([O.Desc(g.view(np.float64).tolist(), "float")], 0, 10) == [3000, 9, 10, 4095, 4096, 0, 1, 2, 3, 4] and sel and cand == n
    # the all-one digits under Asc: INT64_MAX everywhere but at 5 rows
    i = np.full(n, INT64_MAX, dtype=np.int64)
    i[[7, 100, 2047, 2048, 4999]] = [5, INT64_MIN, -1, 0, INT64_MAX - 1]
    got, sel, cand = run(ctx, [O.Asc(i)], n, limit=10)
    assert got == O.order_model([O.Asc(i.tolist(), "int")], 0, 10) == [100, 2047, 2048, 7, 4999, 0, 1, 2, 3, 4] and sel and cand == n
    # INT64_MIN under Desc is the all-one key as well
    j = np.full(n, INT64_MIN, dtype=np.int64)
    j[[1, 4998]] = [3, INT64_MAX]
    got, sel, cand = run(ctx, [O.Desc(j)], n, limit=5)
    assert got == [4998, 1, 0, 2, 3] and sel and cand == n


def test_a_million_rows_of_64_bit_keys(ctx):
    n = (1 << 20) + TILE + 1          # from 2^20 rows on the sort streams its digits (radix_sort.hip: stream_digits)
    v = stretches(np.random.default_rng(14), n, 4)
    order = O.order_model([O.Asc(v.tolist(), "int")])
    assert order == np.argsort(v, kind="stable").tolist()
    got, sel, cand = run(ctx, [O.Asc(v)], n)
    assert got == order and not sel and cand == n
    got, sel, cand = run(ctx, [O.Asc(v)], n, limit=100)
    assert got == order[:100] and sel and cand == 100
    got, sel, cand = run(ctx, [O.Desc(v)], n, skip=50, limit=100)
    assert got == order[::-1][50:150] and sel and cand == 150        # distinct keys: here descending IS the reverse


# ---- memory spaces -------------------------------------------------------------------------------------------------------------
def test_memory_spaces(ctx):
    import torch

    n = 3 * TILE + 1
    rng = np.random.default_rng(15)
    qty = rng.integers(0, 50, n, dtype=np.int64)
    price = float_mix(rng, n)
    want = O.order_model([O.Desc(qty.tolist(), "int"), O.Asc(price.tolist(), "float")])
    t_qty, t_price = torch.from_numpy(qty).to("cuda:0"), torch.from_numpy(price).to("cuda:0")
    for values in ("host", "device"):
        keys = [O.Desc(qty), O.Asc(price)] if values == "host" else [O.Desc(t_qty, "int"), O.Asc(t_price, "float")]
        for out_mem in (HOST, DEVICE):
            assert run(ctx, keys, n, out_mem=out_mem)[0] == want, (values, out_mem)
            assert run(ctx, keys, n, skip=2, limit=200, out_mem=out_mem)[0] == want[2:202], (values, out_mem)
    # a (device pointer, count) pair; a NumCol in device and in host memory
    assert run(ctx, [O.Desc((t_qty.data_ptr(), n), "int"), O.Asc((t_price.data_ptr(), n), "float")], n)[0] == want
    col = StrCol.from_values([str(int(x)) for x in qty])
    for mem in (HOST, DEVICE):
        nc = MZ.to_int(ctx, col, out_mem=mem)
        assert run(ctx, [O.Desc(nc), O.Asc(price)], n)[0] == want
        nc.release()


# ---- errors as data --------------------------------------------------------------------------------------------------------------
def raw_order(ctx, keys, nkeys, n, skip=0, limit=N.CPH_NO_LIMIT, out_mem=HOST):
    out = C.POINTER(N.cph_ordered)()
    rc = ctx.lib.cph_order_rows(ctx.handle, keys, nkeys, n, skip, limit, out_mem, C.byref(out))
    return rc, out


def test_conversion_errors_are_data(ctx):
    n = 1000
    rng = np.random.default_rng(16)
    a, b, c = rng.integers(0, 9, n, dtype=np.int64), rng.random(n), rng.integers(0, 9, n, dtype=np.int64)
    sa, sb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    sa[700] = N.CPH_NUM_ERR_RANGE
    sb[700], sb[40] = N.CPH_NUM_ERR_SYNTAX, N.CPH_NUM_ERR_SYNTAX
    keys = (N.cph_order_key * 3)()
    for k, (vals, st, kind) in enumerate(((c, None, N.CPH_NUM_INT64), (a, sa, N.CPH_NUM_INT64), (b, sb, N.CPH_NUM_FLOAT64))):
        keys[k].kind, keys[k].values, keys[k].values_mem = kind, vals.ctypes.data, HOST
        keys[k].status = st.ctypes.data if st is not None else None
    rc, out = raw_order(ctx, keys, 3, n)
    assert rc == N.CPH_OK
    r = out.contents
    assert (int(r.nerrors), int(r.first_error_row), int(r.first_error_key), int(r.first_error_kind)) == (3, 40, 2, N.CPH_NUM_ERR_SYNTAX)
    assert int(r.nrows) == 0 and not r.ids
    ctx.lib.cph_ordered_release(out)
    sa[40] = N.CPH_NUM_ERR_RANGE          # now two keys fail at row 40: the lowest key is reported
    rc, out = raw_order(ctx, keys, 3, n, 0, 10)
    r = out.contents
    assert rc == N.CPH_OK and (int(r.nerrors), int(r.first_error_row), int(r.first_error_key), int(r.first_error_kind)) == (4, 40, 1, N.CPH_NUM_ERR_RANGE)
    ctx.lib.cph_ordered_release(out)
    # through the Python layer: a NumCol with failed rows
    vals = [str(int(x)) for x in a]
    vals[700], vals[40] = "99999999999999999999", "4o"
    nc = MZ.to_int(ctx, StrCol.from_values(vals), out_mem=DEVICE)
    assert nc.nerrors == 2
    with pytest.raises(O.OrderError, match=r"key 1: the value of row 40 does not convert: invalid syntax \(2 such values\)") as ei:
        MZ.order_rows(ctx, [O.Asc(c), O.Desc(nc)], n)
    assert (ei.value.row, ei.value.key, ei.value.kind, ei.value.nerrors) == (40, 1, N.CPH_NUM_ERR_SYNTAX, 2)
    nc.release()
    # status bytes that are all OK change nothing
    sa[:] = 0
    sb[:] = 0
    rc, out = raw_order(ctx, keys, 3, n)
    assert rc == N.CPH_OK and int(out.contents.nerrors) == 0 and int(out.contents.first_error_row) == N.CPH_NO_ROW
    got = N._ptr_array(out.contents.ids, n, np.uint32).tolist()
    ctx.lib.cph_ordered_release(out)
    assert got == O.order_model([O.Asc(c.tolist(), "int"), O.Asc(a.tolist(), "int"), O.Asc(b.tolist(), "float")])


def test_invalid_calls(ctx):
    n = 100
    v = np.arange(n, dtype=np.int64)
    ix = N.DeviceIndex(ctx, [StrCol.from_values([b"k%d" % (i % 7) for i in range(n)])])
    other = N.DeviceIndex(ctx, [StrCol.from_values([b"a", b"b", b"c"])])

    def key(kind=N.CPH_NUM_INT64, values=v.ctypes.data, mem=HOST, index=None):
        ks = (N.cph_order_key * 1)()
        ks[0].kind, ks[0].values, ks[0].values_mem, ks[0].index = kind, values, mem, index
        return ks

    def expect(keys, nkeys, text, rows=n, out_mem=HOST, out=True):
        o = C.POINTER(N.cph_ordered)()
        rc = ctx.lib.cph_order_rows(ctx.handle, keys, nkeys, rows, 0, N.CPH_NO_LIMIT, out_mem, C.byref(o) if out else None)
        assert rc == N.CPH_ERR_INVALID and not o
        if text:
            assert text in ctx.last_error(), ctx.last_error()

    try:
        expect(key(), 1, None, out=False)                                   # NULL out
        assert ctx.lib.cph_order_rows(None, key(), 1, n, 0, N.CPH_NO_LIMIT, HOST, C.byref(C.POINTER(N.cph_ordered)())) == N.CPH_ERR_INVALID
        expect(None, 1, "keys is NULL")
        expect(key(), 0, "nkeys must be 1..CPH_ORDER_MAX_KEYS")
        expect((N.cph_order_key * 9)(), 9, "nkeys must be 1..CPH_ORDER_MAX_KEYS")
        expect(key(kind=7), 1, "kind must be CPH_NUM_INT64, CPH_NUM_FLOAT64 or CPH_ORDER_BYTES")
        expect(key(mem=5), 1, "bad values_mem")
        expect(key(), 1, "bad out_mem", out_mem=9)
        expect(key(values=None), 1, "a number key needs values")
        expect(key(kind=N.CPH_ORDER_BYTES, values=None), 1, "needs an index")
        expect(key(kind=N.CPH_ORDER_BYTES, values=None, index=other.handle), 1, "another row count")
        expect(key(kind=N.CPH_ORDER_BYTES, values=None, index=ix.handle), 1, "another row count", rows=n - 1)
        # ... and the calls next to them that are legal: no rows at all, 8 keys, an index of exactly these rows
        o = C.POINTER(N.cph_ordered)()
        assert ctx.lib.cph_order_rows(ctx.handle, key(values=None), 1, 0, 0, N.CPH_NO_LIMIT, HOST, C.byref(o)) == N.CPH_OK
        assert int(o.contents.nrows) == 0 and not o.contents.ids and int(o.contents.first_error_row) == N.CPH_NO_ROW
        ctx.lib.cph_ordered_release(o)
        assert run(ctx, [O.Asc(v)] * 8, n)[0] == list(range(n))
        assert run(ctx, [O.Desc(ix)], n)[0] == O.order_model([O.Desc([b"k%d" % (i % 7) for i in range(n)], "bytes")])
        with pytest.raises(TypeError):
            MZ.order_rows(ctx, [v], n)
        with pytest.raises(ValueError):
            MZ.order_rows(ctx, [O.Asc(v)], n + 1)
    finally:
        ix.close()
        other.close()


# ---- consumers -------------------------------------------------------------------------------------------------------------------
def csv_of(header, rows):
    return "".join(",".join(r) + "\n" for r in [header] + rows).encode()


def test_csv_write_through_an_ordered_list(ctx):
    n = 300
    t = orders_table(seed=3, n=n)
    qty = np.array([int(x) for x in t["qty"]], dtype=np.int64)
    cust = np.array([int(x) for x in t["cust_id"]], dtype=np.int64)
    want = O.order_model([O.Desc(qty.tolist(), "int"), O.Asc(cust.tolist(), "int")], 0, 50)
    names = ["order_id", "cust_id", "qty"]
    rows = [[t[c][i] for c in names] for i in want]
    host_cols = [StrCol.from_values(t[c]) for c in names]
    r = MZ.order_rows(ctx, [O.Desc(qty), O.Asc(cust)], n, limit=50)
    assert MZ.csv_write(ctx, host_cols, names, row_ids=[r.to_numpy()] * 3) == csv_of(names, rows)
    r.release()
    dev_cols = [c.to_device() for c in host_cols]
    r = MZ.order_rows(ctx, [O.Desc(qty), O.Asc(cust)], n, limit=50, out_mem=DEVICE)
    assert MZ.csv_write(ctx, dev_cols, names, row_ids=[r.as_row_ids()] * 3) == csv_of(names, rows)
    nc = MZ.to_int(ctx, dev_cols[2], row_ids=r.as_row_ids())
    assert nc.values.tolist() == [int(t["qty"][i]) for i in want]
    taken = MZ.take_rows(ctx, (r.as_row_ids()[0], 32, len(r)), np.arange(5, dtype=np.uint32))
    assert taken.tolist() == want[:5]
    r.release()


def orders_csv(n, seed=21):
    t = orders_table(seed=seed, n=n)
    names = ["order_id", "cust_id", "prod_id", "qty"]
    return t, csv_of(names, [[t[c][i] for c in names] for i in range(n)])


def test_totals_to_csv_ordered(ctx):
    n = 2000
    t, text = orders_csv(n)
    table = PL.read_table(ctx, text)
    try:
        specs = [A.Sum("qty", "int"), A.Max("qty", "int")]
        names = ["orders", "total", "largest"]
        plain = PL.totals_to_csv(ctx, table, ["cust_id"], specs, names=names)
        assert PL.totals_to_csv(ctx, table, ["cust_id"], specs, names=names, order_by=None, limit=None) == plain   # byte-identical
        # the model: groups in key order (strings.Compare), their totals, then the order
        keys_sorted = sorted(set(t["cust_id"]), key=lambda s: s.encode())
        pos = sorted(range(n), key=lambda i: t["cust_id"][i].encode())
        m = A.totals_model([t["cust_id"][i] for i in pos], [[int(t["qty"][i]) for i in pos]] * 2, specs)
        assert plain == csv_of(["cust_id"] + names, [[k, str(c), str(s), str(x)] for k, c, s, x in zip(keys_sorted, m["count"], *m["values"])])
        for order_by, limit in (([O.Desc("total")], 10), ([O.Desc("largest"), O.Asc("orders")], 7), ([O.Desc("by")], None), ([O.Asc("orders"), O.Desc("by")], 200)):
            src = {"orders": m["count"], "total": m["values"][0], "largest": m["values"][1], "by": list(range(m["ngroups"]))}
            order = O.order_model([type(k)(src[k.source], "int") for k in order_by], 0, limit)
            want = csv_of(["cust_id"] + names, [[keys_sorted[g], str(m["count"][g]), str(m["values"][0][g]), str(m["values"][1][g])] for g in order])
            assert PL.totals_to_csv(ctx, table, ["cust_id"], specs, names=names, order_by=order_by, limit=limit) == want, order_by
        with pytest.raises(ValueError):
            PL.totals_to_csv(ctx, table, ["cust_id"], specs, names=names, order_by=[O.Desc("amount")])
    finally:
        table.release()


def test_filter_to_csv_ordered(ctx):
    from csvplus_amd import All, IntCmp, Like

    n = 2000
    t, text = orders_csv(n, seed=22)
    table = PL.read_table(ctx, text)
    try:
        out = ["order_id", "cust_id", "qty"]
        pred = IntCmp("qty", ">=", 50)
        plain = PL.filter_to_csv(ctx, table, pred, out, skip=3, limit=40)
        assert PL.filter_to_csv(ctx, table, pred, out, skip=3, limit=40, order_by=None) == plain                   # byte-identical
        kept = [i for i in range(n) if int(t["qty"][i]) >= 50]
        assert plain == csv_of(out, [[t[c][i] for c in out] for i in kept[3:43]])
        cases = [([O.Desc("qty", "int"), O.Asc("cust_id", "bytes")], 0, 10),
                 ([O.Asc("cust_id", "int"), O.Desc("qty", "float")], 5, 25),
                 ([O.Desc("cust_id", "bytes")], 0, None)]
        for order_by, skip, limit in cases:
            conv = {"int": int, "float": float, "bytes": lambda s: s.encode()}
            mk = [type(k)([conv[k.kind_name](t[k.source][i]) for i in kept], k.kind_name) for k in order_by]
            order = O.order_model(mk, skip, limit)
            want = csv_of(out, [[t[c][kept[p]] for c in out] for p in order])
            assert PL.filter_to_csv(ctx, table, pred, out, skip=skip, limit=limit, order_by=order_by) == want, order_by
        # nothing kept; a key column that does not convert
        assert PL.filter_to_csv(ctx, table, Like({"qty": "none"}), out, order_by=[O.Asc("qty", "int")]) == csv_of(out, [])
    finally:
        table.release()
    bad = csv_of(["id", "v"], [["a", "1"], ["b", "x"], ["c", "3"]])
    table = PL.read_table(ctx, bad)
    try:
        with pytest.raises(O.OrderError, match="row 1"):
            PL.filter_to_csv(ctx, table, All(), ["id"], order_by=[O.Asc("v", "int")])
    finally:
        table.release()
