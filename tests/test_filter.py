"""Filter / TakeWhile / DropWhile / Top / Drop with the named predicates (csvplus.go:276-374, :1243-1293) on the device:
csvplus_amd.predicates (compile / matches, CPU), cph_filter_rows / cph_rowsel_take through materialize.filter_rows /
take_rows, and the consumers of their row lists (csv_write, json_write, cph_join_probe, pipeline.join_to_csv)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.predicates import All, Any, Like, Not
from helpers import PEOPLE_NAMES, PEOPLE_SURNAMES, people_table

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE


# ---- a model of the row-list semantics, independent of the package's own (predicates.select_rows) --------------------
def model_rows(rows, pred, mode="where", first_row=0, nrows=None, skip=0, limit=None):
    """rows: list of dicts.  src.Drop(first_row).Top(nrows) -> Filter / TakeWhile / DropWhile -> Drop(skip).Top(limit);
    the answer is the list of row numbers (positions in `rows`)."""
    n = len(rows) - first_row if nrows is None else nrows
    out, dropping = [], True
    for i in range(first_row, first_row + n):
        ok = P.matches(pred, rows[i])
        if mode == "where":
            if ok:
                out.append(i)
        elif mode == "take_while":
            if not ok:
                break
            out.append(i)
        else:
            dropping = dropping and ok
            if not dropping:
                out.append(i)
    out = out[skip:]
    return out if limit is None else out[:limit]


def rows_of(table):
    names = list(table)
    return [{k: table[k][i] for k in names} for i in range(len(table[names[0]]))]


# ---- CPU: the compiler, matches(), the model, the structs --------------------------------------------------------------
def test_compile_like_of_two_columns():
    names, ops = P.compile(Like({"a": "x", "b": b"y"}), ["b", "a", "c"])
    assert names == ["a", "b"]
    assert ops == [(P.LIKE, 0, b"x"), (P.LIKE, 1, b"y"), (P.ALL, 2, None)]
    assert P.compile(Like(a="x"), ["a"]) == (["a"], [(P.LIKE, 0, b"x")])


def test_compile_nested():
    pred = Any(All(Like(a="1"), Like(b="2")), Not(Like(a="3")))
    names, ops = P.compile(pred, ["a", "b"])
    assert names == ["a", "b"]
    assert ops == [(P.LIKE, 0, b"1"), (P.LIKE, 1, b"2"), (P.ALL, 2, None), (P.LIKE, 0, b"3"), (P.NOT, 0, None), (P.ANY, 2, None)]


def test_compile_empty_combinators_and_missing_column():
    assert P.compile(All(), ["a"]) == ([], [(P.ALL, 0, None)])
    assert P.compile(Any(), ["a"]) == ([], [(P.ANY, 0, None)])
    names, ops = P.compile(Like({"nope": "x", "a": ""}), ["a"])
    assert names == ["a"] and ops == [(P.LIKE, -1, b"x"), (P.LIKE, 0, b""), (P.ALL, 2, None)]


def test_like_of_nothing_raises_and_closures_are_refused():
    with pytest.raises(ValueError):
        Like({})
    with pytest.raises(TypeError):
        All(lambda row: True)
    with pytest.raises(TypeError):
        Not("x")


def test_compile_limits():
    with pytest.raises(ValueError):
        P.compile(All(*[Like(a=str(i)) for i in range(33)]), ["a"])      # 33 LIKE terms
    with pytest.raises(ValueError):
        P.compile(All(*[Not(Like(a="1")) for _ in range(32)]), ["a"])    # 65 ops
    P.compile(Any(*[Like(a=str(i)) for i in range(32)]), ["a"])          # 32 terms, 33 ops, stack 32: fits


def test_matches_known_answers_on_the_people_fixture():
    rows = rows_of(people_table())
    jack_or_amelia = Any(Like(name="Jack"), Like(name="Amelia"))
    assert sum(P.matches(jack_or_amelia, r) for r in rows) == 2 * len(PEOPLE_SURNAMES)      # csvplus_test.go:147
    assert sum(P.matches(Like(surname="Smith"), r) for r in rows) == len(PEOPLE_NAMES)
    assert sum(P.matches(Like(name="Amelia", surname="Smith"), r) for r in rows) == 1
    assert sum(P.matches(Not(Like(name="Amelia")), r) for r in rows) == len(rows) - len(PEOPLE_SURNAMES)
    assert sum(P.matches(All(), r) for r in rows) == len(rows) and not any(P.matches(Any(), r) for r in rows)
    assert not any(P.matches(Like(born="1980"), r) for r in rows)            # no such column: false (:1286)
    assert all(P.matches(Not(Like(born="1980")), r) for r in rows)
    assert jack_or_amelia(rows[0]) and not jack_or_amelia(rows[len(PEOPLE_SURNAMES)])       # callable on a row


def test_compiled_program_agrees_with_matches():
    rows = rows_of(people_table())
    for pred in (Any(Like(name="Jack"), Like(name="Amelia")), All(Like(name="Ava"), Not(Like(surname="Smith"))),
                 Any(All(), Like(zzz="1")), Not(Any()), Like(name="Isla", surname="Lewis", nope="x")):
        names, ops = P.compile(pred, ["id", "name", "surname"])
        for r in rows:
            assert P.run_ops(ops, [r[k] for k in names]) == P.matches(pred, r)


def test_row_list_model_on_hand_made_inputs():
    rows = [{"k": v} for v in "aabacbaa"]
    a = Like(k="a")
    assert model_rows(rows, a) == [0, 1, 3, 6, 7]
    assert model_rows(rows, a, "take_while") == [0, 1]
    assert model_rows(rows, a, "drop_while") == [2, 3, 4, 5, 6, 7]
    assert model_rows(rows, a, first_row=2) == [3, 6, 7]
    assert model_rows(rows, a, first_row=2, nrows=4) == [3]
    assert model_rows(rows, a, "take_while", first_row=2) == []            # fails at its first row
    assert model_rows(rows, a, "drop_while", first_row=2) == [2, 3, 4, 5, 6, 7]
    assert model_rows(rows, a, "drop_while", first_row=6) == []            # never fails: everything dropped
    assert model_rows(rows, a, "take_while", first_row=6) == [6, 7]
    assert model_rows(rows, a, skip=1, limit=2) == [1, 3]
    assert model_rows(rows, a, limit=0) == [] and model_rows(rows, a, skip=5) == [] and model_rows(rows, a, skip=99) == []
    assert model_rows(rows, Like(k="z")) == [] and model_rows(rows, Like(k="z"), "take_while") == []
    assert model_rows(rows, Like(k="z"), "drop_while") == list(range(8))
    assert model_rows(rows, All()) == list(range(8)) and model_rows(rows, All(), "take_while", skip=3, limit=2) == [3, 4]
    assert model_rows(rows, All(), "drop_while") == [] and model_rows(rows, Any(), "drop_while", skip=7) == [7]
    assert model_rows([], a) == [] and model_rows(rows, a, first_row=8) == []
    # the package's own restatement of the same semantics agrees on every one of these
    for mode in ("where", "take_while", "drop_while"):
        for pred in (a, Like(k="z"), All(), Not(a)):
            for first, nr, skip, limit in ((0, None, 0, None), (2, 4, 0, None), (1, None, 1, 2), (0, None, 9, None), (3, 0, 0, 0)):
                flags = [P.matches(pred, r) for r in rows]
                assert P.select_rows(flags, mode, first, nr, skip, limit) == model_rows(rows, pred, mode, first, nr, skip, limit)


def test_filter_struct_sizes_against_the_compiled_header(tmp_path):
    names = ["cph_pred_op", "cph_filter_opts", "cph_rowlist"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "csvplus_hip.h"\nint main(void){'
                   + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
                   + 'printf("ops %d %d %d\\n", CPH_PRED_MAX_OPS, CPH_PRED_MAX_LIKE, CPH_PRED_MAX_STACK);'
                   + 'printf("enums %d %d %d %d %d %d %d\\n", CPH_PRED_LIKE, CPH_PRED_NOT, CPH_PRED_ALL, CPH_PRED_ANY,'
                   + " CPH_FILTER_WHERE, CPH_FILTER_TAKE_WHILE, CPH_FILTER_DROP_WHILE);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert C.sizeof(getattr(N, n)) == int(out[n]), (n, C.sizeof(getattr(N, n)), out[n])
    assert out["ops"].split() == [str(v) for v in (N.CPH_PRED_MAX_OPS, N.CPH_PRED_MAX_LIKE, N.CPH_PRED_MAX_STACK)]
    assert (P.MAX_OPS, P.MAX_LIKE, P.MAX_STACK) == (N.CPH_PRED_MAX_OPS, N.CPH_PRED_MAX_LIKE, N.CPH_PRED_MAX_STACK)
    assert out["enums"].split() == [str(v) for v in (N.CPH_PRED_LIKE, N.CPH_PRED_NOT, N.CPH_PRED_ALL, N.CPH_PRED_ANY,
                                                     N.CPH_FILTER_WHERE, N.CPH_FILTER_TAKE_WHILE, N.CPH_FILTER_DROP_WHILE)]
    assert (P.LIKE, P.NOT, P.ALL, P.ANY) == (N.CPH_PRED_LIKE, N.CPH_PRED_NOT, N.CPH_PRED_ALL, N.CPH_PRED_ANY)


def test_filter_symbols_declared_exported_and_bound():
    lib = C.CDLL(str(N.LIB_PATH))
    bound = {p[0] for p in N.PROTOTYPES}
    for name in ("cph_filter_rows", "cph_rowlist_release", "cph_rowsel_take"):
        assert hasattr(lib, name) and name in bound


# ---- the seeded case generator (restated from the sketch that accompanied the feature request) -----------------------------
ALPHA = np.array([0x00, 0x61, 0x62, 0x2C, 0x80, 0xFF], dtype=np.uint8)
SMALL_SIZES = (0, 1, 63, 64, 65, 1000)
BIG_SIZES = (3_000_001, 3_250_000)
SEED = 20261016


class Case:
    pass


def to_pred(tree):
    if tree[0] == "like":
        keys = [f"c{c}" if c >= 0 else "absent" for c, _ in tree[1]]
        if len(set(keys)) == len(keys):
            return Like({k: v for k, (_, v) in zip(keys, tree[1])})
        return All(*[Like({k: v}) for k, (_, v) in zip(keys, tree[1])])   # a Row holds a name once: two terms on one column
    if tree[0] == "not":
        return Not(to_pred(tree[1]))
    return (All if tree[0] == "all" else Any)(*[to_pred(t) for t in tree[1]])


def gen_case(rng, n):
    """One case: 1..4 columns over pools of 2..5 strings (alphabet with 0x00, ',' and bytes >= 0x80; lengths 0..19, or a
    fixed width of 1..12), a predicate tree of depth 0..4, and how the call is made."""
    k = Case()
    k.n = n
    k.first_row = int(rng.integers(0, 70)) if rng.random() < 0.5 else 0
    k.total = k.first_row + n + (int(rng.integers(0, 5)) if rng.random() < 0.5 else 0)   # rows of the selection
    ncols = int(rng.integers(1, 5))
    k.device = bool(rng.random() < 0.7)
    k.cols = []
    for c in range(ncols):
        col = Case()
        pool_n = int(rng.integers(2, 6))
        col.fixed = int(rng.integers(1, 13)) if rng.random() < 0.4 else 0
        col.offset_bits = 32 if rng.random() < 0.5 else 64
        col.pool = [bytes(rng.choice(ALPHA, col.fixed if col.fixed else int(rng.integers(0, 20)))) for _ in range(pool_n)]
        if rng.random() < 0.35:   # read through row ids (what a Join hands over), some with a base
            col.src_rows = max(1, k.total // 2 + 3)
            col.base = int(rng.choice([0, 7, 1000]))
            col.id_bits = 32 if rng.random() < 0.5 else 64
            col.ids = rng.integers(0, col.src_rows, k.total).astype(np.uint32 if col.id_bits == 32 else np.uint64)
        else:
            col.src_rows, col.ids = k.total, None
        col.src = rng.integers(0, pool_n, col.src_rows).astype(np.int32)     # pool entry of every row of the column
        col.at = col.src if col.ids is None else col.src[col.ids.astype(np.int64)]   # ... of every row of the selection
        k.cols.append(col)

    def tree(d):
        r = rng.random()
        if d == 0 or r < 0.35:
            terms = []
            for _ in range(1 if rng.random() < 0.8 else 2):
                c = int(rng.integers(-1, ncols)) if rng.random() < 0.05 else int(rng.integers(0, ncols))
                if c >= 0 and rng.random() < 0.85:
                    v = k.cols[c].pool[int(rng.integers(0, len(k.cols[c].pool)))]
                else:
                    v = bytes(rng.choice(ALPHA, int(rng.integers(0, 6))))
                terms.append((c, v))
            return ("like", terms)
        if r < 0.5:
            return ("not", tree(d - 1))
        cnt = int(rng.integers(2, 4)) if rng.random() < 0.95 else 0
        return ("all" if r < 0.65 else "any", [tree(d - 1) for _ in range(cnt)])

    k.tree = tree(int(rng.integers(0, 5)))
    k.mode = "where" if rng.random() < 0.5 else ("take_while" if rng.random() < 0.5 else "drop_while")
    k.skip = int(rng.integers(0, max(2, n // 3))) if rng.random() < 0.4 else 0
    k.limit = int(rng.integers(0, max(2, n))) if rng.random() < 0.4 else None
    k.out_bits = 32 if rng.random() < 0.5 else 64
    k.out_mem = HOST if rng.random() < 0.5 else DEVICE
    return k


def model_flags(k):
    """The predicate on every row of the selection, in numpy (a Like term is a lookup of the row's pool entry)."""
    def ev(t):
        if t[0] == "like":
            f = np.ones(k.total, dtype=bool)
            for c, v in t[1]:
                if c < 0:
                    return np.zeros(k.total, dtype=bool)
                f &= np.array([p == v for p in k.cols[c].pool], dtype=bool)[k.cols[c].at]
            return f
        if t[0] == "not":
            return ~ev(t[1])
        fs = [ev(x) for x in t[1]]
        if t[0] == "all":
            return np.logical_and.reduce(fs) if fs else np.ones(k.total, dtype=bool)
        return np.logical_or.reduce(fs) if fs else np.zeros(k.total, dtype=bool)
    return ev(k.tree)


def model_result(k, flags):
    f = flags[k.first_row:k.first_row + k.n]
    if k.mode == "where":
        kept = np.flatnonzero(f)
    else:
        bad = np.flatnonzero(~f)
        stop = int(bad[0]) if len(bad) else k.n
        kept = np.arange(0, stop) if k.mode == "take_while" else np.arange(stop, k.n)
    kept = kept[k.skip:]
    if k.limit is not None:
        kept = kept[:k.limit]
    return (kept + k.first_row).astype(np.uint64)


def gen_cases(sizes, per_size, seed=SEED):
    rng = np.random.default_rng(seed)
    return [gen_case(rng, n) for n in sizes for _ in range(per_size)]


def mid_fraction(cases):
    """Of the WHERE cases with n >= 63: the share whose predicate keeps between 1 and n - 1 of the rows it looks at."""
    mid = tot = 0
    for k in cases:
        if k.mode == "where" and k.n >= 63:
            kept = int(model_flags(k)[k.first_row:k.first_row + k.n].sum())
            tot += 1
            mid += 0 < kept < k.n
    return mid, tot


def test_generator_cases_are_not_degenerate():
    """A condition on the generator alone (no GPU result involved): at least half of its WHERE cases with n >= 63 keep some
    rows but not all of them."""
    mid, tot = mid_fraction(gen_cases(SMALL_SIZES, 40))
    print(f"WHERE cases with n >= 63: {tot}, keeping 1..n-1 rows: {mid}")
    assert tot >= 20 and 2 * mid >= tot, (mid, tot)


def test_generator_model_agrees_with_the_dict_model():
    """The numpy model of the property test against the row-at-a-time model over dicts, on the small cases."""
    for k in gen_cases((0, 1, 63, 65), 6, seed=7):
        rows = [{f"c{c}": col.pool[col.at[i]] for c, col in enumerate(k.cols)} for i in range(k.total)]
        want = model_rows(rows, to_pred(k.tree), k.mode, k.first_row, k.n, k.skip, k.limit)
        assert model_result(k, model_flags(k)).tolist() == want


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def strcol_from_pool(pool, idx, offset_bits=32, fixed=0):
    """The column whose row i holds pool[idx[i]], built with numpy (millions of rows)."""
    lens = np.array([len(p) for p in pool], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    blob = np.frombuffer(b"".join(pool), dtype=np.uint8)
    rl = lens[idx]
    offs = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum(rl, out=offs[1:])
    total = int(offs[-1])
    if total:
        src = np.repeat(starts[idx] - offs[:-1].astype(np.int64), rl) + np.arange(total, dtype=np.int64)
        data = blob[src]
    else:
        data = np.empty(0, np.uint8)
    return StrCol(np.ascontiguousarray(data), offs.astype(np.uint32 if offset_bits == 32 else np.uint64), len(idx), offset_bits,
                  fixed_width=fixed if fixed and len(idx) else 0)


def device_ids(ids, keep):
    import torch
    t = torch.from_numpy(ids.view(np.uint8).copy()).to("cuda:0") if len(ids) else torch.empty(8, dtype=torch.uint8, device="cuda:0")
    keep.append(t)
    return t.data_ptr()


def _hip():
    """The HIP runtime this process already uses (torch loaded it): for reading a device row list back."""
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    return C.CDLL(path)


def device_list_to_numpy(rl):
    """A device RowList's numbers, copied back by the HIP runtime itself."""
    if rl.is_range:
        return rl.to_numpy().astype(np.uint64)
    out = np.empty(rl.nrows, dtype=np.uint32 if rl.bits == 32 else np.uint64)
    assert _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(rl.ids_ptr), C.c_size_t(out.nbytes), 2) == 0   # device to host
    return out.astype(np.uint64)


def run_case(ctx, k):
    from csvplus_amd.materialize import filter_rows
    keep, cols, ids = [], {}, {}
    for c, col in enumerate(k.cols):
        sc = strcol_from_pool(col.pool, col.src, col.offset_bits, col.fixed)
        cols[f"c{c}"] = sc.to_device() if k.device else sc
        if col.ids is not None:   # the ids as a Join hands them over: base added, living where the column lives
            with_base = col.ids + col.ids.dtype.type(col.base)
            ids[f"c{c}"] = (device_ids(with_base, keep), col.id_bits, k.total, col.base) if k.device else (with_base, col.base)
    rl = filter_rows(ctx, cols, to_pred(k.tree), row_ids=ids or None, nrows=k.n, mode=k.mode, first_row=k.first_row, skip=k.skip,
                     limit=k.limit, out_bits=k.out_bits, out_mem=k.out_mem, as_handle=True)
    try:
        assert rl.bits == k.out_bits and rl.mem == k.out_mem
        if k.mode != "where":
            assert rl.is_range
        got = device_list_to_numpy(rl) if k.out_mem == DEVICE else rl.to_numpy().astype(np.uint64)
    finally:
        rl.release()
    del keep
    return got


@pytest.mark.gpu
def test_property_against_the_model(ctx):
    """Random tables, predicate trees, row ids, modes, first_row / skip / limit, widths and memories; every generated case
    is compared with the numpy model."""
    cases = gen_cases(SMALL_SIZES, 40) + gen_cases(BIG_SIZES, 2, seed=SEED + 1)
    mid, tot = mid_fraction(cases)
    print(f"{len(cases)} cases; WHERE with n >= 63: {tot}, of which keep 1..n-1 rows: {mid}")
    assert 2 * mid >= tot, (mid, tot)
    for i, k in enumerate(cases):
        want = model_result(k, model_flags(k))
        got = run_case(ctx, k)
        assert len(got) == len(want) and np.array_equal(got, want), (i, k.n, k.mode, k.tree, k.first_row, k.skip, k.limit)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3_000_001])
def test_many_tiles_where_and_while(ctx, n):
    """More tiles than the grid and more than one scan block: an 8-byte fixed-width id column and a variable-length one."""
    from csvplus_amd.materialize import filter_rows
    rng = np.random.default_rng(5)
    idp = [b"%08d" % i for i in range(5)]
    vp = [b"", b"a", b"abcdefghij", b"abcdefghiJ", b"\x00\xff,"]
    a, b = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32)
    cols = {"id": strcol_from_pool(idp, a, fixed=8).to_device(), "v": strcol_from_pool(vp, b, 64).to_device()}
    pred = Any(All(Like(id=idp[1]), Not(Like(v=b""))), Like(v=b"abcdefghiJ"))
    flags = ((a == 1) & (b != 0)) | (b == 3)
    got = filter_rows(ctx, cols, pred)
    assert got.dtype == np.uint32 and np.array_equal(got, np.flatnonzero(flags))
    got = filter_rows(ctx, cols, pred, skip=1000, limit=100_000, out_bits=64, first_row=77)
    assert got.dtype == np.uint64 and np.array_equal(got, (np.flatnonzero(flags[77:]) + 77)[1000:101_000])
    a[:2_500_000] = 2
    cols["id"] = strcol_from_pool(idp, a, fixed=8).to_device()
    stop = 2_500_000 + int(np.flatnonzero(a[2_500_000:] != 2)[0])
    tw = filter_rows(ctx, cols, Like(id=idp[2]), mode="take_while", as_handle=True)
    assert tw.is_range and (tw.first, tw.nrows) == (0, stop)
    dw = filter_rows(ctx, cols, Like(id=idp[2]), mode="drop_while", skip=5, limit=7, as_handle=True)
    assert dw.is_range and (dw.first, dw.nrows) == (stop + 5, 7)


def people_cols(device, offset_bits=32):
    t = people_table()
    cols = {k: StrCol.from_values(v, offset_bits=offset_bits) for k, v in t.items()}
    return t, ({k: c.to_device() for k, c in cols.items()} if device else cols)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_reference_shaped_cases(ctx, device):
    from csvplus_amd.materialize import filter_rows
    t, cols = people_cols(device)
    rows = rows_of(t)
    S = len(PEOPLE_SURNAMES)
    got = filter_rows(ctx, cols, Any(Like(name="Jack"), Like(name="Amelia")))
    assert len(got) == 2 * S                                                  # csvplus_test.go:147
    assert got.tolist() == model_rows(rows, Any(Like(name="Jack"), Like(name="Amelia")))
    for pred in (Like(surname="Smith"), Like(name="Amelia", surname="Smith"), Not(Like(name="Amelia")), Like(id="77"),
                 All(Like(name="Ava"), Not(Like(surname="Smith"))), Like(name="Ameli"), Like(name="Amelia\x00"), Like(name="")):
        for mode in ("where", "take_while", "drop_while"):
            for kw in ({}, {"first_row": 5}, {"first_row": 3, "nrows": 40, "skip": 2, "limit": 9}, {"limit": 0}, {"skip": 500}):
                got = filter_rows(ctx, cols, pred, mode=mode, **kw)
                assert got.tolist() == model_rows(rows, pred, mode, **kw), (pred, mode, kw)
    # the tail of TestLongChain: Filter(Like(surname: Smith)).Top(10)
    assert filter_rows(ctx, cols, Like(surname="Smith"), limit=10).tolist() == [i * S for i in range(10)]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_empty_combinators_missing_columns_and_tiny_inputs(ctx, device):
    from csvplus_amd.materialize import filter_rows
    t, cols = people_cols(device, 64)
    n = len(t["id"])
    assert filter_rows(ctx, cols, All()).tolist() == list(range(n))
    assert filter_rows(ctx, cols, Any()).tolist() == []
    assert filter_rows(ctx, cols, Not(Any()), first_row=100).tolist() == list(range(100, n))
    assert filter_rows(ctx, cols, Like(born="1980")).tolist() == []           # :1286
    assert filter_rows(ctx, cols, Not(Like(born="1980")), limit=3).tolist() == [0, 1, 2]
    assert filter_rows(ctx, cols, Like(name="Amelia", born="1980")).tolist() == []
    assert filter_rows(ctx, cols, Any(Like(born="1"), Like(id="5"))).tolist() == [5]
    assert filter_rows(ctx, cols, All(), mode="take_while").tolist() == list(range(n))
    assert filter_rows(ctx, cols, All(), mode="drop_while").tolist() == []
    assert filter_rows(ctx, cols, Any(), mode="take_while").tolist() == []
    assert filter_rows(ctx, cols, Any(), mode="drop_while").tolist() == list(range(n))
    for vals in ([], [b"x"], [b""]):
        one = {"k": StrCol.from_values(vals)}
        if device:
            one = {"k": one["k"].to_device()}
        rows = [{"k": v} for v in vals]
        for pred in (Like(k="x"), Like(k=""), Not(Like(k="x")), All(), Any(), Like(q="x")):
            for mode in ("where", "take_while", "drop_while"):
                for bits in (32, 64):
                    got = filter_rows(ctx, one, pred, mode=mode, out_bits=bits)
                    assert got.dtype == (np.uint32 if bits == 32 else np.uint64)
                    assert got.tolist() == model_rows(rows, pred, mode), (vals, pred, mode)


@pytest.mark.gpu
def test_long_literals_and_fixed_width_columns(ctx):
    """Literals beyond the LDS block (read from device memory), a literal as long as a fixed width and one that is not."""
    from csvplus_amd.materialize import filter_rows
    big = [bytes([65 + i]) * 5000 + b"tail%d" % i for i in range(3)]
    idx = np.array([0, 1, 2, 1, 0, 2, 2, 1] * 40, dtype=np.int32)
    col = strcol_from_pool(big, idx, 64).to_device()
    assert filter_rows(ctx, {"b": col}, Like(b=big[1])).tolist() == np.flatnonzero(idx == 1).tolist()
    assert filter_rows(ctx, {"b": col}, Any(Like(b=big[0]), Like(b=big[2][:-1]))).tolist() == np.flatnonzero(idx == 0).tolist()
    for w in (1, 3, 7, 8, 9, 12, 16):
        pool = [bytes([97 + j]) * w for j in range(3)] + [b"a" * (w - 1) + b"\x00"]
        ix = np.arange(500, dtype=np.int32) % 4
        for dev in (True, False):
            c = strcol_from_pool(pool, ix, fixed=w)
            assert c.fixed_width == w
            c = c.to_device() if dev else c
            assert filter_rows(ctx, {"f": c}, Like(f=pool[3])).tolist() == np.flatnonzero(ix == 3).tolist()
            assert filter_rows(ctx, {"f": c}, Like(f=pool[0] + b"a")).tolist() == []
            assert filter_rows(ctx, {"f": c}, Not(Like(f=pool[0][:-1])), limit=4).tolist() == [0, 1, 2, 3]


def host_filtered(table, names, keep_rows):
    return [StrCol.from_values([table[k][i] for i in keep_rows]) for k in names]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_writers_consume_the_row_lists(ctx, device):
    from csvplus_amd.materialize import csv_write, filter_rows, json_write, take_rows
    t, cols = people_cols(device)
    rows = rows_of(t)
    names = ["id", "name", "surname"]
    pred = Any(Like(name="Jack"), All(Like(surname="Evans"), Not(Like(name="Ava"))))
    want_rows = model_rows(rows, pred)
    want_csv = csv_write(ctx, host_filtered(t, names, want_rows), names)
    want_json = json_write(ctx, host_filtered(t, names, want_rows), names)
    assert want_csv.count(b"\n") == len(want_rows) + 1
    rl = filter_rows(ctx, cols, pred, out_mem=DEVICE if device else HOST, as_handle=True)
    ids = rl.as_row_ids() if device else rl.to_numpy()
    assert csv_write(ctx, [cols[k] for k in names], names, row_ids=[ids] * 3, nrows=len(rl)) == want_csv
    assert json_write(ctx, [cols[k] for k in names], names, row_ids=[ids] * 3, nrows=len(rl)) == want_json
    # joined rows: every column read through its own row ids (one of them with a base); the filter looks through them
    # and take_rows narrows them to the rows it kept
    rng = np.random.default_rng(3)
    m = 1000
    sel_a = rng.integers(0, len(rows), m).astype(np.uint32)
    sel_b = rng.integers(0, len(rows), m).astype(np.uint64)
    base = 1000
    joined = [{"id": t["id"][a], "name": t["name"][a], "surname": t["surname"][b]} for a, b in zip(sel_a, sel_b)]
    want_rows = model_rows(joined, pred, skip=3, limit=200)
    jt = {k: [r[k] for r in joined] for k in names}
    want_csv = csv_write(ctx, host_filtered(jt, names, want_rows), names)
    keep = []
    if device:
        ia = (device_ids(sel_a, keep), 32, m)
        ib = (device_ids(sel_b + np.uint64(base), keep), 64, m, base)
    else:
        ia, ib = sel_a, (sel_b + np.uint64(base), base)
    by_col = {"id": ia, "name": ia, "surname": ib}
    mem = DEVICE if device else HOST
    kept = filter_rows(ctx, cols, pred, row_ids=by_col, nrows=m, skip=3, limit=200, out_mem=mem, as_handle=True)
    got_rows = device_list_to_numpy(kept) if device else kept.to_numpy()
    assert got_rows.tolist() == want_rows
    na = take_rows(ctx, ia, kept, out_mem=mem, as_handle=True)
    nb = take_rows(ctx, ib, kept, out_mem=mem, as_handle=True)
    assert (na.bits, nb.bits) == (32, 64)
    if device:
        assert device_list_to_numpy(na).tolist() == sel_a[want_rows].tolist()
        assert device_list_to_numpy(nb).tolist() == sel_b[want_rows].tolist()       # the base is taken off
        a2, b2 = na.as_row_ids(), nb.as_row_ids()
    else:
        a2, b2 = na.to_numpy(), nb.to_numpy()
        assert a2.tolist() == sel_a[want_rows].tolist() and b2.tolist() == sel_b[want_rows].tolist()   # the base is taken off
    assert csv_write(ctx, [cols[k] for k in names], names, row_ids=[a2, a2, b2], nrows=len(kept)) == want_csv
    # identity row ids: a copy of the list; a range stays a range; lists given as numpy arrays
    cp = take_rows(ctx, None, kept, out_mem=HOST)
    assert cp.tolist() == want_rows
    rg = filter_rows(ctx, cols, All(), mode="take_while", first_row=7, nrows=20, as_handle=True)
    assert take_rows(ctx, None, rg).tolist() == list(range(7, 27))
    assert take_rows(ctx, sel_a, rg).tolist() == sel_a[7:27].tolist()
    assert take_rows(ctx, sel_b, np.array([5, 0, 999], dtype=np.uint64)).tolist() == sel_b[[5, 0, 999]].tolist()
    assert take_rows(ctx, sel_a, np.empty(0, np.uint32)).tolist() == []
    for h in (rl, kept, na, nb, rg):
        h.release()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_join_probe_over_the_filtered_rows(ctx, device):
    """cph_join_probe with row_sel = the filter's list equals the probe of the host-filtered columns."""
    from csvplus_amd import DeviceIndex
    from csvplus_amd.materialize import filter_rows
    from helpers import orders_table
    t = people_table()
    o = orders_table(n=5000)
    ix = DeviceIndex(ctx, [StrCol.from_values(t["id"])], unique=True)
    ocols = {k: StrCol.from_values(v) for k, v in o.items()}
    if device:
        ocols = {k: c.to_device() for k, c in ocols.items()}
    pred = Any(Like(prod_id="3"), Like(qty="17"))
    want_rows = model_rows(rows_of(o), pred)
    assert 0 < len(want_rows) < 5000
    rl = filter_rows(ctx, ocols, pred, out_mem=DEVICE if device else HOST, as_handle=True)
    got = ix.probe([ocols["cust_id"]], row_sel=rl.as_row_ids() if device else rl.to_numpy())
    want = ix.probe([StrCol.from_values([o["cust_id"][i] for i in want_rows])])
    assert got.nmatches == want.nmatches == len(want_rows)
    np.testing.assert_array_equal(got.cnt, want.cnt)
    np.testing.assert_array_equal(got.build_row, want.build_row)
    np.testing.assert_array_equal(got.probe_idx, want.probe_idx)
    for h in (got, want, rl):
        h.release()
    ix.close()


def _csv_text(names, cols):
    return ",".join(names).encode() + b"\n" + b"".join(b",".join(c[i] for c in cols) + b"\n" for i in range(len(cols[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("positions", [True, False])
def test_join_to_csv_where_limit(ctx, positions):
    """join_to_csv(where=..., limit=10) equals the unfiltered pipeline's text filtered line by line on the host; the same
    for JSON; filter_to_csv for one table."""
    import json

    from csvplus_amd import pipeline
    from helpers import orders_table, stock_table
    enc = lambda tab: {k: [v.encode() for v in vs] for k, vs in tab.items()}   # noqa: E731
    cv, pv, ov = enc(people_table()), enc(stock_table()), enc(orders_table(n=4000))
    ov["cust_id"][5] = b"99999"   # an order without a customer
    tc = pipeline.read_table(ctx, _csv_text(list(cv), list(cv.values())))
    tp = pipeline.read_table(ctx, _csv_text(list(pv), list(pv.values())))
    to = pipeline.read_table(ctx, _csv_text(list(ov), list(ov.values())))
    steps = [(tc, "id", "cust_id"), (tp, "prod_id", "prod_id")]
    outc = [("order_id", to, "order_id"), ("name", tc, "name"), ("surname", tc, "surname"), ("product", tp, "product"), ("qty", to, "qty")]
    try:
        full = pipeline.join_to_csv(ctx, to, steps, outc, positions=positions)
        lines = full.split(b"\n")
        head, body = lines[0], [ln for ln in lines[1:] if ln]
        assert len(body) == 3999

        def expect(keep, skip=0, limit=None):
            kept = [ln for ln in body if keep(ln.split(b","))][skip:]
            return b"".join(ln + b"\n" for ln in [head] + (kept if limit is None else kept[:limit]))

        smith = expect(lambda f: f[2] == b"Smith", limit=10)
        assert smith.count(b"\n") == 11
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, where=Like(surname="Smith"), limit=10) == smith
        # a predicate over columns that are not written, from all three tables; Drop and Top
        pred = All(Like(price="0.03"), Any(Like(name="Ava"), Like(qty="7")), Not(Like(cust_id="3")))
        orow = {r[0]: r for r in zip(ov["order_id"], ov["cust_id"], ov["prod_id"], ov["qty"])}
        keep = lambda f: orow[f[0]][2] == b"2" and (f[1] == b"Ava" or f[4] == b"7") and orow[f[0]][1] != b"3"   # noqa: E731
        want = expect(keep, skip=2, limit=50)
        assert 3 < want.count(b"\n") <= 51
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, where=pred, skip=2, limit=50) == want
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, skip=3990) == expect(lambda f: True, skip=3990)
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, where=Like(surname="Nobody")) == head + b"\n"
        assert pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, where=Like(nope="1")) == head + b"\n"
        dev = pipeline.join_to_csv(ctx, to, steps, outc, positions=positions, where=Like(surname="Smith"), limit=10, out_mem=DEVICE)
        assert len(dev) == len(smith)
        dev.release()
        js = pipeline.join_to_json(ctx, to, steps, outc, positions=positions, where=Like(surname="Smith"), limit=10)
        assert [[d[k].encode() for k in ("order_id", "name", "surname", "product", "qty")] for d in json.loads(js)] == \
            [ln.split(b",") for ln in smith.split(b"\n")[1:-1]]
        # one table: FromFile(people).Filter(Like(name: Amelia)).ToCsv — the reference's headline example
        am = pipeline.filter_to_csv(ctx, tc, Like(name="Amelia"), ["id", ("last", "surname")])
        assert am == b"id,last\n" + b"".join(b"%d,%s\n" % (i, s.encode()) for i, s in enumerate(PEOPLE_SURNAMES))
        dw = pipeline.filter_to_csv(ctx, tc, Like(name="Amelia"), ["id"], mode="drop_while", limit=3)
        assert dw == b"id\n12\n13\n14\n"
        tw = pipeline.filter_to_csv(ctx, tc, Like(name="Amelia"), ["id"], mode="take_while", skip=10)
        assert tw == b"id\n10\n11\n"
        assert pipeline.filter_to_csv(ctx, tc, Any(), ["id"]) == b"id\n"
    finally:
        for t in (tc, tp, to):
            t.release()


def _call(ctx, cols, ncols, n, ops, mode=0, out_bits=32, first_row=0, sel=None, out_mem=HOST, opts=True, prog=True):
    keep = []
    from csvplus_amd.materialize import _pred_program
    arr = _pred_program(ops, keep)
    o = N.cph_filter_opts(mode, out_bits, first_row, 0, N.CPH_NO_LIMIT)
    out = C.POINTER(N.cph_rowlist)()
    rc = ctx.lib.cph_filter_rows(ctx.handle, cols, sel, ncols, n, arr if prog else None, len(ops), C.byref(o) if opts else None,
                                 out_mem, C.byref(out))
    assert not out or rc == N.CPH_OK
    if out:
        ctx.lib.cph_rowlist_release(out)
    return rc, ctx.last_error()


@pytest.mark.gpu
def test_every_error_has_a_status_and_a_message(ctx):
    a = StrCol.from_values([b"1", b"22", b"1"])
    arr = (N.cph_strcol * 2)()
    arr[0], k0 = a.as_c()
    arr[1], k1 = a.as_c()
    L, NOT, ALL, ANY = P.LIKE, P.NOT, P.ALL, P.ANY
    ok = [(L, 0, b"1")]
    assert _call(ctx, arr, 1, 3, ok)[0] == N.CPH_OK
    bad = [
        ("NULL prog", dict(ops=ok, prog=False)), ("NULL opts", dict(ops=ok, opts=False)),
        ("op 0", dict(ops=[(0, 0, None)])), ("op 5", dict(ops=[(5, 0, None)])),
        ("column 1 of 1", dict(ops=[(L, 1, b"1")])), ("column -2", dict(ops=[(L, -2, b"1")])),
        ("NOT underflow", dict(ops=[(NOT, 0, None)])), ("ALL underflow", dict(ops=ok + [(ALL, 2, None)])),
        ("ANY negative", dict(ops=ok + [(ANY, -1, None)])),
        ("two values left", dict(ops=ok + ok)), ("nothing left", dict(ops=[])),
        ("65 ops", dict(ops=ok + [(NOT, 0, None)] * 64)),
        ("33 LIKE", dict(ops=[(L, 0, b"1")] * 33 + [(ALL, 33, None)])),
        ("stack 33", dict(ops=[(ALL, 0, None)] * 33 + [(ANY, 33, None)])),
        ("out_bits 16", dict(ops=ok, out_bits=16)), ("mode 3", dict(ops=ok, mode=3)), ("out_mem 2", dict(ops=ok, out_mem=2)),
        ("short identity column", dict(ops=ok, n=4)), ("short behind first_row", dict(ops=ok, n=2, first_row=2)),
        ("17 columns", dict(ops=ok, ncols=17)),
    ]
    for what, kw in bad:
        kw = dict(kw)
        rc, msg = _call(ctx, arr, kw.pop("ncols", 1), kw.pop("n", 3), kw.pop("ops"), **kw)
        assert rc == N.CPH_ERR_INVALID and msg, (what, rc, msg)
    # exactly at the limits: fine
    assert _call(ctx, arr, 1, 3, [(L, 0, b"1")] * 32 + [(ANY, 32, None)])[0] == N.CPH_OK
    assert _call(ctx, arr, 1, 3, ok + [(NOT, 0, None)] * 63)[0] == N.CPH_OK
    # a LIKE value with a length but no pointer
    prog = (N.cph_pred_op * 1)()
    prog[0].op, prog[0].arg, prog[0].value.len = L, 0, 3
    o = N.cph_filter_opts(0, 32, 0, 0, N.CPH_NO_LIMIT)
    out = C.POINTER(N.cph_rowlist)()
    assert ctx.lib.cph_filter_rows(ctx.handle, arr, None, 1, 3, prog, 1, C.byref(o), HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert "pointer" in ctx.last_error() and not out
    assert ctx.lib.cph_filter_rows(ctx.handle, None, None, 1, 3, prog, 1, C.byref(o), HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_filter_rows(ctx.handle, arr, None, 1, 3, prog, 1, C.byref(o), HOST, None) == N.CPH_ERR_INVALID
    # row-id bits
    sel = (N.cph_rowsel * 1)()
    ids = np.zeros(3, np.uint32)
    sel[0].ids, sel[0].bits = ids.ctypes.data, 16
    rc, msg = _call(ctx, arr, 1, 3, ok, sel=sel)
    assert rc == N.CPH_ERR_INVALID and "bits" in msg
    # 32-bit row numbers that would not fit
    sel[0].bits = 32
    rc, msg = _call(ctx, arr, 1, 3, ok, sel=sel, first_row=0xFFFFFFFF - 2)
    assert rc == N.CPH_ERR_TOO_MANY_ROWS and msg
    rc, msg = _call(ctx, arr, 1, 0, ok, first_row=0xFFFFFFFF - 2)   # no rows: legal wherever it starts
    assert rc == N.CPH_OK
    assert _call(ctx, arr, 1, 0, ok)[0] == N.CPH_OK
    # cph_rowsel_take
    lst = N.cph_rowlist(2, 0, None, 32, HOST)
    sel[0].bits = 16
    assert ctx.lib.cph_rowsel_take(ctx.handle, sel, HOST, C.byref(lst), HOST, C.byref(out)) == N.CPH_ERR_INVALID and ctx.last_error()
    sel[0].bits = 32
    assert ctx.lib.cph_rowsel_take(ctx.handle, sel, HOST, None, HOST, C.byref(out)) == N.CPH_ERR_INVALID and ctx.last_error()
    assert ctx.lib.cph_rowsel_take(ctx.handle, sel, 5, C.byref(lst), HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_rowsel_take(ctx.handle, sel, HOST, C.byref(lst), 5, C.byref(out)) == N.CPH_ERR_INVALID
    assert not out
    del k0, k1


@pytest.mark.gpu
def test_the_strings_are_read_once(ctx):
    """One WHERE call launches k_pred_eval exactly once (and k_pred_emit once); a WHILE call k_pred_eval alone."""
    from csvplus_amd.materialize import filter_rows
    t, cols = people_cols(True)
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        got = filter_rows(ctx, cols, Any(Like(name="Jack"), Like(surname="Smith"), Like(id="3")))
        st = ctx.profile_read(reset=True)
        assert len(got) == len(PEOPLE_SURNAMES) + len(PEOPLE_NAMES) - 1 + 1
        assert st["k_pred_eval"]["launches"] == 1 and st["k_pred_emit"]["launches"] == 1
        assert st["k_pred_eval"]["algo_bytes"] > 0 and st["k_pred_emit"]["algo_bytes"] > 0
        filter_rows(ctx, cols, Like(name="Amelia"), mode="take_while")
        st = ctx.profile_read(reset=True)
        assert st["k_pred_eval"]["launches"] == 1 and "k_pred_emit" not in st
    finally:
        ctx.profile(False)
