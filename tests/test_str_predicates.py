"""The string conditions on the device (cph_filter_rows ops 32..37 and 40..42 through materialize.filter_rows): StrCmp,
HasPrefix, HasSuffix, Contains.  The oracle is Python's bytes: comparison, startswith, endswith, `in`.  Results are equal,
not close.

Shapes: row counts at the wave and at the 2048-row tile of k_pred_eval; value and literal lengths around the 8-byte chunk
(0 1 7 8 9 15 16 17 24 25); values packed back to back, so they begin at every offset mod 8, and the column's last value
ends where its buffer ends; an alphabet of four symbols with 0x00 and 0x80.  Every value of the pool is a piece of ONE master
string (a head, a tail, a middle, or one of those with a byte changed), and the literals are pool values: ties, near
misses and matches are dense, and every (op, literal) of the matrix holds for some rows and fails for others."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.predicates import All, Any, Contains, FloatCmp, HasPrefix, HasSuffix, IntCmp, Like, Not, StrCmp

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
ROWS = (1, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 5)
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)
SYMS = (0x00, 0x61, 0x62, 0x80)


def _master():
    rng = np.random.default_rng(20261020)
    m = bytearray(int(s) for s in rng.choice(SYMS, 25))
    m[0] = 0x61   # neither the smallest nor the largest first byte
    return bytes(m)


MASTER = _master()


def _changed(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([SYMS[(SYMS.index(b[at]) + 1) % 4]]) + b[at + 1:]


def _pool():
    m = MASTER
    heads = [m[:n] for n in LENS]
    tails = [m[25 - n:] for n in LENS if 0 < n < 25]
    mids = [m[3:3 + n] for n in (1, 7, 8, 9, 15, 16, 17)]
    near = [_changed(m[:n], n - 1) for n in (1, 8, 9, 16, 17, 25)] + [_changed(m[25 - n:], 0) for n in (8, 9, 17)]
    ends = [b"\x80" * 25, b"\x00"]   # above and below every literal but themselves
    pool = []
    for v in heads + tails + mids + near + ends:
        if v not in pool:
            pool.append(v)
    return pool


POOL = _pool()
LITERALS = [v for v in POOL if v and v != b"\x80" * 25 and v != b"\x00"]   # every length of LENS but 0, from three places of the master
assert len(POOL) <= 63 and {len(v) for v in LITERALS} == set(LENS) - {0}

OPS = [("cmp", rel) for rel in P.RELS] + [("prefix", None), ("suffix", None), ("contains", None)]


def make_pred(op, column, literal):
    kind, rel = op
    return {"cmp": lambda: StrCmp(column, rel, literal), "prefix": lambda: HasPrefix(column, literal),
            "suffix": lambda: HasSuffix(column, literal), "contains": lambda: Contains(column, literal)}[kind]()


def oracle(op, value: bytes, literal: bytes) -> bool:
    kind, rel = op
    if kind == "prefix":
        return value.startswith(literal)
    if kind == "suffix":
        return value.endswith(literal)
    if kind == "contains":
        return literal in value
    return {"<": value < literal, "<=": value <= literal, "==": value == literal, "!=": value != literal, ">=": value >= literal,
            ">": value > literal}[rel]


def pool_flags(op, literal, pool=None):
    return np.array([oracle(op, v, literal) for v in (POOL if pool is None else pool)], dtype=bool)


def row_index(n, seed, pool_size=None):
    """Pool entry of every row: the first rows walk the whole pool in a shuffled order, the rest are random."""
    p = len(POOL) if pool_size is None else pool_size
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, p, n).astype(np.int64)
    walk = rng.permutation(p)
    idx[:min(n, p)] = walk[:min(n, p)]
    return idx


def packed_col(pool, idx, offset_bits=32, fixed=0):
    """Row i holds pool[idx[i]]; the values lie back to back and the data array ends with the last value."""
    vals = [pool[i] for i in idx]
    return StrCol.from_values(vals, offset_bits=offset_bits, fixed_width=fixed if fixed else 0)


def exact_device_col(col: StrCol) -> StrCol:
    """The column on the device in a buffer of exactly its bytes: the last value ends where the allocation's request ends."""
    import torch
    nb = col.data.nbytes
    d = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda:0")
    if nb:
        d[:nb].copy_(torch.from_numpy(np.ascontiguousarray(col.data)))
    o = None
    if not col.fixed_width:
        o = torch.from_numpy(np.ascontiguousarray(col.offsets).view(np.uint8).copy()).to("cuda:0")
    return StrCol(d, o, col.nrows, col.offset_bits, DEVICE, fixed_width=col.fixed_width)


def where(ctx, cols, pred, **kw):
    from csvplus_amd.materialize import filter_rows
    return filter_rows(ctx, cols, pred, **kw)


def check_where(ctx, cols, pred, flags, what, both=True, **kw):
    if both:
        assert flags.any() and not flags.all(), ("the expected bitmap lacks an outcome", what)
    got = where(ctx, cols, pred, **kw)
    assert np.array_equal(got, np.flatnonzero(flags)), what


# ---- the matrix: every op x every literal at the largest row count; every op at every row count and column kind -------------

@pytest.mark.gpu
def test_every_op_and_literal_length(ctx):
    """2 * 2048 + 5 rows of a device column with 32-bit offsets: all nine ops against every literal of the pool (lengths 1..25,
    heads, tails and middles of the master; the 9-byte and longer ones live in the literal block in LDS)."""
    n = ROWS[-1]
    idx = row_index(n, 1)
    cols = {"v": exact_device_col(packed_col(POOL, idx))}
    begins = np.asarray(packed_col(POOL, idx).offsets[:-1], dtype=np.int64) % 8
    assert set(begins.tolist()) == set(range(8))   # values begin at every offset mod 8
    for op in OPS:
        for lit in LITERALS:
            check_where(ctx, cols, make_pred(op, "v", lit), pool_flags(op, lit)[idx], (op, lit))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_row_counts_and_column_kinds(ctx, n):
    """Every row count at the wave and tile edges, over 32-bit offsets, 64-bit offsets and a fixed width of 8, host- and
    device-resident.  One row cannot show both outcomes: there every op runs on a row that holds and on one that fails."""
    fixed_pool = [MASTER[:8], MASTER[17:], MASTER[3:11], _changed(MASTER[:8], 7), _changed(MASTER[:8], 0), b"\x80" * 8, b"\x00" * 8]
    fixed_lits = {"cmp": [MASTER[:8], MASTER[3:11]], "prefix": [MASTER[:7], MASTER[:1], MASTER[:8]],
                  "suffix": [MASTER[1:8], MASTER[17:], MASTER[24:]], "contains": [MASTER[4:7], MASTER[:1], MASTER[18:24]]}
    k = 0
    for kind in ("o32", "o64", "fix8"):
        pool = fixed_pool if kind == "fix8" else POOL
        for device in (True, False):
            for op in OPS:
                lits = fixed_lits[op[0]] if kind == "fix8" else LITERALS   # 8-byte values: literals that can match them
                lit = lits[k % len(lits)]
                k += 1
                pf = pool_flags(op, lit, pool)
                assert pf.any() and not pf.all(), (kind, op, lit)
                if n == 1:
                    picks = [np.array([int(np.flatnonzero(pf)[0])]), np.array([int(np.flatnonzero(~pf)[0])])]
                else:
                    picks = [row_index(n, 100 + k, len(pool))]
                for idx in picks:
                    col = packed_col(pool, idx, 64 if kind == "o64" else 32, 8 if kind == "fix8" else 0)
                    assert col.fixed_width == (8 if kind == "fix8" else 0)
                    cols = {"v": exact_device_col(col) if device else col}
                    check_where(ctx, cols, make_pred(op, "v", lit), pf[idx], (kind, device, op, lit, n), both=n > 1)


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [0, 5, 2047, 2048, 2049, 4096, 4100, 2 * 2048 + 5])
def test_while_modes(ctx, stop):
    """TAKE_WHILE / DROP_WHILE at 2 * 2048 + 5 rows with the first failing row in the first tile, at a tile boundary and in
    the last, partial tile (and no failing row at all)."""
    from csvplus_amd.materialize import filter_rows
    n = ROWS[-1]
    rng = np.random.default_rng(stop)
    for op, lit in ((("cmp", ">="), MASTER[:9]), (("prefix", None), MASTER[:7]), (("suffix", None), MASTER[25 - 9:]), (("contains", None), MASTER[3:10])):
        pf = pool_flags(op, lit)
        good, bad = np.flatnonzero(pf), np.flatnonzero(~pf)
        assert len(good) and len(bad)
        idx = row_index(n, stop + 7)
        idx[:stop] = rng.choice(good, stop)
        if stop < n:
            idx[stop] = bad[0]
        cols = {"v": exact_device_col(packed_col(POOL, idx, 64))}
        pred = make_pred(op, "v", lit)
        tw = filter_rows(ctx, cols, pred, mode="take_while", as_handle=True)
        assert tw.is_range and (tw.first, tw.nrows) == (0, stop), (op, stop)
        dw = filter_rows(ctx, cols, pred, mode="drop_while", as_handle=True)
        assert dw.is_range and dw.nrows == n - stop and (dw.first == stop or stop == n), (op, stop)
        tw.release()
        dw.release()


# ---- semantic edges: their outcomes are known, not mixed -------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_semantic_edges(ctx, device):
    vals = [b"a", b"a\x00", b"", b"\x7f", b"\x80", b"10", b"9", b"abc", b"\xff" * 25, b"\x00"]
    col = StrCol.from_values(vals, fixed_width=0)
    cols = {"v": exact_device_col(col) if device else col}
    table = [(op, lit) for op in OPS for lit in (b"", b"a", b"a\x00", b"\x7f", b"\x80", b"9", b"10", b"abcd", b"\xff" * 26, b"\x00\x00")]
    for op, lit in table:
        want = [i for i, v in enumerate(vals) if oracle(op, v, lit)]
        assert where(ctx, cols, make_pred(op, "v", lit)).tolist() == want, (op, lit)
    # the header's examples, spelled out
    assert where(ctx, cols, StrCmp("v", "<", b"a\x00")).tolist() == [0, 2, 5, 6, 9]        # "a" < "a\0", and so is everything below "a"
    assert 3 in where(ctx, cols, StrCmp("v", "<", b"\x80")).tolist() and 4 not in where(ctx, cols, StrCmp("v", "<", b"\x80")).tolist()
    assert where(ctx, cols, All(StrCmp("v", "<", b"9"), StrCmp("v", ">=", b"10"))).tolist() == [5]   # "10" < "9"
    n = len(vals)
    for kind in ("prefix", "suffix", "contains"):   # the empty literal: every present value, the empty one included
        assert where(ctx, cols, make_pred((kind, None), "v", b"")).tolist() == list(range(n))
        assert where(ctx, cols, make_pred((kind, None), "v", b"\xff" * 26)).tolist() == []          # longer than every value
    for op in OPS:   # no such column: false under all nine, NE included — and true under Not
        for lit in (b"", b"a"):
            assert where(ctx, cols, All(Like(v=b"a"), make_pred(op, "gone", lit))).tolist() == []
            assert where(ctx, cols, Any(Not(make_pred(op, "gone", lit)), Like(v=b"zz"))).tolist() == list(range(n))


@pytest.mark.gpu
def test_adversarial_contains(ctx):
    """2049 rows of 25 bytes: a...a (the search verifies at every position and fails), and a...ab (it succeeds at the last)."""
    n = 2049
    rng = np.random.default_rng(3)
    pool = [b"a" * 25, b"a" * 24 + b"b", b"a" * 23 + b"ba", b"b" + b"a" * 24]
    idx = rng.integers(0, 4, n)
    cols = {"v": exact_device_col(packed_col(pool, idx))}
    for lit in (b"a" * 8 + b"b", b"a" * 16 + b"b", b"a" * 24 + b"b", b"ab", b"a" * 7 + b"ba"):
        check_where(ctx, cols, Contains("v", lit), pool_flags(("contains", None), lit, pool)[idx], lit)


# ---- literals beyond LDS, joined rows, the term limit ----------------------------------------------------------------------

@pytest.mark.gpu
def test_literal_block_in_global_memory(ctx):
    """Literals totalling more than 4096 bytes: the block stays in global memory, and the 17-byte literal is read from there."""
    n = 2049
    idx = row_index(n, 11)
    cols = {"v": exact_device_col(packed_col(POOL, idx))}
    big = MASTER[:16] + b"a" * 4090
    lit17 = MASTER[:17]
    f_cmp = np.array([v < big for v in POOL])[idx]
    f_pre = pool_flags(("prefix", None), lit17)[idx]
    f_suf = pool_flags(("suffix", None), MASTER[25 - 9:])[idx]
    check_where(ctx, cols, StrCmp("v", "<", big), f_cmp, "cmp big")
    check_where(ctx, cols, Any(Contains("v", big), HasPrefix("v", lit17)), f_pre, "contains big | prefix")
    check_where(ctx, cols, All(StrCmp("v", "<", big), Not(HasSuffix("v", MASTER[25 - 9:]))), f_cmp & ~f_suf, "cmp big & !suffix")
    check_where(ctx, cols, Any(Like(v=big), HasSuffix("v", big), HasSuffix("v", MASTER[25 - 9:])), f_suf, "like big | suffix")


def _device_ids(ids, keep):
    import torch
    t = torch.from_numpy(ids.view(np.uint8).copy()).to("cuda:0")
    keep.append(t)
    return t.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("id_bits", [32, 64])
def test_joined_rows(ctx, device, id_bits):
    """A column read through row ids with a base, as a Join hands it over."""
    n, src_rows, base = 2049, 300, 1000
    rng = np.random.default_rng(id_bits + device)
    src = row_index(src_rows, 5)
    ids = rng.integers(0, src_rows, n).astype(np.uint32 if id_bits == 32 else np.uint64)
    col = packed_col(POOL, src, 64 if id_bits == 64 else 32)
    with_base = ids + ids.dtype.type(base)
    keep = []
    cols = {"v": exact_device_col(col) if device else col}
    row_ids = {"v": (_device_ids(with_base, keep), id_bits, n, base) if device else (with_base, base)}
    at = src[ids.astype(np.int64)]
    for k, op in enumerate(OPS):
        lit = LITERALS[(3 * k + id_bits) % len(LITERALS)]
        check_where(ctx, cols, make_pred(op, "v", lit), pool_flags(op, lit)[at], (op, lit), row_ids=row_ids, nrows=n)
    del keep


def _mixed_program(nterms):
    """LIKE, IntCmp, FloatCmp and the new terms under All / Any / Not: `nterms` terms in all."""
    lits = LITERALS
    terms = [Like(v=lits[0]), IntCmp("i", ">", 3), FloatCmp("f", "<=", 1.5), StrCmp("v", ">=", lits[5]), HasPrefix("v", MASTER[:7]),
             Contains("v", MASTER[3:4])]
    k = 0
    while len(terms) < nterms:
        terms.append([StrCmp("v", P.RELS[k % 6], lits[k % len(lits)]), HasSuffix("v", lits[(k + 7) % len(lits)]),
                      Contains("v", lits[(k + 3) % len(lits)])][k % 3])
        k += 1
    a, b, c = terms[:6], terms[6:20], terms[20:]
    return Any(All(a[1], Not(a[0]), a[3]), All(a[2], Any(*b)), All(Not(Any(*c)), a[4], a[5]))


@pytest.mark.gpu
def test_exactly_32_mixed_terms_pass_and_33_do_not(ctx):
    from csvplus_amd.materialize import _pred_program, _rowsel
    n = 2049
    idx = row_index(n, 21)
    rng = np.random.default_rng(22)
    ints = [b"%d" % v for v in rng.integers(-5, 12, n)]
    ints[7] = b"x"
    floats = [b"%.2f" % v for v in rng.uniform(0, 3, n)]
    floats[9] = b""
    hostcols = {"v": packed_col(POOL, idx), "i": StrCol.from_values(ints, fixed_width=0), "f": StrCol.from_values(floats, fixed_width=0)}
    cols = {k: exact_device_col(c) for k, c in hostcols.items()}
    pred = _mixed_program(32)
    names, ops = P.compile(pred, list(cols))
    assert sum(1 for op, _, v in ops if v is not None) == 32
    assert {op for op, _, _ in ops} >= {P.LIKE, P.INT_LT + 5, P.FLT_LT + 1, P.HAS_PREFIX, P.HAS_SUFFIX, P.CONTAINS, P.NOT, P.ALL, P.ANY}
    flags = np.array([P.matches(pred, {"v": POOL[idx[r]], "i": ints[r], "f": floats[r]}) for r in range(n)])
    check_where(ctx, cols, pred, flags, "32 terms")
    # 33 terms: the Python compiler refuses, and so does the ABI
    with pytest.raises(ValueError):
        P.compile(Any(pred, Contains("v", b"a")), list(cols))
    ops33 = ops + [(P.CONTAINS, 0, b"a"), (P.ANY, 2, None)]
    keep = []
    arr, sel, _ = _rowsel([cols[nm] for nm in names], None, n, keep)
    for prog_ops, want in ((ops, N.CPH_OK), (ops33, N.CPH_ERR_INVALID)):
        prog = _pred_program(prog_ops, keep)
        opts = N.cph_filter_opts(N.CPH_FILTER_WHERE, 32, 0, 0, N.CPH_NO_LIMIT)
        out = C.POINTER(N.cph_rowlist)()
        rc = ctx.lib.cph_filter_rows(ctx.handle, arr, sel, len(names), n, prog, len(prog_ops), C.byref(opts), HOST, C.byref(out))
        assert rc == want, ctx.last_error()
        if rc == N.CPH_OK:
            ctx.lib.cph_rowlist_release(out)
        else:
            assert not out and "32" in ctx.last_error()


@pytest.mark.gpu
def test_argument_errors(ctx):
    from csvplus_amd.materialize import _pred_program
    col = StrCol.from_values([b"1", b"22", b"1"], fixed_width=0)
    arr = (N.cph_strcol * 1)()
    arr[0], k0 = col.as_c()

    def call(ops, patch=None):
        keep = []
        prog = _pred_program(ops, keep)
        if patch:
            patch(prog)
        opts = N.cph_filter_opts(N.CPH_FILTER_WHERE, 32, 0, 0, N.CPH_NO_LIMIT)
        out = C.POINTER(N.cph_rowlist)()
        rc = ctx.lib.cph_filter_rows(ctx.handle, arr, None, 1, 3, prog, len(ops), C.byref(opts), HOST, C.byref(out))
        if out:
            assert rc == N.CPH_OK
            ctx.lib.cph_rowlist_release(out)
        return rc, ctx.last_error()

    for op in (32, 33, 34, 35, 36, 37, 40, 41, 42):
        assert call([(op, 0, b"1")])[0] == N.CPH_OK
        assert call([(op, -1, b"1")])[0] == N.CPH_OK
        assert call([(op, 0, b"")])[0] == N.CPH_OK            # a NULL pointer with len 0
        rc, msg = call([(op, 1, b"1")])                        # column ncols
        assert rc == N.CPH_ERR_INVALID and msg, op
        rc, msg = call([(op, -2, b"1")])
        assert rc == N.CPH_ERR_INVALID and msg, op

        def no_pointer(prog):
            prog[0].value.data, prog[0].value.len = None, 3
        rc, msg = call([(op, 0, b"123")], no_pointer)          # a length without a pointer
        assert rc == N.CPH_ERR_INVALID and msg, op
    for op in (31, 38, 39, 43, 44, 64):
        rc, msg = call([(op, 0, b"1")])
        assert rc == N.CPH_ERR_INVALID and msg, op
    del k0
