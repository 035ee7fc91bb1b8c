"""The order of an id-column index build on the host and on the streams: the jobs of a two-stream batch go on per stream at the
first synchronisation (the main stream's jobs run phase 2 while the side stream still delivers), and k_win_place reads its
window two entries per load.  Whatever the order, the index is the oracle's, its codec block is complete when the call returns,
and a sample miss or a duplicate leaves nothing behind for the next build."""
import ctypes as C

import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc

pytestmark = pytest.mark.gpu

# the sampled path needs 2^20 rows (codec_sample_applies): that size, a tail tile of one row with an odd count in the last
# window, and a tail tile that ends inside a group of four keys
SIZES = [1 << 20, (1 << 20) + 1, (1 << 20) + 8192 + 3]


def digits8(ids) -> np.ndarray:
    """ids -> their 8 decimal digits, zero padded, as an (n, 8) byte matrix."""
    v = np.asarray(ids, dtype=np.int64).copy()
    out = np.empty((len(v), 8), np.uint8)
    for p in range(7, -1, -1):
        out[:, p] = v % 10 + 48
        v //= 10
    return out


def letters8(ids, positions: int) -> np.ndarray:
    """ids -> `positions` base-16 digits written 'a'..'p' behind constant bytes: 16^positions ids fill their code space."""
    v = np.asarray(ids, dtype=np.int64)
    out = np.full((len(v), 8), ord("k"), np.uint8)
    for p in range(positions):
        out[:, 7 - p] = ord("a") + ((v >> (4 * p)) & 15)
    return out


def fixed_col(mat: np.ndarray) -> StrCol:
    n, w = mat.shape
    return StrCol.from_arrays(np.ascontiguousarray(mat).reshape(-1), np.arange(n + 1, dtype=np.uint32) * w, fixed_width=w)


def alphabet_product(mat: np.ndarray) -> int:
    prod = 1
    for p in range(mat.shape[1]):
        prod *= len(np.unique(mat[:, p]))
    return prod


class Table:
    """A key column on the host and on the device, and what the oracle says about it (computed once, never changed)."""

    def __init__(self, col: StrCol, device: bool = True):
        self.host = col
        self.dev = col.to_device("cuda:0") if device else col
        self.oracle = orc.OracleIndex([col])
        self.perm = self.oracle.perm
        self.perm.setflags(write=False)


@pytest.fixture(scope="module")
def products():
    """Unpadded decimal ids, 1000 rows: the small neighbour of the flagship batch."""
    return Table(StrCol.from_values([b"%d" % int(i) for i in np.random.default_rng(71).permutation(1000)]), device=False)


@pytest.fixture(scope="module")
def regions():
    """A third job for the batch: 100 000 unpadded ids (statistics pass + read-back, no sample)."""
    return Table(StrCol.from_values([b"%d" % int(i) for i in np.random.default_rng(72).permutation(100_000)]), device=False)


_ids_cache = {}


def dense_ids(n: int) -> Table:
    """Unique fixed-8 decimal ids 0 .. n-1 in random order (at these sizes 2e6 codes: the windows' offsets come from a scan)."""
    if n not in _ids_cache:
        _ids_cache[n] = Table(fixed_col(digits8(np.random.default_rng(n).permutation(n))))
    return _ids_cache[n]


@pytest.fixture(scope="module")
def full_space():
    """2^20 ids over five positions of sixteen letters: every code of the code space is taken (no offsets, identity Join)."""
    n = 1 << 20
    mat = letters8(np.random.default_rng(73).permutation(n), 5)
    assert alphabet_product(mat) == n
    return Table(fixed_col(mat))


def check_built(g, table: Table, what=""):
    assert g.status == N.CPH_OK and g.first_dup is None, what
    np.testing.assert_array_equal(g.perm(), table.perm, err_msg=str(what))


def check_find(g, table: Table, keys):
    """cph_index_find_many against the oracle.  [lower, upper) are the positions of the equal keys; where there are none the
    library leaves the position open (csvplus_hip.h), so it is compared only for a non-empty range."""
    lo, hi = g.find_many(keys)
    for a, b, key in zip(lo.tolist(), hi.tolist(), keys):
        olo, ohi = table.oracle.find(key)
        assert b - a == ohi - olo and (ohi == olo or a == olo), (key, (a, b), (olo, ohi))


def flagship_orders(eng, big: Table, products: Table, regions: Table):
    """The batch as (large, small), swapped (the large job on the side stream), as three jobs, and on one stream."""
    for name, tables, side in (("main", [big, products], 1), ("swapped", [products, big], 1), ("three", [big, products, regions], 1),
                               ("one stream", [big, products], 0)):
        eng.ctx.set_option("build_side_stream", side)
        try:
            built = eng.index_on_many([[t.dev] for t in tables], unique=True)
        finally:
            eng.ctx.set_option("build_side_stream", 1)
        for g, t in zip(built, tables):
            check_built(g, t, name)
            g.close()


# ---- 1. the flagship batch at its smallest ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_flagship_batch_in_every_order(n, products, regions):
    from csvplus_amd.engine import Engine

    eng = Engine(0)
    try:
        flagship_orders(eng, dense_ids(n), products, regions)
    finally:
        eng.close()


def test_flagship_batch_over_a_full_code_space(full_space, products, regions):
    from csvplus_amd.engine import Engine

    eng = Engine(0)
    try:
        flagship_orders(eng, full_space, products, regions)
    finally:
        eng.close()


# ---- 2. the codec block is on the device when the call returns ----------------------------------------------------------------

@pytest.mark.parametrize("swapped", [False, True])
def test_codec_block_is_complete_when_the_batch_returns(swapped, products):
    """Consumers that read the uploaded codec block (not the arithmetic plan), straight behind the batch: cph_index_find_many,
    a chain Join with chain_arith = 0; then the lean chain Join."""
    from csvplus_amd import Context

    n = SIZES[1]
    big = dense_ids(n)
    rng = np.random.default_rng(79)
    present = rng.integers(0, n, 1000)
    absent = np.concatenate([rng.integers(n, 2_000_000, 800), rng.integers(2_000_000, 10 ** 8, 200)])
    keys = [bytes(r) for r in digits8(np.concatenate([present, absent]))]
    ctx = Context(0)
    tables = [products, big] if swapped else [big, products]
    built = DeviceIndex.build_many(ctx, [([t.dev], True) for t in tables])
    g = built[1 if swapped else 0]
    check_find(g, big, keys)
    lo, hi = g.find_many(keys)
    assert int((hi - lo).sum()) == 1000
    probe = fixed_col(digits8(rng.integers(0, 2 * n, 50_001)))
    oj = big.oracle.join([probe])
    ctx.set_option("chain_arith", 0)
    try:
        ch = join_chain(ctx, [(g, [probe])], positions=True)
    finally:
        ctx.set_option("chain_arith", 1)
    assert ch.positions and ch.nrows == oj["nmatches"]
    np.testing.assert_array_equal(ch.stream_row, oj["probe_idx"])
    np.testing.assert_array_equal(big.perm[ch.build_row(0)], oj["build_row"])
    ch.release()
    # the lean chain Join of the table with itself: every row joins, result row m is row m
    ch = join_chain(ctx, [(g, [big.dev])], positions=True)
    assert ch.positions and ch.nrows == n
    np.testing.assert_array_equal(big.perm[ch.build_row(0)], np.arange(n, dtype=np.uint32))
    ch.release()
    for t, b in zip(tables, built):
        check_built(b, t)
        b.close()
    ctx.close()


# ---- 3. a sample miss ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swapped", [False, True])
def test_sample_miss_goes_round_again_and_leaves_nothing_behind(swapped, products):
    """One key with a byte no sampled row shows, at a row the sample skips (it takes rows 0, step, 2 step, ... with
    step = n >> 16): the sort launched from the sample's alphabets flags the row and the build comes back through the exact
    pass.  The next batch on the same ctx finds the sample accumulator and the window cursors zero and its own codec block."""
    from csvplus_amd import Context

    n = SIZES[1]
    step = n >> 16
    assert step > 1
    clean = dense_ids(n)
    mat = np.ascontiguousarray(clean.host.data).reshape(n, 8).copy()
    row = 5 * step + 3
    mat[row, 7] = ord("a")
    planted = Table(fixed_col(mat))
    ctx = Context(0)
    for big in (planted, clean, planted, clean):
        tables = [products, big] if swapped else [big, products]
        ctx.profile(True)
        ctx.profile_read(reset=True)
        built = DeviceIndex.build_many(ctx, [([t.dev], True) for t in tables])
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        # the first attempt is the sample + the sort that codes the keys itself; only the second attempt of a planted build runs
        # the exact statistics pass (the 1000-row neighbour is a one-launch build: no statistics kernel of its own)
        assert prof["k_split_count"]["launches"] == 1 and "k_win_partition" in prof and "k_small_build" in prof, sorted(prof)
        assert ("k_col_stats" in prof) == (big is planted), sorted(prof)
        for t, b in zip(tables, built):
            check_built(b, t)
        g = built[1 if swapped else 0]
        if big is clean:
            assert g.info()["table_entries"] == 2_000_000   # (nothing of the planted build's alphabets is left in the accumulator)
        check_find(g, big, [bytes(mat[row]), bytes(mat[row - 1])])   # (reads the codec block of THIS build)
        for b in built:
            b.close()
    ctx.close()


# ---- 4. a planted duplicate ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swapped", [False, True])
def test_planted_duplicate_in_the_large_job(swapped, products):
    from csvplus_amd import Context

    n = SIZES[2]
    mat = np.ascontiguousarray(dense_ids(n).host.data).reshape(n, 8).copy()
    mat[900_001] = mat[7]
    dup = Table(fixed_col(mat))
    want = dup.oracle.first_dup()
    assert want is not None
    ctx = Context(0)
    tables = [products, dup] if swapped else [dup, products]
    built = DeviceIndex.build_many(ctx, [([t.dev], True) for t in tables])
    g, p = (built[1], built[0]) if swapped else (built[0], built[1])
    assert g.status == N.CPH_ERR_DUPLICATE and g.first_dup == want
    np.testing.assert_array_equal(g.perm(), dup.perm)
    check_built(p, products)
    for b in built:
        b.close()
    ctx.close()


# ---- 5. one job of the batch fails validation -----------------------------------------------------------------------------------

def build_many_statuses(ctx, specs):
    """cph_index_build_many without DeviceIndex.build_many's raise: [(DeviceIndex or None, status), ...] and the call's code."""
    k = len(specs)
    arr = (N.cph_index_spec * k)()
    keep = []
    for i, (cols, unique) in enumerate(specs):
        ca, kp = N._cols_array(cols)
        keep.append((ca, kp))
        arr[i].keycols = ca
        arr[i].nkeycols = len(cols)
        arr[i].unique = 1 if unique else 0
    outs = (N._P * k)()
    dups = (C.c_uint64 * k)()
    sts = (C.c_int32 * k)()
    rc = ctx.lib.cph_index_build_many(ctx.handle, arr, k, outs, dups, sts)
    del keep
    res = []
    for i in range(k):
        ix = None
        if outs[i]:
            ix = DeviceIndex._from_handle(ctx, N._P(outs[i]))
            ix.status = int(sts[i])
            ix.first_dup = None if dups[i] == N.UINT64_MAX else int(dups[i])
        res.append((ix, int(sts[i])))
    return res, rc


@pytest.mark.parametrize("bad_at", [0, 1, 2])
def test_one_job_fails_validation_the_others_build(bad_at, products):
    """Two key columns of different row counts: refused in phase 1.  The jobs around it keep their streams and build."""
    from csvplus_amd import Context

    big = dense_ids(SIZES[0])
    good = [big, products]
    specs = [([t.dev], True) for t in good]
    specs.insert(bad_at, ([products.dev, big.dev], True))
    ctx = Context(0)
    res, rc = build_many_statuses(ctx, specs)
    assert rc == N.CPH_ERR_INVALID
    assert res[bad_at] == (None, N.CPH_ERR_INVALID)
    rest = [r for i, r in enumerate(res) if i != bad_at]
    for (g, st), t in zip(rest, good):
        assert st == N.CPH_OK
        check_built(g, t)
        g.close()
    ctx.close()


# ---- 6. a half-filled code space ------------------------------------------------------------------------------------------------

def test_half_filled_code_space_through_the_sampled_path():
    """Ids drawn from 60 % of [0, 1.6 n): windows that are not full — offsets from the scan, the rank table left behind by the
    placement — built alone, on one stream."""
    from csvplus_amd import Context

    n = SIZES[2]
    rng = np.random.default_rng(83)
    ids = rng.permutation(int(1.6 * n))[:n]
    t = Table(fixed_col(digits8(ids)))
    ctx = Context(0)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    g = DeviceIndex(ctx, [t.dev], unique=True)
    prof = ctx.profile_read(reset=True)
    ctx.profile(False)
    assert "k_win_partition" in prof and "k_win_place" in prof and prof["k_split_count"]["launches"] == 1, sorted(prof)
    check_built(g, t)
    np.testing.assert_array_equal(g.perm(), np.argsort(ids, kind="stable").astype(np.uint32))
    probe = rng.integers(0, int(1.7 * n), 20_000)
    pcol = fixed_col(digits8(probe))
    oj = t.oracle.join([pcol])
    ch = join_chain(ctx, [(g, [pcol])], positions=True)
    assert ch.positions and ch.nrows == oj["nmatches"] and 0 < ch.nrows < len(probe)
    np.testing.assert_array_equal(ch.stream_row, oj["probe_idx"])
    np.testing.assert_array_equal(t.perm[ch.build_row(0)], oj["build_row"])
    srt = np.sort(ids)
    np.testing.assert_array_equal(ch.build_row(0), np.searchsorted(srt, probe[oj["probe_idx"].astype(np.int64)]).astype(np.uint32))
    ch.release()
    g.close()
    ctx.close()


# ---- 7. the placement's read phase alone --------------------------------------------------------------------------------------

def build_both_ways(ctx, dcol):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    g = DeviceIndex(ctx, [dcol], unique=True)
    prof = ctx.profile_read(reset=True)
    ctx.profile(False)
    ctx.set_option("direct_sort", 0)
    try:
        r = DeviceIndex(ctx, [dcol], unique=True)
    finally:
        ctx.set_option("direct_sort", 1)
    return g, r, prof


def placement_ids(n: int, space: str) -> np.ndarray:
    rng = np.random.default_rng(n + len(space))
    if space == "full":
        return rng.permutation(n)
    # 100 000 codes (five positions of ten digits: code = id) without those of window 2: its count is zero, the others'
    # are whatever the draw gives, odd and even
    pool = np.concatenate([np.arange(0, 2 << 14), np.arange(3 << 14, 100_000)])
    return rng.permutation(pool)[:n]


@pytest.mark.parametrize("space", ["full", "half"])
@pytest.mark.parametrize("n", [65_536, 65_537, 9 * 8192 - 3])
def test_placement_reads_pairs_of_entries(n, space):
    from csvplus_amd import Context

    ids = placement_ids(n, space)
    assert len(ids) == n == len(np.unique(ids))
    ctx = Context(0)
    g, r, prof = build_both_ways(ctx, fixed_col(digits8(ids)).to_device("cuda:0"))
    assert 1 <= prof["k_win_partition"]["launches"] <= 2 and "k_win_place" in prof, sorted(prof)
    assert g.status == r.status == N.CPH_OK and g.first_dup is None
    np.testing.assert_array_equal(g.perm(), r.perm())
    np.testing.assert_array_equal(g.perm(), np.argsort(ids, kind="stable").astype(np.uint32))
    g.close(); r.close(); ctx.close()


def test_placement_of_full_windows():
    """16^4 ids over four positions of sixteen letters: states == n, every window holds exactly 2^14 entries."""
    from csvplus_amd import Context

    n = 65_536
    ids = np.random.default_rng(89).permutation(n)
    mat = letters8(ids, 4)
    assert alphabet_product(mat) == n
    ctx = Context(0)
    g, r, prof = build_both_ways(ctx, fixed_col(mat).to_device("cuda:0"))
    assert "k_win_partition" in prof and "k_win_place" in prof, sorted(prof)
    assert g.status == r.status == N.CPH_OK and g.first_dup is None
    assert g.info()["table_entries"] == n
    np.testing.assert_array_equal(g.perm(), r.perm())
    np.testing.assert_array_equal(g.perm(), np.argsort(ids, kind="stable").astype(np.uint32))
    g.close(); r.close(); ctx.close()
