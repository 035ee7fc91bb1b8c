"""The kernels on the build side of the flagship step and the Join's match count: the sample of a fixed-width id column
(keycodec.hip: k_sample_fixed8), the total of the chain's per-wave counts (chain.hip: k_sum_counts_report) and the tile edges of
the window sort's partition (window_sort.hip).  The first two gather in self-cleaning device accumulators that must be zero again
when the kernel ends, whatever its grid; all expected values here come from numpy or from the CPU oracle."""
import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc

pytestmark = pytest.mark.gpu

N_SAMPLED = (1 << 20) + 4321   # the smallest size band at which the statistics come from a sample (codec_sample_applies)


def digits8(ids) -> np.ndarray:
    """ids -> their 8 decimal digits, zero padded, as an (n, 8) byte matrix."""
    v = np.asarray(ids, dtype=np.int64).copy()
    out = np.empty((len(v), 8), np.uint8)
    for p in range(7, -1, -1):
        out[:, p] = v % 10 + 48
        v //= 10
    return out


def fixed_col(mat: np.ndarray) -> StrCol:
    n, w = mat.shape
    return StrCol.from_arrays(np.ascontiguousarray(mat).reshape(-1), np.arange(n + 1, dtype=np.uint32) * w, fixed_width=w)


def alphabet_product(mat: np.ndarray) -> int:
    prod = 1
    for p in range(mat.shape[1]):
        prod *= len(np.unique(mat[:, p]))
    return prod


@pytest.fixture(scope="module")
def sampled_columns():
    """(letters, digits): two unique fixed-8 columns of N_SAMPLED rows.  `letters` holds a..f at position 5 — byte values the
    digits column never shows, in a mask word of the accumulator the digits never set."""
    rng = np.random.default_rng(41)
    k = rng.permutation(N_SAMPLED)
    letters = digits8((k // 600) * 1000 + k % 100)
    letters[:, 5] = ord("a") + (k // 100) % 6
    digits = digits8(rng.permutation(N_SAMPLED))
    out = []
    for mat in (letters, digits):
        col = fixed_col(mat)
        out.append((col.to_device("cuda:0"), orc.OracleIndex([col]).perm, alphabet_product(mat)))
    return out


def test_sample_accumulator_is_zero_at_rest_between_builds(sampled_columns):
    """Two sampled builds on one ctx: what the first left in the sample's accumulator would show up as extra alphabet entries
    (a larger code space) of the second."""
    from csvplus_amd import Context

    ctx = Context(0)
    for dcol, perm, states in sampled_columns:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        g = DeviceIndex(ctx, [dcol], unique=True)
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert prof["k_split_count"]["launches"] == 1, sorted(prof)
        assert g.status == N.CPH_OK and g.first_dup is None
        if dcol is sampled_columns[1][0]:
            assert g.info()["table_entries"] == states
        np.testing.assert_array_equal(g.perm(), perm)
        g.close()
    ctx.close()


def test_sample_accumulators_of_both_stream_slots(sampled_columns):
    """The same pair as one batch (cph_index_build_many: one build per stream slot, each with its own accumulator), twice, the
    second time in the other order so that either slot sees the letters first."""
    from csvplus_amd import Context

    ctx = Context(0)
    for order in ((0, 1), (1, 0)):
        cols = [sampled_columns[i] for i in order]
        built = DeviceIndex.build_many(ctx, [([c[0]], True) for c in cols])
        for g, (dcol, perm, states) in zip(built, cols):
            assert g.status == N.CPH_OK and g.first_dup is None
            if dcol is sampled_columns[1][0]:
                assert g.info()["table_entries"] == states
            np.testing.assert_array_equal(g.perm(), perm)
            g.close()
    ctx.close()


def test_sample_of_a_width_5_column():
    """W < 8 (only the first W bytes of a loaded word count) and a row count that is a multiple of the sampling step."""
    from csvplus_amd import Context

    ctx = Context(0)
    n = 1 << 20
    k = np.random.default_rng(43).permutation(n)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    mat = np.stack([hexd[(k >> (4 * (4 - p))) & 15] for p in range(5)], axis=1)
    col = fixed_col(mat)
    o = orc.OracleIndex([col])
    for _ in range(2):
        g = DeviceIndex(ctx, [col.to_device("cuda:0")], unique=True)
        assert g.status == N.CPH_OK and g.first_dup is None
        assert g.info()["table_entries"] == 16 ** 5 == alphabet_product(mat)
        np.testing.assert_array_equal(g.perm(), o.perm)
        g.close()
    ctx.close()


# ---- the count kernel -------------------------------------------------------------------------------------------------------

def expect_join(inv: np.ndarray, probe_ids: np.ndarray):
    """inv[id] = build row of id, or -1.  -> (stream rows, build rows) of the joined rows in stream order."""
    hit = np.zeros(len(probe_ids), bool)
    inside = probe_ids < len(inv)
    hit[inside] = inv[probe_ids[inside]] >= 0
    rows = np.nonzero(hit)[0]
    return rows.astype(np.uint64), inv[probe_ids[rows]].astype(np.uint32)


def test_count_kernel_totals_back_to_back():
    """One ctx, one index, Joins whose totals differ, back to back: every launch starts from the accumulator the launch before
    left behind.  The half-joining case has 4 counts per 2048 stream rows = 17 580 counts: more than two sweeps of 32 workgroups
    of 256 threads (16 384) and no multiple of one, with whole 16-byte groups, a partly filled round of loads and a remainder."""
    from csvplus_amd import Context

    ctx = Context(0)
    rng = np.random.default_rng(47)
    nb = 100_000
    build_ids = rng.permutation(nb)
    inv = np.full(2 * nb, -1, np.int64)
    inv[build_ids] = np.arange(nb)
    g = DeviceIndex(ctx, [fixed_col(digits8(build_ids)).to_device("cuda:0")], unique=True)
    assert g.status == N.CPH_OK
    cases = [
        ("all", rng.integers(0, nb, 300_001)),
        ("none", rng.integers(2 * nb, 3 * nb, 300_001)),
        ("half", rng.integers(0, 2 * nb, 9_000_001)),
        ("one", np.array([int(build_ids[5])])),
        ("2049", rng.integers(0, 2 * nb, 2049)),
        ("all again", rng.integers(0, nb, 4099)),
    ]
    for name, ids in cases:
        es, eb = expect_join(inv, ids)
        ctx.profile(True)
        ctx.profile_read(reset=True)
        ch = join_chain(ctx, [(g, [fixed_col(digits8(ids))])])
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert "k_sum_counts" in prof, (name, sorted(prof))
        assert ch.nrows == len(es), name
        if name.startswith("all"):
            assert ch.identity, name
        if ch.nrows:
            np.testing.assert_array_equal(ch.stream_row, es, err_msg=name)
            np.testing.assert_array_equal(ch.build_row(0), eb, err_msg=name)
        ch.release()
    g.close()
    ctx.close()


def test_count_kernel_behind_build_side_keys():
    """The count's other launch sites: a second step keyed by a column of the first build table, answered from pre-joined
    tables (chain_prejoin = 1) and by the kernel that gathers the key per stream row (0); and, with duplicate keys in the first
    index, the general path's pre-joined tuples."""
    from csvplus_amd import Context

    ctx = Context(0)
    rng = np.random.default_rng(53)
    nc, nreg, m = 30_000, 200, 200_003
    cust_ids = rng.permutation(40_000)[:nc]
    cust_region = rng.integers(0, 260, nc)           # some regions do not exist
    regions = rng.permutation(260)[:nreg]
    okeys = rng.integers(0, 40_000, m)               # some customers do not exist
    cinv = np.full(40_000, -1, np.int64)
    cinv[cust_ids] = np.arange(nc)
    rinv = np.full(260, -1, np.int64)
    rinv[regions] = np.arange(nreg)
    crow = cinv[okeys]
    rrow = np.where(crow >= 0, rinv[cust_region[np.maximum(crow, 0)]], -1)
    keep = np.nonzero((crow >= 0) & (rrow >= 0))[0]
    gc = DeviceIndex(ctx, [fixed_col(digits8(cust_ids))], unique=True)
    gr = DeviceIndex(ctx, [fixed_col(digits8(regions))], unique=True)
    steps = [(gc, [fixed_col(digits8(okeys))], 0), (gr, [fixed_col(digits8(cust_region))], 1)]
    try:
        for pj in (1, 0):
            ctx.set_option("chain_prejoin", pj)
            ctx.profile(True)
            ctx.profile_read(reset=True)
            ch = join_chain(ctx, steps, probe_base=7)
            prof = ctx.profile_read(reset=True)
            ctx.profile(False)
            assert "k_sum_counts" in prof and ("k_chain_prejoined" in prof) == bool(pj), (pj, sorted(prof))
            assert ch.nrows == len(keep) and 0 < len(keep) < m
            np.testing.assert_array_equal(ch.stream_row, keep.astype(np.uint64) + 7)
            np.testing.assert_array_equal(ch.build_row(0), crow[keep].astype(np.uint32))
            np.testing.assert_array_equal(ch.build_row(1), rrow[keep].astype(np.uint32))
            ch.release()
    finally:
        ctx.set_option("chain_prejoin", 1)
    # duplicates in the first index: people.Join(IndexOn(orders.cust_id)).Join(products, prod_id of the orders row)
    npeople, nord, nprod = 4000, 50_000, 300
    people = rng.permutation(npeople + 500)[:npeople]
    o_cust = rng.integers(0, npeople + 500, nord)
    o_prod = rng.integers(0, nprod + 60, nord)       # some products do not exist
    prods = rng.permutation(nprod)
    pinv = np.full(nprod + 60, -1, np.int64)
    pinv[prods] = np.arange(nprod)
    go = DeviceIndex(ctx, [fixed_col(digits8(o_cust))])
    gp = DeviceIndex(ctx, [fixed_col(digits8(prods))], unique=True)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    ch = join_chain(ctx, [(go, [fixed_col(digits8(people))], 0), (gp, [fixed_col(digits8(o_prod))], 1)])
    prof = ctx.profile_read(reset=True)
    ctx.profile(False)
    assert "k_prejoin_tuples" in prof and "k_sum_counts" in prof, sorted(prof)
    order = np.argsort(o_cust, kind="stable")        # an index keeps equal keys in row order
    lo = np.searchsorted(o_cust[order], people, "left")
    hi = np.searchsorted(o_cust[order], people, "right")
    es = np.repeat(np.arange(npeople), hi - lo)
    eo = np.concatenate([order[a:b] for a, b in zip(lo, hi)])
    ep = pinv[o_prod[eo]]
    ok = ep >= 0
    assert ch.nrows == int(ok.sum())
    np.testing.assert_array_equal(ch.stream_row, es[ok].astype(np.uint64))
    np.testing.assert_array_equal(ch.build_row(0), eo[ok].astype(np.uint32))
    np.testing.assert_array_equal(ch.build_row(1), ep[ok].astype(np.uint32))
    ch.release()
    for g in (gc, gr, go, gp):
        g.close()
    ctx.close()


# ---- the partition's tiles --------------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize("n", [65_536, 65_537, 9 * 8192 - 3])
def test_partition_tile_edges(n):
    """Unique dense fixed-8 ids at the direct path's smallest table, with a last tile of one row, and with a last group of four
    keys that straddles the end of the table (tiles hold 8192 rows, a thread loads its keys four at a time)."""
    from csvplus_amd import Context

    ctx = Context(0)
    dcol = fixed_col(digits8(np.random.default_rng(n).permutation(n))).to_device("cuda:0")
    g, r, prof = build_both_ways(ctx, dcol)
    assert 1 <= prof["k_win_partition"]["launches"] <= 2 and "k_win_place" in prof, sorted(prof)
    assert g.status == r.status == N.CPH_OK and g.first_dup is None
    np.testing.assert_array_equal(g.perm(), r.perm())
    g.close(); r.close(); ctx.close()


def test_partition_into_a_half_filled_code_space():
    """Ids drawn from 60 % of [0, 1.6 n): windows that are not full (their offsets come from a scan) and the Join's rank table,
    which the placement leaves behind: positions of 20 000 probes against numpy.searchsorted."""
    from csvplus_amd import Context

    ctx = Context(0)
    rng = np.random.default_rng(59)
    n = 300_000
    ids = rng.permutation(int(1.6 * n))[:n]
    dcol = fixed_col(digits8(ids)).to_device("cuda:0")
    g, r, prof = build_both_ways(ctx, dcol)
    assert "k_win_partition" in prof and "k_win_place" in prof, sorted(prof)
    assert g.status == r.status == N.CPH_OK and g.first_dup is None
    np.testing.assert_array_equal(g.perm(), r.perm())
    np.testing.assert_array_equal(g.perm(), np.argsort(ids, kind="stable").astype(np.uint32))
    probe = rng.integers(0, int(1.7 * n), 20_000)
    srt = np.sort(ids)
    pos = np.searchsorted(srt, probe)
    hit = (pos < n) & (srt[np.minimum(pos, n - 1)] == probe)
    ch = join_chain(ctx, [(g, [fixed_col(digits8(probe))])], positions=True)
    assert ch.positions and ch.nrows == int(hit.sum())
    np.testing.assert_array_equal(ch.stream_row, np.nonzero(hit)[0].astype(np.uint64))
    np.testing.assert_array_equal(ch.build_row(0), pos[hit].astype(np.uint32))
    ch.release()
    g.close(); r.close(); ctx.close()


def test_partition_with_a_planted_duplicate():
    """Rows 7 and 200 001 share a key: the optimistic sort notices and the general path says where, exactly as without it."""
    from csvplus_amd import Context

    ctx = Context(0)
    n = 300_000
    ids = np.random.default_rng(61).permutation(n)
    ids[200_001] = ids[7]
    dcol = fixed_col(digits8(ids)).to_device("cuda:0")
    g, r, prof = build_both_ways(ctx, dcol)
    assert "k_win_partition" in prof, sorted(prof)
    assert g.status == r.status == N.CPH_ERR_DUPLICATE
    assert g.first_dup == r.first_dup and g.first_dup is not None
    np.testing.assert_array_equal(g.perm(), r.perm())
    g.close(); r.close(); ctx.close()
