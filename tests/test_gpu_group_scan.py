"""cph_index_dup_groups and cph_index_select over more rows than one scan tile.

dup_groups scans one flag per index row (exclusive_scan_u32, radix_sort.hip): 4096 flags per workgroup, one launch with
decoupled look-back up to 512 tiles, three kernels beyond — whose middle kernel, k_scan_block_sums, walks the tile sums
256 at a time and carries between the steps.  The tables here put the row count on the tile edge (4096 | 4097), past
the first 256-tile step of the three kernels (2^20 + 4097 rows under scan_lookback 0: 258 tiles) and past the point
where scan_lookback_pays hands over on its own (2^21 + 4097 rows: 514 tiles, three steps).

Keys are 7 decimal digits (a 32-bit code), about 3 rows per key, one group of 10 000 rows (half the table where the
table is smaller than that) and 100 keys that occur once on purpose; any build path will do.  The reference is numpy
run lengths over the oracle-sorted keys, never the library.
"""
import collections
import functools

import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol
from oracle import orc
from tests.test_gpu_code_widths import _profiled

SEED = 20260408
SCAN_TILE = 4096                 # kScanTile: 256 threads x 16 items
SCAN_STEP = 256                  # k_scan_block_sums: tile sums per step of its loop
LOOKBACK_MAX_TILES = 512         # scan_lookback_pays
KEY_LEN, KEY_SPACE = 7, 10 ** 7
BIG_GROUP, SINGLES, NPROBE = 10_000, 100, 2000

# (rows, scan_lookback settings)
CASES = ((4096, (1, 0)), (4097, (1, 0)), ((1 << 20) + 4097, (1, 0)), ((1 << 21) + 4097, (1,)))


def scan_tiles(n):
    return (n + SCAN_TILE - 1) // SCAN_TILE


def lookback_pays(n, scan_lookback=1):
    """scan_lookback_pays (radix_sort.hip)."""
    return bool(scan_lookback and 0 < n <= LOOKBACK_MAX_TILES * SCAN_TILE)


def scan_algo_bytes(n, scan_lookback=1):
    """What one exclusive_scan_u32 over n values reports to the profile: the look-back reads and writes every value
    once, the three kernels read twice and write once."""
    return (2 if lookback_pays(n, scan_lookback) else 3) * 4 * n


def decimal_keys(values):
    """(len(values), 7) bytes: the values as zero-padded decimal digits."""
    v = np.asarray(values, np.int64)
    return ((v[:, None] // 10 ** np.arange(KEY_LEN - 1, -1, -1)) % 10 + ord("0")).astype(np.uint8)


def column(data):
    n = len(data)
    return StrCol.from_arrays(np.ascontiguousarray(data).reshape(-1), (np.arange(n + 1, dtype=np.uint64) * KEY_LEN).astype(np.uint32))


GroupTable = collections.namedtuple("GroupTable", "n values col big")


def build_table(n):
    rng = np.random.default_rng([SEED, n])
    big = min(BIG_GROUP, n // 2)
    body = n - big - SINGLES
    space = rng.permutation(KEY_SPACE)[:body // 3 + SINGLES + 1]
    pool, once, big_value = space[:body // 3], space[body // 3:-1], space[-1]
    values = np.concatenate([pool[rng.integers(0, len(pool), body)], once, np.full(big, big_value)])[rng.permutation(n)]
    return GroupTable(n, values, column(decimal_keys(values)), big)


Ref = collections.namedtuple("Ref", "table perm lower upper firsts absent")


@functools.lru_cache(maxsize=1)
def reference(n):
    """Order, duplicate groups and every run's first position: numpy run lengths over the oracle-sorted keys."""
    t = build_table(n)
    perm = orc.OracleIndex([t.col]).perm
    sv = t.values[perm]
    firsts = np.flatnonzero(np.concatenate([[True], sv[1:] != sv[:-1]]))
    ends = np.append(firsts[1:], n)
    dup = ends - firsts >= 2
    absent = np.setdiff1d(np.arange(0, KEY_SPACE, 997), t.values)[:NPROBE // 4]
    return Ref(t, perm, firsts[dup].astype(np.uint64), ends[dup].astype(np.uint64), firsts.astype(np.uint64), absent)


def check_fixtures():
    """The CPU half (run by tests/test_gpu_general_sort.py's unmarked test): the row counts sit where the docstring says."""
    assert [n for n, _ in CASES] == [SCAN_TILE, SCAN_TILE + 1, (1 << 20) + 4097, (1 << 21) + 4097]
    assert [scan_tiles(n) for n, _ in CASES] == [1, 2, 258, 514]
    assert [lookback_pays(n) for n, _ in CASES] == [True, True, True, False] and not any(lookback_pays(n, 0) for n, _ in CASES)
    assert lookback_pays(LOOKBACK_MAX_TILES * SCAN_TILE) and not lookback_pays(LOOKBACK_MAX_TILES * SCAN_TILE + 1)
    # k_scan_block_sums' loop: a second step under scan_lookback 0 at 2^20 + 4097 rows, a third at 2^21 + 4097
    assert [-(-scan_tiles(n) // SCAN_STEP) for n, _ in CASES] == [1, 1, 2, 3]
    assert scan_algo_bytes(4097) == 8 * 4097 and scan_algo_bytes(4097, 0) == 12 * 4097 == scan_algo_bytes(4097 + (1 << 21)) - 12 * (1 << 21)
    for n in (4096, 4097, 50_001):
        r = reference(n)
        t = r.table
        assert t.col.nrows == n == len(t.values) and t.col.fixed_width == KEY_LEN and t.values.max() < KEY_SPACE
        assert [bytes(k) for k in decimal_keys([0, 42, KEY_SPACE - 1])] == [b"0000000", b"0000042", b"9999999"]
        sizes = np.diff(np.append(r.firsts, n))
        assert sizes.max() == t.big == min(BIG_GROUP, n // 2) and (sizes == t.big).sum() == 1
        assert (sizes == 1).sum() >= SINGLES and 2.0 < (n - t.big) / (len(sizes) - 1) < 4.0
        assert len(r.lower) == (sizes >= 2).sum() and (r.upper - r.lower).sum() == n - (sizes == 1).sum()
        # the same order from numpy's stable sort over the byte keys
        keys = decimal_keys(t.values).view("S%d" % KEY_LEN).reshape(-1)
        assert np.array_equal(np.argsort(keys, kind="stable"), r.perm)
        assert len(r.absent) and not np.isin(r.absent, t.values).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,lookbacks", CASES, ids=[str(n) for n, _ in CASES])
def test_groups_and_select_beyond_one_scan_tile(ctx, n, lookbacks):
    r = reference(n)
    t = r.table
    rng = np.random.default_rng([SEED, n, 1])
    probe_values = np.concatenate([t.values[rng.integers(0, n, NPROBE - len(r.absent))], r.absent])[rng.permutation(NPROBE)]
    probe = [column(decimal_keys(probe_values))]
    kept = r.perm[r.firsts.astype(np.int64)]            # the rows select keeps, in index order
    sub = orc.OracleIndex([column(decimal_keys(t.values[kept]))])
    assert np.array_equal(sub.perm, np.arange(len(kept)))   # distinct and already sorted
    want = sub.join(probe)
    ix = DeviceIndex(ctx, [t.col])
    try:
        assert ix.info()["key_bytes"] == 4
        assert np.array_equal(ix.perm(), r.perm)
        for lookback in lookbacks:
            ctx.set_option("scan_lookback", lookback)
            (lower, upper), prof = _profiled(ctx, ix.dup_groups)
            assert np.array_equal(lower, r.lower) and np.array_equal(upper, r.upper), (n, lookback)
            scans = prof["exclusive_scan_u32"]   # one scan per pass (lower bounds, upper bounds), by the kernels the setting names
            assert (scans["launches"], scans["algo_bytes"]) == (2, 2 * scan_algo_bytes(n, lookback)), (n, lookback, scans)
            nx = ix.select(r.firsts)
            try:
                assert nx.nrows == len(kept) and np.array_equal(nx.perm(), kept), (n, lookback)
                assert nx.dup_groups()[0].size == 0
                m = nx.probe(probe)
                assert np.array_equal(m.cnt, want["cnt"]) and m.nmatches == want["nmatches"]
                hit = m.cnt > 0
                assert np.array_equal(m.lo[hit], want["lo"][hit])
                assert np.array_equal(m.probe_idx, want["probe_idx"]) and np.array_equal(m.build_row, kept[want["build_row"]])
                m.release()
            finally:
                nx.close()
    finally:
        ctx.set_option("scan_lookback", 1)
        ix.close()
