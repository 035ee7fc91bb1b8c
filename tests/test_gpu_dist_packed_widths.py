"""Every width edge of the bit-packed exchange (CPH_DIST_PACKED, dist.hip: k_pack_rows / k_unpack_rows) on the device:
rows that straddle two 64-bit words, 32, 33 and 64 bits per row, the fallback at 65, and step 0's absent code pushing its
width over a power of two — with chunk lengths on both sides of the 64-row group, the 256-row pack tile and the 2048-row
chain tile.  Loopback transport, thread ranks on one GPU; every rank's gathered arrays equal the oracle's nested joins over
the whole stream and the arrays of the same call without packing.

Bits per row as dist.hip states them: step 0 needs bit_length(rows) (values 0 .. rows-1 and the absent code `rows`), a later
step bit_length(rows - 1), each at least 1.  The expected numbers below are literals.
"""
import functools

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N
from oracle import orc
from tests.test_gpu_chain import oracle_chain
from tests.test_gpu_dist import gathered_array, loopback_factory, run_ranks

pytestmark = pytest.mark.gpu

# (index rows per step, bits per row on the wire; 0 = the chain does not pack)
WIDTHS = [((1,), 1), ((2,), 2), ((3, 4), 4), ((4, 4), 5), ((65535, 65536), 32), ((65536, 65536), 33), ((16383, 16384, 8192), 41),
          ((65535, 65535, 65535, 65535), 64), ((65535, 65536, 65536, 65536), 64), ((65536, 65535, 65535, 65535), 0),
          ((65535, 65537, 65535, 65535), 0)]
# (the one-row index: a code of 0 bits, and the dense pipeline takes it — 1 bit per row, 0 = the row, 1 = absent)

# (shard rows, nchunks): chunk lengths 64 63 65 64 | 256 255 2048 2047 | 1 2049 | 257 256 0 0 2049 2048 | 1 0 1024 1024 0 0
SHARDS = [((127, 129), 2), ((511, 4095), 2), ((1, 2049), 1), ((513, 0, 4097), 2), ((1, 2048, 0), 2)]


def wire_bytes(world, rows, nchunks, bits):
    """Bytes a rank sends: whole groups of 64 rows, an even number of 64-bit words per non-empty chunk, to every peer
    (the wire format of csvplus_amd/dist.py: pack_rows)."""
    total = 0
    for c in range(nchunks):
        n = rows // nchunks + (1 if c < rows % nchunks else 0)
        if n:
            total += ((-(-n // 64)) * bits + 1) & ~1
    return 8 * (world - 1) * total


@functools.lru_cache(maxsize=None)
def table(n, seed):
    """%08d ids 0 .. n-1 in shuffled row order."""
    rng = np.random.default_rng(1000 + seed)
    col = StrCol.from_values([b"%08d" % int(i) for i in rng.permutation(n)])
    return col, orc.OracleIndex([col])


def stream_columns(rows, m, misses, seed):
    """One fixed-width key column per step for m stream rows.  misses: about a third of the rows do not join — a ninth
    at step 0, the others at one later step only (step 0 for a chain of one step)."""
    rng = np.random.default_rng(seed)
    ids = [rng.integers(0, n, m) for n in rows]
    if misses:
        who = rng.integers(0, 9, m)
        late = 1 + rng.integers(0, max(1, len(rows) - 1), m)                # the one later step at which such a row misses
        for k, n in enumerate(rows):
            if len(rows) == 1:
                at = who < 3
            else:
                at = (who == 0) if k == 0 else ((who == 1) | (who == 2)) & (late == k)
            ids[k] = np.where(at, n + rng.integers(0, 5, m), ids[k])      # an id just past the table
    return [StrCol.from_values([b"%08d" % int(i) for i in col]) for col in ids]


def rank_indexes(ctx, rows):
    gix = [DeviceIndex(ctx, [table(n, k)[0]], unique=True) for k, n in enumerate(rows)]
    for g, n in zip(gix, rows):
        assert g.status == N.CPH_OK and g.nrows == n
    return gix


def check_gathered(g, es, erows, perms, positions, m, shards, all_join):
    assert g.total == len(es) and sum(g.counts) == g.total and len(g.counts) == len(shards)
    assert g.identity == all_join
    first = 0
    if g.identity:
        assert g.stream_base == 0 and g.total == m and g.counts == list(shards) and g.narrays == len(erows)
    else:
        assert g.narrays == len(erows) + 1
        np.testing.assert_array_equal(gathered_array(g, 0, np.uint64), es)
        first = 1
    got = [gathered_array(g, first + k, np.uint32) for k in range(len(erows))]
    for k in range(len(erows)):
        np.testing.assert_array_equal(perms[k][got[k]] if positions else got[k], erows[k])
    return ([gathered_array(g, 0, np.uint64)] if first else []) + got


@pytest.mark.parametrize("misses", [False, True], ids=["all_join", "third_miss"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("rows,bits", WIDTHS, ids=["+".join(map(str, r)) for r, _ in WIDTHS])
def test_packed_exchange_width_edges(rows, bits, world, misses):
    """all_join: every stream row joins (identity: the slots are the result, no absent code in flight).  third_miss: about a
    third do not, some at step 0 and some at a later step only — k_mark_absent must have run before the pack, and whatever
    sits in the later arrays of a row that did not join must not leak."""
    shard_sets = [s for s in SHARDS if len(s[0]) == world]
    oix = [table(n, k)[1] for k, n in enumerate(rows)]
    work = []
    for shards, nchunks in shard_sets:
        m = sum(shards)
        cols = stream_columns(rows, m, misses, seed=m + misses)
        es, erows = oracle_chain(oix, cols)
        assert (len(es) == m) if not misses else (0 < len(es) < m)
        work.append((shards, nchunks, cols, es.astype(np.uint64), erows))

    def rank_body(r):
        ctx = Context(0)
        ctx.set_option("pool_guard", 1)
        d = loopback_factory("widths-" + "-".join(map(str, rows)) + f"-w{world}-{int(misses)}", world)(ctx, r)
        gix = rank_indexes(ctx, rows)
        perms = [g.perm() for g in gix]
        failures = []
        for shards, nchunks, cols, es, erows in work:
            b = sum(shards[:r])
            e = b + shards[r]
            steps = [(g, [c.slice(b, e)]) for g, c in zip(gix, cols)]
            for positions in (False, True):
                got = {}
                for packed in (False, True):   # every rank makes the same calls in the same order, whatever it finds
                    g = d.join_chain(steps, probe_base=b, shard_rows=list(shards), nchunks=nchunks, positions=positions, packed=packed)
                    ctx.synchronize()
                    try:
                        assert g.stats["chunks"] == nchunks and g.mem == N.CPH_MEM_DEVICE, g.stats
                        assert g.stats["packed_bits"] == (bits if packed else 0), g.stats
                        if packed and bits:
                            assert g.stats["bytes_sent"] == wire_bytes(world, shards[r], nchunks, bits), g.stats
                        got[packed] = check_gathered(g, es, erows, perms, positions, sum(shards), shards, not misses)
                    except Exception as err:   # noqa: BLE001 — a rank that stopped here would leave the others waiting for it
                        failures.append(((shards, nchunks, misses, positions, packed), err))
                    g.release()
                if len(got) == 2:
                    for x, y in zip(got[False], got[True]):
                        if not np.array_equal(x, y):
                            failures.append(((shards, nchunks, misses, positions), "packed != plain"))
        d.close()
        try:
            ctx.set_option("pool_guard_check", 0)
        finally:
            ctx.close()
        assert not failures, failures[:3]

    run_ranks(world, rank_body)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("shards", [(511, 513), (1, 2049, 0)], ids=["511+513", "1+2049+0"])
def test_plain_dense_pipeline_rank_boundaries_inside_a_slot_wave(shards, host):
    """The unpacked dense pipeline with misses: the ranks' slots meet inside a 512-slot wave of k_slots_count /
    k_slots_compact (slot 511 is rank 0's last, slot 1 is rank 1's first)."""
    rows, world, m = (16383, 16384, 8192), len(shards), sum(shards)
    oix = [table(n, k)[1] for k, n in enumerate(rows)]
    cols = stream_columns(rows, m, True, seed=77)
    es, erows = oracle_chain(oix, cols)
    es = es.astype(np.uint64)
    assert 0 < len(es) < m

    def rank_body(r):
        ctx = Context(0)
        ctx.set_option("pool_guard", 1)
        d = loopback_factory("plain-" + "-".join(map(str, shards)) + f"-{int(host)}", world)(ctx, r)
        gix = rank_indexes(ctx, rows)
        perms = [g.perm() for g in gix]
        b = sum(shards[:r])
        steps = [(g, [c.slice(b, b + shards[r])]) for g, c in zip(gix, cols)]
        failures = []
        for positions in (False, True):
            for nchunks in (1, 2):
                g = d.join_chain(steps, probe_base=b, shard_rows=list(shards), nchunks=nchunks, positions=positions, host=host)
                ctx.synchronize()
                try:
                    assert g.stats["chunks"] == nchunks and g.stats["packed_bits"] == 0, g.stats
                    assert g.mem == (N.CPH_MEM_HOST if host else N.CPH_MEM_DEVICE)
                    check_gathered(g, es, erows, perms, positions, m, shards, False)
                except Exception as err:   # noqa: BLE001 — as above
                    failures.append(((positions, nchunks), err))
                g.release()
        d.close()
        try:
            ctx.set_option("pool_guard_check", 0)
        finally:
            ctx.close()
        assert not failures, failures[:3]

    run_ranks(world, rank_body)
