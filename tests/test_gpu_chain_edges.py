"""Row-count edges of every fused chain-Join path (chain.hip) against the oracle's nested joins, bit for bit.

The geometry under test: a wave ballots 64 rows (kWave), the R = 4 instantiations walk a wave's rows in parts of 256, a wave
owns 512 consecutive rows (kWaveTile), a workgroup tile is 2048 rows (kChainTile).  Stream lengths sit on, one below and one
above each of these; the hit patterns put the miss on the last row, on every row but the last / the first, and on both ends
of every ballot word, at every step of the chain in turn.  Each family is named by the host decision in enqueue_dense /
run_fast that selects its kernel; where the library exposes nothing that tells two instantiations apart, both settings of
the option run and must give the oracle's result.

Everything runs on a ctx of this module with the pool's canaries on (pool_guard), checked at the end of every test: a store
one row past the stream, or one mask / count word too far, is reported instead of being lost in the pool's slack.
"""
import contextlib
import functools

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc
from tests.test_gpu_chain import oracle_chain
from tests.test_gpu_chain_sources import oracle_chain_sources, take_rows

pytestmark = pytest.mark.gpu

M_ALL = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 511)
M_FEW = (1, 65, 257, 513, 2049, 4097)
P_ALL = "abcdef"
P_FEW = "abce"
MASTER = M_ALL[-1]
DEFAULTS = {"chain_arith": 1, "chain_identity": 1, "chain_rank_lds": 1, "chain_rows4": 1, "chain_nt_streams": 0,
            "chain_prejoin": 1}


def miss_rows(pattern, m):
    """True where the row must not join."""
    r = np.arange(m)
    return {"a": np.zeros(m, bool), "b": r == m - 1, "c": r != m - 1, "d": r != 0,
            "e": (r % 64 == 0) | (r % 64 == 63), "f": np.ones(m, bool)}[pattern]


# ---- build tables and the master columns of the streams that ask for them ---------------------------------------------------
def fixed8(vals):
    col = StrCol.from_values(vals)
    assert col.fixed_width == 8
    return col


def var32(vals):
    return StrCol.from_values(vals).as_variable()


def var64(vals):
    return StrCol.from_values(vals, offset_bits=64).as_variable()


class Side:
    """One build table (a single key column) and two master columns of MASTER rows for the stream: hit[i] is a key of the
    table, miss[i] is not (the kinds rotate so that both ends of a ballot word meet every kind).  special = keys that must
    occur among the hits (rows 0, 50, 100, ...)."""

    def __init__(self, name, keys, miss_kinds, col=var32, build_col=None, special=(), seed=1):
        assert len(set(keys)) == len(keys)
        self.name, self.keys, self.col = name, list(keys), col
        self.build_col = (build_col or col)(self.keys)
        rng = np.random.default_rng(seed)
        self.hit = [self.keys[int(j)] for j in rng.integers(0, len(self.keys), MASTER)]
        for n, k in enumerate(special):
            for i in range(50 * n, MASTER, 50 * len(special)):
                self.hit[i] = k
        self.miss = [miss_kinds[(i + i // 64) % len(miss_kinds)](i) for i in range(MASTER)]
        have = set(self.keys)
        assert not any(v in have for v in self.miss), name

    @functools.cached_property
    def oracle(self):
        return orc.OracleIndex([self.build_col])


def _id_side(name, n, seed, extra_miss=()):
    """%08d ids 0 .. n-1 in shuffled order, n = d * 10^k: every code of the code space occurs.  Such a stream can only miss
    with a symbol outside an alphabet."""
    rng = np.random.default_rng(seed)
    digits = len(str(n - 1))
    lead = b"0" * (8 - digits)
    kinds = [lambda i: b"%08d" % (n + i % (10 ** digits - n)),                           # leading digit beyond its alphabet
             lambda i: lead[:-1] + b"1" + b"%0*d" % (digits, i % n) if lead else b"%07d:" % (i % 10 ** 7),
             lambda i: (b"%08d" % (i % n))[:7] + b":",                                    # just above '9'
             lambda i: (b"%08d" % (i % n))[:7] + b"/",                                    # just below '0'
             lambda i: (b"%08d" % (i % n))[:6] + b"\x80" + b"%d" % (i % 10),
             lambda i: b"\x00" + (b"%08d" % (i % n))[1:]]
    return Side(name, [b"%08d" % int(i) for i in rng.permutation(n)], kinds + list(extra_miss), col=fixed8, seed=seed)


def _sparse_id_side(name, radices, keep, seed):
    """%08d ids whose last digits run over 0 .. radix-1 each: prod(radices) codes, of which about `keep` are index keys —
    the first and the last code among them, the one before the last not."""
    rng = np.random.default_rng(seed)
    combos = [b""]
    for r in radices:
        combos = [c + b"%d" % d for c in combos for d in range(r)]
    lead = b"0" * (8 - len(radices))
    allk = [lead + c for c in combos]
    pick = rng.random(len(allk)) < keep
    pick[0] = pick[-1] = True
    pick[-2] = False
    keys = [k for k, p in zip(allk, pick) if p]
    gone = [k for k, p in zip(allk, pick) if not p]
    for pos in range(8):
        assert {k[pos] for k in keys} == {k[pos] for k in allk}          # every alphabet is complete
    order = rng.permutation(len(keys))
    kinds = [lambda i: gone[i % len(gone)],                                # inside the alphabets, absent
             lambda i: gone[-1 - i % 40],                                  # ... in the last rank blocks
             lambda i: lead + b"%d" % radices[0] + allk[i % len(allk)][len(lead) + 1:],   # digit just beyond its alphabet
             lambda i: allk[i % len(allk)][:7] + b":",
             lambda i: b"1" + allk[i % len(allk)][1:]]
    s = Side(name, [keys[int(j)] for j in order], kinds, col=fixed8, special=(allk[-1], allk[0], keys[-2]), seed=seed)
    s.states = len(allk)
    return s


def _var_side(name, fmt, domain, keep, seed, col=var32, build_col=None, longer=b"9"):
    """Variable-length keys fmt % id for `keep` of the ids below `domain`.  Misses: an id that is not there, a symbol outside
    the alphabet, a value longer than every key, the empty value."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(domain)
    keys = [fmt % int(i) for i in ids[:keep]]
    gone = [fmt % int(i) for i in ids[keep:]]
    maxlen = max(len(k) for k in keys)
    kinds = [lambda i: gone[i % len(gone)],
             lambda i: keys[i % len(keys)][:-1] + b"x",
             lambda i: (keys[i % len(keys)] + longer * maxlen)[:maxlen + 1 + i % 3],     # over-long by 1..3 bytes
             lambda i: b"X" + keys[i % len(keys)][1:],
             lambda i: gone[-1 - i % len(gone)]]
    if b"" not in keys:
        kinds.append(lambda i: b"")
    return Side(name, keys, kinds, col=col, build_col=build_col or var32, seed=seed)


def _letters_side(name, n, seed):
    """Random keys of 6..9 lower-case letters: a sparse code space (no direct table), codes wider than 32 bits."""
    rng = np.random.default_rng(seed)
    def word(lo, hi, alpha=26):
        return bytes(rng.integers(97, 97 + alpha, int(rng.integers(lo, hi + 1))).astype(np.uint8))
    pool = sorted({word(6, 9) for _ in range(2 * n)})
    order = rng.permutation(len(pool))
    keys = [pool[int(j)] for j in order[:n]]
    gone = [pool[int(j)] for j in order[n:]]
    kinds = [lambda i: gone[i % len(gone)],
             lambda i: keys[i % len(keys)][:-1] + b"0",
             lambda i: (keys[i % len(keys)] + b"zzzz")[:10 + i % 2],
             lambda i: keys[i % len(keys)][:5]]                               # shorter than every key
    return Side(name, keys, kinds, seed=seed)


@functools.lru_cache(maxsize=None)
def side(name):
    if name == "id4000":
        return _id_side(name, 4000, 11)
    if name == "id300":
        return _id_side(name, 300, 12)
    if name == "id20000":
        return _id_side(name, 20000, 13)
    if name == "id70":
        return _id_side(name, 70, 14)
    if name == "sparse2625":       # 3 * 5 * 5 * 5 * 7 = 2625 = 41 * 64 + 1 codes: the last rank block holds one code
        return _sparse_id_side(name, (3, 5, 5, 5, 7), 0.6, 15)
    if name == "sparse60000":
        return _sparse_id_side(name, (6, 10, 10, 10, 10), 0.6, 16)
    if name == "kvar":             # variable length: never lean
        return _var_side(name, b"k%d", 3000, 2000, 17)
    if name.startswith("itoa"):    # unpadded decimal ids of at most 4 bytes
        dom = int(name[4:])
        return _var_side(name, b"%d", dom, dom * 3 // 4, 18 + dom)
    if name == "wide1000":
        return _var_side(name, b"%d", 1000, 750, 31, col=var64)
    if name == "wide300":
        return _var_side(name, b"w%d", 300, 200, 32, col=var64)
    if name == "long13":           # keys of 10 .. 13 bytes
        return _var_side(name, b"order-id:%d", 5000, 4000, 33)
    if name == "long16":           # keys of 14 .. 16 bytes
        return _var_side(name, b"order-number:%d", 1000, 700, 34)
    if name == "long13w":
        return _var_side(name, b"order-id:%d", 5000, 4000, 35, col=var64)
    if name == "letters":
        return _letters_side(name, 3000, 36)
    raise KeyError(name)


# ---- the ctx of this module ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ectx():
    c = Context(0)
    c.set_option("pool_guard", 1)
    yield c
    c.close()


_built = {}


def device_index(ctx, s: Side):
    """One DeviceIndex per build table and ctx for the whole module."""
    key = (id(ctx), s.name)
    if key not in _built:
        ix = DeviceIndex(ctx, [s.build_col])
        assert ix.status == N.CPH_OK and ix.first_dup is None, (s.name, ix.status)
        _built[key] = ix
    return _built[key]


@contextlib.contextmanager
def options(ctx, **kv):
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kv:
            ctx.set_option(k, DEFAULTS[k])


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        out = fn()
        prof = ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)
    return out, prof


def assert_fused(prof):
    assert "k_chain_dense" in prof and not any(k.startswith("k_probe") for k in prof), sorted(prof)


_perms = {}


def perm_of(g):
    if id(g) not in _perms:
        _perms[id(g)] = (g, g.perm())
    return _perms[id(g)][1]


def compare(ch, gix, es, erows, m, positions, what):
    assert ch.positions == positions, what
    assert ch.nrows == len(es), what
    assert ch.identity == (len(es) == m), what          # every row joined: no stream_row array, and exactly m rows — a
                                                        # clamped lane that re-reads the last row is not a row
    np.testing.assert_array_equal(ch.stream_row, es, err_msg=str(what))
    for k, g in enumerate(gix):
        got = ch.build_row(k)
        if positions:
            assert len(got) == 0 or int(got.max()) < g.nrows, what
            got = perm_of(g)[got]
        np.testing.assert_array_equal(got, erows[k], err_msg=str(what))
    ch.release()


def cases(sizes, patterns, nsteps):
    for m in sizes:
        for p in patterns:
            for ms in ([0] if p == "a" else range(nsteps)):
                yield m, p, ms


def run_family(ctx, names, sizes, patterns, probe_base=0):
    """The chain over the build tables `names`, keyed by the stream, at every (length, pattern, step that misses)."""
    sides = [side(n) for n in names]
    gix = [device_index(ctx, s) for s in sides]
    oix = [s.oracle for s in sides]
    ncases = 0
    for m, p, ms in cases(sizes, patterns, len(sides)):
        miss = miss_rows(p, m)
        cols = [s.col([s.miss[i] if (k == ms and miss[i]) else s.hit[i] for i in range(m)]) for k, s in enumerate(sides)]
        es, erows = oracle_chain(oix, cols, probe_base)
        assert len(es) == m - int(miss.sum())                    # the oracle agrees about what misses
        for positions in (False, True):
            steps = [(g, [c]) for g, c in zip(gix, cols)]
            ch, prof = profiled(ctx, lambda: join_chain(ctx, steps, probe_base=probe_base, positions=positions))
            assert_fused(prof)
            compare(ch, gix, es, erows, m, positions, (names, m, p, ms, positions))
        ncases += 1
    return ncases


def info_is(ix, **want):
    inf = ix.info()
    assert {k: inf[k] for k in want} == want, inf


# ---- 1. lean identity: %08d ids that fill their code space ---------------------------------------------------------------------
def check_identity_tables(ctx, names):
    for n in names:
        s = side(n)
        ix = device_index(ctx, s)
        info_is(ix, direct_table=1, table_entries=len(s.keys), key_bytes=4, key_positions=8)
        assert ix.nrows == len(s.keys)


def test_lean_identity_two_steps_every_edge(ectx):
    """The benchmark's shape: two lean steps, both answered from the code itself.  All lengths x all patterns."""
    check_identity_tables(ectx, ("id4000", "id300"))
    run_family(ectx, ("id4000", "id300"), M_ALL, P_ALL, probe_base=3)
    ectx.set_option("pool_guard_check", 0)


@pytest.mark.parametrize("names", [("id4000",), ("id4000", "kvar"), ("kvar", "id4000"), ("id4000", "id300", "id20000"),
                                   ("id4000", "id300", "id20000", "id70")],
                         ids=["s1", "mask01", "mask10", "s3", "s4"])
def test_lean_identity_other_chains(ectx, names):
    """One lean step; two steps of which the first / the second alone is lean; three and four lean steps."""
    check_identity_tables(ectx, [n for n in names if n.startswith("id")])
    run_family(ectx, names, M_FEW, P_FEW)
    ectx.set_option("pool_guard_check", 0)


# ---- 2. lean, rank table in LDS / in global memory ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rank_lds", [1, 0], ids=["lds", "global"])
@pytest.mark.parametrize("names", [("sparse2625",), ("sparse60000", "sparse2625"), ("sparse2625", "id300")],
                         ids=["s1", "s2", "rank_then_identity"])
def test_lean_rank_table(ectx, names, rank_lds):
    """Sparse %08d ids: the sorted position comes from the rank table.  Nothing the library exposes says where the table
    sat, so both settings of chain_rank_lds run and both must give the oracle's result."""
    for n in names:
        if n.startswith("sparse"):
            s = side(n)
            info_is(device_index(ectx, s), direct_table=1, table_entries=s.states, key_bytes=4, key_positions=8)
    assert side("sparse2625").states % 64 == 1
    with options(ectx, chain_rank_lds=rank_lds):
        run_family(ectx, names, M_FEW, P_FEW, probe_base=1)
    ectx.set_option("pool_guard_check", 0)


# ---- 3. the same tables through the general kernel (LUT walk, 12-byte rank pairs in LDS, row table in row-id mode) -------------------------
@pytest.mark.parametrize("names", [("id4000", "id300"), ("sparse2625",), ("sparse60000", "sparse2625"),
                                   ("id4000", "id300", "id20000", "id70")], ids=["identity_s2", "rank_s1", "rank_s2", "identity_s4"])
@pytest.mark.parametrize("rank_lds", [1, 0], ids=["lds", "global"])
def test_lean_tables_through_the_general_kernel(ectx, names, rank_lds):
    with options(ectx, chain_arith=0, chain_identity=0, chain_rank_lds=rank_lds):
        run_family(ectx, names, M_FEW, P_FEW)
    ectx.set_option("pool_guard_check", 0)


# ---- 4. variable-length keys of at most 8 bytes --------------------------------------------------------------------------------------
ITOA = ("itoa1000", "itoa2000", "itoa3000", "itoa4000")


def check_short_tables(ctx, names):
    for n in names:
        ix = device_index(ctx, side(n))
        inf = ix.info()
        assert inf["direct_table"] == 1 and inf["key_bytes"] == 4 and inf["key_positions"] <= 8 and inf["code_bits"] <= 32, inf


def test_short_keys_two_steps_every_edge(ectx):
    """The general twin of the benchmark's shape.  All lengths x all patterns."""
    check_short_tables(ectx, ITOA[:2])
    run_family(ectx, ITOA[:2], M_ALL, P_ALL, probe_base=5)
    ectx.set_option("pool_guard_check", 0)


@pytest.mark.parametrize("nsteps,rows4,nt", [(s, r, t) for s in (1, 2, 3, 4) for r in (0, 1, 2) for t in (0, 1) if (s, r, t) != (2, 1, 0)],
                         ids=lambda v: str(v))
def test_short_keys_rows_per_lane_and_nt_streams(ectx, nsteps, rows4, nt):
    """chain_rows4 = 2 walks a wave's rows in two parts of 256 (R = 4), 0 in one of 512 (R = 8); the default takes R = 4 from
    four steps on; chain_nt_streams = 1 loads the stream and stores the results non-temporally.  No observable tells the
    instantiations apart: every setting must give the oracle's result.  (Two steps at the defaults: the test above.)"""
    check_short_tables(ectx, ITOA[:nsteps])
    with options(ectx, chain_rows4=rows4, chain_nt_streams=nt):
        run_family(ectx, ITOA[:nsteps], M_FEW, P_FEW)
    ectx.set_option("pool_guard_check", 0)


# ---- 5. LONG keys, WIDE offsets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("long13",), ("long16", "itoa1000"), ("wide1000",), ("wide1000", "wide300"),
                                   ("long13w", "wide300"), ("long13w", "wide300", "itoa1000")],
                         ids=["long_s1", "long_s2", "wide_s1", "wide_s2", "long_wide_s2", "long_wide_s3"])
@pytest.mark.parametrize("rows4", [1, 0], ids=["default", "r8"])
def test_long_keys_and_wide_offsets(ectx, names, rows4):
    """Index keys of 9 .. 16 bytes (bytes 8 .. 15 are prefetched), stream columns with 64-bit offsets, and both: two such
    steps take R = 4 by default, chain_rows4 = 0 sends them through R = 8."""
    for n in names:
        inf = device_index(ectx, side(n)).info()
        if n.startswith("long"):
            assert 9 <= inf["key_positions"] <= 16, inf
            assert min(len(k) for k in side(n).keys) >= 9
        else:
            assert inf["key_positions"] <= 8, inf
        if n.startswith("wide") or n.endswith("w"):
            assert side(n).col([b"1"]).offset_bits == 64
    with options(ectx, chain_rows4=rows4):
        run_family(ectx, names, M_FEW, P_FEW, probe_base=2)
    ectx.set_option("pool_guard_check", 0)


# ---- 6. sparse code space: hash probe / sorted search inside the fused kernel ------------------------------------------------------------
@pytest.mark.parametrize("join_hash", [1, 0], ids=["hash", "search"])
@pytest.mark.parametrize("names", [("letters",), ("letters", "itoa1000")], ids=["s1", "s2"])
def test_sparse_code_space(names, join_hash):
    ctx = Context(0)                 # the lookup structure is chosen when the index is first joined: a ctx of its own
    ctx.set_option("pool_guard", 1)
    ctx.set_option("join_hash", join_hash)
    try:
        ix = device_index(ctx, side("letters"))
        info_is(ix, direct_table=0, table_entries=0, key_bytes=8)
        run_family(ctx, names, M_FEW, P_FEW)
        inf = ix.info()
        assert (inf["hash_mode"] != 0) == bool(join_hash) and (inf["hash_bytes"] != 0) == bool(join_hash), inf
        ctx.set_option("pool_guard_check", 0)
    finally:
        for k in [k for k in _built if k[0] == id(ctx)]:
            _built.pop(k).close()
        ctx.close()


# ---- 7. a step keyed by an earlier build table ---------------------------------------------------------------------------------------
class SourceChain:
    """stream -> A (stream key) -> B (key = column `region` of the A row that matched) [-> C (stream key)].  A has 32 rows:
    the region of the first 20 is a key of B, the others name a region that is absent, has a symbol outside the alphabet or
    is too long."""

    def __init__(self):
        rng = np.random.default_rng(51)
        ids = rng.permutation(40)
        self.a_id = [b"c%d" % int(i) for i in ids[:32]]
        self.a_gone = [b"c%d" % int(i) for i in ids[32:]] + [b"cx", b"c123", b"", b"d1"]
        reg = rng.permutation(30)
        self.b_id = [b"r%d" % int(i) for i in reg[:24]]
        bad = [b"r%d" % int(i) for i in reg[24:]] + [b"rX", b"r123", b"", b"r1x", b"q2", b"r100"]
        self.a_region = [self.b_id[int(j)] for j in rng.integers(0, 24, 20)] + bad
        assert len(self.a_region) == 32
        self.good = self.a_id[:20]
        self.badrow = self.a_id[20:]
        self.h = [self.good[int(j)] for j in rng.integers(0, 20, MASTER)]
        self.x0 = [self.a_gone[(i + i // 64) % len(self.a_gone)] for i in range(MASTER)]
        self.x1 = [self.badrow[(i + i // 64) % len(self.badrow)] for i in range(MASTER)]
        self.A, self.B = var32(self.a_id), var32(self.b_id)
        self.region = var32(self.a_region)
        self.oracle = [orc.OracleIndex([self.A]), orc.OracleIndex([self.B])]


@pytest.mark.parametrize("third", [False, True], ids=["s2", "s3"])
@pytest.mark.parametrize("prejoin", [1, 0], ids=["prejoined", "dep"])
def test_step_keyed_by_an_earlier_build_table(ectx, prejoin, third):
    """chain_prejoin = 1 and a stream at least twice as long as table A: the build sides are joined with each other first
    and k_chain_prejoined answers the step with one gather; shorter streams and chain_prejoin = 0 take the DEP kernel."""
    sc = SourceChain()
    ga, gb = DeviceIndex(ectx, [sc.A]), DeviceIndex(ectx, [sc.B])
    assert ga.first_dup is None and gb.first_dup is None and ga.nrows == 32
    gix, oix = [ga, gb], list(sc.oracle)
    c_side = side("itoa1000")
    if third:
        gix.append(device_index(ectx, c_side))
        oix.append(c_side.oracle)
    perm_a = ga.perm()
    with options(ectx, chain_prejoin=prejoin):
        for m, p, ms in cases(M_FEW, P_FEW, len(gix)):
            miss = miss_rows(p, m)
            x = [sc.x0, sc.x1, None][ms]
            s_a = var32([x[i] if (x is not None and miss[i]) else sc.h[i] for i in range(m)])
            osteps = [([s_a], 0), ([sc.region], 1)]
            if third:
                osteps.append(([c_side.col([c_side.miss[i] if (ms == 2 and miss[i]) else c_side.hit[i] for i in range(m)])], 0))
            es, erows = oracle_chain_sources(oix, osteps, 9)
            assert len(es) == m - int(miss.sum())
            sorted_region = take_rows(sc.region, perm_a)               # the same column in A's sorted order: source -1
            for positions, region, src in ((False, sc.region, 1), (True, sc.region, 1), (True, sorted_region, -1)):
                steps = [(g, c, s) for g, (c, s) in zip(gix, osteps)]
                steps[1] = (gb, [region], src)
                ch, prof = profiled(ectx, lambda: join_chain(ectx, steps, probe_base=9, positions=positions))
                assert_fused(prof)
                assert ("k_chain_prejoined" in prof) == (bool(prejoin) and m >= 2 * ga.nrows), (m, sorted(prof))
                compare(ch, gix, es, erows, m, positions, ("source", m, p, ms, positions, src))
    ga.close()
    gb.close()
    ectx.set_option("pool_guard_check", 0)


# ---- 8. k_chain_codes: the dense pass over key codes the host formed -------------------------------------------------------------------
@pytest.mark.parametrize("positions", [False, True], ids=["rows", "positions"])
def test_host_formed_codes(ectx, positions):
    """StreamJoin.submit_codes with chunks of every length of M_ALL.  Where a row must miss, the host hands over the code of
    an absent key, CPH_CODE_ABSENT, or a code equal to table_entries (one past the table).  A stream join runs its chunks
    on slot contexts of its own, which the ctx's profile does not see: chunk["dense"] is what says that the codes went
    through the dense pass (submit_codes has no other)."""
    from csvplus_amd.streaming import HostEncoder, StreamJoin, bitmap_to_rows

    sides = [side("id4000"), side("sparse2625"), side("itoa1000")]
    gix = [device_index(ectx, s) for s in sides]
    oix = [s.oracle for s in sides]
    entries = [g.info()["table_entries"] for g in gix]
    assert entries[0] == 4000 and entries[1] == 2625 and entries[2] > 0
    encs = [HostEncoder(g, nthreads=1) for g in gix]
    perms = [g.perm() for g in gix]
    sj = StreamJoin(ectx, gix, nslots=2, positions=positions)
    base = 0
    for m, p, ms in cases(M_ALL, "bce", 3):
        miss = miss_rows(p, m)
        cols = [s.col([s.miss[i] if (k == ms and miss[i]) else s.hit[i] for i in range(m)]) for k, s in enumerate(sides)]
        es, erows = oracle_chain(oix, cols, base)
        assert len(es) == m - int(miss.sum())
        codes = [np.zeros(m, np.uint32) for _ in sides]
        for k in range(3):
            encs[k].run([cols[k]], codes[k])
        past = np.nonzero(miss)[0][::2]                   # every other missing row: one past the table instead
        codes[ms][past] = entries[ms]
        sj.submit_codes(codes, m, probe_base=base)
        r = sj.next()
        assert r["dense"] and r["nrows"] == m and r["probe_base"] == base and r["nmatches"] == len(es), (m, p, ms)
        hit = bitmap_to_rows(r["bitmap"], m)
        np.testing.assert_array_equal(hit.astype(np.uint64) + base, es, err_msg=str((m, p, ms)))
        assert not np.unpackbits(r["bitmap"].view(np.uint8), bitorder="little")[m:].any(), (m, p, ms)   # no bit past the chunk
        for k in range(3):
            got = r["build_row"][k][hit]
            np.testing.assert_array_equal(perms[k][got] if positions else got, erows[k], err_msg=str((m, p, ms, k)))
        base += m
    sj.close()
    for e in encs:
        e.close()
    ectx.set_option("pool_guard_check", 0)
