"""The direct sort of distinct keys through LDS windows (window_sort.hip: k_win_partition, k_win_offsets, k_win_place) at
its window, tile and threshold edges, one partition level (two levels need 16.7 million rows: tests/test_gpu_window_sort.py).

Key families.  Fixed-width keys whose byte position p holds exactly r_p distinct values, all of them present: the code
space is states = prod r_p and a key's code is its mixed-radix rank (tests/test_gpu_code_widths.py: PyCodec, restated
here in numpy as `restated_codes`).  Binary alphabets {a, b} give states = 2^b (b = 16, 17, 18: 4, 8, 16 windows of
2^14 codes); {a, b, c} over 11 positions gives 3^11 = 177147, no multiple of 16384, 64 or 32; zero-padded decimal ids
of 8 bytes give the arithmetic codec and with it the pass that codes the keys itself (k_win_partition<2>).  "The first
product-form code space above x" is the first integer above x all of whose prime factors are at most 61 (one position
per prime factor, neighbours merged while the product stays below 64: the symbols stay below 0x80).

The restated codes only PLACE rows on edges.  The reference is independent of them: np.argsort(kind="stable") /
np.lexsort over the key bytes read as big-endian integers, the first duplicate from that order, np.searchsorted over the
sorted keys for Find and Join; every table's reference is also compared with oracle.orc.OracleIndex.

Statistics sampling: codec_sample_applies takes tables of 2^20 rows and more; every table here is smaller, so the exact
statistics pass runs whatever stats_sample says and no fixture has to keep its symbols on a sample's stride.  host_build
is 0 throughout (the host-coded path has its own file).

All GPU cases run on a Context of this module with pool_guard 1 (canaries behind every device block, checked after
every test): a store past perm, the sorted codes or an entry buffer is reported, not survived.
"""
import collections
import functools
import math

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc
from tests.test_gpu_code_widths import PyCodec, _profiled, bits_needed, plan_table_entries, split_words

SEED = 20260519

# ---- the library's rules, restated (window_sort.hip, index_build.hip, cph_internal.hpp) ------------------------------
WIN_BITS = 14
WIN = 1 << WIN_BITS          # kWinSlots: codes per window
TILE = 8192                  # kWpTile: rows per partition tile (1024 threads x 8 rows on one level)
MAX_BUCKETS = 2048           # kWpMaxBuckets: windows of one partition level
DIRECT_FROM = 1 << 16        # direct_sort_applies: rows
PLACE_ROUND = 2 * 4 * 512    # k_win_place: kRound = 2 entries x kPlaceLoads x kPlaceThreads per round


def direct_sort_applies(unique, n, states, direct_sort=1):
    return bool(unique and direct_sort and n >= DIRECT_FROM and n <= states <= 2 * n and states < 0xFFFFFFFF)


def windows_of(states):
    return (states + WIN - 1) >> WIN_BITS


def one_level(states):
    return windows_of(states) <= MAX_BUCKETS


def ranktab_blocks(states):
    """cph_internal.hpp: 32-code blocks, an even number of them."""
    return ((states + 31) // 32 + 1) & ~1


def ranktab_expected(states, n, direct_ranktab=1):
    """build_encode_sort: the window sort leaves the Join's rank table behind unless the code space is full."""
    return bool(direct_ranktab and states != n and states <= 1 << 30)


# ---- key families ------------------------------------------------------------------------------------------------------
def prime_factors(x):
    out, p = [], 2
    while p * p <= x:
        while x % p == 0:
            out.append(p)
            x //= p
        p += 1
    if x > 1:
        out.append(x)
    return out


def first_product_form_above(x):
    """(states, radix per position) of the first integer above x whose prime factors are all <= 61."""
    y = x + 1
    while max(prime_factors(y)) > 61:
        y += 1
    radix = []
    for p in sorted(prime_factors(y), reverse=True):
        if radix and radix[-1] * p < 64:
            radix[-1] *= p
        else:
            radix.append(p)
    assert math.prod(radix) == y
    return y, radix


class Space:
    """Fixed-width keys: position p holds the bytes base .. base + radix[p] - 1."""

    def __init__(self, radix, base):
        self.radix, self.base, self.npos = [int(r) for r in radix], base, len(radix)
        self.states = math.prod(self.radix)
        words, _ = split_words(self.radix)
        assert words == [self.states] and self.states <= 1 << 32 and base + max(self.radix) <= 0x80
        self.bits = bits_needed(self.states)

    def keys(self, codes):
        """(len(codes), npos) key bytes of the codes (mixed radix, position 0 most significant)."""
        c = np.asarray(codes, np.int64).copy()
        assert c.size == 0 or (0 <= c.min() and c.max() < self.states)
        out = np.empty((c.size, self.npos), np.uint8)
        for p in range(self.npos - 1, -1, -1):
            out[:, p] = self.base + c % self.radix[p]
            c //= self.radix[p]
        return out


def binary(b):
    return Space([2] * b, ord("a"))


TERNARY11 = Space([3] * 11, ord("a"))


def decimal8(states):
    """Zero-padded decimal ids 0 .. states - 1 in 8 bytes: states = d * 10^k, the leading positions constant."""
    k = len(str(states)) - 1
    assert states % 10 ** k == 0 and 2 <= states // 10 ** k <= 9
    return Space([1] * (8 - k - 1) + [states // 10 ** k] + [10] * k, ord("0"))


def restated_codes(data):
    """The radix rule (PyCodec, tests/test_gpu_code_widths.py) in numpy for fixed-width keys: per position the rank of
    the byte among the distinct bytes seen there.  -> (radix per position, code of every row)."""
    radix, code = [], np.zeros(len(data), np.int64)
    for p in range(data.shape[1]):
        present = np.bincount(data[:, p], minlength=256) > 0
        rank = np.cumsum(present) - 1
        radix.append(int(present.sum()))
        code = code * radix[-1] + rank[data[:, p]]
    return radix, code


def column(data):
    n, w = data.shape
    col = StrCol.from_arrays(np.ascontiguousarray(data).reshape(-1), (np.arange(n + 1, dtype=np.uint64) * w).astype(np.uint32),
                             fixed_width=w if w == 8 else None)
    assert col.fixed_width == w
    return col


# ---- the reference: numpy over the key bytes ---------------------------------------------------------------------------
def big_endian_words(data):
    """(n, nwords) uint64: the key bytes read as one big-endian integer, most significant word first."""
    n, w = data.shape
    nw = (w + 7) // 8
    padded = np.zeros((n, 8 * nw), np.uint8)
    padded[:, 8 * nw - w:] = data
    return padded.view(">u8").astype(np.uint64)


def stable_order(data):
    words = big_endian_words(data)
    if words.shape[1] == 1:
        return np.argsort(words[:, 0], kind="stable").astype(np.uint32)
    return np.lexsort(words[:, ::-1].T).astype(np.uint32)   # (lexsort: last key first, stable)


def as_strings(data):
    return np.ascontiguousarray(data).view("S%d" % data.shape[1]).reshape(-1)   # bytewise order == big-endian integer order (no NULs)


Ref = collections.namedtuple("Ref", "perm first_dup sorted_keys")


def reference_of(data):
    perm = stable_order(data)
    s = as_strings(data)[perm]
    dup = np.flatnonzero(s[1:] == s[:-1])
    perm.setflags(write=False)
    return Ref(perm, int(dup[0]) + 1 if dup.size else None, s)


def lookup(ref, probe_data):
    """np.searchsorted over the sorted keys: (lower, upper) sorted positions of every probe key."""
    p = as_strings(probe_data)
    return np.searchsorted(ref.sorted_keys, p, "left"), np.searchsorted(ref.sorted_keys, p, "right")


# ---- the tables --------------------------------------------------------------------------------------------------------
Table = collections.namedtuple("Table", "name space codes data col")


def table(name, space, codes):
    data = space.keys(codes)
    return Table(name, space, np.asarray(codes, np.int64), data, column(data))


def subset(space, n, seed, include=(), exclude=()):
    """n distinct codes of the space in random row order; `include` are in, `exclude` are not."""
    rng = np.random.default_rng([SEED, seed])
    pool = np.setdiff1d(np.arange(space.states), np.asarray(list(include) + list(exclude), np.int64))
    rest = rng.choice(pool, n - len(include), replace=False)
    return rng.permutation(np.concatenate([np.asarray(include, np.int64), rest]))


# case 3: the rows per window of one table over 2^18 codes (16 windows)
OCCUPANCY = (WIN, WIN - 1, PLACE_ROUND - 1, 0, PLACE_ROUND, 1, PLACE_ROUND + 1) + (10001,) * 9
EMPTY_WINDOW = OCCUPANCY.index(0)


def occupancy_codes(counts, seed):
    rng = np.random.default_rng([SEED, seed])
    parts = [(w << WIN_BITS) + rng.choice(WIN, c, replace=False) for w, c in enumerate(counts)]
    return rng.permutation(np.concatenate(parts).astype(np.int64))


def with_pair(codes, dst_row, src_row):
    out = codes.copy()
    out[dst_row] = out[src_row]
    return out


ABOVE_2N = first_product_form_above(2 * DIRECT_FROM)   # case 1: the first code space that is not direct at 65536 rows
FUSED_ROWS = ((65537, 70000), (73728, 80000), (73729, 80000), (65539, 70000))   # case 5: (rows, states)
TAIL_ROWS = 120_001


@functools.lru_cache(maxsize=None)
def fixture(name):
    b16, b17, b18 = binary(16), binary(17), binary(18)
    if name == "below-threshold":          # 65535 rows: one under direct_sort_applies
        return table(name, b16, subset(b16, DIRECT_FROM - 1, 1, include=(0, b16.states - 1)))
    if name == "full-4w":                  # states == n: off == nullptr, 4 windows, 8 whole tiles
        return table(name, b16, subset(b16, b16.states, 2))
    if name == "states-n+1":               # states == n + 1 (the code left out lies in the middle)
        return table(name, b17, subset(b17, b17.states - 1, 3, exclude=(70_000,)))
    if name == "states-2n":                # states == 2 n
        return table(name, b17, subset(b17, DIRECT_FROM, 4, include=(0, b17.states - 1)))
    if name == "above-2n":
        sp = Space(ABOVE_2N[1], ord("0"))
        return table(name, sp, subset(sp, DIRECT_FROM, 5, include=(0, sp.states - 1)))
    if name.startswith("tile-"):           # case 2: rows around the tile
        n = int(name[5:])
        return table(name, b17, subset(b17, n, 6, include=(0, b17.states - 1)))
    if name == "occupancy":
        return table(name, b18, occupancy_codes(OCCUPANCY, 7))
    if name == "primer":                   # random rows over the same space: about 12500 per window
        return table(name, b18, subset(b18, 200_000, 8))
    if name == "tail-with-max":
        return table(name, TERNARY11, subset(TERNARY11, TAIL_ROWS, 9, include=(0, TERNARY11.states - 1)))
    if name == "tail-without-max":
        return table(name, TERNARY11, subset(TERNARY11, TAIL_ROWS, 10, include=(0, TERNARY11.states - 2), exclude=(TERNARY11.states - 1,)))
    if name.startswith("fused-"):
        n, states = FUSED_ROWS[int(name[6:])]
        sp = decimal8(states)
        return table(name, sp, subset(sp, n, 11, include=(0, states - 1)))
    # case 6: duplicates over the 8-window table of 73727 rows
    base = fixture("tile-73727").codes
    if name == "dup-one-tile":             # rows 100 and 4000: tile 0
        return table(name, b17, with_pair(base, 4000, 100))
    if name == "dup-two-tiles":            # rows 100 (tile 0) and 5 * 8192 + 77 (tile 5)
        return table(name, b17, with_pair(base, 5 * TILE + 77, 100))
    if name == "dup-code-0":
        return table(name, b17, with_pair(base, 60_001, int(np.flatnonzero(base == 0)[0])))
    if name == "dup-code-max":
        return table(name, b17, with_pair(base, 60_001, int(np.flatnonzero(base == b17.states - 1)[0])))
    if name in ("dup-overflow-first", "dup-overflow-last"):   # a window's whole code range and more rows on top
        w = 0 if name.endswith("first") else windows_of(b17.states) - 1
        extra = 100 if w == 0 else 1
        rng = np.random.default_rng([SEED, 12, w])
        inside = (w << WIN_BITS) + np.arange(WIN)
        others = np.setdiff1d(np.arange(b17.states), inside)
        rows = np.concatenate([inside, rng.choice(inside, extra, replace=False), rng.choice(others, 73727 - WIN - extra, replace=False)])
        return table(name, b17, rng.permutation(rows.astype(np.int64)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(fixture(name).data)


TILE_ROWS = (8 * TILE + 1, 9 * TILE - 1, 70_002)                 # (8 * TILE itself: "full-4w")
DIRECT_CASES = ("full-4w", "states-n+1", "states-2n") + tuple("tile-%d" % n for n in TILE_ROWS)
DUP_CASES = ("dup-one-tile", "dup-two-tiles", "dup-code-0", "dup-code-max", "dup-overflow-first", "dup-overflow-last")
RANKTAB_CASES = ("occupancy", "tail-with-max", "tail-without-max")
FUSED_CASES = tuple("fused-%d" % i for i in range(len(FUSED_ROWS)))
CURSOR_ORDER = ("tile-73727", "dup-overflow-first", "full-4w", "occupancy")   # case 7
ALL_CASES = ("below-threshold", "above-2n", "primer") + DIRECT_CASES + RANKTAB_CASES + FUSED_CASES + DUP_CASES


def per_window(t):
    return np.bincount(t.codes >> WIN_BITS, minlength=windows_of(t.space.states))


# ---- the CPU test: every fixture sits on the edge it claims ---------------------------------------------------------------
def test_window_sort_fixtures_sit_on_their_edges():
    assert first_product_form_above(16)[0] == 17 and first_product_form_above(66)[0] == 68 and max(prime_factors(67 * 2)) == 67
    for name in ALL_CASES:
        t = fixture(name)
        radix, codes = restated_codes(t.data)
        assert radix == t.space.radix and np.array_equal(codes, t.codes), name   # every symbol present; the code is the rank
        assert one_level(t.space.states) and t.col.nrows == len(t.codes) < 1 << 20, name   # below the sample's threshold
        ref = reference(name)
        o = orc.OracleIndex([t.col])
        assert np.array_equal(o.perm, ref.perm) and o.first_dup() == ref.first_dup, name   # numpy's reference is the oracle's
        assert np.array_equal(t.codes[ref.perm], np.sort(t.codes, kind="stable")), name
        assert (ref.first_dup is not None) == name.startswith("dup-"), name
    small = fixture("fused-0")
    pc = PyCodec([[bytes(k) for k in small.data]])
    assert pc.radix == small.space.radix and [pc.encode((bytes(k),)) for k in small.data[:500]] == small.codes[:500].tolist()
    # case 1: the thresholds of direct_sort_applies
    shape = {name: (len(fixture(name).codes), fixture(name).space.states) for name in ALL_CASES}
    assert shape["below-threshold"] == (65535, 65536) and not direct_sort_applies(True, *shape["below-threshold"])
    assert shape["full-4w"] == (65536, 65536) and windows_of(65536) == 4
    assert shape["states-n+1"] == (131071, 131072) and shape["states-2n"] == (65536, 131072)
    assert ABOVE_2N[0] == shape["above-2n"][1] > 2 * 65536 and shape["above-2n"][0] == 65536
    assert all(max(prime_factors(y)) > 61 for y in range(2 * 65536 + 1, ABOVE_2N[0]))
    assert not direct_sort_applies(True, *shape["above-2n"]) and not direct_sort_applies(False, *shape["full-4w"])
    for name in DIRECT_CASES + RANKTAB_CASES + FUSED_CASES + DUP_CASES + ("primer",):
        n, states = shape[name]
        assert direct_sort_applies(True, n, states) and 65536 <= n <= states <= 2 * n, name
        assert plan_table_entries([states], n) == states, name
    # case 2: tiles of 8192 rows; the scalar tail (a last tile that is not whole) with n % 4 in {1, 2, 3}
    assert shape["full-4w"][0] == 8 * TILE and [n for n in TILE_ROWS] == [8 * TILE + 1, 9 * TILE - 1, 70_002]
    assert sorted(n % 4 for n in TILE_ROWS) == [1, 2, 3] and all(n % TILE for n in TILE_ROWS)
    assert all(windows_of(shape["tile-%d" % n][1]) == 8 for n in TILE_ROWS)
    # case 3: the rows per window
    occ = per_window(fixture("occupancy"))
    assert tuple(occ) == OCCUPANCY and len(occ) == 16 and PLACE_ROUND == 4096
    assert {WIN, WIN - 1, 4095, 4096, 4097, 1, 0} <= set(occ.tolist()) and 0 < EMPTY_WINDOW < 15 and any(c % 2 for c in occ)
    assert occ[EMPTY_WINDOW - 1] and occ[EMPTY_WINDOW + 1]
    prim = per_window(fixture("primer"))   # its entries lie behind the last entry of the odd windows of "occupancy"
    assert all(prim[w] > c for w, c in enumerate(OCCUPANCY) if c % 2 and c < WIN - 1) and prim.max() < WIN
    # case 4: the last window is partial, the rank table ends inside it
    states = TERNARY11.states
    assert states == 177147 and states % WIN and states % 64 and states % 32 and windows_of(states) == 11
    assert ranktab_blocks(states) < (windows_of(states) << WIN_BITS) // 32
    assert states - 1 in fixture("tail-with-max").codes and states - 1 not in fixture("tail-without-max").codes
    assert per_window(fixture("tail-with-max"))[-1] > 0 and per_window(fixture("tail-without-max"))[-1] > 0
    # case 5: 8-byte decimal ids, rows on the tile and off it by one, one table with n % 4 == 3
    assert [n for n, _ in FUSED_ROWS] == [65537, 73728, 73729, 65539] and 73728 == 9 * TILE and 65539 % 4 == 3
    for name in FUSED_CASES:
        t = fixture(name)
        assert t.data.shape[1] == 8 and t.col.fixed_width == 8 and t.space.states <= 1 << 31
        assert all(t.data[:, p].max() - t.data[:, p].min() + 1 == r for p, r in enumerate(t.space.radix))   # contiguous: codec_arith_plan
    # case 6: where the pairs are
    base = fixture("tile-73727")
    for name, rows in (("dup-one-tile", (100, 4000)), ("dup-two-tiles", (100, 5 * TILE + 77))):
        c = fixture(name).codes
        assert c[rows[0]] == c[rows[1]] and np.array_equal(np.delete(c, rows[1]), np.delete(base.codes, rows[1]))
    assert 100 // TILE == 4000 // TILE == 0 and (5 * TILE + 77) // TILE == 5
    assert (fixture("dup-code-0").codes == 0).sum() == 2 and (fixture("dup-code-max").codes == (1 << 17) - 1).sum() == 2
    assert reference("dup-code-0").first_dup == 1 and reference("dup-code-max").first_dup == 73726
    first, last = per_window(fixture("dup-overflow-first")), per_window(fixture("dup-overflow-last"))
    assert first[0] == WIN + 100 and last[-1] == WIN + 1 and len(last) == 8   # beyond the capacity; one entry AT the capacity
    # case 7: the order of the cursor test grows the cursor block at its end
    assert [windows_of(fixture(nm).space.states) for nm in CURSOR_ORDER] == [8, 8, 4, 16]


# ---- the gpu checks ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gctx():
    c = Context(0)
    c.set_option("pool_guard", 1)
    c.set_option("host_build", 0)
    try:
        yield c
    finally:
        c.set_option("host_build", 1)
        c.set_option("pool_guard_check", 0)   # raises CphError when a canary behind a device block was overwritten
        c.close()


def launches(prof, name):
    return prof[name]["launches"] if name in prof else 0


def assert_window_profile(prof, label):
    assert launches(prof, "k_win_partition") == 1 and "k_win_place" in prof, (label, sorted(prof))
    assert not [k for k in prof if k.startswith(("k_radix_scatter", "k_cs_"))], (label, sorted(prof))


def assert_info(g, t, label):
    info = g.info()
    n, states = len(t.codes), t.space.states
    assert (info["nrows"], info["code_bits"], info["code_words"], info["key_bytes"]) == (n, t.space.bits, 1, 4), (label, info)
    assert info["table_entries"] == plan_table_entries([states], n) and info["dict_entries"] == 0 and info["build_path"] == 0, (label, info)
    return info


def window_edge_keys(t):
    """First and last key present in two neighbouring windows that hold rows, and a key that is absent."""
    occ = per_window(t)
    w = next(w for w in range(len(occ) - 1) if occ[w] and occ[w + 1])
    keys = []
    for v in (w, w + 1):
        inside = t.codes[t.codes >> WIN_BITS == v]
        keys += [int(inside.min()), int(inside.max())]
    data = t.space.keys(keys)
    missing = np.setdiff1d(np.arange(min(t.space.states, 4 * WIN)), t.codes)[:1]
    absent = t.space.keys(missing) if missing.size else np.full((1, t.space.npos), ord("z"), np.uint8)
    return np.concatenate([data, absent])


def check_answers(g, t, ref, label):
    """Every key of the table probed (reads all of the sorted codes), Find across a window boundary."""
    lo, hi = lookup(ref, t.data)
    assert np.array_equal(hi - lo, np.ones(len(lo), np.int64))
    m = g.probe([t.col])
    try:
        assert m.nmatches == len(t.codes), label
        assert np.array_equal(m.probe_idx, np.arange(len(t.codes))), label
        assert np.array_equal(m.build_row, ref.perm[lo]), label
    finally:
        m.release()
    keys = window_edge_keys(t)
    klo, khi = lookup(ref, keys)
    assert list(khi - klo) == [1, 1, 1, 1, 0]
    for key, a, b in zip(keys, klo, khi):
        flo, fhi = g.find(bytes(key))
        assert fhi - flo == b - a and (a == b or flo == a), (label, bytes(key), (flo, fhi), (a, b))


def check_direct(ctx, t, ref, col=None):
    """One unique build that must go through the window sort and nothing else."""
    g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, [t.col if col is None else col], unique=True))
    try:
        assert np.array_equal(g.perm(), ref.perm), t.name
        assert g.first_dup is None and ref.first_dup is None and g.status == N.CPH_OK, t.name
        info = assert_info(g, t, t.name)
        assert_window_profile(prof, t.name)
        assert bool(info["lookup_built"] & 8) == ranktab_expected(t.space.states, len(t.codes)), (t.name, info)
        check_answers(g, t, ref, t.name)
    except BaseException:
        g.close()
        raise
    return g, prof


def check_not_direct(ctx, t, ref, unique):
    g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, [t.col], unique=unique))
    try:
        assert not [k for k in prof if k.startswith(("k_win_", "k_cs_"))] and "k_radix_scatter_u32" in prof, (t.name, sorted(prof))
        assert np.array_equal(g.perm(), ref.perm) and g.first_dup is None and g.status == N.CPH_OK, t.name
        assert_info(g, t, t.name)
        check_answers(g, t, ref, t.name)
    finally:
        g.close()


def check_duplicate(ctx, t, ref):
    """The optimistic sort notices, the general path builds the index and says where the first duplicate is."""
    g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, [t.col], unique=True))
    try:
        assert launches(prof, "k_win_partition") == 1 and "k_radix_scatter_u32" in prof, (t.name, sorted(prof))
        assert ref.first_dup is not None and g.first_dup == ref.first_dup and g.status == N.CPH_ERR_DUPLICATE, (t.name, g.first_dup, ref.first_dup)
        assert np.array_equal(g.perm(), ref.perm), t.name
        assert_info(g, t, t.name)
    finally:
        g.close()


@pytest.mark.gpu
def test_thresholds_of_the_direct_sort(gctx):
    """Case 1: one row under the threshold, the full code space (no offsets, no rank table), states == n + 1 and == 2 n
    (both direct, with offsets), the first code space above 2 n and a non-unique build (neither direct)."""
    check_not_direct(gctx, fixture("below-threshold"), reference("below-threshold"), True)
    for name in ("full-4w", "states-n+1", "states-2n"):
        g, prof = check_direct(gctx, fixture(name), reference(name))
        assert bool(g.info()["lookup_built"] & 8) == (name != "full-4w")
        assert prof["k_win_place"]["launches"] == (1 if name == "full-4w" else 2), (name, prof["k_win_place"])   # + k_win_offsets
        g.close()
    check_not_direct(gctx, fixture("above-2n"), reference("above-2n"), True)
    check_not_direct(gctx, fixture("full-4w"), reference("full-4w"), False)
    gctx.set_option("pool_guard_check", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TILE_ROWS)
def test_tile_edges_of_the_partition(gctx, n):
    """Case 2: one row in the last tile, one row short of a whole one, and a last tile whose row count is 2 modulo 4
    (8 whole tiles: the full table of case 1)."""
    name = "tile-%d" % n
    check_direct(gctx, fixture(name), reference(name))[0].close()
    gctx.set_option("pool_guard_check", 0)


def ranktab_probes(t):
    """Keys on the edges of the windows, of the 32- and 64-code blocks of the rank table, inside the empty window, the last
    code, and keys outside the alphabets."""
    rng = np.random.default_rng([SEED, 20])
    states, nwin = t.space.states, windows_of(t.space.states)
    codes = [np.arange(nwin) << WIN_BITS, np.minimum((np.arange(nwin) << WIN_BITS) + WIN - 1, states - 1)]
    blocks = rng.integers(0, states // 64 - 1, 400) * 64
    codes += [blocks, blocks + 31, blocks + 32, blocks + 63]
    if t.name == "occupancy":
        codes.append((EMPTY_WINDOW << WIN_BITS) + rng.integers(0, WIN, 200))
    codes += [np.array([states - 1, states - 2, 0, 1]), rng.integers(0, states, 2000), t.codes[:2000]]
    data = t.space.keys(np.concatenate(codes))
    foreign = t.data[:64].copy()
    foreign[:32, -1], foreign[32:, 0] = ord("z"), ord("`")
    return np.concatenate([data, foreign])[rng.permutation(len(data) + 64)]


def check_chain_positions(ctx, g, t, ref, probes):
    lo, hi = lookup(ref, probes)
    hit = np.flatnonzero(hi > lo)
    assert 0 < len(hit) < len(probes)
    ch = join_chain(ctx, [(g, [column(probes)])], positions=True)
    try:
        assert ch.positions and ch.nrows == len(hit), t.name
        assert np.array_equal(ch.stream_row, hit), t.name
        pos = ch.build_row(0)
        assert np.array_equal(pos, lo[hit]) and np.array_equal(g.perm()[pos], ref.perm[lo[hit]]), t.name
    finally:
        ch.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", RANKTAB_CASES)
def test_window_occupancy_tail_window_and_rank_table(gctx, name):
    """Cases 3, 4 and 8: windows that are full, one short, on either side of a round of k_win_place, odd, of one row and
    empty (behind a build that left entries where the odd windows' stale pair halves are read); a code space whose last
    window and last rank-table block are partial, with and without its last code.  The rank table the window sort leaves
    behind answers a Join that reports positions exactly like the one the Join builds itself."""
    t, ref = fixture(name), reference(name)
    if name == "occupancy":
        check_direct(gctx, fixture("primer"), reference("primer"))[0].close()
    g, _ = check_direct(gctx, t, ref)
    probes = ranktab_probes(t)
    try:
        assert g.info()["lookup_built"] & 8
        check_chain_positions(gctx, g, t, ref, probes)
        gctx.set_option("direct_ranktab", 0)
        g2 = DeviceIndex(gctx, [t.col], unique=True)
        try:
            assert not g2.info()["lookup_built"] & 8 and np.array_equal(g2.perm(), ref.perm)
            check_chain_positions(gctx, g2, t, ref, probes)
        finally:
            g2.close()
    finally:
        gctx.set_option("direct_ranktab", 1)
        g.close()
    gctx.set_option("pool_guard_check", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED_CASES)
def test_keys_coded_by_the_partition_pass(gctx, name):
    """Case 5: 8-byte decimal ids on the device, 16-byte aligned: k_win_partition<2> codes them itself (no k_encode_build);
    with direct_fused_encode 0 the encode kernel runs once.  The same permutation either way."""
    t, ref = fixture(name), reference(name)
    dcol = t.col.to_device("cuda:0")
    assert dcol.data.data_ptr() % 16 == 0
    perms = []
    try:
        for fused in (1, 0):
            gctx.set_option("direct_fused_encode", fused)
            g, prof = check_direct(gctx, t, ref, col=dcol)
            perms.append(g.perm())
            g.close()
            assert launches(prof, "k_encode_build") == (0 if fused else 1), (name, fused, sorted(prof))
    finally:
        gctx.set_option("direct_fused_encode", 1)
    assert np.array_equal(perms[0], perms[1])
    gctx.set_option("pool_guard_check", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DUP_CASES)
def test_duplicates_fall_back_to_the_general_path(gctx, name):
    """Case 6: a pair inside one tile, across tiles, on code 0 and on code states - 1; a window whose code range holds more
    rows than the window has slots (pos[k] >= cap), in the first window and — one row over — in the last, where an entry
    written AT the capacity would land behind the entry buffer (pool_guard)."""
    check_duplicate(gctx, fixture(name), reference(name))
    gctx.set_option("pool_guard_check", 0)


@pytest.mark.gpu
def test_cursors_are_zero_at_rest():
    """Case 7: the cursors are cleaned by k_win_place, not by a memset: a dense 8-window build, a build that overflows a
    window, a full 4-window build, a build with more windows than any before — every one the reference's, through the
    window sort (a cursor left behind shifts the next build's entries: wrong rows, or the flag and the general path)."""
    ctx = Context(0)
    try:
        ctx.set_option("pool_guard", 1)
        ctx.set_option("host_build", 0)
        for name in CURSOR_ORDER:
            if name.startswith("dup-"):
                check_duplicate(ctx, fixture(name), reference(name))
            else:
                check_direct(ctx, fixture(name), reference(name))[0].close()
        ctx.set_option("pool_guard_check", 0)
    finally:
        ctx.close()
