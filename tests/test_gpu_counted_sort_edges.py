"""The counted window sort of 32-bit codes with duplicates (counted_sort.hip: k_cs_hist, k_cs_scan, k_cs_partition<1|2>,
k_cs_window; index_build.hip: sort_codes_after_overflow) at its row, width, level, capacity and group-size edges.

Tables have 2^21 rows or a few more: the smallest counted_sort_plan takes.  Keys are fixed-width with exactly r_p distinct
bytes at position p, all present (tests/test_gpu_window_sort_edges.py: Space, restated_codes), at most 8 bytes long:
positions of 16 symbols ('a' .. 'p') give the powers of two, "the first product-form code space above / below x" is the
nearest integer whose prime factors are all <= 61.  The restated codes only place rows on edges; the reference is numpy's
stable argsort over the key bytes read as big-endian integers, the first duplicate from that order, np.searchsorted over
the sorted keys for the probes — and, for the smallest table, oracle.orc.OracleIndex agrees with it.

Statistics sampling: a one-column fixed-width table of 2^20 rows and more takes its alphabets from every 32nd row
(codec_sample_applies).  The planted rows of these tables (one giant key, groups at chosen codes) are scattered at
random, not laid on that stride, so the module's ctx runs with stats_sample 0: the exact statistics pass, one attempt.
host_build is 0 (the host-coded path has its own file).  Both options and every switch a test flips are set back in a
`finally`.  The ctx runs with pool_guard 1 and is checked after every test.
"""
import collections
import functools

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, _native as N
from oracle import orc
from tests.test_gpu_code_widths import _profiled, bits_needed, classic_passes, plan_table_entries
from tests.test_gpu_window_sort_edges import (Space, column, direct_sort_applies, launches, lookup, prime_factors, reference_of,
                                              restated_codes)

SEED = 20260520

# ---- the library's rules, restated (counted_sort.hip, index_build.hip) -------------------------------------------------
CS_TILE = 8192               # kCsTile: rows / entries per partition tile
CS_THREADS = 512             # kCsThreads
CS_MAX_BUCKETS = 2048        # kCsMaxBuckets: buckets one partition tile tracks
CS_CAP = 16384               # kCsCap: rows one window workgroup holds
CS_MAX_WBITS, CS_MIN_WBITS = 11, 3
CS_MAX_WINDOWS = 32768       # kCsMaxWindows
CS_SMALL_GROUP = 32          # kCsSmallGroup: up to here ranked by counting, beyond by a wave's bitonic network
CS_MIN_ROWS = 1 << 21
NARROWER_ATTEMPTS = 2        # resort_overflowed

Plan = collections.namedtuple("Plan", "wbits two k2 nb1 nwt nwin")


def counted_sort_plan(n, states, max_wbits=31, min_rows=CS_MIN_ROWS, counted_sort=1):
    if not counted_sort or n < min_rows or n == 0 or n >= (1 << 32) - 1 or states == 0 or states >= 0xFFFFFFFF:
        return None
    w = min(max_wbits, CS_MAX_WBITS)
    while w >= CS_MIN_WBITS and float(n) / float(states) * float(1 << w) > 0.72 * float(CS_CAP):
        w -= 1
    if w < CS_MIN_WBITS:
        return None
    nwin = (states + (1 << w) - 1) >> w
    if nwin > CS_MAX_WINDOWS:
        return None
    wb = 0
    while (1 << wb) < nwin:
        wb += 1
    two = nwin > CS_MAX_BUCKETS
    k2 = (wb + 1) // 2 if two else 0
    nb1 = (nwin + (1 << k2) - 1) >> k2
    nwt = nb1 << k2
    return Plan(w, two, k2, nb1, nwt, nwin) if nb1 <= CS_MAX_BUCKETS and nwt <= 2 * CS_MAX_WINDOWS else None


def plans_tried(n, states):
    """The first plan and the narrower ones sort_codes_after_overflow may try behind it (None first: no counted sort)."""
    first = counted_sort_plan(n, states)
    if first is None:
        return []
    out, wb = [first], first.wbits
    for _ in range(NARROWER_ATTEMPTS):
        wb -= 2
        if wb <= 0:
            break
        p = counted_sort_plan(n, states, wb)
        if p is None or p.wbits != wb:
            break
        out.append(p)
    return out


def expected_path(codes, states):
    """(plans whose kernels run, True when the last of them sorts the table / False: the classic passes do)."""
    plans = plans_tried(len(codes), states)
    for i, p in enumerate(plans):
        if np.bincount(codes >> p.wbits).max() <= CS_CAP:
            return plans[:i + 1], True
    return plans, False


def level2_buckets(plan):
    """CountedSort::partition: the buckets a level-2 tile tracks in LDS."""
    return min(CS_MAX_BUCKETS, (2 * (1 << plan.k2) + CS_THREADS - 1) // CS_THREADS * CS_THREADS)


def level1_bases(codes, plan):
    """base1 of k_cs_scan: where every level-1 bucket's entries begin."""
    per = np.bincount(codes >> (plan.wbits + plan.k2), minlength=plan.nb1)
    return np.concatenate([[0], np.cumsum(per)])


# ---- key families --------------------------------------------------------------------------------------------------------
def product_form(states):
    radix = []
    for p in sorted(prime_factors(states), reverse=True):
        assert p <= 61
        if radix and radix[-1] * p < 64:
            radix[-1] *= p
        else:
            radix.append(p)
    return Space(radix, ord("0"))


def nearest_product_form(x, step):
    y = x + step
    while max(prime_factors(y)) > 61:
        y += step
    return y


def pow2(b):
    return Space(([1 << (b % 4)] if b % 4 else []) + [16] * (b // 4), ord("a"))


BELOW_W3 = nearest_product_form(1423, -1)
ABOVE_ONE_LEVEL = nearest_product_form(1 << 22, 1)
ABOVE_ALL = nearest_product_form(1 << 26, 1)

ROWS = CS_MIN_ROWS + 3
ROW_EDGES = (CS_MIN_ROWS - 1, CS_MIN_ROWS, CS_MIN_ROWS + 1, CS_MIN_ROWS + CS_TILE - 1)
CAP_WINDOW = 100             # case 4: the window (of 2048 codes, states 2^20) that is filled to the brim
GROUP_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 4096, 4097)
LAST_W = 2047                # the last window of 2^22 codes under wbits 11
# case 5: where each group sits — (window, code inside the window)
GROUP_AT = {1: (0, 5), 2: (0, 2047), 31: (3, 0), 32: (3, 1), 33: (3, 2047), 63: (1000, 7), 64: (1000, 2047), 65: (1001, 0),
            128: (1500, 100), 129: (LAST_W, 2047), 4096: (LAST_W, 0), 4097: (700, 1)}
DUP_LATER_WINDOW = 1234
EMPTY_BUCKETS = (60, 61)     # case 7: level-1 buckets (2^19 codes each under states 2^26) without a row
ROWS_BELOW_GAP = 120 * CS_TILE

Table = collections.namedtuple("Table", "name space codes data col")


def _table(name, space, codes):
    data = space.keys(codes)
    return Table(name, space, np.asarray(codes, np.int64), data, column(data))


def _uniform(rng, n, states, avoid=()):
    """n codes, uniform over the space without the codes in `avoid`."""
    c = rng.integers(0, states, n)
    avoid = np.asarray(sorted(avoid), np.int64)
    while avoid.size:
        hit = np.isin(c, avoid)
        if not hit.any():
            break
        c[hit] = rng.integers(0, states, int(hit.sum()))
    return c


def _distinct(rng, n, states):
    c = np.unique(rng.integers(0, states, n + n // 2))
    assert len(c) >= n
    return rng.permutation(c)[:n]


@functools.lru_cache(maxsize=2)
def fixture(name):
    rng = np.random.default_rng([SEED, sum(name.encode())])
    if name.startswith("rows-"):             # case 1 (and the widest window, wbits 11): the same rows, cut at the edges
        n = int(name[5:])
        return _table(name, pow2(20), np.random.default_rng([SEED, 1]).integers(0, 1 << 20, ROW_EDGES[-1])[:n])
    if name == "width-3":                    # 8 codes per window, about 1024 rows per code: every group beyond 32
        return _table(name, pow2(11), rng.integers(0, 1 << 11, ROWS))
    if name == "width-8":
        return _table(name, pow2(16), rng.integers(0, 1 << 16, ROWS))
    if name == "below-width-3":
        return _table(name, product_form(BELOW_W3), rng.integers(0, BELOW_W3, CS_MIN_ROWS))
    if name == "one-level-max":
        return _table(name, pow2(22), rng.integers(0, 1 << 22, ROWS))
    if name == "two-levels-first":
        return _table(name, product_form(ABOVE_ONE_LEVEL), rng.integers(0, ABOVE_ONE_LEVEL, ROWS))
    if name == "two-levels-max":
        return _table(name, pow2(26), rng.integers(0, 1 << 26, ROWS))
    if name == "no-plan":
        return _table(name, product_form(ABOVE_ALL), rng.integers(0, ABOVE_ALL, CS_MIN_ROWS))
    if name in ("cap-exact", "cap-plus-one"):  # 8 rows on every code of one window, one more on one of them
        inside = (CAP_WINDOW << 11) + np.repeat(np.arange(2048), 8)
        if name == "cap-plus-one":
            inside = np.append(inside, (CAP_WINDOW << 11) + 777)
        rest = rng.integers(0, (1 << 20) - 2048, ROWS - len(inside))
        rest[rest >= CAP_WINDOW << 11] += 2048
        return _table(name, pow2(20), rng.permutation(np.concatenate([inside, rest])))
    if name == "cap-one-key-fits":           # one key fills a window on its own: the widest bitonic network (16384 slots)
        rest = rng.integers(0, (1 << 20) - 2048, ROWS - CS_CAP)
        rest[rest >= CAP_WINDOW << 11] += 2048
        return _table(name, pow2(20), rng.permutation(np.concatenate([np.full(CS_CAP, (CAP_WINDOW << 11) + 777), rest])))
    if name == "cap-one-key":
        key = (CAP_WINDOW << 11) + 777
        codes = np.concatenate([np.full(CS_CAP + 1, key), _uniform(rng, ROWS - CS_CAP - 1, 1 << 20, avoid=[key])])
        return _table(name, pow2(20), rng.permutation(codes))
    if name == "groups":
        at = {s: (w << 11) + c for s, (w, c) in GROUP_AT.items()}
        planted = np.concatenate([np.full(s, at[s]) for s in GROUP_SIZES])
        codes = np.concatenate([planted, _uniform(rng, ROWS - len(planted), 1 << 22, avoid=at.values())])
        return _table(name, pow2(22), rng.permutation(codes))
    if name.startswith("firstdup-"):
        codes = _distinct(np.random.default_rng([SEED, 2]), ROWS, 1 << 22)
        s = np.sort(codes)
        where = name[9:]
        if where != "none":
            key = {"first": s[0], "later-window": s[s >= DUP_LATER_WINDOW << 11][0], "last": s[-1]}[where]
            spare = int(np.flatnonzero((codes != s[0]) & (codes != s[-1]) & (codes >> 11 != DUP_LATER_WINDOW))[1000])
            codes[spare] = key
        return _table(name, pow2(22), codes)
    if name == "sparse-tiles":               # a dense block in the first 2^22 codes and a thin spread over the other 15/16
        codes = np.concatenate([rng.integers(0, 1 << 22, ROWS - 40_000), rng.integers(1 << 22, 1 << 26, 40_000)])
        return _table(name, pow2(26), rng.permutation(codes))
    if name == "empty-buckets":              # no row in two level-1 buckets; the tile behind them starts exactly at their base
        lo, hi = EMPTY_BUCKETS[0] << 19, (EMPTY_BUCKETS[-1] + 1) << 19
        codes = np.concatenate([rng.integers(0, lo, ROWS_BELOW_GAP), rng.integers(hi, 1 << 26, ROWS - ROWS_BELOW_GAP)])
        return _table(name, pow2(26), rng.permutation(codes))
    raise KeyError(name)


@functools.lru_cache(maxsize=2)
def reference(name):
    return reference_of(fixture(name).data)


ROW_CASES = tuple("rows-%d" % n for n in ROW_EDGES)
WIDTH_CASES = ("width-3", "width-8", "below-width-3")
LEVEL_CASES = ("one-level-max", "two-levels-first", "two-levels-max", "no-plan")
CAP_CASES = ("cap-exact", "cap-plus-one", "cap-one-key-fits", "cap-one-key")
FIRSTDUP_CASES = ("firstdup-first", "firstdup-later-window", "firstdup-last", "firstdup-none")
LEVEL2_CASES = ("sparse-tiles", "empty-buckets")
ALL_CASES = ROW_CASES + WIDTH_CASES + LEVEL_CASES + CAP_CASES + ("groups",) + FIRSTDUP_CASES + LEVEL2_CASES


def group_sizes(codes, states):
    return np.bincount(codes, minlength=states)


# ---- the CPU test: the restated plan, and every fixture on the edge it claims -----------------------------------------------
def test_counted_sort_fixtures_sit_on_their_edges():
    n = CS_MIN_ROWS
    # the plan at 2^21 rows
    assert counted_sort_plan(n, 1422) is None and counted_sort_plan(n, 1423).wbits == 3 and counted_sort_plan(n, 2844).wbits == 3
    assert counted_sort_plan(n, 2845).wbits == 4 and counted_sort_plan(n, 364088).wbits == 10 and counted_sort_plan(n, 364089).wbits == 11
    assert counted_sort_plan(n, 1 << 22) == Plan(11, False, 0, 2048, 2048, 2048)
    assert counted_sort_plan(n, (1 << 22) + 1).two and counted_sort_plan(n, 129 << 15)[:5] == (11, True, 6, 33, 33 << 6)
    assert counted_sort_plan(n, 1 << 26) == Plan(11, True, 8, 128, 32768, 32768) and counted_sort_plan(n, (1 << 26) + 1) is None
    assert counted_sort_plan(n - 1, 1 << 20) is None and counted_sort_plan(n, 1 << 20, counted_sort=0) is None
    assert (BELOW_W3, ABOVE_ONE_LEVEL, ABOVE_ALL) == (1421, nearest_product_form(1 << 22, 1), nearest_product_form(1 << 26, 1))
    assert all(max(prime_factors(y)) > 61 for y in list(range((1 << 22) + 1, ABOVE_ONE_LEVEL)) + [1422])
    shape, path, codes_of = {}, {}, {}
    for name in ALL_CASES:
        t = fixture(name)
        radix, codes = restated_codes(t.data)
        assert radix == t.space.radix and np.array_equal(codes, t.codes), name   # every symbol present; the code is the rank
        assert t.data.shape[1] <= 8 and t.space.states <= 1 << 32, name
        shape[name], path[name], codes_of[name] = (len(t.codes), t.space.states), expected_path(t.codes, t.space.states), t.codes.astype(np.int32)
    kernels = {name: ([(p.wbits, 2 if p.two else 1) for p in path[name][0]], path[name][1]) for name in ALL_CASES}
    # case 1: rows
    assert [shape[c] for c in ROW_CASES] == [(n - 1, 1 << 20), (n, 1 << 20), (n + 1, 1 << 20), (n + 8191, 1 << 20)]
    assert kernels[ROW_CASES[0]] == ([], False) and all(kernels[c] == ([(11, 1)], True) for c in ROW_CASES[1:])
    assert [(shape[c][0] - 1) // CS_TILE + 1 for c in ROW_CASES] == [256, 256, 257, 257] and [shape[c][0] % CS_TILE for c in ROW_CASES[2:]] == [1, 8191]
    # case 2: widths
    assert kernels["width-3"] == ([(3, 1)], True) and kernels["width-8"] == ([(8, 1)], True) and kernels["below-width-3"] == ([], False)
    assert group_sizes(codes_of["width-3"], 2048).min() > CS_SMALL_GROUP and shape["below-width-3"][1] == 1421
    # case 3: levels
    assert kernels["one-level-max"] == ([(11, 1)], True) and path["one-level-max"][0][0].nwin == CS_MAX_BUCKETS
    assert kernels["two-levels-first"] == ([(11, 2)], True) and path["two-levels-first"][0][0].nwin == CS_MAX_BUCKETS + 1
    assert kernels["two-levels-max"] == ([(11, 2)], True) and path["two-levels-max"][0][0][:5] == (11, True, 8, 128, 32768)
    assert kernels["no-plan"] == ([], False) and shape["no-plan"][1] > 1 << 26 and bits_needed(shape["no-plan"][1]) == 27
    # case 4: capacity.  cap-one-key: every narrower plan overflows too — three k_cs_scan launches, then the classic passes
    per = {c: np.bincount(codes_of[c] >> 11, minlength=512) for c in CAP_CASES}
    assert per["cap-exact"][CAP_WINDOW] == CS_CAP and per["cap-plus-one"][CAP_WINDOW] == CS_CAP + 1
    assert np.delete(per["cap-exact"], CAP_WINDOW).max() < CS_CAP // 2 and np.delete(per["cap-plus-one"], CAP_WINDOW).max() < CS_CAP // 2
    assert group_sizes(codes_of["cap-plus-one"], 1 << 20)[CAP_WINDOW << 11: (CAP_WINDOW + 1) << 11].max() == 9
    assert group_sizes(codes_of["cap-one-key"], 1 << 20).max() == CS_CAP + 1
    assert group_sizes(codes_of["cap-one-key-fits"], 1 << 20).max() == CS_CAP == per["cap-one-key-fits"][CAP_WINDOW] and kernels["cap-one-key-fits"] == ([(11, 1)], True)
    assert kernels["cap-exact"] == ([(11, 1)], True) and kernels["cap-plus-one"] == ([(11, 1), (9, 1)], True)
    assert kernels["cap-one-key"] == ([(11, 1), (9, 1), (7, 2)], False)
    # case 5: the groups, exactly, where they are said to be, their rows all over the table
    g = codes_of["groups"]
    sizes = group_sizes(g, 1 << 22)
    for s, (w, c) in GROUP_AT.items():
        code = (w << 11) + c
        assert sizes[code] == s, s
        rows = np.flatnonzero(g == code)
        assert s < 31 or (rows.min() < ROWS // 4 and rows.max() > 3 * ROWS // 4 and not np.array_equal(rows, np.arange(rows[0], rows[0] + s))), s
    assert tuple(sorted(GROUP_AT)) == GROUP_SIZES and kernels["groups"] == ([(11, 1)], True)
    assert {c for _, c in GROUP_AT.values()} >= {0, 2047} and {w for w, _ in GROUP_AT.values()} >= {0, LAST_W}
    assert np.bincount(g >> 11).max() < CS_CAP
    # case 6: one duplicate pair (or none), and where it sorts to
    for name, first_dup in zip(FIRSTDUP_CASES, (1, None, ROWS - 1, None)):
        c = codes_of[name]
        sizes = np.bincount(c)
        assert sizes.max() == (1 if name == "firstdup-none" else 2) and (sizes == 2).sum() == (0 if name == "firstdup-none" else 1), name
        if name != "firstdup-none":
            at = int(np.searchsorted(np.sort(c), np.flatnonzero(sizes == 2)[0])) + 1
            assert first_dup in (None, at), name
            if name == "firstdup-later-window":   # the first key of its window
                key = int(np.flatnonzero(sizes == 2)[0])
                assert key >> 11 == DUP_LATER_WINDOW and not sizes[DUP_LATER_WINDOW << 11: key].any() and 1 < at < ROWS - 1
        assert kernels[name] == ([(11, 1)], True) and direct_sort_applies(True, *shape[name]), name
    # case 7: level 2 — a tile that spans more windows than it tracks; a tile that starts where two empty buckets do
    for name in LEVEL2_CASES:
        plan = path[name][0][0]
        assert kernels[name] == ([(11, 2)], True) and plan.k2 == 8 and level2_buckets(plan) == 512, name
    assert {level2_buckets(counted_sort_plan(n, s)) for s in ((1 << 22) + 1, ABOVE_ONE_LEVEL, 129 << 15, 1 << 24, 1 << 26)} == {512}
    c, plan = codes_of["sparse-tiles"], path["sparse-tiles"][0][0]
    base1 = level1_bases(c, plan)
    starts = np.arange(0, len(c), CS_TILE)
    first_bucket = np.searchsorted(base1[:plan.nb1], starts, "right") - 1          # the largest sb with base1[sb] <= t0
    last_entry = np.minimum(starts + CS_TILE, len(c)) - 1
    last_bucket = np.searchsorted(base1[:plan.nb1], last_entry, "right") - 1
    assert (last_bucket - first_bucket).max() >= 2   # windows at least 2 << k2 = 512 = nbk behind the tile's first: the per-entry path
    assert np.bincount(c >> 11).max() < CS_CAP
    plan = path["empty-buckets"][0][0]
    base1 = level1_bases(codes_of["empty-buckets"], plan)
    e0, e1 = EMPTY_BUCKETS
    assert e1 == e0 + 1 and 0 < e0 and e1 < plan.nb1 - 1
    assert base1[e0] == base1[e1] == base1[e1 + 1] == ROWS_BELOW_GAP and ROWS_BELOW_GAP % CS_TILE == 0 and base1[e0 - 1] < base1[e0] < base1[e1 + 2]
    # the anchor: numpy's reference is the oracle's on the smallest table the counted sort takes
    t, ref = fixture(ROW_CASES[1]), reference(ROW_CASES[1])
    o = orc.OracleIndex([t.col])
    assert np.array_equal(o.perm, ref.perm) and o.first_dup() == ref.first_dup


# ---- the gpu checks --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gctx():
    c = Context(0)
    c.set_option("pool_guard", 1)
    c.set_option("host_build", 0)
    c.set_option("stats_sample", 0)
    try:
        yield c
    finally:
        c.set_option("stats_sample", 1)
        c.set_option("host_build", 1)
        c.set_option("pool_guard_check", 0)   # raises CphError when a canary behind a device block was overwritten
        c.close()


def probe_keys(t, rng):
    """Keys on the edges of the windows (under the first plan's width, or 2048 codes), rows of the table, absent codes and
    keys outside the alphabets; few enough that the pairs stay in the low millions."""
    n, states = len(t.codes), t.space.states
    plan = counted_sort_plan(n, states)
    wbits = plan.wbits if plan else CS_MAX_WBITS
    count = max(16, min(1000, 500_000 // max(1, n // states)))
    w = rng.integers(0, (states + (1 << wbits) - 1) >> wbits, count)
    edges = np.concatenate([w << wbits, np.minimum((w << wbits) + (1 << wbits) - 1, states - 1), [0, states - 1]])
    codes = np.concatenate([edges, t.codes[rng.integers(0, n, count)], rng.integers(0, states, count)])
    data = t.space.keys(codes)
    foreign = t.data[:8].copy()
    foreign[:4, -1], foreign[4:, 0] = ord("z"), ord("!")
    return np.concatenate([data, foreign])


def check_probe(g, t, ref, label):
    rng = np.random.default_rng([SEED, 5])
    probes = probe_keys(t, rng)
    lo, hi = lookup(ref, probes)
    cnt = hi - lo
    total = int(cnt.sum())
    starts = np.cumsum(cnt) - cnt
    pos = np.repeat(lo, cnt) + (np.arange(total) - np.repeat(starts, cnt))
    m = g.probe([column(probes)])
    try:
        assert m.nmatches == total and (cnt == 0).any() and total > 0, label
        assert np.array_equal(m.cnt, cnt), label
        assert np.array_equal(m.probe_idx, np.repeat(np.arange(len(probes)), cnt)), label
        assert np.array_equal(m.build_row, ref.perm[pos]), label
    finally:
        m.release()


def check_build(ctx, t, ref, unique=False, counted=1, probe=True):
    """One build: the reference's permutation and first duplicate; with unique=False also the proof of the path."""
    n, states = len(t.codes), t.space.states
    label = (t.name, unique, counted)
    try:
        ctx.set_option("counted_sort", counted)
        g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, [t.col], unique=unique))
    finally:
        ctx.set_option("counted_sort", 1)
    try:
        assert np.array_equal(g.perm(), ref.perm), label
        assert g.first_dup == ref.first_dup, (label, g.first_dup, ref.first_dup)
        assert g.status == (N.CPH_ERR_DUPLICATE if unique and ref.first_dup is not None else N.CPH_OK), label
        info = g.info()
        assert (info["nrows"], info["code_bits"], info["code_words"], info["key_bytes"]) == (n, t.space.bits, 1, 4), (label, info)
        assert info["table_entries"] == plan_table_entries([states], n) and info["dict_entries"] == 0 and info["build_path"] == 0, (label, info)
        if not unique:
            plans, sorts = expected_path(t.codes, states) if counted else ([], False)
            assert launches(prof, "k_cs_scan") == launches(prof, "k_cs_hist") == launches(prof, "k_cs_window") == len(plans), (label, sorted(prof))
            assert launches(prof, "k_cs_partition") == sum(2 if p.two else 1 for p in plans), (label, prof.get("k_cs_partition"))
            assert not [k for k in prof if k.startswith("k_win_")], (label, sorted(prof))
            if sorts:
                assert not [k for k in prof if k.startswith("k_radix_scatter")] and info["sort_passes"] == 0, (label, sorted(prof), info)
            else:
                assert launches(prof, "k_radix_scatter_u32") == info["sort_passes"] == classic_passes([states]), (label, sorted(prof), info)
        if probe:
            check_probe(g, t, ref, label)
    finally:
        g.close()
    return prof


def check_both_ways(ctx, name, unique_too=False):
    t, ref = fixture(name), reference(name)
    check_build(ctx, t, ref)
    check_build(ctx, t, ref, counted=0, probe=False)
    if unique_too:
        check_build(ctx, t, ref, unique=True, probe=False)
        check_build(ctx, t, ref, unique=True, counted=0, probe=False)
    ctx.set_option("pool_guard_check", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_CASES)
def test_row_threshold_and_tiles(gctx, name):
    """Case 1: one row under counted_sort_plan's threshold (classic passes), on it, one row and 8191 rows in a last tile."""
    check_both_ways(gctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDTH_CASES)
def test_window_widths(gctx, name):
    """Case 2: 8 codes per window (every group beyond 32 rows: the bitonic network alone), 256 codes per window, and the
    first code space too small for any window (classic passes).  2048 codes per window: every other case."""
    check_both_ways(gctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEVEL_CASES)
def test_partition_levels(gctx, name):
    """Case 3: 2048 windows (one level), 2049 (two), 32768 (the most), and the first code space beyond (classic passes)."""
    check_both_ways(gctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CAP_CASES)
def test_window_capacity(gctx, name):
    """Case 4: a window of exactly 16384 rows fits (one k_cs_scan), also when they are ONE key (a bitonic network as wide as
    the window); 16385 rows over many keys are sorted by the narrower retry (two); one key of 16385 rows overflows every
    retry (three) and the classic passes sort the same codes."""
    check_both_ways(gctx, name)


@pytest.mark.gpu
def test_group_sizes_keep_input_order(gctx):
    """Case 5: groups of 1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 4096 and 4097 rows scattered over the table, on the first
    and the last code of a window, in the first and the last window: every group in input order."""
    t, ref = fixture("groups"), reference("groups")
    check_both_ways(gctx, "groups")
    for s, (w, c) in GROUP_AT.items():   # (implied by the comparison above; said once more per group, for the message)
        rows = np.flatnonzero(t.codes == (w << 11) + c)
        at = int(np.searchsorted(t.codes[ref.perm], (w << 11) + c))
        assert np.array_equal(ref.perm[at:at + s], rows), s


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIRSTDUP_CASES)
def test_first_duplicate(gctx, name):
    """Case 6: the only duplicate pair on the very first key, on the first key of a later window, on the last two rows, and
    none at all; IndexOn and UniqueIndexOn, counted windows and classic passes."""
    ref = reference(name)
    assert ref.first_dup == {"firstdup-first": 1, "firstdup-last": ROWS - 1, "firstdup-none": None}.get(name, ref.first_dup)
    assert (ref.first_dup is None) == (name == "firstdup-none")
    check_both_ways(gctx, name, unique_too=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEVEL2_CASES)
def test_level_two_sparse_tiles_and_empty_buckets(gctx, name):
    """Case 7: level-2 tiles that span more windows than they track (one atomic per entry), and a level-2 tile that starts
    exactly where two empty level-1 buckets and the bucket behind them begin (the search over equal base1 entries)."""
    check_both_ways(gctx, name)
