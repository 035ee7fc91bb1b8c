"""The general radix sort (radix_sort.hip, sort_words_lsd / sort_single_word in index_build.hip) where it can go wrong:
across tiles, across the XCD tile remap, through the digit stream, over 64-bit and several-word codes.

Every index build ends in this sort or can restart into it, and it carries the index contract that rows with equal keys
keep their input order — a sort that puts the KEYS in order but swaps equal ones passes every "perm is a permutation,
keys ascend" check.  So every case here compares the permutation bit for bit with oracle.orc.OracleIndex (a stable CPU
sort of the same rows, never the code under test) and proves from info() and the ctx profile that the radix passes —
and nothing else — produced it.

Key families: fixed-length keys over {a, b} with b positions have a code space of exactly b bits (binary alphabets are
immune to the dictionary stage, tests/test_gpu_code_widths.py).  b = 9, 27: 32-bit codes; 33, 40, 63: one 64-bit word;
65, 80: two words (63 + 2, 63 + 17); 127: THREE words (63 + 63 + 1 — codec_split_words closes a word at 2^63, so the
64 positions behind the first word do not fit one word).

Every table is built from: uniformly random keys; one key repeated over about half the rows, scattered (from the second
pass on its rows fill whole waves with peers, and at the larger sizes its digit bin is longer than a tile); and, for
several-word keys, one group of keys per word that differ in that word alone (an unstable pass over word 0 then breaks
the order the passes over the later words left, and the other way round).

What the library's own rules make of the cases (checked by the unmarked test, restated from radix_plan):
  * below 2^22 rows radix_plan takes 9-bit digits whenever they save a pass, and the digit stream only exists for 8-bit
    digits.  A 63-bit word (8 passes of 8 bits, 7 of 9) therefore never streams on the automatic setting; the digit
    stream cases of b = 63 and b = 80 run on the automatic setting (no stream: both settings must read the same bytes)
    AND under sort_rbits 8, where the 63-bit word streams — and so does the 17-bit word of b = 80 (3 passes of 8 bits).
  * a table whose rows are ALL equal has a code space of one state: no bits, no pass.  It is checked as such (the
    identity permutation, sort_passes 0), and next to it the table that is all equal but for ONE last row holding the
    complement key, which keeps the full code width.  A several-word key needs more: with two distinct keys the
    dictionary stage (codec_try_groups) recodes it into 11 bits, so those tables end in 256 other rows (four waves)
    and every wave in front of them is still full of peers in every pass.
"""
import collections
import contextlib
import functools

import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol, _native as N
from oracle import orc
from tests import test_gpu_group_scan as group_scan
from tests.test_gpu_code_widths import _profiled, bits_needed, classic_passes, dictionary_pays, premultiplied_bits, split_words

SEED = 20260407

# ---- the library's rules, restated (radix_sort.hip, cph_internal.hpp) ------------------------------------------------
SORT_ITEMS = 16            # kSortItems: keys per thread
WIDE_BELOW = 1 << 22       # radix_plan: 9-bit digits when they save a pass, below this many rows
STREAM_FROM = 1 << 20      # radix_sort_pairs: the digit stream, from this many rows
XCD_FROM_TILES = 64        # radix_pass: the XCD tile remap, from this many tiles
XCDS = 8

Plan = collections.namedtuple("Plan", "npass rbits threads tile ntiles digits")


def radix_plan(n, bits, threads=0, rbits=0):
    """radix_plan + the digit widths radix_sort_pairs balances over the passes (sort_threads / sort_rbits 0: automatic)."""
    th = threads if threads in (256, 512) else 256
    tile = th * SORT_ITEMS
    if n == 0 or bits <= 0:
        return Plan(0, 8, th, tile, 0, ())
    p8, p9 = (bits + 7) // 8, (bits + 8) // 9
    wide = p9 < p8 and n < WIDE_BELOW
    if rbits == 8:
        wide = False
    if rbits == 9:
        wide = True
    npass = p9 if wide else p8
    digits, shift = [], 0
    for p in range(npass):
        nb = (bits - shift + (npass - p) - 1) // (npass - p)
        digits.append(nb)
        shift += nb
    assert shift == bits and max(digits) <= (9 if wide else 8)
    return Plan(npass, 9 if wide else 8, th, tile, (n + tile - 1) // tile, tuple(digits))


def stream_applies(key_bytes, plan, n, digit_stream=1):
    """radix_sort_pairs: 64-bit keys, 8-bit digits, at least 2 passes, at least 2^20 rows."""
    return bool(key_bytes == 8 and plan.rbits == 8 and plan.npass >= 2 and n >= STREAM_FROM and digit_stream)


def xcd_grid(ntiles, xcd_tiles=1):
    """radix_pass: (tiles per XCD, workgroups launched); 0 tiles per XCD = tile == workgroup."""
    per = (ntiles + XCDS - 1) // XCDS if xcd_tiles and ntiles >= XCD_FROM_TILES else 0
    return per, per * XCDS if per else ntiles


def xcd_tile_of(block, per_xcd):
    return (block & 7) * per_xcd + (block >> 3) if per_xcd else block


class Family:
    """Keys of b positions over {a, b}: the words codec_split_words cuts and what follows from them."""

    def __init__(self, b):
        self.b = b
        self.words, word_of = split_words([2] * b)
        self.nwords = len(self.words)
        self.word_bits = [bits_needed(w) for w in self.words]
        self.spans = [(word_of.index(w), b - word_of[::-1].index(w)) for w in range(self.nwords)]   # positions of word w
        self.key32 = self.nwords == 1 and self.words[0] <= 1 << 32
        self.key_bytes = 4 if self.key32 else 8
        # the encode kernel with pre-multiplied LUTs leaves the first pass's histogram behind (build_encode_sort)
        self.first_hist_by_encode = self.nwords == 1 and premultiplied_bits(self.words, b) != 0

    def plans(self, n, threads=0, rbits=0):
        return [radix_plan(n, wb, threads, rbits) for wb in self.word_bits]

    def passes(self, n, threads=0, rbits=0):
        return sum(p.npass for p in self.plans(n, threads, rbits))

    def streams(self, n, threads=0, rbits=0, digit_stream=1):
        return [stream_applies(self.key_bytes, p, n, digit_stream) for p in self.plans(n, threads, rbits)]

    def hist(self, n, threads=0, rbits=0, digit_stream=1):
        """(launches, algo_bytes) of k_radix_hist_u32 / _u64 over the whole build: a pass that reads its keys
        contributes key_bytes * n, a pass that reads the digit stream n, a pass whose histogram the encode kernel left none."""
        launches = nbytes = 0
        for plan, streams in zip(self.plans(n, threads, rbits), self.streams(n, threads, rbits, digit_stream)):
            for p in range(plan.npass):
                if p == 0 and self.first_hist_by_encode:
                    continue
                launches += 1
                nbytes += n if streams and p > 0 else self.key_bytes * n
        return launches, nbytes


@functools.lru_cache(maxsize=None)
def family(b):
    return Family(b)


# ---- the tables -------------------------------------------------------------------------------------------------------
ROLE_RANDOM, ROLE_REPEATED, ROLE_WORD0 = 0, 1, 2   # ROLE_WORD0 + w: the group that differs in word w alone

Table = collections.namedtuple("Table", "b n kind data role col")


def _column(data):
    n, b = data.shape
    col = StrCol.from_arrays(np.ascontiguousarray(data).reshape(-1), (np.arange(n + 1, dtype=np.uint64) * b).astype(np.uint32))
    assert col.fixed_width == b
    return col


def near_equal_others(fam):
    """Rows of a near_equal table that differ from the rest, at its end: the complement key alone for one word; for
    several words 256 rows (the complement and random keys), enough to keep every 7-position window of the key above half
    of its 128 combinations — the dictionary stage recodes a several-word key that holds fewer (codec_try_groups)."""
    return 1 if fam.nwords == 1 else 256


def build_table(b, n, kind="mixed"):
    """n keys of b bytes over {a, b} (module docstring).  kind: mixed | equal (every row) | near_equal (every row but a few)."""
    rng = np.random.default_rng([SEED, b, n])
    fam = family(b)
    role = np.zeros(n, np.uint8)
    if kind != "mixed":
        key = rng.integers(0, 2, b, dtype=np.uint8)
        sym = np.broadcast_to(key, (n, b)).copy()
        role[:] = ROLE_REPEATED
        if kind == "near_equal":
            others = near_equal_others(fam)
            sym[n - others:] = rng.integers(0, 2, size=(others, b), dtype=np.uint8)
            sym[n - others] = 1 - key
            role[n - others:] = ROLE_RANDOM
    else:
        sym = rng.integers(0, 2, size=(n, b), dtype=np.uint8)
        order = rng.permutation(n)
        at = n // 2
        sym[order[:at]] = rng.integers(0, 2, b, dtype=np.uint8)
        role[order[:at]] = ROLE_REPEATED
        if fam.nwords > 1:
            base = rng.integers(0, 2, b, dtype=np.uint8)
            size = max(64, n // 16)
            for w, (s, e) in enumerate(fam.spans):
                rows = order[at:at + size]
                at += size
                own = sym[rows, s:e].copy()
                sym[rows] = base
                sym[rows, s:e] = own
                role[rows] = ROLE_WORD0 + w
    data = sym + np.uint8(ord("a"))
    return Table(b, n, kind, data, role, _column(data))


Ref = collections.namedtuple("Ref", "table perm first_dup")


@functools.lru_cache(maxsize=2)
def reference(b, n, kind="mixed"):
    """The oracle's order and first duplicate, once per (family, rows); shared by every option setting of a case."""
    t = build_table(b, n, kind)
    o = orc.OracleIndex([t.col])
    perm = o.perm.copy()
    perm.setflags(write=False)
    return Ref(t, perm, o.first_dup())


def planted_pair_table(b, n, where):
    """n - 1 distinct keys and one of them once more, so that the pair sorts to 0|1 ("first"), to 4095|4096 ("tile")
    or to the last two positions ("last").  Returns (table, the sorted position of the pair's second row)."""
    rng = np.random.default_rng([SEED, b, n, 77])
    codes = set()
    while len(codes) < n - 1:
        codes.update(int(c) for c in rng.integers(0, 1 << min(b, 62), n - 1 - len(codes), dtype=np.uint64))
    codes = np.array(sorted(codes), dtype=np.uint64)
    at = {"first": 0, "tile": 4095, "last": n - 2}[where]
    codes = np.append(codes, codes[at])[rng.permutation(n)]
    sym = ((codes[:, None] >> np.arange(min(b, 62) - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    if b > 62:   # the positions behind the distinct part: random, but equal for equal codes
        tail = rng.integers(0, 2, size=(n, b - 62), dtype=np.uint8)
        first_of = {}
        for i, c in enumerate(codes.tolist()):
            tail[i] = tail[first_of.setdefault(c, i)]
        sym = np.concatenate([sym, tail], axis=1)
    data = sym + np.uint8(ord("a"))
    return Table(b, n, "pair-" + where, data, np.zeros(n, np.uint8), _column(data)), at + 1


# ---- forcing and proving the path -------------------------------------------------------------------------------------
# (option, the value that forces the general sort, the ctx default it goes back to)
FORCED = (("direct_sort", 0, 1), ("counted_sort", 0, 1), ("small_build_rows", 0, 8192), ("codec_split", 0, 1),
          ("speculative_groups", 0, 1), ("host_build", 0, 1))
SWITCHES = {"sort_threads": 0, "sort_rbits": 0, "sort_digit_stream": 1, "sort_xcd_tiles": 1}   # and their defaults


@contextlib.contextmanager
def general_sort(ctx, **switches):
    assert set(switches) <= set(SWITCHES)
    try:
        for name, value, _ in FORCED:
            ctx.set_option(name, value)
        for name, value in switches.items():
            ctx.set_option(name, value)
        yield
    finally:
        for name, _, default in FORCED:
            ctx.set_option(name, default)
        for name, default in SWITCHES.items():
            ctx.set_option(name, default)


def launches(prof, name):
    return prof[name]["launches"] if name in prof else 0


def check_general_build(ctx, ref, unique, **switches):
    """One build on the general path: the oracle's permutation and first duplicate, and the proof of the path."""
    t = ref.table
    fam, n = family(t.b), t.n
    threads, rbits = switches.get("sort_threads", 0), switches.get("sort_rbits", 0)
    stream = switches.get("sort_digit_stream", 1)
    with general_sort(ctx, **switches):
        g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, [t.col], unique=unique))
    try:
        label = (t.b, n, t.kind, unique, switches)
        assert np.array_equal(g.perm(), ref.perm), label
        assert g.first_dup == ref.first_dup, label
        assert g.status == (N.CPH_ERR_DUPLICATE if unique and ref.first_dup is not None else N.CPH_OK), label
        info = g.info()
    finally:
        g.close()
    if t.kind == "equal":   # one state: nothing to sort
        assert info["code_bits"] == 0 and info["sort_passes"] == 0 and not any(k.startswith("k_radix_scatter") for k in prof), (label, info)
        return info, prof
    assert (info["nrows"], info["code_bits"], info["code_words"], info["key_bytes"]) == (n, t.b, fam.nwords, fam.key_bytes), (label, info)
    assert info["build_path"] == 0 and info["dict_entries"] == 0 and info["split"] == 0, (label, info)
    assert not [k for k in prof if k.startswith(("k_win_", "k_cs_", "k_small_build"))], (label, sorted(prof))
    ran, other = ("k_radix_scatter_u32", "k_radix_scatter_u64") if fam.key32 else ("k_radix_scatter_u64", "k_radix_scatter_u32")
    want = fam.passes(n, threads, rbits)
    assert launches(prof, ran) == info["sort_passes"] == want and other not in prof, (label, info, sorted(prof))
    if not threads and not rbits:
        assert want == classic_passes(fam.words)
    # sort_words_lsd: every word but the last is gathered before its passes, every word but the first behind the last pass
    assert launches(prof, "k_gather_u64") == 2 * (fam.nwords - 1), (label, sorted(prof))
    hist = "k_radix_hist_u32" if fam.key32 else "k_radix_hist_u64"
    hl, hb = fam.hist(n, threads, rbits, stream)
    assert launches(prof, hist) == hl and (prof[hist]["algo_bytes"] if hl else 0) == hb, (label, prof.get(hist), hl, hb)
    return info, prof


def check_both(ctx, ref, **switches):
    for unique in (False, True):
        check_general_build(ctx, ref, unique, **switches)


# ---- the cases ----------------------------------------------------------------------------------------------------------
TILE_EDGE_ROWS = (4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1)
TILE_EDGE_BITS = (9, 27, 33, 63, 80)
SORT_SETTINGS = ((0, 0), (256, 8), (256, 9), (512, 8), (512, 9))   # (sort_threads, sort_rbits); (0, 0): automatic

XCD_BITS = (27, 40)
XCD_CASES = [(256, t) for t in (63, 64, 65, 71, 72)] + [(512, t) for t in (64, 65)]   # (sort_threads, tiles)

STREAM_ROWS = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 15, (1 << 20) + 4096 + 17)
STREAM_BITS = (40, 63, 80)
STREAM_RBITS = {40: (0,), 63: (0, 8), 80: (0, 8)}   # sort_rbits settings per family (module docstring)

MULTI_WORD_BITS = (65, 80, 127)
MULTI_WORD_ROWS = (4097, 70_001)

ALL_EQUAL_ROWS = 3 * 4096 + 1
ALL_BITS = (9, 27, 33, 40, 63, 65, 80, 127)

PAIR_ROWS = 3 * 4096 + 1
PAIR_BITS = (27, 40, 80)
PAIR_PLACES = ("tile", "last", "first")


def xcd_rows(threads, ntiles):
    return ntiles * threads * SORT_ITEMS - 5   # the last tile is partial


# ---- the CPU test: the restated rules and the fixtures on their boundaries -------------------------------------------
def test_general_sort_fixtures_sit_on_their_edges():
    # the key families
    shape = {b: (family(b).word_bits, family(b).key_bytes) for b in ALL_BITS}
    assert shape == {9: ([9], 4), 27: ([27], 4), 33: ([33], 8), 40: ([40], 8), 63: ([63], 8), 65: ([63, 2], 8), 80: ([63, 17], 8),
                     127: ([63, 63, 1], 8)}
    assert family(80).spans == [(0, 63), (63, 80)] and family(127).spans == [(0, 63), (63, 126), (126, 127)]
    # only the 32-bit families get their first histogram from the encode kernel (64-bit LUTs end at 23 positions)
    assert {b for b in ALL_BITS if family(b).first_hist_by_encode} == {9, 27}
    # radix_plan: balanced digits, 9 bits where they save a pass
    assert radix_plan(4097, 33, 256, 8).digits == (7, 7, 7, 6, 6)
    assert radix_plan(4097, 9).digits == (9,) and radix_plan(4097, 27).digits == (9, 9, 9) and radix_plan(4097, 27, 0, 8).npass == 4
    assert radix_plan(4097, 63).digits == (9,) * 7 and radix_plan(4097, 63, 0, 8).digits == (8,) * 7 + (7,)
    assert radix_plan(4097, 40).rbits == 8 and radix_plan(4097, 40).npass == 5 == radix_plan(4097, 40, 0, 9).npass
    assert radix_plan(4097, 17).digits == (9, 8) and radix_plan(4097, 2).digits == (2,) and radix_plan(4097, 1).digits == (1,)
    assert radix_plan(WIDE_BELOW, 27).npass == 4 and radix_plan(WIDE_BELOW - 1, 27).npass == 3
    for b in ALL_BITS:
        for n in (4097, 1 << 20):
            assert family(b).passes(n) == classic_passes(family(b).words)
    assert (1 << 9) // 256 == 2   # k_radix_scatter's DPT: two digits per thread under 9-bit digits and 256 threads
    # case A: every row count sits one under, on, or one over a multiple of either tile, and tiles 1..4 / 1..2 occur
    for n in TILE_EDGE_ROWS:
        assert n % 4096 in (4095, 0, 1)
    assert [radix_plan(n, 9, 256).ntiles for n in TILE_EDGE_ROWS] == [1, 1, 2, 2, 2, 3, 4]
    assert [radix_plan(n, 9, 512).ntiles for n in TILE_EDGE_ROWS] == [1, 1, 1, 1, 1, 2, 2]
    assert all(radix_plan(n, 9, th).tile == th * 16 for n in TILE_EDGE_ROWS for th in (256, 512))
    # case B: the remap starts at 64 tiles, covers every tile exactly once, and surplus workgroups fall behind the last tile
    surplus = {}
    for threads, ntiles in XCD_CASES:
        n = xcd_rows(threads, ntiles)
        for b in XCD_BITS:
            plan = radix_plan(n, family(b).word_bits[0], threads)
            assert (plan.ntiles, plan.tile) == (ntiles, threads * 16) and n % plan.tile == plan.tile - 5 and n < STREAM_FROM
        per, grid = xcd_grid(ntiles)
        assert (per != 0) == (ntiles >= XCD_FROM_TILES) and xcd_grid(ntiles, 0) == (0, ntiles)
        tiles = [xcd_tile_of(blk, per) for blk in range(grid)]
        assert sorted(t for t in tiles if t < ntiles) == list(range(ntiles))
        surplus[threads, ntiles] = sum(t >= ntiles for t in tiles)
    assert surplus == {(256, 63): 0, (256, 64): 0, (256, 65): 7, (256, 71): 1, (256, 72): 0, (512, 64): 0, (512, 65): 7}
    # case C: the stream starts at exactly 2^20 rows, only for 8-bit digits; the byte histogram's scalar tail is there
    assert [n % 16 for n in STREAM_ROWS] == [15, 0, 1, 15, 1]
    for b in STREAM_BITS:
        fam = family(b)
        for n in STREAM_ROWS:
            for rbits in STREAM_RBITS[b]:
                on, off = fam.hist(n, 0, rbits, 1), fam.hist(n, 0, rbits, 0)
                streams = fam.streams(n, 0, rbits, 1)
                assert off == (fam.passes(n, 0, rbits), 8 * n * fam.passes(n, 0, rbits)) and on[0] == off[0]
                eight = [p.rbits == 8 and p.npass >= 2 for p in fam.plans(n, 0, rbits)]
                assert streams == [n >= STREAM_FROM and e for e in eight]
                assert (on != off) == any(streams)
                assert on[1] == off[1] - 7 * n * sum(p.npass - 1 for p, s in zip(fam.plans(n, 0, rbits), streams) if s)
        assert any(fam.streams(1 << 20, 0, r, 1) != fam.streams((1 << 20) - 1, 0, r, 1) for r in STREAM_RBITS[b])
    assert family(40).streams(1 << 20) == [True] and family(63).streams(1 << 20) == [False] and family(80).streams(1 << 20) == [False, False]
    assert family(63).streams(1 << 20, 0, 8) == [True] and family(80).streams(1 << 20, 0, 8) == [True, True]
    assert family(40).hist(1 << 20) == (5, (8 + 4) << 20) and family(40).hist(1 << 20, 0, 0, 0) == (5, 40 << 20)
    # case D / the tables: the parts the docstring promises
    for b in ALL_BITS:
        fam = family(b)
        t = build_table(b, 5000)
        keys = t.data.view("S%d" % b).reshape(-1)
        assert t.col.nrows == 5000 and not (t.data == 0).any() and set(np.unique(t.data)) == {ord("a"), ord("b")}
        assert all(len(np.unique(t.data[:, q])) == 2 for q in range(b))   # the code space is exactly b bits
        rep = keys[t.role == ROLE_REPEATED]
        assert len(rep) == 2500 and len(set(rep.tolist())) == 1
        assert np.abs(np.diff(np.flatnonzero(t.role == ROLE_REPEATED))).max() < 40   # scattered, not one block
        for w, (s, e) in enumerate(fam.spans if fam.nwords > 1 else ()):
            rows = t.data[t.role == ROLE_WORD0 + w]
            assert len(rows) == 312 and len(np.unique(rows[:, s:e], axis=0)) > 1
            rest = np.delete(rows, np.s_[s:e], axis=1)
            assert (rest == rest[0]).all()
        # numpy's stable order over the byte keys is the oracle's (the two references of these modules agree)
        o = orc.OracleIndex([t.col])
        assert np.array_equal(np.argsort(keys, kind="stable"), o.perm)
        assert o.first_dup() is not None
        near = build_table(b, 5000, "near_equal")
        assert all(len(np.unique(near.data[:, q])) == 2 for q in range(b))
        assert (near.role == ROLE_RANDOM).sum() == near_equal_others(fam) and (near.role[-near_equal_others(fam):] == ROLE_RANDOM).all()
        assert len(np.unique(near.data[near.role == ROLE_REPEATED], axis=0)) == 1
        if fam.nwords > 1:   # no window of the key is worth a dictionary: the code keeps its words
            for tab in (t, near):
                assert not dictionary_pays([[bytes(k) for k in tab.data]])
        assert len(np.unique(build_table(b, 5000, "equal").data, axis=0)) == 1
    assert radix_plan(ALL_EQUAL_ROWS, 9, 256).ntiles == 4 and radix_plan(ALL_EQUAL_ROWS, 9, 512).ntiles == 2
    assert [radix_plan(n, 63).ntiles for n in MULTI_WORD_ROWS] == [2, 18] and all(family(b).nwords > 1 for b in MULTI_WORD_BITS)
    # case E: one pair, where it is said to be
    for b in PAIR_BITS:
        for where, second in zip(PAIR_PLACES, (4096, PAIR_ROWS - 1, 1)):
            t, pos = planted_pair_table(b, PAIR_ROWS, where)
            o = orc.OracleIndex([t.col])
            keys = t.data.view("S%d" % b).reshape(-1)
            assert pos == second == o.first_dup() and len(set(keys.tolist())) == PAIR_ROWS - 1
            assert keys[o.perm[pos]] == keys[o.perm[pos - 1]] and o.perm[pos - 1] < o.perm[pos]
            assert all(len(np.unique(t.data[:, q])) == 2 for q in range(b))
    group_scan.check_fixtures()   # tests/test_gpu_group_scan.py: its row counts against the scan's tile, step and hand-over


# ---- the gpu tests ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", TILE_EDGE_ROWS)
@pytest.mark.parametrize("b", TILE_EDGE_BITS)
def test_tile_edges(ctx, b, n):
    """Case A: one row under, on and one row over a tile of 4096 and of 8192 keys, under both workgroup sizes and both
    digit widths (9-bit digits: two digits per thread at 256 threads) and on the automatic setting."""
    ref = reference(b, n)
    for threads, rbits in SORT_SETTINGS:
        check_both(ctx, ref, sort_threads=threads, sort_rbits=rbits)


@pytest.mark.gpu
@pytest.mark.parametrize("threads,ntiles", XCD_CASES)
@pytest.mark.parametrize("b", XCD_BITS)
def test_xcd_tile_remap(ctx, b, threads, ntiles):
    """Case B: tile = (block & 7) * per_xcd + (block >> 3) from 64 tiles on, with surplus workgroups (65, 71 tiles) and
    without (64, 72), one tile under the threshold (63), the last tile partial; remap on and off."""
    ref = reference(b, xcd_rows(threads, ntiles))
    for xcd in (1, 0):
        check_both(ctx, ref, sort_threads=threads, sort_xcd_tiles=xcd)


@pytest.mark.gpu
@pytest.mark.parametrize("n", STREAM_ROWS)
@pytest.mark.parametrize("b", STREAM_BITS)
def test_digit_stream(ctx, b, n):
    """Case C: the scatter's digit stream and k_radix_hist_bytes (16-byte groups and the scalar tail of the last one),
    on and off around 2^20 rows.  check_general_build proves from the histograms' algo_bytes which passes read the
    stream (n bytes) and which their keys (8 n); here: the settings differ exactly where the restated rule says so."""
    ref = reference(b, n)
    fam = family(b)
    differed = []
    for rbits in STREAM_RBITS[b]:
        read = {}
        for stream in (1, 0):
            for unique in (False, True):
                _, prof = check_general_build(ctx, ref, unique, sort_rbits=rbits, sort_digit_stream=stream)
                read[stream] = prof["k_radix_hist_u64"]["algo_bytes"]
        assert (read[1] != read[0]) == any(fam.streams(n, 0, rbits, 1)), (b, n, rbits, read)
        differed.append(read[1] != read[0])
    assert any(differed) == (n >= STREAM_FROM), (b, n, differed)


@pytest.mark.gpu
@pytest.mark.parametrize("n", MULTI_WORD_ROWS)
@pytest.mark.parametrize("b", MULTI_WORD_BITS)
def test_multi_word_lsd(ctx, b, n):
    """Case D: sort_words_lsd over two and three words, with the groups that differ in one word alone."""
    ref = reference(b, n)
    assert all((ref.table.role == ROLE_WORD0 + w).any() for w in range(family(b).nwords))
    for threads, rbits in ((0, 0), (512, 8)):
        check_both(ctx, ref, sort_threads=threads, sort_rbits=rbits)


@pytest.mark.gpu
@pytest.mark.parametrize("b", ALL_BITS)
def test_all_rows_equal(ctx, b):
    """Four tiles (two of 8192) of one key: every wave is full of peers in every pass.  All equal but the last row (the
    last 256 for several words) keeps the code width; all equal is a code space of one state and no pass at all."""
    n = ALL_EQUAL_ROWS
    near = reference(b, n, "near_equal")
    for threads, rbits in SORT_SETTINGS:
        check_both(ctx, near, sort_threads=threads, sort_rbits=rbits)
    equal = reference(b, n, "equal")
    assert np.array_equal(equal.perm, np.arange(n)) and equal.first_dup == 1
    check_both(ctx, equal)


@pytest.mark.gpu
@pytest.mark.parametrize("where", PAIR_PLACES)
@pytest.mark.parametrize("b", PAIR_BITS)
def test_first_duplicate_of_one_pair(ctx, b, where):
    """Case E: distinct keys but one pair, sorted to 4095|4096, to the last two positions and to 0|1: the position is
    the oracle's, and the whole order with it."""
    t, pos = planted_pair_table(b, PAIR_ROWS, where)
    o = orc.OracleIndex([t.col])
    ref = Ref(t, o.perm, o.first_dup())
    assert ref.first_dup == pos
    check_both(ctx, ref)
    check_both(ctx, ref, sort_threads=512, sort_rbits=8)
