"""The chain Join's arithmetic (lean) step for variable-length keys of at most 8 bytes (chain.hip: the VAR mask of k_chain_dense;
codec_device.hpp: encode_rows_arith_var; keycodec.hip: codec_arith_plan) against the oracle's nested joins, bit for bit, and against
the same call with chain_arith = 0 (the LUT walk), in both output modes and with chain_rank_lds 0 and 1.

What the kernel can get wrong and where this file looks for it:
  * the bytes past a value belong to its neighbour and must be masked out: every stream here is packed, and `prefix3` misses with a
    valid prefix whose next byte is a valid symbol of the following value;
  * the length test (shorter than the shortest key, one byte longer than the longest) and the range test of every position (the byte
    just below and just above the alphabet, 0x80 and above, NUL): each kind on the first row, the last row and both ends of every
    ballot word;
  * the wave-uniform choice between the plain 8-byte load and the clamped one at the column's end: streams of every length around a
    ballot word (64), a wave-tile (512) and a workgroup tile (2048), and device columns whose data ends exactly at its buffer's end
    with the longest / the shortest value last;
  * the rank table in LDS read as one 8-byte block, and in global memory.
The fallbacks (keys of 9 bytes, an alphabet with a gap, bytes from 0x80 on, 64-bit offsets) must still give the oracle's result.
Nothing the library reports tells the lean instantiations from the LUT ones — both are launched as k_chain_dense — so the dispatch
assertion is the one the issue names (k_chain_dense ran, no k_probe* did), and `qualifies` states in Python, from the keys alone,
which sides meet the plan's conditions.  A codec whose pad does not start at the shortest key's length cannot be built: codec_build
puts the pad into exactly the positions from minlen on.

Runs on a ctx with the pool's canaries on (pool_guard), checked at the end of every test.
"""
import functools

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc
from tests.test_gpu_chain import oracle_chain
from tests.test_gpu_chain_edges import assert_fused, options, profiled

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
MASTER = LENGTHS[-1]


def var32(vals):
    return StrCol.from_values(vals).as_variable()


def var64(vals):
    return StrCol.from_values(vals, offset_bits=64).as_variable()


def fixed(width):
    def make(vals):
        col = StrCol.from_values(vals)
        assert col.nrows == 0 or col.fixed_width == width, (col.fixed_width, width)
        return col
    return make


def edge_rows(m):
    """The first row, the last row and both ends of every ballot word."""
    r = np.arange(m)
    return (r == 0) | (r == m - 1) | (r % 64 == 0) | (r % 64 == 63)


def alphabets(keys):
    """Per byte position: the sorted byte values of the keys that have the position."""
    return [sorted({k[p] for k in keys if len(k) > p}) for p in range(max(len(k) for k in keys))]


def qualifies(keys):
    """codec_arith_plan's conditions on a single key column, from the keys alone."""
    if max(len(k) for k in keys) > 8:
        return False
    return all(a[-1] < 0x80 and a[-1] - a[0] + 1 == len(a) for a in alphabets(keys))


class Side:
    """A build table of one key column, the master hit column of a stream that joins it, and the miss kinds: name -> f(i) = a
    value that is not a key (i = the stream row, so that the kinds walk the positions and the keys)."""

    def __init__(self, name, keys, lean, col=var32, seed=1, hit_filter=None):
        assert len(set(keys)) == len(keys)
        self.name, self.keys, self.col, self.lean = name, list(keys), col, lean
        assert qualifies(self.keys) == lean, name
        self.build_col = var32(self.keys)
        rng = np.random.default_rng(seed)
        pool = [k for k in self.keys if hit_filter is None or hit_filter(k)]
        self.hit = [pool[int(j)] for j in rng.integers(0, len(pool), MASTER)]
        self.minlen, self.maxlen = min(len(k) for k in keys), max(len(k) for k in keys)
        self.alpha = alphabets(self.keys)
        self.kinds = {}
        have = set(self.keys)
        longest = [k for k in pool if len(k) == self.maxlen] or [k for k in self.keys if len(k) == self.maxlen]

        def at_every_position(byte_of):
            # a key with its byte at position p replaced, p walking the positions the key has
            def f(i):
                k = pool[i % len(pool)] if len(pool[i % len(pool)]) else longest[i % len(longest)]
                p = (i + i // 64) % len(k)
                return k[:p] + bytes([byte_of(p)]) + k[p + 1:]
            return f

        if col is var32 or col is var64:
            self.kinds["too_long"] = lambda i: longest[i % len(longest)] + bytes([self.alpha[0][0]])
            if self.minlen > 0:
                self.kinds["too_short"] = lambda i: pool[i % len(pool)][:self.minlen - 1]
        if all(a[0] > 0 for a in self.alpha):
            self.kinds["below"] = at_every_position(lambda p: self.alpha[p][0] - 1)
            self.kinds["nul"] = at_every_position(lambda p: 0)
        if all(a[-1] < 0x7F for a in self.alpha):
            self.kinds["above"] = at_every_position(lambda p: self.alpha[p][-1] + 1)
            self.kinds["high"] = at_every_position(lambda p: 0x80 + (p * 37) % 128)
        for name_, f in self.kinds.items():
            for i in (0, 1, 63, 64, 65, 511, MASTER - 1):
                assert f(i) not in have, (name, name_, i)

    @functools.cached_property
    def oracle(self):
        return orc.OracleIndex([self.build_col])


@functools.lru_cache(maxsize=None)
def side(name):
    if name.startswith("itoa"):          # unpadded decimal ids 0 .. n-1
        n = int(name[4:])
        return Side(name, [b"%d" % i for i in np.random.default_rng(n).permutation(n)], True, seed=n)
    if name == "prefix3":                # lengths 0, 1 and 3 over '1'..'3': every two-byte string is a valid prefix and no key
        d = [b"1", b"2", b"3"]
        s = Side(name, [b""] + d + [a + b + c for a in d for b in d for c in d], True, seed=2)
        s.kinds["prefix"] = lambda i: d[i % 3] + d[(i // 3) % 3]     # the next value starts with a digit that would complete it
        return s
    if name == "abc8":                   # keys of 3, 5 and exactly 8 bytes over 'a'..'c'
        rng = np.random.default_rng(3)
        def word(n):
            return bytes(rng.integers(97, 100, n).astype(np.uint8))
        keys = {bytes([c]) * 8 for c in b"abc"} | {bytes([a, b, c]) for a in b"abc" for b in b"abc" for c in b"abc"}
        keys |= {word(5) for _ in range(150)} | {word(8) for _ in range(2000)}
        s = Side(name, sorted(keys), True, seed=4)
        s.kinds["absent"] = lambda i: bytes([97 + i % 3, 97 + (i // 3) % 3])                  # inside the alphabets, no key
        gone8 = [w for w in (b"abcabcab", b"cabcabca", b"bcabcabc", b"aabbccaa", b"ccbbaacc", b"abababab") if w not in keys]
        s.kinds["absent8"] = lambda i: gone8[i % len(gone8)]
        return s
    if name == "fixed5":                 # unpadded ids below 100000 joined by a fixed-width-5 column: only 5-byte values occur
        s = Side(name, side("itoa100000").keys, True, col=fixed(5), seed=5, hit_filter=lambda k: len(k) == 5)
        s.kinds["absent"] = lambda i: b"0%04d" % (i % 10000)                                  # valid symbols, a code no key has
        return s
    # ---- fallbacks: the LUT walk --------------------------------------------------------------------------------------------
    if name == "len9":                   # keys of up to 9 bytes
        return Side(name, [b"%d" % i for i in list(range(300)) + list(range(100000000, 100000700))], False, seed=6)
    if name == "gap":                    # '3' is missing from every alphabet
        d = [b"1", b"2", b"4"]
        s = Side(name, d + [a + b for a in d for b in d] + [a + b + c for a in d for b in d for c in d if (a, b, c) != (d[2],) * 3], False, seed=7)
        s.kinds["in_gap"] = lambda i: [b"3", b"13", b"31", b"123", b"321"][i % 5]
        return s
    if name == "high":                   # bytes from 0x80 on
        d = [b"\x7f", b"\x80", b"\x81"]
        return Side(name, d + [a + b for a in d for b in d], False, seed=8)
    if name == "wide":                   # 64-bit offsets in the stream column
        return Side(name, side("itoa1000").keys, True, col=var64, seed=9)
    raise KeyError(name)


@pytest.fixture(scope="module")
def sctx():
    c = Context(0)
    c.set_option("pool_guard", 1)
    yield c
    for ix in _built.values():
        ix.close()
    _built.clear()
    c.close()


_built = {}
_perms = {}


def device_index(ctx, s):
    if s.name not in _built:
        ix = DeviceIndex(ctx, [s.build_col])
        assert ix.status == N.CPH_OK and ix.first_dup is None, (s.name, ix.status)
        _built[s.name] = ix
        _perms[s.name] = ix.perm()
    return _built[s.name]


def stream_values(s, m, kind):
    """m rows of the side's stream: hits, and a miss of `kind` on every edge row (kind None: every row joins; 'mixed': the kinds in
    turn, so that every kind meets both ends of a ballot word)."""
    vals = list(s.hit[:m])
    if kind is None:
        return vals
    names = sorted(s.kinds)
    n = 0
    for i in np.flatnonzero(edge_rows(m)):
        f = s.kinds[names[(n + n // 4) % len(names)] if kind == "mixed" else kind]
        vals[int(i)] = f(int(i))
        n += 1
    return vals


def run_chain(ctx, sides, cols, host_cols=None, what=None):
    """join_chain over the build tables `sides` keyed by the stream columns `cols` (host_cols: the same columns for the oracle when
    `cols` are on the device): every setting of (positions, chain_rank_lds, chain_arith) gives the oracle's rows, hence each other's."""
    gix = [device_index(ctx, s) for s in sides]
    es, erows = oracle_chain([s.oracle for s in sides], list(host_cols or cols))
    m = cols[0].nrows
    steps = [(g, [c]) for g, c in zip(gix, cols)]
    for positions in (False, True):
        for rank_lds in (1, 0):
            got = {}
            for arith in (1, 0):
                tag = (what, m, positions, rank_lds, arith)
                with options(ctx, chain_arith=arith, chain_rank_lds=rank_lds):
                    ch, prof = profiled(ctx, lambda: join_chain(ctx, steps, positions=positions))
                assert_fused(prof)
                assert ch.positions == positions and ch.nrows == len(es), tag
                assert ch.identity == (len(es) == m), tag
                np.testing.assert_array_equal(ch.stream_row, es, err_msg=str(tag))
                raw = [ch.build_row(k).copy() for k in range(len(sides))]
                for k, s in enumerate(sides):
                    rows = raw[k]
                    if positions:
                        assert len(rows) == 0 or int(rows.max()) < gix[k].nrows, tag
                        rows = _perms[s.name][rows]
                    np.testing.assert_array_equal(rows, erows[k], err_msg=str(tag))
                got[arith] = raw
                ch.release()
            for k in range(len(sides)):      # the arithmetic step and the LUT walk: the same words
                np.testing.assert_array_equal(got[1][k], got[0][k], err_msg=str((what, m, positions, rank_lds, k)))
    return len(es)


def run_lengths(ctx, s, lengths=LENGTHS):
    for m in lengths:
        for kind in (None, "mixed"):
            vals = stream_values(s, m, kind)
            joined = run_chain(ctx, [s], [s.col(vals)], what=(s.name, kind))
            assert joined == (m if kind is None else m - int(edge_rows(m).sum())), (s.name, m, kind)


# ---- 1. every stream length x every build side ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["itoa1", "itoa10", "itoa11", "itoa100", "itoa1000", "itoa100000", "prefix3", "abc8", "fixed5"])
def test_lengths(sctx, name):
    """Unpadded ids 0 .. n-1 (n = 1: one key of one byte; 10 / 11, 100: the second / third position appears), keys of lengths 0 - 3
    with the empty key, keys of exactly 8 bytes among shorter ones, a fixed-width-5 column against keys of 1 - 5 bytes."""
    run_lengths(sctx, side(name))
    sctx.set_option("pool_guard_check", 0)


# ---- 2. every kind of miss on the first row, the last row and both ends of every ballot word ---------------------------------------------
@pytest.mark.parametrize("name", ["itoa100000", "itoa11", "prefix3", "abc8", "fixed5"])
def test_miss_kinds(sctx, name):
    s = side(name)
    want = {"itoa100000": {"too_long", "too_short", "below", "above", "high", "nul"}, "prefix3": {"too_long", "prefix", "below", "above"},
            "fixed5": {"below", "above", "high", "nul", "absent"}}.get(name)
    assert want is None or want <= set(s.kinds), sorted(s.kinds)
    for kind in sorted(s.kinds):
        for m in (1, 64, 577):                 # 577 = nine ballot words and one row
            vals = stream_values(s, m, kind)
            joined = run_chain(sctx, [s], [s.col(vals)], what=(name, kind))
            assert joined == m - int(edge_rows(m).sum()), (name, kind, m)
    sctx.set_option("pool_guard_check", 0)


# ---- 3. the column's end --------------------------------------------------------------------------------------------------------------
def exact_device_col(col):
    """The column in device memory with NO slack behind its data: the buffer ends with the last value's last byte."""
    import torch

    assert not col.fixed_width and col.offset_bits == 32
    d = torch.from_numpy(np.ascontiguousarray(col.data)).to("cuda:0")
    o = torch.from_numpy(np.ascontiguousarray(col.offsets).view(np.uint8).copy()).to("cuda:0")
    assert d.numel() == int(col.offsets[col.nrows])
    return StrCol(d, o, col.nrows, 32, N.CPH_MEM_DEVICE, fixed_width=0)


@pytest.mark.parametrize("last", [b"99999", b"7", b"99999x", b""], ids=["longest", "shortest", "too_long", "empty"])
@pytest.mark.parametrize("m", [2, 9, 512, 513, 2049])
def test_column_end(sctx, m, last):
    """The stream's last value is the longest key, the shortest key, one byte too long, or empty (both misses), and the column's data
    ends exactly at its buffer's end: within 8 bytes of it the kernel may only load aligned words that hold bytes of the column."""
    s = side("itoa100000")
    vals = stream_values(s, m, None)
    vals[-1] = last
    if m >= 9:
        vals[-8:-1] = [b"5"] * 7           # the last eight values inside the column's last eight bytes or so
    host = var32(vals)
    joined = run_chain(sctx, [s], [exact_device_col(host)], host_cols=[host], what=("end", last))
    assert joined == m - (0 if last in (b"99999", b"7") else 1)
    sctx.set_option("pool_guard_check", 0)


# ---- 4. two steps: the benchmark's shape and its itoa_ids variant -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def id8_side():
    """%08d ids 0 .. 3999 in a fixed-width-8 column: the lean step of one aligned load."""
    s = Side("id8", [b"%08d" % i for i in np.random.default_rng(21).permutation(4000)], True, col=fixed(8), seed=21)
    s.kinds = {"above": lambda i: (b"%08d" % (i % 4000))[:7] + b":", "absent": lambda i: b"%08d" % (4000 + i % 1000)}
    return s


@pytest.mark.parametrize("names", [("id8", "itoa100000"), ("itoa1000", "itoa100000"), ("itoa100000", "id8"), ("abc8", "fixed5"), ("gap", "itoa1000"),
                                   ("itoa1000", "gap")],
                         ids=["fixed8_var", "var_var", "var_fixed8", "var_fixed5", "lut_var", "var_lut"])
def test_two_steps(sctx, names):
    sides = [id8_side() if n == "id8" else side(n) for n in names]
    for m in (1, 65, 513, 2049, 4097):
        for miss_step in (None, 0, 1):
            cols = [s.col(stream_values(s, m, "mixed" if k == miss_step else None)) for k, s in enumerate(sides)]
            joined = run_chain(sctx, sides, cols, what=(names, miss_step))
            assert joined == (m if miss_step is None else m - int(edge_rows(m).sum())), (names, m, miss_step)
    sctx.set_option("pool_guard_check", 0)


# ---- 5. fallbacks: the LUT walk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["len9", "gap", "high", "wide"])
def test_fallbacks(sctx, name):
    """Keys of 9 bytes, an alphabet with a gap, alphabets with bytes from 0x80 on, a stream column with 64-bit offsets: none of them
    may take the arithmetic step (Side asserts what `qualifies` says about the keys), all of them give the oracle's rows."""
    s = side(name)
    run_lengths(sctx, s, (1, 65, 513, 2049))
    for kind in sorted(s.kinds):
        vals = stream_values(s, 577, kind)
        assert run_chain(sctx, [s], [s.col(vals)], what=(name, kind)) == 577 - int(edge_rows(577).sum())
    sctx.set_option("pool_guard_check", 0)
