"""Where a value begins and ends: the chunk loads of the fused chain Join (load_chunk_nobranch, wave_spans) at every start
offset and length, with neighbours whose bytes would form another key of the index.

The index keys are strings over {a, b}, closed under "drop the last byte", and the stream is laid out so that a row's key
extended by the byte that follows it in the buffer, and shortened by its own last byte, are both keys of OTHER index rows:
a shift that is off by one byte, or a straddle test that is off by one, joins the wrong row instead of none.  Checked bit
for bit against the oracle, as row ids and as sorted positions.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc

pytestmark = pytest.mark.gpu

MAXLEN = 17
LAST_ROW_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17)


@pytest.fixture(scope="module")
def vctx():
    c = Context(0)
    c.set_option("pool_guard", 1)
    yield c
    c.close()


class Keys:
    """Every string over {a, b} of 0 .. 5 bytes, and every prefix of 6 .. 17 bytes of 300 random 17-byte strings: a few
    hundred keys of each length, and dropping the last byte of a key gives a key."""

    def __init__(self):
        rng = np.random.default_rng(71)
        short = [bytes(t) for n in range(6) for t in itertools.product(b"ab", repeat=n)]
        full = sorted({bytes(rng.integers(97, 99, MAXLEN).astype(np.uint8)) for _ in range(300)})
        longer = sorted({t[:n] for t in full for n in range(6, MAXLEN + 1)})
        allk = short + longer
        order = rng.permutation(len(allk))
        self.all = [allk[int(j)] for j in order]                      # table order is not key order
        self.have = set(allk)
        self.short = [k for k in self.all if len(k) <= 8]
        # keys by (length, first byte), and for a key the bytes that extend it to another key
        self.by = {}
        for k in allk:
            self.by.setdefault((len(k), k[:1]), []).append(k)
        for n in range(1, MAXLEN + 1):
            assert min(len(self.by[(n, b"a")]), len(self.by[(n, b"b")])) >= min(2 ** (n - 1), 48) // 2 + (n == 1)

    def next_bytes(self, k):
        return [c for c in (b"a", b"b") if k + c in self.have]


@functools.lru_cache(maxsize=None)
def keys():
    return Keys()


@functools.lru_cache(maxsize=None)
def stream_values(last_len):
    """About 3000 values: every length 0 .. 17 at every start offset mod 8, every value a key of the long index that can be
    extended by the byte that follows it; the last value has `last_len` bytes."""
    K = keys()
    rng = np.random.default_rng(72)
    need = {(n, o) for n in range(MAXLEN + 1) for o in range(8)}
    vals, off, first = [], 0, None           # first: the byte the next non-empty value has to begin with, or None
    def pick(n):
        nonlocal first
        if n == 0:
            return b""
        c = first if first is not None else (b"a", b"b")[int(rng.integers(0, 2))]
        pool = K.by[(n, c)]
        for _ in range(64):
            k = pool[int(rng.integers(0, len(pool)))]
            nb = K.next_bytes(k)
            if nb or n == MAXLEN:
                first = nb[int(rng.integers(0, len(nb)))] if nb else None
                return k
        raise AssertionError("no extendable key")
    while len(vals) < 3000 or need:
        want = [n for (n, o) in need if o == off % 8]
        n = want[int(rng.integers(0, len(want)))] if want else int(rng.integers(0, MAXLEN + 1))
        need.discard((n, off % 8))
        vals.append(pick(n))
        off += n
        assert len(vals) < 6000
    vals.append(pick(last_len))
    # the property the module is about, stated on the finished buffer
    data = b"".join(vals)
    pos = 0
    for v in vals:
        pos += len(v)
        assert v in K.have and (not v or v[:-1] in K.have)
        if len(v) < MAXLEN and pos < len(data):
            assert v + data[pos:pos + 1] in K.have
    return vals


def device_column(col, shift, drop_first=False, filler=b"ab"):
    """The column in device memory with its data at an address = `shift` (mod 8) and 8 readable bytes behind the last
    value (what StrCol.to_device provides); bytes around the values spell more keys.  drop_first: rows 1 .. n-1 through the
    offsets from element 1 on — offsets[0] != 0 and a pointer that is only 4-byte aligned (the form StrCol.slice documents)."""
    nb = col.data.nbytes
    raw = torch.from_numpy(np.frombuffer((filler * (nb // 2 + 16))[: nb + 24], dtype=np.uint8).copy()).to("cuda:0")
    assert raw.data_ptr() % 8 == 0
    if nb:
        raw[shift: shift + nb].copy_(torch.from_numpy(col.data))
    data = raw[shift: shift + nb + 8]
    if col.fixed_width:
        return StrCol(data, None, col.nrows, 32, N.CPH_MEM_DEVICE, fixed_width=col.fixed_width)
    offs = torch.from_numpy(np.ascontiguousarray(col.offsets).view(np.uint8).copy()).to("cuda:0")
    if drop_first:
        assert col.offset_bits == 32 and int(col.offsets[1]) != 0
        offs = offs[4:]
        assert offs.data_ptr() % 8 == 4
        return StrCol(data, offs, col.nrows - 1, 32, N.CPH_MEM_DEVICE, fixed_width=0)
    return StrCol(data, offs, col.nrows, col.offset_bits, N.CPH_MEM_DEVICE, fixed_width=0)


def check(ctx, ix, perm, dcol, want, what):
    for positions in (False, True):
        ctx.profile(True)
        ctx.profile_read(reset=True)
        ch = join_chain(ctx, [(ix, [dcol])], positions=positions)
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert "k_chain_dense" in prof and not any(k.startswith("k_probe") for k in prof), sorted(prof)
        assert ch.nrows == want["nmatches"], what
        np.testing.assert_array_equal(ch.stream_row, want["probe_idx"], err_msg=str(what))
        got = ch.build_row(0)
        np.testing.assert_array_equal(perm[got] if positions else got, want["build_row"], err_msg=str(what))
        ch.release()


@pytest.mark.parametrize("index", ["short", "long"])
def test_value_bounds_at_every_offset_and_length(vctx, index):
    """Keys of 0 .. 8 bytes (the short kernels; longer stream values must not join) and of 0 .. 17 bytes (LONG: bytes 8 .. 15
    prefetched, byte 16 fetched on demand).  The data pointer shifted by 0 .. 7 bytes, 32-bit offsets, the offsets from element 1
    on, 64-bit offsets; the last value of the column of 0, 1, 7, 8, 9, 15, 16 and 17 bytes."""
    K = keys()
    table = StrCol.from_values(K.short if index == "short" else K.all).as_variable()
    ix = DeviceIndex(vctx, [table])
    assert ix.first_dup is None
    assert ix.info()["key_positions"] == (8 if index == "short" else MAXLEN), ix.info()
    oix = orc.OracleIndex([table])
    perm = ix.perm()
    for last_len in LAST_ROW_LENGTHS:
        vals = stream_values(last_len)
        assert len(vals[-1]) == last_len
        col32 = StrCol.from_values(vals).as_variable()
        col64 = StrCol.from_values(vals, offset_bits=64).as_variable()
        first = next(i for i, v in enumerate(vals) if v)
        tail = col32.slice(first + 1, col32.nrows)                       # its offsets[0] is not 0
        want = oix.join([col32])
        want_tail = oix.join([tail])
        head = StrCol.from_values(vals[first:]).as_variable()           # rows first+1 .. n-1 of it: the offsets from element 1 on
        assert want["nmatches"] == (len(vals) if index == "long" else sum(len(v) <= 8 for v in vals))
        for shift in range(8):
            check(vctx, ix, perm, device_column(col32, shift), want, (index, last_len, shift, 32))
            check(vctx, ix, perm, device_column(col64, shift), want, (index, last_len, shift, 64))
            check(vctx, ix, perm, device_column(head, shift, drop_first=True), want_tail, (index, last_len, shift, "from 1"))
    ix.close()
    vctx.set_option("pool_guard_check", 0)


@pytest.mark.parametrize("width", [1, 3, 7, 9, 16])
def test_fixed_width_columns_as_wide_as_the_longest_key(vctx, width):
    """A fixed-width stream column whose width is the index's longest key: encode_rows compares no lengths.  Not 8 bytes
    wide, so never lean.  65 and 513 rows, the data pointer shifted by 0 .. 7 bytes, and the host column."""
    rng = np.random.default_rng(80 + width)
    if width <= 9:
        allk = [bytes(t) for t in itertools.product(b"ab", repeat=width)]
    else:
        allk = sorted({bytes(rng.integers(97, 99, width).astype(np.uint8)) for _ in range(1500)})
    order = rng.permutation(len(allk))
    nkeep = len(allk) if width <= 3 else len(allk) * 2 // 3
    tkeys = [allk[int(j)] for j in order[:nkeep]]
    gone = [allk[int(j)] for j in order[nkeep:]]
    table = StrCol.from_values(tkeys)
    assert table.fixed_width == width
    ix = DeviceIndex(vctx, [table])
    assert ix.first_dup is None and ix.info()["key_positions"] == width, ix.info()
    oix = orc.OracleIndex([table])
    perm = ix.perm()
    for m in (65, 513):
        vals = [tkeys[int(j)] for j in rng.integers(0, len(tkeys), m)]
        for i in range(0, m, 5):                                     # misses: a byte just outside the alphabet somewhere, NUL
            v = bytearray(vals[i])
            v[int(rng.integers(0, width))] = (0x60, 0x63, 0x00, 0xE1)[(i // 5) % 4]
            vals[i] = bytes(v)
        for i in range(3, m, 7):                                     # inside the alphabet, absent
            if gone:
                vals[i] = gone[int(rng.integers(0, len(gone)))]
        for tail in (tkeys[0], vals[0]):                             # the last row joins / does not
            vals[-1] = tail
            col = StrCol.from_values(vals)
            assert col.fixed_width == width
            want = oix.join([col])
            assert 0 < want["nmatches"] < m
            check(vctx, ix, perm, col, want, (width, m, "host"))
            for shift in range(8):
                check(vctx, ix, perm, device_column(col, shift), want, (width, m, shift))
    ix.close()
    vctx.set_option("pool_guard_check", 0)
