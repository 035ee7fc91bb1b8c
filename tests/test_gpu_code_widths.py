"""The mixed-radix key codec at every code-width threshold.

Every kernel choice of an index build, probe, Find and chained Join follows from one number: the size of the code
space (`states`, the product of the per-position alphabet sizes) and `bits = bits_needed(states)`.  The key families
below have an EXACTLY known code space that sits on, or one step over, each power of two the library branches on
(keycodec.hip: codec_split_words / codec_premultiplied_bits / codec_arith_plan, codec_device.hpp: encode_position,
radix_sort.hip: radix_plan, small_build.hip, probe.hip: index_plan_table and the sorted search, host_encode.hip,
index_ops.hip: the load check), and every table holds the all-minimum and the all-maximum key (code states - 1).

The unmarked test restates the radix rule and codec_split_words in exact Python integers and keeps the fixtures on
their boundaries on a machine without a GPU; the gpu tests compare everything bit for bit with oracle.orc.OracleIndex.

Two deviations from a plain "one table of < 2200 rows per case", both forced by rules of the library itself:
  * a per-position code of several words is handed to the dictionary stage (keycodec.hip: codec_try_groups), which
    recodes windows of up to 7 positions whenever the table holds fewer than half of a window's combinations.  Binary
    alphabets are immune (128 combinations, all present); a radix-8 key of 22 positions is not, so the case
    `B-r8x22` is marked `dictionary`: its plain code needs two words (checked on the CPU), the index the library
    builds has dictionary entries and at most as many words, and every answer is still compared with the oracle.
  * the host coder (host_encode.hip: build_from_host_codes) only takes tables of at least 2^20 rows and keys of at
    most 8 bytes: the host-coder build test tiles the 8-byte cases at 2^31 and at 3 * 2^30 up to 2^20 + 4321 rows.
"""
import functools
import math

import numpy as np
import pytest

from csvplus_amd import Context, DeviceIndex, StrCol, _native as N, join_chain
from oracle import orc
from tests.helpers import assert_bounds_equal, assert_join_equal

SEED = 20260118
N_RANDOM, N_REPEAT = 1500, 300
MAX_ROWS, MAX_PROBES, MAX_KEY = 2200, 4000, 127

# ---- the library's constants, restated (cph_internal.hpp) -------------------------------------------------------
K_MAX_WORDS = 20
K_SMALL_MAX_POS = 64
K_LUT_STRIDE = 257
K_LUT_LDS = 48 * 1024
K_GROUP_SPAN = 7


def bits_needed(states: int) -> int:
    """keycodec.hip: bits to represent 0 .. states - 1."""
    return 0 if states <= 1 else (states - 1).bit_length()


def split_words(radix):
    """codec_split_words in exact integers: (states per word, word of every position).  A word closes when
    prod * radix > 2^63; exactly 2^63 stays one word."""
    words, word_of, prod = [], [], 1
    for r in radix:
        if prod * r > 1 << 63:
            words.append(prod)
            prod = 1
        word_of.append(len(words))
        prod *= r
    words.append(prod)
    assert len(words) <= K_MAX_WORDS
    return words, word_of


def symbol_matrix(vals):
    """One row per value, one column per byte position: 0 where the value has ended (pad), else 1 + byte."""
    lens = np.fromiter(map(len, vals), np.int64, len(vals))
    mat = np.zeros((len(vals), int(lens.max())), np.int64)
    mat[np.arange(mat.shape[1]) < lens[:, None]] = np.frombuffer(b"".join(vals), np.uint8).astype(np.int64) + 1
    return mat


class PyCodec:
    """The radix rule restated: per position of every key column, the distinct bytes seen there in byte order, behind
    the pad symbol when some value ends before that position (codec_build)."""

    def __init__(self, columns):
        self.col_maxlen, self.col_minlen, self.alphabet = [], [], []   # alphabet[p]: symbol (0 pad, 1 + byte) -> rank
        for vals in columns:
            mat = symbol_matrix(vals)
            self.col_maxlen.append(mat.shape[1])
            self.col_minlen.append(min(map(len, vals)))
            for q in range(mat.shape[1]):   # (the pad symbol occurs at q exactly when some value ends before q)
                self.alphabet.append({int(s): r for r, s in enumerate(np.unique(mat[:, q]))})
        self.radix = [len(a) for a in self.alphabet]
        self.npos = len(self.radix)
        self.words, self.word_of = split_words(self.radix)
        self.nwords = len(self.words)
        self.bits = sum(bits_needed(w) for w in self.words)
        self.key32 = self.nwords == 1 and self.words[0] <= 1 << 32
        self.total = math.prod(self.radix)

    def encode(self, key, ncols=None):
        """The key's code as ONE exact integer over the leading ncols columns (None: not encodable — a symbol outside
        a position's alphabet or a value longer than the column's longest)."""
        code, p = 0, 0
        for c, v in enumerate(key[:ncols]):
            if len(v) > self.col_maxlen[c]:
                return None
            for q in range(self.col_maxlen[c]):
                r = self.alphabet[p].get(1 + v[q] if q < len(v) else 0)
                if r is None:
                    return None
                code = code * self.radix[p] + r
                p += 1
        return code

    def decode(self, code):
        """The key tuple of a code of the whole key (the pad symbol only ever trails in the codes asked for here)."""
        digits = []
        for r in reversed(self.radix):
            digits.append(code % r)
            code //= r
        digits.reverse()
        key, p = [], 0
        for mx in self.col_maxlen:
            v, ended = bytearray(), False
            for _ in range(mx):
                sym = {r: s for s, r in self.alphabet[p].items()}[digits[p]]
                if sym == 0:
                    ended = True
                else:
                    assert not ended, "a byte behind a pad: not a key"
                    v.append(sym - 1)
                p += 1
            key.append(bytes(v))
        return tuple(key)


# ---- the rules the gpu checks predict from, each restated from the file named -------------------------------------
def small_build_fits(words, npos):
    """small_build.hip: one word of at most 2^63 states, at most kSmallMaxPos byte positions."""
    return len(words) == 1 and words[0] <= 1 << 63 and npos <= K_SMALL_MAX_POS


def premultiplied_bits(words, npos):
    """codec_premultiplied_bits: 32-bit entries iff states <= 2^31, else 64-bit; none beyond 48 KiB of LDS."""
    if len(words) != 1 or npos <= 0:
        return 0
    w = 32 if words[0] <= 1 << 31 else 64
    return w if npos * K_LUT_STRIDE * (w // 8) <= K_LUT_LDS else 0


def plan_table_entries(words, nrows):
    """index_plan_table: direct table iff states <= max(24 n, 2^20) and <= 2^30."""
    if len(words) != 1 or nrows == 0:
        return 0
    return words[0] if words[0] <= max(24 * nrows, 1 << 20) and words[0] <= 1 << 30 else 0


def classic_passes(words):
    """radix_plan for n < 2^22, per word: 9-bit digits iff they save a pass."""
    return sum(min((b + 7) // 8, (b + 8) // 9) for b in (bits_needed(w) for w in words))


def arith_plan_applies(case):
    """codec_arith_plan: one fixed-length column of at most 8 bytes, contiguous ranges below 0x80, states <= 2^31."""
    if len(case.cols) != 1 or len(case.words) != 1 or case.words[0] > 1 << 31:
        return False
    alph, lens = case.cols[0]
    if len(set(lens)) != 1 or len(alph) > 8:
        return False
    return all(a[-1] < 0x80 and a[-1] - a[0] + 1 == len(a) for a in alph)


def host_coder_takes(words):
    """host_encode.hip: cph_host_encoder_create and build_from_host_codes refuse states > 2^31."""
    return len(words) == 1 and words[0] <= 1 << 31


def dictionary_pays(columns):
    """codec_try_groups' candidate rule: some window of 2..7 positions of a column holds so few of its combinations
    that coding it by a dictionary saves a bit or more."""
    for vals in columns:
        mat = symbol_matrix(vals)
        mx = mat.shape[1]
        radix = [len(np.unique(mat[:, q])) for q in range(mx)]
        for q0 in range(mx - 1):
            for span in range(2, K_GROUP_SPAN + 1):
                if q0 + span > mx:
                    break
                count = len(np.unique(mat[:, q0:q0 + span] @ (K_LUT_STRIDE ** np.arange(span, dtype=np.int64))))
                if math.log2(math.prod(radix[q0:q0 + span])) - math.log2(count) >= 1.0:
                    return True
    return False


# ---- the case table ------------------------------------------------------------------------------------------------
AB, ABC = b"ab", b"abc"
R4, R5, R8, R12, R16 = b"abcd", b"abcde", b"abcdefgh", b"abcdefghijkl", b"abcdefghijklmnop"
G16, G8 = b"ACEacegikmoqsuwy", b"ACEacegi"   # the same sizes, no two neighbours: no contiguous range
PLUS_B = (8, 16, 24, 31, 32, 40, 48, 56, 62, 63)


class Case:
    def __init__(self, name, family, cols, words, bits, key32, variable=False, dictionary=False):
        self.name, self.family = name, family
        self.cols = [(list(a), tuple(l) if l else (len(a),)) for a, l in cols]   # per column: alphabets, value lengths
        self.words, self.bits, self.nwords, self.key32 = list(words), bits, len(words), key32
        self.variable, self.dictionary = variable, dictionary
        self.npos = sum(len(a) for a, _ in self.cols)
        self.total = math.prod(words)
        self.fixed8 = len(self.cols) == 1 and self.cols[0][1] == (8,)


def _binary_words(nbits):
    """Claimed words of a key of nbits binary positions."""
    return [1 << 63] * (nbits // 63) + ([1 << nbits % 63] if nbits % 63 else [])


@functools.lru_cache(maxsize=None)
def case_table():
    t = []

    def add(*a, **k):
        t.append(Case(*a, **k))

    for b in range(1, 64):   # A: binary, every width — every bits from 1 to 63 is a sort plan of its own
        add("A-b%02d" % b, "A", [([AB] * b, None)], [1 << b], b, b <= 32)
    for b in PLUS_B:         # A+: a third symbol at the most / least significant position; A-pad: the same through the pad
        one = b <= 62
        add("A+first-b%02d" % b, "A+", [([ABC] + [AB] * (b - 1), None)], [3 << (b - 1)] if one else [3 << 61, 2], b + 1, b <= 31)
        add("A+last-b%02d" % b, "A+", [([AB] * (b - 1) + [ABC], None)], [3 << (b - 1)] if one else [1 << 62, 3], b + 1, b <= 31)
        add("Apad-b%02d" % b, "A-pad", [([AB] * b, (b - 1, b))], [3 << (b - 1)] if one else [1 << 62, 3], b + 1, b <= 31)
    # B: compact keys (the pre-multiplied LUTs need npos <= 47 / 23)
    add("B-r4x15-r2", "B", [([R4] * 15 + [AB], None)], [1 << 31], 31, True)
    add("B-r4x15-r3", "B", [([R4] * 15 + [ABC], None)], [3 << 30], 32, True)
    add("B-r4x16", "B", [([R4] * 16, None)], [1 << 32], 32, True)
    add("B-r4x15-r5", "B", [([R4] * 15 + [R5], None)], [5 << 30], 33, False)
    add("B-r8x21", "B", [([R8] * 21, None)], [1 << 63], 63, False)
    add("B-r8x22", "B", [([R8] * 22, None)], [1 << 63, 8], 66, False, dictionary=True)
    for var in (False, True):   # eight bytes, as a fixed_width == 8 column and as a variable-length one
        s = "-var" if var else ""
        add("B-f8-r16x7-r8" + s, "B", [([R16] * 7 + [R8], None)], [1 << 31], 31, True, variable=var)
        add("B-f8-r16x8" + s, "B", [([R16] * 8, None)], [1 << 32], 32, True, variable=var)
        add("B-f8-gaps" + s, "B", [([G16] * 7 + [G8], None)], [1 << 31], 31, True, variable=var)
    add("B-f8-r16x7-r12", "B", [([R16] * 7 + [R12], None)], [3 << 30], 32, True)   # the host coder's first refusal
    # the LDS bound of the LUTs, one word of 64 / 65 positions: constant positions (radix 1) behind the key
    add("B-lut32-pos47", "B", [([AB] * 31 + [b"a"] * 16, None)], [1 << 31], 31, True)
    add("B-lut32-pos48", "B", [([AB] * 31 + [b"a"] * 17, None)], [1 << 31], 31, True)
    add("B-lut64-pos23", "B", [([R4] * 17 + [b"a"] * 6, None)], [1 << 34], 34, False)
    add("B-lut64-pos24", "B", [([R4] * 17 + [b"a"] * 7, None)], [1 << 34], 34, False)
    add("B-pos64-one-word", "B", [([AB] * 62 + [b"a"] * 2, None)], [1 << 62], 62, False)
    add("B-pos65-one-word", "B", [([AB] * 62 + [b"a"] * 3, None)], [1 << 62], 62, False)
    # C: words and columns
    for b in (64, 65, 126, 127):
        add("C-b%d" % b, "C", [([AB] * b, None)], _binary_words(b), b, False)
    for l0, l1 in ((16, 16), (16, 17), (31, 32), (32, 32)):   # (32, 32): the word boundary falls inside column 1
        add("C-cols-%d-%d" % (l0, l1), "C", [([AB] * l0, None), ([AB] * l1, None)], _binary_words(l0 + l1), l0 + l1, l0 + l1 <= 32)
    assert len({c.name for c in t}) == len(t)
    return {c.name: c for c in t}


CASE_NAMES = list(case_table())
TWO_COLUMN = [n for n in CASE_NAMES if n.startswith("C-cols-")]
FIXED8 = [n for n in CASE_NAMES if n.startswith("B-f8-")]
LOOKUP_AB = ["B-r4x15-r2", "B-r4x15-r3", "B-r4x16", "B-r4x15-r5", "B-r8x21", "C-b64", "B-r8x22"]
PERSIST = ["B-r4x15-r2", "B-r4x16", "B-r8x21", "C-b64", "A-b31", "A-b32", "A-b63", "A+first-b63"]
SORT_SWITCH = ["A-b%02d" % b for b in (9, 17, 18, 27, 33, 36, 45, 54, 63)]
HOST_CODER = ["B-f8-r16x7-r8", "B-f8-r16x7-r12"]


class Table:
    """The rows of one case: keys are tuples of one bytes value per key column."""

    def __init__(self, case):
        rng = np.random.default_rng([SEED, CASE_NAMES.index(case.name)])
        self.case = case
        radix = [len(a) + (q >= min(lens)) for alph, lens in case.cols for q, a in enumerate(alph)]
        assert math.prod(radix) == case.total
        # a codec over synthetic rows that hold every symbol: only used to decode the extreme codes into keys
        full = PyCodec([[bytes(a[j % len(a)] for a in alph[:ln]) for ln in lens for j in range(max(map(len, alph)))]
                        for alph, lens in case.cols])
        assert full.radix == radix
        first = math.prod(radix[1:])
        self.kmin, self.kmax, self.kpred = full.decode(0), full.decode(case.total - 1), full.decode(max(case.total - 2, 0))
        self.kfirst = full.decode((radix[0] - 1) * first)      # the maximum symbol at position 0, the minimum elsewhere
        self.kmirror = full.decode(first - 1)                  # and its mirror
        self.extremes = [self.kmin, self.kmax, self.kpred, self.kfirst, self.kmirror]
        rows = list(self.extremes)
        maxr, p0 = max(radix), 0
        for j in range(maxr):   # every symbol at every position, whatever the random rows hold (never all-maximum: the shift)
            key, p0 = [], 0
            for alph, lens in case.cols:
                key.append(bytes(a[(j + p0 + q) % len(a)] for q, a in enumerate(alph)))
                p0 += len(alph)
            rows.append(tuple(key))
        rand = []
        for alph, lens in case.cols:   # uniform symbols at every position, uniform over the value lengths
            lut = np.zeros((len(alph), maxr), np.uint8)
            for q, a in enumerate(alph):
                lut[q, :len(a)] = list(a)
            idx = rng.integers(0, [len(a) for a in alph], size=(N_RANDOM, len(alph)))
            sym = lut[np.arange(len(alph)), idx]
            ln = np.asarray(lens)[rng.integers(0, len(lens), N_RANDOM)]
            rand.append([sym[i, :ln[i]].tobytes() for i in range(N_RANDOM)])
        rows += list(zip(*rand))
        rows += [rows[int(i)] for i in rng.integers(0, len(rows), N_REPEAT)]
        order = rng.permutation(len(rows))
        self.full = [rows[int(i)] for i in order]
        # the all-maximum key left out, every symbol still present everywhere (impossible with a single position)
        self.nomax = [k for k in self.full if k != self.kmax] if case.npos >= 2 else None
        self.unique = list(dict.fromkeys(self.full))
        self.absent = self._absent_key(rng)
        self.probes = self._probes(rng)
        # the probes whose values all have full length: handed over, they make fixed-width columns
        self.probes_fixed = [k for k in self.probes if all(len(v) == len(alph) for v, (alph, _) in zip(k, case.cols))]

    def _absent_key(self, rng):
        have = set(self.full)
        while True:   # encodable, not in the table (a one-position key has no such key: then an unencodable one)
            key = tuple(bytes(a[int(rng.integers(0, len(a)))] for a in alph) for alph, _ in self.case.cols)
            if key not in have:
                return key
            if self.case.total <= len(have):
                return tuple(b"`" * len(alph) for alph, _ in self.case.cols)

    def _probes(self, rng):
        case = self.case
        out = list(self.full) + list(self.extremes) + [self.absent]

        def mutated(key, c, q, byte):
            v = bytearray(key[c])
            v[q] = byte
            return key[:c] + (bytes(v),) + key[c + 1:]

        def bad_bytes(c, q):
            a = case.cols[c][0][q]
            gap = [b for b in range(a[0], a[-1]) if b not in a][:1]   # inside the range, not in the alphabet
            return [0x60, a[-1] + 1, 0x00, 0x80, 0xFF, a[0] - 1] + gap

        nc = len(case.cols)
        spots = [(self.kmax, 0, 0), (self.kmax, nc - 1, len(self.kmax[nc - 1]) - 1), (self.kmin, 0, 0)]
        for _ in range(6):
            key = self.full[int(rng.integers(0, len(self.full)))]
            c = int(rng.integers(0, nc))
            if len(key[c]):
                spots.append((key, c, int(rng.integers(0, len(key[c])))))
        for key, c, q in spots:
            if q < len(key[c]):
                out += [mutated(key, c, q, b) for b in bad_bytes(c, q)]
        for c in range(nc):   # the maximum key plus one more byte, minus its last byte; the empty value
            v = self.kmax[c]
            out.append(self.kmax[:c] + (v + v[-1:],) + self.kmax[c + 1:])
            out.append(self.kmax[:c] + (v[:-1],) + self.kmax[c + 1:])
            out.append(self.kmax[:c] + (b"",) + self.kmax[c + 1:])
        out.append(tuple(b"" for _ in range(nc)))
        return out

    def columns(self, rows):
        cols = [StrCol.from_values([k[c] for k in rows]) for c in range(len(self.case.cols))]
        return [c.as_variable() for c in cols] if self.case.variable else cols


@functools.lru_cache(maxsize=None)
def table_of(name):
    return Table(case_table()[name])


# ---- the CPU test: the fixtures sit where the table says ----------------------------------------------------------
def test_case_table_sits_on_the_thresholds():
    cases = case_table()
    for name, case in cases.items():
        t = table_of(name)
        assert len(t.full) < MAX_ROWS and len(t.probes) < MAX_PROBES, name
        assert max(sum(len(v) for v in k) for k in t.full) <= MAX_KEY or name.startswith("C-cols"), name
        assert max(len(v) for k in t.probes for v in k) <= MAX_KEY + 1, name
        assert len(t.unique) == len(set(t.full)) and len(t.unique) + 250 < len(t.full) or case.total < 2000, name
        for rows in (t.full, t.nomax, t.unique):
            if rows is None:
                assert case.npos == 1, name
                continue
            pc = PyCodec([[k[c] for k in rows] for c in range(len(case.cols))])
            assert pc.words == case.words, (name, pc.words)
            assert (pc.bits, pc.nwords, pc.key32, pc.npos) == (case.bits, case.nwords, case.key32, case.npos), name
            if case.nwords == 1:
                assert case.bits == bits_needed(case.words[0]), name
            has_max = rows is not t.nomax
            assert (t.kmax in rows) == has_max, name
            assert pc.encode(t.kmax) == case.total - 1 and pc.encode(t.kmin) == 0, name   # the probe still encodes to states - 1
            assert pc.encode(t.kpred) == max(case.total - 2, 0), name
            assert pc.decode(case.total - 1) == t.kmax, name
            # a several-word code goes to the dictionary stage: only the case marked so may gain from it
            if case.nwords > 1:
                assert dictionary_pays([[k[c] for k in rows] for c in range(len(case.cols))]) == case.dictionary, name
        assert [n for n, c in cases.items() if c.dictionary] == ["B-r8x22"]

    def one(c):
        return c.nwords == 1

    def s(c):
        return c.words[0]

    # (rule, a case just at the threshold, a case just over it)
    both_sides = {
        "codec_split_words: 2^63 stays one word": (lambda c: one(c) and s(c) == 1 << 63, lambda c: c.nwords == 2 and c.words[0] == 1 << 63),
        "codec_split_words: two words, three words": (lambda c: c.nwords == 2 and c.total == 1 << 126, lambda c: c.nwords == 3),
        "key32: states <= 2^32": (lambda c: c.key32 and s(c) == 1 << 32, lambda c: one(c) and not c.key32 and 1 << 32 < s(c) < 1 << 33),
        "32-bit LUT: states <= 2^31": (lambda c: premultiplied_bits(c.words, c.npos) == 32 and s(c) == 1 << 31,
                                       lambda c: premultiplied_bits(c.words, c.npos) == 64 and s(c) == 3 << 30),
        "32-bit LUT: 47 positions": (lambda c: premultiplied_bits(c.words, c.npos) == 32 and c.npos == 47,
                                     lambda c: one(c) and s(c) <= 1 << 31 and c.npos == 48 and premultiplied_bits(c.words, c.npos) == 0),
        "64-bit LUT: 23 positions": (lambda c: premultiplied_bits(c.words, c.npos) == 64 and c.npos == 23,
                                     lambda c: one(c) and s(c) > 1 << 31 and c.npos == 24 and premultiplied_bits(c.words, c.npos) == 0),
        "saturating sum: largest valid sum 2^31 - 1": (lambda c: premultiplied_bits(c.words, c.npos) == 32 and c.total - 1 == (1 << 31) - 1,
                                                        lambda c: premultiplied_bits(c.words, c.npos) == 64 and c.key32),
        "codec_arith_plan: states <= 2^31": (lambda c: c.fixed8 and arith_plan_applies(c) and s(c) == 1 << 31,
                                             lambda c: c.fixed8 and not arith_plan_applies(c) and s(c) == 1 << 32),
        "codec_arith_plan: contiguous ranges": (lambda c: c.fixed8 and arith_plan_applies(c), lambda c: c.fixed8 and not arith_plan_applies(c) and s(c) == 1 << 31),
        "host coder: states <= 2^31": (lambda c: c.fixed8 and host_coder_takes(c.words) and s(c) == 1 << 31,
                                       lambda c: c.fixed8 and not host_coder_takes(c.words) and s(c) == 3 << 30),
        "small build: states <= 2^63": (lambda c: small_build_fits(c.words, c.npos) and s(c) == 1 << 63, lambda c: c.nwords == 2 and c.npos <= K_SMALL_MAX_POS),
        "small build: 64 positions": (lambda c: small_build_fits(c.words, c.npos) and c.npos == 64, lambda c: one(c) and c.npos == 65),
        "small build: key32": (lambda c: small_build_fits(c.words, c.npos) and s(c) == 1 << 32, lambda c: small_build_fits(c.words, c.npos) and s(c) == (1 << 32) + (1 << 30)),
        "index_plan_table: states <= 2^20": (lambda c: plan_table_entries(c.words, 1800) == 1 << 20, lambda c: one(c) and s(c) == 1 << 21),
        "prefix search: vhi == states - 1, one word": (lambda c: len(c.cols) == 2 and one(c) and s(c) == 1 << 63, lambda c: len(c.cols) == 2 and c.nwords == 2),
        "prefix search: key32": (lambda c: len(c.cols) == 2 and c.key32 and s(c) == 1 << 32, lambda c: len(c.cols) == 2 and one(c) and s(c) == 1 << 33),
        "load check: code == states - 1": (lambda c: c.name in PERSIST and one(c), lambda c: c.name in PERSIST and c.nwords == 2),
    }
    for rule, (at, over) in both_sides.items():
        assert any(at(c) for c in cases.values()), "no case at the threshold of: " + rule
        assert any(over(c) for c in cases.values()), "no case over the threshold of: " + rule
    # radix_plan: every bits from 1 to 63 is its own (npass, rbits, digit widths); small_build: npass = (bits + 7) / 8
    assert {c.bits for c in cases.values() if one(c)} >= set(range(1, 64))
    for names in (LOOKUP_AB, PERSIST, SORT_SWITCH, HOST_CODER):
        assert set(names) <= set(cases)


# ---- the gpu checks ------------------------------------------------------------------------------------------------
def _cols(t, keys, ncols=None, variable=None):
    """Probe / stream columns of a list of key tuples (the leading ncols columns)."""
    nc = len(t.case.cols) if ncols is None else ncols
    cols = [StrCol.from_values([k[c] for k in keys]) for c in range(nc)]
    return [c.as_variable() for c in cols] if variable else cols


def _profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        out = fn()
        return out, ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)


def check_build(ctx, t, rows, path, unique=False):
    """Check 1: order, first duplicate, and the path info() and the profile show."""
    case = t.case
    cols = t.columns(rows)
    g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, cols, unique=unique))
    o = orc.OracleIndex(cols)
    np.testing.assert_array_equal(g.perm(), o.perm)
    assert g.first_dup == o.first_dup()
    assert g.status == (N.CPH_OK if (not unique or g.first_dup is None) else N.CPH_ERR_DUPLICATE)
    info = g.info()
    assert info["nrows"] == len(rows) and info["key_positions"] == case.npos
    if case.dictionary:   # codec_try_groups recoded the two-word plain code (module docstring)
        assert info["dict_entries"] > 0 and info["code_words"] <= case.nwords and info["code_bits"] < case.bits, info
        assert info["build_path"] == 0 and info["table_entries"] == 0
        return g, o, info, prof
    assert info["dict_entries"] == 0 and info["split"] == 0, info
    assert (info["code_bits"], info["code_words"], info["key_bytes"]) == (case.bits, case.nwords, 4 if case.key32 else 8), info
    small = path == "small_path" and small_build_fits(case.words, case.npos)
    assert info["build_path"] == (1 if small else 0), info
    assert ("k_small_build" in prof) == (path == "small_path"), sorted(prof)
    if not small:
        scatters = sum(v["launches"] for k, v in prof.items() if k.startswith("k_radix_scatter"))
        if not any(k.startswith(("k_cs_", "k_direct")) for k in prof):   # only the classic radix passes ran
            assert scatters == info["sort_passes"] == classic_passes(case.words), (info, sorted(prof))
    else:
        assert info["sort_passes"] == (case.bits + 7) // 8, info
    assert info["table_entries"] == plan_table_entries(case.words, len(rows)), info
    assert info["direct_table"] == (1 if info["table_entries"] else 0)
    return g, o, info, prof


def check_probe(t, g, o):
    """Check 2: pairs and bounds for the whole probe set."""
    pcols = _cols(t, t.probes)
    want = o.join(pcols)
    m = g.probe(pcols)
    assert_join_equal(m, want)
    m.release()
    assert_bounds_equal(g, pcols, want)
    return want


def check_find(t, g, o, ncols=None, keys=None):
    """Check 3: Find one by one and in one batch.  [lower, upper) are the positions of the equal keys: where there
    are none the library leaves the position open (csvplus_hip.h), so it is compared only for a non-empty range."""
    keys = [k[:ncols] for k in (keys if keys is not None else t.extremes + [t.absent])]
    lo, hi = g.find_many(keys)
    for j, key in enumerate(keys):
        olo, ohi = o.find(*key)
        glo, ghi = g.find(*key)
        for a, b in ((glo, ghi), (int(lo[j]), int(hi[j]))):
            assert b - a == ohi - olo and (ohi == olo or a == olo), (t.case.name, key, (a, b), (olo, ohi))


def check_chain(ctx, t, g, o, keys, ncols=None, expect_dense=None, variable=None):
    """Check 4: the chained Join of one step, reporting rows and reporting sorted positions (tests/test_gpu_chain.py)."""
    if not keys:
        return
    cols = _cols(t, keys, ncols, variable)
    want = o.join(cols, probe_base=7)
    ch, prof = _profiled(ctx, lambda: join_chain(ctx, [(g, cols)], probe_base=7))
    if expect_dense is not None:
        assert ("k_chain_dense" in prof) == expect_dense, (t.case.name, sorted(prof))
    assert ch.nrows == want["nmatches"] and not ch.positions
    np.testing.assert_array_equal(ch.stream_row, want["probe_idx"])
    np.testing.assert_array_equal(ch.build_row(0), want["build_row"])
    ch.release()
    chp, prof = _profiled(ctx, lambda: join_chain(ctx, [(g, cols)], probe_base=7, positions=True))
    if expect_dense is not None:
        assert ("k_chain_dense" in prof) == expect_dense, (t.case.name, sorted(prof))
    assert chp.positions and chp.nrows == want["nmatches"]
    np.testing.assert_array_equal(chp.stream_row, want["probe_idx"])
    pos = chp.build_row(0)
    assert len(pos) == 0 or int(pos.max()) < g.nrows
    np.testing.assert_array_equal(g.perm()[pos], want["build_row"])
    chp.release()


def dense_expected(case, info):
    """chain.hip: chain_fast_path_ok — one key column, a duplicate-free index, one word with a pre-multiplied LUT."""
    if case.dictionary:
        return None
    return len(case.cols) == 1 and premultiplied_bits(case.words, case.npos) != 0


def check_prefix(ctx, t, g, o):
    """Check 6: probe, Find and chain on column 0 alone; column 0's all-maximum value searches [v, v + mult - 1] with
    v + mult - 1 == states - 1."""
    assert_join_equal(g.probe(_cols(t, t.probes, 1)), o.join(_cols(t, t.probes, 1)))
    alph = t.case.cols[0][0]
    have = {k[0] for k in g_rows(t, g)}
    absent0 = next(v for v in (bytes(a[(i * 2654435761 >> q) & 1] for q, a in enumerate(alph)) for i in range(1, 1 << 16)) if v not in have)
    keys = [t.kmax, t.kmin, t.kfirst, t.kmirror, (absent0, b""), (t.kmax[0][:-1], b""), (t.kmax[0] + b"b", b"")]
    assert o.find(t.kmax[0])[1] == g.nrows   # the last group of the index: its upper bound is the end
    check_find(t, g, o, ncols=1, keys=keys)
    check_chain(ctx, t, g, o, t.probes, ncols=1)


def g_rows(t, g):
    return t.full if g.nrows == len(t.full) else t.nomax


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_code_width_case(ctx, both_build_paths, name):
    """Checks 1-4 and 6 for one case: the table with the all-maximum key, the table without it (the probe then encodes
    to states - 1 and misses), and the distinct keys under unique=True (the fused chain kernel)."""
    t = table_of(name)
    case = t.case
    for rows in (t.full, t.nomax):
        if rows is None:
            continue
        g, o, info, _ = check_build(ctx, t, rows, both_build_paths)
        want = check_probe(t, g, o)
        hit = want["cnt"][len(t.full) + 1] > 0   # the probe behind the build keys and kmin: the all-maximum key
        assert hit == (rows is t.full), name
        check_find(t, g, o)
        check_chain(ctx, t, g, o, t.probes, expect_dense=False if not case.dictionary else None)   # duplicates: the general chain
        if len(case.cols) == 2:
            check_prefix(ctx, t, g, o)
        g.close()
    g, o, info, _ = check_build(ctx, t, t.unique, both_build_paths, unique=True)
    assert g.first_dup is None and g.status == N.CPH_OK
    dense = dense_expected(case, info)
    check_chain(ctx, t, g, o, t.probes, expect_dense=dense)
    check_chain(ctx, t, g, o, t.probes_fixed, expect_dense=dense)
    if case.fixed8:
        assert dense and _cols(t, t.probes_fixed)[0].fixed_width == 8
        check_chain(ctx, t, g, o, t.probes_fixed, expect_dense=True, variable=True)
    check_find(t, g, o)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXED8)
def test_fixed8_chain_without_arith_and_identity(both_build_paths, name):
    """Check 4, second half: the 8-byte cases once more on a ctx of their own with chain_arith = 0 and
    chain_identity = 0 (the LUT walk and the rank table instead of the arithmetic encode and the code itself)."""
    t = table_of(name)
    c2 = Context(0)
    try:
        c2.set_option("chain_arith", 0)
        c2.set_option("chain_identity", 0)
        c2.set_option("small_build_rows", 16384 if both_build_paths == "small_path" else 0)
        g, o, info, _ = check_build(c2, t, t.unique, both_build_paths, unique=True)
        check_chain(c2, t, g, o, t.probes_fixed, expect_dense=True)
        check_chain(c2, t, g, o, t.probes, expect_dense=True)
        g.close()
    finally:
        c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOOKUP_AB)
def test_lookup_ab_join_hash_off(ctx, name, capsys):
    """Check 5: probe and chain with the hash probe switched off on a second ctx (the sorted search answers), and what
    lookup structure either ctx built."""
    t = table_of(name)
    c2 = Context(0)
    try:
        c2.set_option("join_hash", 0)
        built = {}
        for label, c in (("join_hash=1", ctx), ("join_hash=0", c2)):
            for rows, unique in ((t.full, False), (t.nomax, False), (t.unique, True)):
                cols = t.columns(rows)
                g, o = DeviceIndex(c, cols, unique=unique), orc.OracleIndex(cols)
                np.testing.assert_array_equal(g.perm(), o.perm)
                check_probe(t, g, o)
                check_find(t, g, o)
                check_chain(c, t, g, o, t.probes)
                info = g.info()
                built[label, len(rows)] = (info["lookup_built"], info["direct_table"])
                if c is c2:
                    assert info["lookup_built"] & 4 == 0 and info["hash_mode"] == 0, info   # no hash table on this ctx
                g.close()
        labels = sorted({k[1] for k in built})
        for nrows in labels:
            assert built["join_hash=1", nrows][1] == built["join_hash=0", nrows][1]   # the table decision is the ctx's neither way
        with capsys.disabled():
            print("\n%s lookup_built/direct_table: %s" % (name, built))
    finally:
        c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SORT_SWITCH)
def test_sort_switches_keep_the_order(ctx, name):
    """Check 7: the general path under sort_rbits 8 / 9 and sort_threads 256 / 512: the same permutation."""
    t = table_of(name)
    cols = t.columns(t.full)
    want = orc.OracleIndex(cols).perm
    bits = t.case.bits
    try:
        ctx.set_option("small_build_rows", 0)
        for rbits in (8, 9):
            for threads in (256, 512):
                ctx.set_option("sort_rbits", rbits)
                ctx.set_option("sort_threads", threads)
                g, prof = _profiled(ctx, lambda: DeviceIndex(ctx, cols))
                np.testing.assert_array_equal(g.perm(), want)
                info = g.info()
                assert info["build_path"] == 0 and info["code_bits"] == bits
                assert info["sort_passes"] == (bits + rbits - 1) // rbits, (rbits, threads, info)
                assert sum(v["launches"] for k, v in prof.items() if k.startswith("k_radix_scatter")) == info["sort_passes"]
                g.close()
    finally:
        ctx.set_option("sort_rbits", 0)
        ctx.set_option("sort_threads", 0)
        ctx.set_option("small_build_rows", 8192)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PERSIST)
def test_saved_index_keeps_the_last_code(ctx, tmp_path, name):
    """Check 8: save and load (tests/test_index_ops.py: test_gpu_save_load_roundtrip); the loaded index answers the
    probe set identically, and the load check (code >= word_states[w] is damage) accepts the code states - 1."""
    t = table_of(name)
    cols = t.columns(t.full)
    ix, o = DeviceIndex(ctx, cols), orc.OracleIndex(cols)
    path = tmp_path / "index.cph"
    ix.save(str(path))
    ld = N.DeviceIndex.load(ctx, str(path))
    assert ld.nrows == len(t.full)
    np.testing.assert_array_equal(ld.perm(), o.perm)
    a, b = ix.info(), ld.info()
    for k in ("code_bits", "code_words", "key_bytes", "key_positions", "table_entries"):
        assert a[k] == b[k], (k, a, b)
    check_probe(t, ld, o)
    check_find(t, ld, o)
    ld.close()
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASE_NAMES if len(case_table()[n].cols) == 1 and case_table()[n].nwords == 1
                                  and (case_table()[n].family == "B" or case_table()[n].name in ("A-b31", "A-b32", "A+first-b31", "Apad-b31"))])
def test_host_encoder_codes(ctx, name):
    """Check 9, at the tables' own size: the host coder (cph_host_encoder_create) takes a code of one word up to 2^31
    states and forms exactly the codes of the restated codec — 2^31 - 1 for the all-maximum key, ABSENT for a key the
    index cannot hold — and refuses one state more."""
    from csvplus_amd.streaming import HostEncoder

    t = table_of(name)
    case = t.case
    ix = DeviceIndex(ctx, t.columns(t.full))
    if not host_coder_takes(case.words):
        with pytest.raises(N.CphError):
            HostEncoder(ix)
        ix.close()
        return
    enc = HostEncoder(ix, nthreads=2)
    pc = PyCodec([[k[0] for k in t.full]])
    for keys, variable in ((t.probes, False), (t.probes_fixed, False), (t.probes_fixed, True)):
        codes = np.zeros(len(keys), np.uint32)
        enc.run(_cols(t, keys, variable=variable), codes)
        want = np.array([0xFFFFFFFF if (c := pc.encode(k)) is None else c for k in keys], dtype=np.uint32)
        np.testing.assert_array_equal(codes, want)
    assert pc.encode(t.kmax) == case.total - 1
    enc.close()
    ix.close()


HOST_ROWS = (1 << 20) + 4321


@pytest.mark.gpu
def test_host_coded_build_at_the_bound():
    """Check 9: IndexOn through host-formed codes (tests/test_gpu_host_build.py).  The host coder only takes tables of
    2^20 rows or more, so the rows of the two 8-byte cases are tiled to that size (all-maximum key included): at
    states == 2^31 the host codes the keys (build_path 2), at 3 * 2^30 it declines (build_path 0); the permutation
    is the device build's and the oracle's either way."""
    ctx = Context(0)
    try:
        for name, path in zip(HOST_CODER, (2, 0)):
            t = table_of(name)
            rng = np.random.default_rng([SEED, 99])
            base = np.frombuffer(b"".join(k[0] for k in t.full), np.uint8).reshape(len(t.full), 8)
            data = base[rng.integers(0, len(base), HOST_ROWS)]
            data[:len(base)] = base
            col = StrCol.from_arrays(np.ascontiguousarray(data).reshape(-1), (np.arange(HOST_ROWS + 1, dtype=np.uint64) * 8).astype(np.uint32))
            assert col.fixed_width == 8
            ctx.set_option("host_build", 1)
            h = DeviceIndex(ctx, [col])
            ctx.set_option("host_build", 0)
            g = DeviceIndex(ctx, [col])
            ctx.set_option("host_build", 1)
            hi, gi = h.info(), g.info()
            assert hi["build_path"] == path and gi["build_path"] == 0, (name, hi, gi)
            assert hi["code_bits"] == gi["code_bits"] == t.case.bits and hi["key_bytes"] == 4
            assert h.first_dup == g.first_dup
            np.testing.assert_array_equal(h.perm(), g.perm())
            o = orc.OracleIndex([col])
            np.testing.assert_array_equal(h.perm(), o.perm)
            pcols = _cols(t, t.probes)
            want = o.join(pcols)
            assert_join_equal(h.probe(pcols), want)
            h.close()
            g.close()
    finally:
        ctx.close()
