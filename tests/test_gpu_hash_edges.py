"""The Join hash table (csrc/hash_device.hpp, probe.hip) at the edges its five "home sector is full, go on" loops share:
probe sequences of several sectors, sequences that wrap from the last sector to sector 0, sequences that wrap at a SLICE
end back into the same slice, the slice that gives up, runs of duplicate keys behind the wrap, 32-bit codes, every load
factor, tables of two to four sectors — through k_probe<kLookHash>, k_probe_fast, the hash step of k_chain_dense,
k_window_lookup and k_hash_set_ends.

Nothing here hopes for a seed to produce an edge.  tests/hash_model.py restates the hash (pinned against the C++ by
tests/test_hash_model_cpp.py); DeviceIndex.select keeps the parent's codec and therefore its codes, which are read from
the parent's saved file (descriptor, sorted codes, perm).  So every test
  * builds a parent index over a POOL of keys (at least 24 per sector of the table to come — asserted),
  * computes every pool key's hash and home sector, chooses with the model which keys go into the table, selects them,
  * asserts its preconditions: the hash mode, hash_bytes == 64 * nsec by the restated sizing rule, the kernels that
    built the table, and the model's count of lookups that cross each edge,
  * probes with the whole pool (unselected pool keys are absent keys with known home sectors) plus keys that cannot be
    encoded, and with 2047 / 2048 / 2049 rows whose last rows are the edge keys (k_probe's tile is 2048 rows: a last
    tile of 2047 rows, none, and one of a single row),
  * compares with orc.OracleIndex built fresh over the selected rows; build rows are mapped back to parent rows.
For a key that is absent the model's walk length is exact; for the entries of the table it gives the exact number that
moved across each sector boundary (hash_model.Occupancy.carry).

k_probe_fast and the generic k_probe share the profile name k_probe_hash: which of them runs follows from the shape (one
key column with a one-word code and a pre-multiplied LUT -> k_probe_fast; two key columns or a multi-word code -> k_probe).

Left out on purpose: two distinct keys sharing a 64-bit tag (accel_failed) — constructing them means inverting the hash."""
import numpy as np
import pytest

from csvplus_amd import DeviceIndex, StrCol, join_chain
from oracle import orc
from tests import hash_model as hm
from tests.test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu

ALNUM36 = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
ALNUM62 = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
BYTES = np.arange(256, dtype=np.uint8)
HASH_BUILT = 4
TILE = 2048   # probe.hip kProbeTile

# kind -> (columns as (width | (min, max), alphabet), hash mode, code words (None: >= 4), key bytes, pool rows)
KINDS = {
    "k1": ([(12, ALNUM36)], hm.HASH_K1, 1, 8, 50_000),              # one 64-bit code word
    "k1_32": ([(5, ALNUM36)], hm.HASH_K1, 1, 4, 50_000),            # key32 codes, 36^5 states > max(24 n, 2^20): no direct table
    "k3_2w": ([(12, ALNUM62)], hm.HASH_K3, 2, 8, 50_000),
    "k3_3w": ([(16, BYTES)], hm.HASH_K3, 3, 8, 50_000),
    "tag": ([((20, 30), BYTES)], hm.HASH_TAG, None, 8, 50_000),
    "tag_win": ([((330, 400), BYTES)], hm.HASH_TAG, None, 8, 2_100),    # several codec windows
    "k1_2col": ([(5, ALNUM36), (6, ALNUM36)], hm.HASH_K1, 1, 8, 50_000),
    "k3_2col": ([(7, ALNUM62), (7, ALNUM62)], hm.HASH_K3, 2, 8, 50_000),
}
DUP_DISTINCT = 10_100   # distinct keys of a pool with duplicates (tables of 418 sectors: 24 * 418 = 10 032)


# ---- pools and parents -------------------------------------------------------------------------------------------------
def _column(rng, n, width, alphabet, prefix=b""):
    if isinstance(width, tuple):
        lens = rng.integers(width[0] - len(prefix), width[1] - len(prefix) + 1, n)
        mat = alphabet[rng.integers(0, len(alphabet), (n, width[1] - len(prefix)))]
        return [prefix + mat[i, :lens[i]].tobytes() for i in range(n)]
    raw = alphabet[rng.integers(0, len(alphabet), (n, width))].tobytes()
    return [raw[i * width:(i + 1) * width] for i in range(n)]


def make_pool(kind, seed, nrows):
    """nrows distinct keys as a list of columns (each a list of bytes)."""
    spec = KINDS[kind][0]
    rng = np.random.default_rng(seed)
    prefix = rng.integers(97, 123, 300, dtype=np.uint8).tobytes() if kind == "tag_win" else b""   # only the tail tells keys apart
    extra = nrows + nrows // 20 + 16
    cols = [_column(rng, extra, w, a, prefix) for w, a in spec]
    rows = list(dict.fromkeys(zip(*cols)))[:nrows]
    assert len(rows) == nrows
    return [list(c) for c in zip(*rows)]


def read_codes(ix, path):
    """The sorted codes of an index from its saved file: descriptor (desc_bytes at offset 8), codes, perm.
    -> (uint64 [words][n], perm uint32 [n])."""
    ix.save(str(path))
    raw = path.read_bytes()
    assert raw[:6] == b"CPHIDX"
    desc = int(np.frombuffer(raw[8:16], dtype=np.uint64)[0])
    n = int(np.frombuffer(raw[16:24], dtype=np.uint64)[0])
    inf = ix.info()
    assert n == ix.nrows == inf["nrows"]
    if inf["key_bytes"] == 4:
        assert len(raw) == desc + 8 * n
        codes = np.frombuffer(raw[desc:desc + 4 * n], dtype=np.uint32).astype(np.uint64)[None, :]
    else:
        nw = inf["code_words"]
        assert len(raw) == desc + (8 * nw + 4) * n
        codes = np.frombuffer(raw[desc:desc + 8 * nw * n], dtype=np.uint64).reshape(nw, n)
    perm = np.frombuffer(raw[len(raw) - 4 * n:], dtype=np.uint32)
    return codes, perm


class Parent:
    """An index over a pool, with what the model needs: per DISTINCT key (sorted order) its hash and its run of sorted positions."""

    def __init__(self, ctx, kind, cols, path):
        self.kind, self.cols, self.nrows = kind, cols, len(cols[0])
        self.mode = KINDS[kind][1]
        self.slots = hm.slots_of(self.mode)
        self.ix = DeviceIndex(ctx, [StrCol.from_values(c) for c in cols])
        inf = self.ix.info()
        words, key_bytes = KINDS[kind][2], KINDS[kind][3]
        assert inf["key_bytes"] == key_bytes and (inf["code_words"] == words if words else inf["code_words"] >= 4), inf
        codes, perm = read_codes(self.ix, path)
        np.testing.assert_array_equal(perm, self.ix.perm())
        self.perm = perm.astype(np.int64)
        head = np.ones(self.nrows, dtype=bool)
        head[1:] = (codes[:, 1:] != codes[:, :-1]).any(axis=0)
        self.run_start = np.flatnonzero(head)                       # sorted position of every distinct key's first row
        self.run_end = np.append(self.run_start[1:], self.nrows)
        self.ndistinct = len(self.run_start)
        self.hashes = hm.np_codes_hash(codes[:, self.run_start])    # per distinct key, sorted order
        # the codes tell the keys apart exactly as the bytes do
        keyrow = list(zip(*cols))
        assert self.ndistinct == len(set(keyrow))
        self.run_of_row = np.empty(self.nrows, dtype=np.int64)      # pool row -> distinct key
        self.run_of_row[self.perm] = np.repeat(np.arange(self.ndistinct), self.run_end - self.run_start)

    def positions(self, dsel):
        """Sorted positions of the whole runs of the distinct keys dsel (ascending)."""
        if self.ndistinct == self.nrows:
            return np.sort(dsel).astype(np.uint64)
        return np.concatenate([np.arange(self.run_start[d], self.run_end[d]) for d in np.sort(dsel)]).astype(np.uint64)


@pytest.fixture(scope="module")
def parent_of(ctx, tmp_path_factory):
    """Parents are built once per pool and shared by the tests (they are never changed: select makes new indexes)."""
    _parents = {}

    def get(kind, dups=False):
        key = (kind, dups)
        if key not in _parents:
            if dups:
                cols = make_pool(kind, 900 + len(kind), DUP_DISTINCT)
                rng = np.random.default_rng(77)
                rows = rng.permutation(np.repeat(np.arange(DUP_DISTINCT), rng.integers(1, 4, DUP_DISTINCT)))
                cols = [[c[r] for r in rows] for c in cols]
            else:
                cols = make_pool(kind, 500 + len(kind) + sum(kind.encode()), KINDS[kind][4])
            _parents[key] = Parent(ctx, kind, cols, tmp_path_factory.mktemp("parent") / "parent.cph")
        return _parents[key]

    yield get
    for par in _parents.values():
        par.ix.close()


# ---- a designed table ----------------------------------------------------------------------------------------------------
class Table:
    pass


def make_table(ctx, par, dsel, pct, partitioned, sliced, designed=True):
    """Selects the distinct keys dsel of the parent, builds the hash table under (hash_load_pct, hash_partitioned), and asserts
    what every test rests on: hash mode, the table's size by the restated rule, the kernels that built it.
    sliced: True = the slice-by-slice build must have answered; False = the CAS build alone; "gave_up" = both ran.
    designed: dsel puts chosen numbers of keys into chosen sectors, which takes a pool of 24 candidate keys per sector."""
    t = Table()
    t.par, t.dsel = par, np.sort(np.asarray(dsel))
    t.ndistinct = len(t.dsel)
    pos = par.positions(t.dsel)
    t.want = par.perm[pos.astype(np.int64)]                        # parent rows of the table's rows, in sorted order
    t.ix = par.ix.select(pos)
    assert t.ix.info()["direct_table"] == 0 and t.ix.info()["lookup_built"] == 0
    ctx.set_option("hash_load_pct", pct)
    ctx.set_option("hash_partitioned", partitioned)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        t.ix.prepare_join()
    finally:
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        ctx.set_option("hash_load_pct", 50)
        ctx.set_option("hash_partitioned", 1)
    inf = t.ix.info()
    assert inf["lookup_built"] == HASH_BUILT and inf["hash_mode"] == par.mode, inf
    t.mask = hm.SLICE_SECTORS - 1 if sliced is True else 0
    t.nsec = hm.sliced_sectors(t.ndistinct, par.mode, pct) if sliced is True else hm.cas_sectors(t.ndistinct, par.mode, pct)
    assert inf["hash_bytes"] == hm.SECTOR_BYTES * t.nsec, (inf, t.nsec)
    assert not designed or par.ndistinct >= 24 * t.nsec, (par.ndistinct, t.nsec)
    assert ("k_hash_window" in prof) == (sliced is not False) and ("k_hash_build" in prof) == (sliced is not True), sorted(prof)
    assert ("k_hash_homes" in prof) == (sliced is not False)
    t.in_table = np.zeros(par.ndistinct, dtype=bool)
    t.in_table[t.dsel] = True
    t.homes = hm.np_hash_home(par.hashes, t.nsec)                  # of every distinct pool key
    t.occ = hm.Occupancy(t.homes[t.in_table], t.nsec, par.slots, t.mask)
    t.steps, t.wraps = t.occ.walks(t.homes)                        # exact for the keys that are not in the table
    sub = [StrCol.from_values([c[r] for r in t.want]) for c in par.cols]
    t.o = orc.OracleIndex(sub)
    np.testing.assert_array_equal(t.o.perm, np.arange(len(t.want)))   # already in index order: oracle positions == index positions
    return t


def not_encodable(par, rng):
    """A few keys the codec cannot encode: a byte outside the alphabet, too long, empty."""
    rows = []
    for r in rng.integers(0, par.nrows, 5):
        key = [c[r] for c in par.cols]
        k = int(rng.integers(0, len(key)))
        bad = list(key)
        bad[k] = key[k][:-1] + b"!" if KINDS[par.kind][0][k][1] is not BYTES else key[k] + b"\x00" * 200
        rows.append(bad)
        rows.append([b""] * len(key))
        rows.append(key[:k] + [key[k] + key[k]] + key[k + 1:])
    return rows


def edge_rows(t):
    """Pool rows (one per distinct key) whose lookups cross an edge, the most interesting last: keys of the table homed in a
    full sector, absent keys that walk >= 3 sectors, absent keys that cross a ring's end."""
    par = t.par
    first_row = par.perm[par.run_start]                             # a pool row of every distinct key
    full_home = t.occ.fill[t.homes] >= par.slots
    present = np.flatnonzero(t.in_table & full_home)
    walk3 = np.flatnonzero(~t.in_table & (t.steps >= 3))
    cross = np.flatnonzero(~t.in_table & t.wraps)
    ring_end_homes = np.flatnonzero(t.in_table & np.isin(t.homes % t.occ.ring, [t.occ.ring - 2, t.occ.ring - 1, 0, 1]))
    d = np.concatenate([present, walk3, ring_end_homes, cross])
    return first_row[d]


def run_probes(ctx, t, rng, expect_kernel):
    """The whole pool + not-encodable keys, then 2047 / 2048 / 2049 rows ending in the edge keys; pairs and counts only."""
    par = t.par
    bad = not_encodable(par, rng)
    edge = edge_rows(t)[-1500:]
    probes = [(np.arange(par.nrows), bad)]
    for length in (TILE - 1, TILE, TILE + 1):
        filler = rng.integers(0, par.nrows, length - len(edge) - 3)
        probes.append((np.concatenate([filler, edge]), bad[:3]))
    for rows, extra in probes:     # the not-encodable keys first, the edge keys last
        cols = [StrCol.from_values([e[k] for e in extra] + [c[r] for r in rows]) for k, c in enumerate(par.cols)]
        oj = t.o.join(cols)
        # the oracle agrees with the model about what is in the table (one match per row of the key's run)
        runs = par.run_of_row[rows]
        expect_cnt = np.where(t.in_table[runs], par.run_end[runs] - par.run_start[runs], 0)
        np.testing.assert_array_equal(oj["cnt"][len(extra):], expect_cnt)
        assert not oj["cnt"][:len(extra)].any()
        ctx.profile(True)
        ctx.profile_read(reset=True)
        m = t.ix.probe(cols)
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert expect_kernel in prof and "k_probe_search" not in prof and "k_probe_window" not in prof, sorted(prof)
        np.testing.assert_array_equal(m.cnt, oj["cnt"])
        nz = m.cnt > 0
        np.testing.assert_array_equal(m.lo[nz], oj["lo"][nz])
        assert m.nmatches == oj["nmatches"]
        np.testing.assert_array_equal(m.probe_idx, oj["probe_idx"])
        np.testing.assert_array_equal(m.build_row, t.want[oj["build_row"].astype(np.int64)])
        m.release()
        m2 = t.ix.probe(cols, want_pairs=False)       # Except / counting: the same lookups without pairs
        np.testing.assert_array_equal(m2.cnt, oj["cnt"])
        np.testing.assert_array_equal(m2.lo[nz], oj["lo"][nz])
        m2.release()


def assert_wrap_preconditions(t):
    """Per ring of the table: >= 4 entries placed beyond the wrap, >= 8 absent probes walking >= 3 sectors, >= 2 absent probes
    crossing the ring's end (and so a longest walk of >= 5: end-1, end, start, start+1, start+2)."""
    par, occ = t.par, t.occ
    want = hm.wrap_overfill(par.slots)
    for r in range(t.nsec // occ.ring):
        r0 = r * occ.ring
        assert [int(occ.home_count[s]) for s in (r0 + occ.ring - 2, r0 + occ.ring - 1, r0, r0 + 1)] == list(want)
        assert occ.carry[occ.ring_end(r)] >= 4 and occ.carry[r0 + 1] >= 3
        m = ~t.in_table & (t.homes // occ.ring == r)
        print(f"{par.kind}: nsec {t.nsec} ring {r}: {int(occ.carry[occ.ring_end(r)])} entries beyond the wrap, absent walks >= 3: "
              f"{int((t.steps[m] >= 3).sum())}, absent across the end: {int(t.wraps[m].sum())}, longest absent walk {int(t.steps[m].max())}")
        assert int((t.steps[m] >= 3).sum()) >= 8 and int(t.wraps[m].sum()) >= 2 and int(t.steps[m].max()) >= 5


def wrap_table(ctx, par, n, partitioned, sliced, per_ring=None, seed=1):
    """The wrap design (hash_model.design_wrap_subset) at load 90 as a table, preconditions asserted."""
    rng = np.random.default_rng(seed)
    nsec = hm.sliced_sectors(n, par.mode, 90) if sliced else hm.cas_sectors(n, par.mode, 90)
    mask = hm.SLICE_SECTORS - 1 if sliced else 0
    dsel = hm.design_wrap_subset(par.hashes, n, nsec, par.slots, rng, mask, per_ring)
    t = make_table(ctx, par, dsel, 90, partitioned, sliced)
    assert t.nsec == nsec
    assert_wrap_preconditions(t)
    return t, rng


def probe_kernel(kind):
    return "k_window_lookup" if kind == "tag_win" else "k_probe_hash"


# ---- long sequences and the wrap, CAS build -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_cas_table_wraps_from_the_last_sector_to_sector_0(ctx, parent_of, kind):
    """hash_partitioned = 0, hash_load_pct = 90; sectors nsec-2, nsec-1, 0, 1 hold slots+2, slots+2, slots, slots-1 home keys
    (6, 6, 4, 3 with four slots), the rest of the table is random.  Asserted before any lookup: >= 4 entries placed beyond
    the wrap and >= 3 pushed on into sector 2, >= 8 absent probes walking >= 3 sectors, >= 2 absent probes crossing the
    table end, a longest absent walk of >= 5 sectors; hash_bytes == 64 * (ceil(100 n / (90 slots)) + 1); k_hash_build built
    it.  One table per entry format: K1 over 64-bit codes, K1 over key32 codes, K3 with two and with three words, tags,
    tags over several codec windows (k_window_lookup; n = 300 -> 85 sectors), and K1 / K3 over two key columns (generic k_probe;
    the one-column K1 tables go through k_probe_fast)."""
    par = parent_of(kind)
    n = 300 if kind == "tag_win" else 1500 if par.slots == 2 else 3000
    t, rng = wrap_table(ctx, par, n, 0, False)
    if kind == "tag_win":
        assert t.nsec == 85
    run_probes(ctx, t, rng, probe_kernel(kind))
    t.ix.close()


# ---- the chain kernel's hash step -----------------------------------------------------------------------------------------
def run_chain(ctx, t, rng, positions):
    """join_chain with the sparse table as one step next to a direct-table step: the fused kernel's own continuation code."""
    par = t.par
    npd = 700
    prod = [b"%d" % i for i in rng.permutation(npd)]
    dcol = [StrCol.from_values(prod)]
    d, od = DeviceIndex(ctx, dcol, unique=True), orc.OracleIndex(dcol)
    assert d.info()["direct_table"] == 1
    edge = edge_rows(t)
    rows = np.concatenate([np.arange(par.nrows), edge, rng.integers(0, par.nrows, 1500), edge])
    kc = StrCol.from_values([par.cols[0][r] for r in rows] + [b"!", b""])
    kp = [prod[i] for i in rng.integers(0, npd, len(rows) + 2)]
    kp[::9] = [b"nope"] * len(kp[::9])
    kp = StrCol.from_values(kp)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    ch = join_chain(ctx, [(t.ix, [kc]), (d, [kp])], probe_base=31, positions=positions)
    prof = ctx.profile_read(reset=True)
    ctx.profile(False)
    assert "k_chain_dense" in prof and not any(k.startswith("k_probe") for k in prof), sorted(prof)
    es, erows = oracle_chain([t.o, od], [kc, kp], 31)
    assert ch.nrows == len(es) and 0 < ch.nrows < len(rows) and ch.positions == positions
    np.testing.assert_array_equal(ch.stream_row, es)
    b0, b1 = ch.build_row(0), ch.build_row(1)
    if positions:
        b0, b1 = t.ix.perm()[b0], d.perm()[b1]
    np.testing.assert_array_equal(b0, t.want[erows[0].astype(np.int64)])
    np.testing.assert_array_equal(b1, erows[1])
    ch.release()
    d.close()


@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("kind", ["k1", "k1_32"])
def test_chain_hash_step_follows_the_wrap_of_a_cas_table(ctx, parent_of, kind, positions):
    """The CAS wrap table (same design and preconditions as above: >= 4 entries beyond the wrap, >= 8 absent walks of >= 3
    sectors, >= 2 absent probes across the table end) as one step of join_chain next to a direct-table step: hash_continue16 in
    k_chain_dense (asserted from the profile: no k_probe* ran), in both positions modes, for 64-bit and for key32 codes."""
    par = parent_of(kind)
    t, rng = wrap_table(ctx, par, 3000, 0, False, seed=2)
    run_chain(ctx, t, rng, positions)
    t.ix.close()


# ---- slices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["k1", "k1_32", "k3_2w", "k3_3w", "tag", "k1_2col", "k3_2col"])
def test_one_slice_wraps_inside_itself(ctx, parent_of, kind):
    """hash_partitioned = 2, load 90: n = 3680 (16-byte entries) / 1840 (K3) is exactly one 1024-sector slice, built by
    k_hash_window alone (k_hash_build must not run; hash_bytes == 65536).  Sectors 1022, 1023, 0, 1 are overfilled as in
    the CAS tables, with the same asserted minimums (>= 4 entries beyond the wrap, >= 8 absent walks >= 3, >= 2 absent
    probes across the slice end): the LDS build's (s + 1) & (S - 1) against the lookups' slice_mask step."""
    par = parent_of(kind)
    t, rng = wrap_table(ctx, par, 1840 if par.slots == 2 else 3680, 2, True)
    assert t.nsec == 1024
    run_probes(ctx, t, rng, probe_kernel(kind))
    t.ix.close()


def two_slice_n(par):
    return 3683 if par.slots == 2 else 7366   # ceil(100 n / (90 slots)) + 1 == 2048


@pytest.mark.parametrize("kind", ["k1", "k3_2w", "tag", "k1_2col"])
def test_two_slices_each_wrap_into_themselves(ctx, parent_of, kind):
    """n = 7366 (K3: 3683) at load 90 is two slices; by home, each slice gets half of the keys (3683 + 3683).  Sectors 1022-1023
    and 0-1 of slice 0 and 2046-2047 and 1024-1025 of slice 1 are overfilled.  Asserted PER SLICE: >= 4 entries placed after
    wrapping inside the slice, >= 8 absent walks of >= 3 sectors, >= 2 absent probes across the slice end; k_hash_window ran
    and k_hash_build did not; hash_bytes == 2 * 65536.  A lookup that went on from 1023 into 1024 would miss those keys (and
    one from 2047 would leave the table)."""
    par = parent_of(kind)
    n = two_slice_n(par)
    t, rng = wrap_table(ctx, par, n, 2, True, per_ring=[n // 2, n - n // 2])
    assert t.nsec == 2048 and t.occ.ring == 1024
    assert [int(t.occ.home_count[:1024].sum()), int(t.occ.home_count[1024:].sum())] == [n // 2, n - n // 2]
    run_probes(ctx, t, rng, probe_kernel(kind))
    t.ix.close()


@pytest.mark.parametrize("positions", [False, True])
def test_chain_hash_step_wraps_inside_a_slice(ctx, parent_of, positions):
    """The two-slice K1 table (3683 + 3683 keys, both slice ends overfilled, per-slice minimums as above) as a join_chain
    step: k_chain_dense's hash step with a slice mask."""
    par = parent_of("k1")
    t, rng = wrap_table(ctx, par, 7366, 2, True, per_ring=[3683, 3683], seed=3)
    run_chain(ctx, t, rng, positions)
    t.ix.close()


@pytest.mark.parametrize("kind", ["k1", "k3_2w"])
def test_a_slice_that_gives_up_is_rebuilt_by_cas(ctx, parent_of, kind):
    """Two slices (n = 7366; K3: 3683) with 3841 (K3: 1921) keys homed in slice 0 — one over k_hash_window's S * slots * 15 / 16:
    the slice build gives up and index_ensure_hash builds the table by CAS.  Asserted: k_hash_window AND k_hash_build ran,
    hash_bytes is the CAS size with no slice mask in the model, the wrap minimums hold for the table end (slice 1's end),
    and the answers are the oracle's."""
    par = parent_of(kind)
    n = two_slice_n(par)
    over = hm.slice_giveup_bound(par.mode) + 1
    assert over == (1921 if par.slots == 2 else 3841)
    rng = np.random.default_rng(4)
    dsel = hm.design_wrap_subset(par.hashes, n, 2048, par.slots, rng, hm.SLICE_SECTORS - 1, [over, n - over])
    t = make_table(ctx, par, dsel, 90, 2, "gave_up")
    assert t.nsec == 2048 == hm.cas_sectors(n, par.mode, 90) and t.mask == 0 and t.occ.ring == 2048
    assert int(t.occ.home_count[:1024].sum()) == over
    assert_wrap_preconditions(t)
    run_probes(ctx, t, rng, "k_probe_hash")
    t.ix.close()


# ---- duplicate keys -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["k1", "k3_2w"])
def test_duplicate_keys_behind_the_wrap(ctx, parent_of, kind):
    """A pool with every key 1-3 times, whole runs selected, the CAS wrap design over the DISTINCT keys (1500; K3: 750 -> 418
    sectors).  k_hash_set_ends must find its entry beyond the wrap (>= 4 entries there, asserted) to store the run's end:
    lo / cnt per probe row equal the oracle's.  hash_bytes is the size for the distinct count, not the row count
    (k_hash_count_heads) — the two differ, asserted."""
    par = parent_of(kind, dups=True)
    n = 750 if par.slots == 2 else 1500
    t, rng = wrap_table(ctx, par, n, 0, False, seed=5)
    assert t.nsec == 418 and len(t.want) > n + n // 2
    assert hm.cas_sectors(len(t.want), par.mode, 90) != t.nsec
    assert t.ix.info()["nrows"] == len(t.want)
    run_probes(ctx, t, rng, "k_probe_hash")
    t.ix.close()


# ---- load factors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partitioned", [0, 2])
@pytest.mark.parametrize("pct", [25, 50, 90, 10, 99])
@pytest.mark.parametrize("kind", ["k1", "k3_3w"])
def test_every_load_factor_sizes_the_table_by_the_rule(ctx, parent_of, kind, pct, partitioned):
    """hash_load_pct 25, 50, 90, and 10 / 99 which clamp to 25 / 90, over one random subset (3000 keys; K3: 1500), CAS and
    slice-by-slice: hash_bytes == 64 * nsec by the restated rule (make_table asserts it, and which kernels built the table),
    answers equal the oracle's."""
    par = parent_of(kind)
    rng = np.random.default_rng(6)
    n = 1500 if par.slots == 2 else 3000
    dsel = rng.permutation(par.ndistinct)[:n]
    t = make_table(ctx, par, dsel, pct, partitioned, partitioned == 2, designed=False)
    k = par.slots * hm.clamp_pct(pct)
    assert t.nsec >= -(-n * 100 // k) + 1 and (partitioned == 2) == (t.nsec % 1024 == 0)
    run_probes(ctx, t, rng, "k_probe_hash")
    t.ix.close()


# ---- degenerate sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("kind", ["k1", "k3_2w", "tag"])
def test_tables_of_two_to_six_sectors_at_load_90(ctx, parent_of, kind, n):
    """n = 1, 2, 4, 5, 8 keys at load 90 (CAS): 2 to 4 sectors (K3: 2 to 6).  All n keys are homed in the LAST sector, so
    n - slots entries are placed beyond the wrap and, from n >= slots on, every absent key homed there crosses the table end
    (both asserted, >= 2 such absent keys).  Probed with present, absent and not-encodable keys."""
    par = parent_of(kind)
    nsec = hm.cas_sectors(n, par.mode, 90)
    assert 2 <= nsec <= 6
    homes = hm.np_hash_home(par.hashes, nsec)
    last = np.flatnonzero(homes == nsec - 1)
    assert len(last) >= n + 2
    rng = np.random.default_rng(n)
    t = make_table(ctx, par, rng.permutation(last)[:n], 90, 0, False)
    assert t.nsec == nsec and t.occ.carry[nsec - 1] == max(0, n - par.slots)
    absent_last = ~t.in_table & (t.homes == nsec - 1)
    if n >= par.slots:
        assert int(t.wraps[absent_last].sum()) == int(absent_last.sum()) >= 2
        assert int(t.steps[absent_last].min()) == 2 + (n - par.slots) // par.slots
    else:
        assert not t.wraps.any()
    run_probes(ctx, t, rng, "k_probe_hash")
    t.ix.close()
