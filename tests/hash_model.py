"""A Python model of the Join hash table (csvplus_amd/csrc/hash_device.hpp, probe.hip: index_ensure_hash /
hash_build_partitioned): the hash itself, the sizing rule, and where entries end up under claim-the-first-empty-slot.

tests/test_hash_model_cpp.py pins the hash functions against the C++ ones line by line (tests/cpp/test_hash_model.hip);
tests/test_gpu_hash_edges.py uses the model to DESIGN tables — which pool keys to put into an index so that probe sequences
run long, cross the table end, or wrap inside a slice — and to count, before anything runs on the device, how many lookups
cross each of those edges.  A plain helper module: no fixtures, no tests.

Sector occupancy under claim-the-first-empty-slot does not depend on the insertion order (linear probing over buckets), so
for a key that is NOT in the table the number of sectors a lookup visits is exact: it stops at the first sector with an
empty slot.  For the keys that are in the table the model gives the exact NUMBER of entries pushed across every sector
boundary (carry), not which keys they are."""
import numpy as np

M64 = (1 << 64) - 1
HASH_SEED = 0x9E3779B97F4A7C15
HASH_NONE, HASH_K1, HASH_K3, HASH_TAG = 0, 1, 2, 3
SLICE_BITS = 10                       # hash_build_partitioned: slices of 1024 sectors = 64 KB
SLICE_SECTORS = 1 << SLICE_BITS
SECTOR_BYTES = 64


# ---- the hash, on Python ints -----------------------------------------------------------------------------------
def hash_fmix(h):
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def hash_step(s, word):
    return ((s ^ word) * 0x9FB21C651E98DF25 + 0x2545F4914F6CDD1D) & M64


def hash_finish(s):
    return hash_fmix(s)


def hash_one(code):
    return hash_finish(hash_step(HASH_SEED, code))


def hash_tag(h):
    return h & 0x7FFFFFFFFFFFFFFF


def hash_home(h, nsectors):
    return (((h >> 32) * nsectors) >> 32) & 0xFFFFFFFF


def hash_next_sector(s, nsectors, slice_mask=0):
    if slice_mask:
        return (s & ~slice_mask & 0xFFFFFFFF) | ((s + 1) & slice_mask)
    return 0 if s + 1 == nsectors else s + 1


def codes_hash(words):
    """probe.hip codes_hash: the code words of one key, most significant first."""
    s = HASH_SEED
    for w in words:
        s = hash_step(s, int(w))
    return hash_finish(s)


# ---- the same on numpy uint64 arrays (wrapping arithmetic) --------------------------------------------------------
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def np_hash_fmix(h):
    h = _u64(h).copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xFF51AFD7ED558CCD)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xC4CEB9FE1A85EC53)
    h ^= h >> np.uint64(33)
    return h


def np_hash_step(s, word):
    with np.errstate(over="ignore"):
        return (_u64(s) ^ _u64(word)) * np.uint64(0x9FB21C651E98DF25) + np.uint64(0x2545F4914F6CDD1D)


def np_codes_hash(words):
    """words: uint64 array [nwords][n], word-major, most significant word first (the layout of an index's sorted codes;
    a key32 index: its u32 codes widened, one word) -> uint64 hashes [n]."""
    words = _u64(words)
    if words.ndim == 1:
        words = words[None, :]
    with np.errstate(over="ignore"):
        s = np.full(words.shape[1], HASH_SEED, dtype=np.uint64)
        for w in words:
            s = np_hash_step(s, w)
        return np_hash_fmix(s)


def np_hash_home(h, nsectors):
    return (((_u64(h) >> np.uint64(32)) * np.uint64(nsectors)) >> np.uint64(32)).astype(np.int64)


# ---- sizing (probe.hip: index_ensure_hash, hash_build_partitioned) --------------------------------------------------
def slots_of(mode):
    return 2 if mode == HASH_K3 else 4


def clamp_pct(pct):
    return 25 if pct < 25 else 90 if pct > 90 else pct


def cas_sectors(distinct, mode, pct):
    """Sectors of the table built by compare-and-swap: one slot per DISTINCT key at pct per cent, plus one sector."""
    k = slots_of(mode) * clamp_pct(pct)
    return (distinct * 100 + k - 1) // k + 1


def sliced_sectors(distinct, mode, pct):
    """The slice-by-slice table: the same, rounded up to whole slices."""
    n = cas_sectors(distinct, mode, pct)
    return (n + SLICE_SECTORS - 1) >> SLICE_BITS << SLICE_BITS


def slice_giveup_bound(mode):
    """k_hash_window gives up on a slice with MORE than this many keys (S * slots * 15 / 16)."""
    cap = SLICE_SECTORS * slots_of(mode)
    return cap - cap // 16


# ---- occupancy ----------------------------------------------------------------------------------------------------
class Occupancy:
    """Where the entries of a table end up.  homes: home sector of every key in the table; slots: 4 or 2; slice_mask:
    0 = one ring over all nsectors (CAS build), else rings of slice_mask + 1 sectors.
      fill[s]   entries stored in sector s
      carry[s]  entries whose probe sequence went on from sector s to hash_next_sector(s) (s was full for them)"""

    def __init__(self, homes, nsectors, slots, slice_mask=0):
        self.nsectors, self.slots, self.slice_mask = int(nsectors), int(slots), int(slice_mask)
        ring = self.slice_mask + 1 if self.slice_mask else self.nsectors
        assert self.nsectors % ring == 0
        self.ring = ring
        homes = np.asarray(homes, dtype=np.int64)
        assert len(homes) == 0 or (0 <= homes.min() and homes.max() < self.nsectors)
        self.home_count = np.bincount(homes, minlength=self.nsectors).astype(np.int64)
        self.fill = np.zeros(self.nsectors, dtype=np.int64)
        self.carry = np.zeros(self.nsectors, dtype=np.int64)
        for r0 in range(0, self.nsectors, ring):
            cnt = self.home_count[r0:r0 + ring].tolist()
            assert sum(cnt) < ring * self.slots, "a ring without an empty slot: probe sequences would not end"
            carry_in, fill, carry = 0, [0] * ring, [0] * ring
            for _ in range(ring + 1):            # until the carry across the ring's end is a fixed point
                c = carry_in
                for i in range(ring):
                    t = cnt[i] + c
                    fill[i] = t if t < self.slots else self.slots
                    c = t - fill[i]
                    carry[i] = c
                if c == carry_in:
                    break
                carry_in = c
            else:
                raise AssertionError("no fixed point")
            self.fill[r0:r0 + ring] = fill
            self.carry[r0:r0 + ring] = carry
        assert int(self.fill.sum()) == len(homes)

    def next(self, s):
        return hash_next_sector(s, self.nsectors, self.slice_mask)

    def walk(self, home):
        """(sectors an ABSENT key homed here visits, does the walk go from a ring's last sector to its first)."""
        s, steps, wraps = int(home), 1, False
        while self.fill[s] >= self.slots:
            nx = self.next(s)
            wraps |= nx < s
            s = nx
            steps += 1
        return steps, wraps

    def walks(self, homes):
        """walk() for an array of homes -> (steps int64[n], wraps bool[n]); one walk per distinct home."""
        homes = np.asarray(homes, dtype=np.int64)
        steps = np.zeros(len(homes), dtype=np.int64)
        wraps = np.zeros(len(homes), dtype=bool)
        memo = {}
        for i, h in enumerate(homes.tolist()):
            if h not in memo:
                memo[h] = (1, False) if self.fill[h] < self.slots else self.walk(h)
            steps[i], wraps[i] = memo[h]
        return steps, wraps

    def ring_end(self, r):
        """The last sector of ring r (its carry = entries placed beyond the wrap)."""
        return (r + 1) * self.ring - 1


# ---- table design ---------------------------------------------------------------------------------------------------
def wrap_overfill(slots):
    """Home keys for the sectors (end-1, end, start, start+1) of a ring: with 4 slots 6, 6, 4, 3.  Sector end-1 pushes >= 2
    entries on, end >= 4 across the wrap, start >= 4, start+1 >= 3 into start+2 — whatever else the table holds."""
    return (slots + 2, slots + 2, slots, slots - 1)


def design_wrap_subset(pool_hashes, n, nsectors, slots, rng, slice_mask=0, per_ring=None):
    """Chooses n of the pool's keys (pool_hashes: uint64 hash of every pool key, all keys distinct) for a table of nsectors:
    in every ring the sectors end-1, end, start, start+1 get exactly wrap_overfill(slots) home keys, the rest of the table is
    filled at random from the keys homed elsewhere.  per_ring: keys per ring by home (default: whatever the random fill gives;
    one ring: n).  Returns the sorted pool indexes chosen.  Raises AssertionError when the pool cannot supply a sector."""
    homes = np_hash_home(pool_hashes, nsectors)
    ring = slice_mask + 1 if slice_mask else nsectors
    nrings = nsectors // ring
    assert ring >= 5 and nsectors % ring == 0
    if per_ring is None:
        assert nrings == 1
        per_ring = [n]
    assert len(per_ring) == nrings and sum(per_ring) == n
    order = rng.permutation(len(homes))
    by_home_sorted = order[np.argsort(homes[order], kind="stable")]
    starts = np.searchsorted(homes[by_home_sorted], np.arange(nsectors + 1))
    chosen = []
    for r in range(nrings):
        r0 = r * ring
        designated = {r0 + ring - 2: 0, r0 + ring - 1: 1, r0: 2, r0 + 1: 3}
        want = wrap_overfill(slots)
        taken = 0
        for s, k in designated.items():
            cand = by_home_sorted[starts[s]:starts[s + 1]]
            assert len(cand) >= want[k], f"sector {s}: {len(cand)} pool keys, {want[k]} wanted"
            chosen.append(cand[:want[k]])
            taken += want[k]
        rest = order[(homes[order] >= r0 + 2) & (homes[order] < r0 + ring - 2)]
        need = per_ring[r] - taken
        assert 0 <= need <= len(rest), f"ring {r}: {need} keys wanted, {len(rest)} in the pool"
        chosen.append(rest[:need])
    sel = np.sort(np.concatenate(chosen))
    assert len(sel) == n and len(np.unique(sel)) == n
    return sel


def wrap_preconditions(pool_hashes, sel, nsectors, slots, slice_mask=0):
    """What a designed table guarantees, per ring: dict with
      placed_beyond_wrap  entries stored after their probe sequence went from the ring's last sector to its first
      absent_walk3        pool keys NOT in the table whose lookup visits >= 3 sectors (homed in this ring)
      absent_cross        ... whose lookup crosses the ring's end
      longest             the longest absent walk, in sectors"""
    homes = np_hash_home(pool_hashes, nsectors)
    mask = np.zeros(len(homes), dtype=bool)
    mask[sel] = True
    occ = Occupancy(homes[mask], nsectors, slots, slice_mask)
    steps, wraps = occ.walks(homes[~mask])
    ring_of = homes[~mask] // occ.ring
    out = []
    for r in range(nsectors // occ.ring):
        m = ring_of == r
        out.append({"placed_beyond_wrap": int(occ.carry[occ.ring_end(r)]),
                    "absent_walk3": int((steps[m] >= 3).sum()),
                    "absent_cross": int(wraps[m].sum()),
                    "longest": int(steps[m].max()) if m.any() else 0,
                    "keys": int(occ.home_count[r * occ.ring:(r + 1) * occ.ring].sum())})
    return occ, out
