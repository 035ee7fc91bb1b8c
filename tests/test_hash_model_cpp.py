"""Pins tests/hash_model.py — the Python restatement of the Join hash table's hash, home sector and probe-sequence step —
against csvplus_amd/csrc/hash_device.hpp itself: tests/cpp/test_hash_model (host code only, built by hipcc, no HIP call)
prints hash_one / hash_tag / the multi-word hash / hash_home / hash_next_sector for a table of inputs, and the model must
reproduce every line.  The GPU edge tests (tests/test_gpu_hash_edges.py) design their tables with this model and assert
their preconditions from it: a wrong model would make those preconditions vacuous.

The second half runs the table DESIGN of those tests on synthetic random 64-bit codes standing in for real ones, a few
thousand times: with the pool size the GPU tests use (24 keys per sector) the design always finds its subset and every
precondition the GPU tests assert holds.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import hash_model as hm

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_hash_model"


@pytest.fixture(scope="module")
def cpp_lines():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_hash_model"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) > 5000
    return lines


def test_model_reproduces_every_line_of_the_cpp_program(cpp_lines):
    seen = {"one": 0, "multi": 0, "home": 0, "next": 0}
    nsecs, next_cases = set(), set()
    for f in cpp_lines:
        kind, v = f[0], [int(x) for x in f[1:]]
        seen[kind] += 1
        if kind == "one":
            code, h, tag = v
            assert hm.hash_one(code) == h and hm.hash_tag(h) == tag, f
            assert hm.codes_hash([code]) == h
            assert int(hm.np_codes_hash(np.array([code], dtype=np.uint64))[0]) == h, f
        elif kind == "multi":
            nw, words, h = v[0], v[1:-1], v[-1]
            assert len(words) == nw and hm.codes_hash(words) == h, f
            assert int(hm.np_codes_hash(np.array(words, dtype=np.uint64)[:, None])[0]) == h, f
        elif kind == "home":
            h, ns, home = v
            nsecs.add(ns)
            assert hm.hash_home(h, ns) == home and 0 <= home < ns, f
            assert int(hm.np_hash_home(np.array([h], dtype=np.uint64), ns)[0]) == home, f
        else:
            s, ns, mask, nx = v
            assert hm.hash_next_sector(s, ns, mask) == nx, f
            if mask:   # stays inside the slice
                assert nx // (mask + 1) == s // (mask + 1)
            next_cases.add((ns, mask, "slice0_end" if mask and s == mask else "slice1_end" if mask and s == 2 * mask + 1
                            else "end" if s == ns - 1 else "other"))
    assert seen["one"] >= 400 and seen["multi"] >= 300 and seen["home"] >= 5000 and seen["next"] >= 100, seen
    assert {2, 1024, 1025, 2048} <= nsecs
    # the wraps the GPU tests rest on are in the table: the table end without slices, both slice ends with them
    assert (1025, 0, "end") in next_cases and (2048, 0, "end") in next_cases and (2, 0, "end") in next_cases
    assert (2048, 1023, "slice0_end") in next_cases and (2048, 1023, "slice1_end") in next_cases
    assert hm.hash_next_sector(1023, 2048, 1023) == 0 and hm.hash_next_sector(2047, 2048, 1023) == 1024
    assert hm.hash_next_sector(2047, 2048, 0) == 0 and hm.hash_next_sector(1023, 2048, 0) == 1024


def test_sizing_rule():
    """index_ensure_hash / hash_build_partitioned restated: the sizes the issue's slice tables rest on."""
    assert hm.cas_sectors(3680, hm.HASH_K1, 90) == 1024 == hm.sliced_sectors(3680, hm.HASH_K1, 90)
    assert hm.cas_sectors(1840, hm.HASH_K3, 90) == 1024 == hm.sliced_sectors(1840, hm.HASH_K3, 90)
    assert hm.cas_sectors(7366, hm.HASH_TAG, 90) == 2048 == hm.sliced_sectors(7366, hm.HASH_K1, 90)
    assert hm.cas_sectors(3683, hm.HASH_K1, 90) == 1025 and hm.sliced_sectors(3683, hm.HASH_K1, 90) == 2048
    assert hm.cas_sectors(300, hm.HASH_TAG, 90) == 85
    assert [hm.cas_sectors(n, hm.HASH_K1, 90) for n in (1, 2, 4, 5, 8)] == [2, 2, 3, 3, 4]
    assert hm.cas_sectors(1000, hm.HASH_K1, 10) == hm.cas_sectors(1000, hm.HASH_K1, 25) == 1001
    assert hm.cas_sectors(1000, hm.HASH_K1, 99) == hm.cas_sectors(1000, hm.HASH_K1, 90) == 279
    assert hm.cas_sectors(1000, hm.HASH_K1, 50) == 501 and hm.cas_sectors(1000, hm.HASH_K3, 50) == 1001
    assert hm.slice_giveup_bound(hm.HASH_K1) == 3840 and hm.slice_giveup_bound(hm.HASH_K3) == 1920


def brute_force_table(homes, nsectors, slots, slice_mask):
    """Inserts key by key, in the given order, claiming the first empty slot: what k_hash_build / k_hash_window do."""
    fill = [0] * nsectors
    stored, crossed = [], []
    for h in homes:
        s, wrapped = int(h), False
        while fill[s] == slots:
            nx = hm.hash_next_sector(s, nsectors, slice_mask)
            wrapped |= nx < s
            s = nx
        fill[s] += 1
        stored.append(s)
        crossed.append(wrapped)
    return fill, stored, crossed


@pytest.mark.parametrize("slots", [4, 2])
def test_occupancy_is_the_brute_force_table_in_any_insertion_order(slots):
    rng = np.random.default_rng(7 + slots)
    for trial in range(300):
        mask = [0, 0, 3, 7][trial % 4]
        ring = mask + 1 if mask else int(rng.integers(2, 40))
        nsec = ring * (int(rng.integers(1, 4)) if mask else 1)
        cap = ring * slots
        homes = np.concatenate([r * ring + rng.integers(0, ring, int(rng.integers(0, cap))) ** (1 + trial % 2) % ring
                                for r in range(nsec // ring)]).astype(np.int64)
        occ = hm.Occupancy(homes, nsec, slots, mask)
        for order in (homes, homes[::-1], rng.permutation(homes)):
            fill, stored, crossed = brute_force_table(order, nsec, slots, mask)
            assert fill == occ.fill.tolist()
            for r in range(nsec // ring):
                inside = [c for h, c in zip(order, crossed) if h // ring == r]
                assert sum(inside) == occ.carry[occ.ring_end(r)]
        for h in range(nsec):
            steps, wraps = occ.walk(h)
            s, k, w = h, 1, False
            while occ.fill[s] == slots:
                nx = hm.hash_next_sector(s, nsec, mask)
                w |= nx < s
                s, k = nx, k + 1
            assert (steps, wraps) == (k, w)
            assert mask == 0 or s // ring == h // ring


def check_design(rng, n, mode, sliced, per_ring=None):
    """One trial of the GPU tests' design on synthetic codes: pool of 24 keys per sector, designed subset, preconditions."""
    slots = hm.slots_of(mode)
    nsec = hm.sliced_sectors(n, mode, 90) if sliced else hm.cas_sectors(n, mode, 90)
    mask = hm.SLICE_SECTORS - 1 if sliced else 0
    codes = rng.integers(0, 1 << 63, 24 * nsec, dtype=np.uint64)
    hashes = hm.np_codes_hash(codes)
    sel = hm.design_wrap_subset(hashes, n, nsec, slots, rng, mask, per_ring)
    occ, pre = hm.wrap_preconditions(hashes, sel, nsec, slots, mask)
    for p in pre:
        assert p["placed_beyond_wrap"] >= 4 and p["absent_walk3"] >= 8 and p["absent_cross"] >= 2 and p["longest"] >= 5, p
    if per_ring:
        assert [p["keys"] for p in pre] == list(per_ring)
    return pre


def test_design_finds_its_subset_on_synthetic_codes():
    """A few thousand trials: small and mid-size CAS tables in both slot counts, then the issue's own sizes — n = 3000 (CAS),
    3680 / 1840 (one slice), 7366 (two slices with 3683 keys each)."""
    rng = np.random.default_rng(2024)
    trials = 0
    for n in list(range(24, 124)) * 6 + [300] * 400 + [1000] * 100:
        check_design(rng, n, hm.HASH_K1, False)
        check_design(rng, max(12, n // 2), hm.HASH_K3, False)
        trials += 2
    for _ in range(40):
        check_design(rng, 3000, hm.HASH_K1, False)
        check_design(rng, 3000, hm.HASH_K3, False)
        check_design(rng, 3680, hm.HASH_K1, True)
        check_design(rng, 1840, hm.HASH_K3, True)
        check_design(rng, 7366, hm.HASH_K1, True, per_ring=[3683, 3683])
        trials += 5
    assert trials >= 2000


def model_lookup_misses(homes, nsec, slots, build_mask, step):
    """Builds the table key by key (claim the first empty slot, sequences wrapping as build_mask says) and looks every key up
    with `step` as the lookup's idea of the next sector (None: outside the table): the number of keys it does not find."""
    sectors = [[] for _ in range(nsec)]
    for k, h in enumerate(homes.tolist()):
        s = h
        while len(sectors[s]) == slots:
            s = hm.hash_next_sector(s, nsec, build_mask)
        sectors[s].append(k)
    missed = 0
    for k, h in enumerate(homes.tolist()):
        s, visited = h, 0
        while s is not None and k not in sectors[s] and len(sectors[s]) == slots and visited < nsec:
            s, visited = step(s, visited + 1), visited + 1
        missed += s is None or k not in sectors[s]
    return missed


def test_designed_tables_catch_a_wrong_step_in_a_model_lookup():
    """Why the GPU tests need no broken kernel to show that they bite: on the designed tables a lookup that steps wrongly at the
    table end, at a slice end, or stops after two sectors misses keys that are there — in a model of the lookup, on the CPU."""
    rng = np.random.default_rng(99)
    for mode in (hm.HASH_K1, hm.HASH_K3):
        slots = hm.slots_of(mode)
        # CAS table
        n = 3000 // (4 // slots)
        nsec = hm.cas_sectors(n, mode, 90)
        hashes = hm.np_codes_hash(rng.integers(0, 1 << 63, 24 * nsec, dtype=np.uint64))
        homes = hm.np_hash_home(hashes, nsec)[hm.design_wrap_subset(hashes, n, nsec, slots, rng)]
        assert model_lookup_misses(homes, nsec, slots, 0, lambda s, v: hm.hash_next_sector(s, nsec, 0)) == 0
        assert model_lookup_misses(homes, nsec, slots, 0, lambda s, v: s + 1 if s + 1 < nsec else None) >= 4       # no wrap
        assert model_lookup_misses(homes, nsec, slots, 0, lambda s, v: hm.hash_next_sector(s, nsec, 0) if v < 2 else None) >= 3
        # two slices
        n = 7366 // (4 // slots)
        mask = hm.SLICE_SECTORS - 1
        hashes = hm.np_codes_hash(rng.integers(0, 1 << 63, 24 * 2048, dtype=np.uint64))
        sel = hm.design_wrap_subset(hashes, n, 2048, slots, rng, mask, [n // 2, n - n // 2])
        homes = hm.np_hash_home(hashes, 2048)[sel]
        assert model_lookup_misses(homes, 2048, slots, mask, lambda s, v: hm.hash_next_sector(s, 2048, mask)) == 0
        # a lookup that ignores the slices: on from 1023 into 1024, from 2047 to 0
        assert model_lookup_misses(homes, 2048, slots, mask, lambda s, v: hm.hash_next_sector(s, 2048, 0)) >= 8
