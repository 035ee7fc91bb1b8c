"""Totals over a Join: Count / Sum / Min / Max per build row of a chain step on the device (cph_chain_aggregate,
csvplus_amd.aggregate.join_totals, pipeline.join_totals_to_csv) against aggregate.join_totals_model — the contract in pure
Python.  The group of every joined row is worked out HERE from the keys the test made (which build row carries the stream
row's key), never read back from the code under test.  Float values are multiples of 2^-10 below 2^20 unless a test says
otherwise, so every association order is exact and sums compare bit for bit."""
from __future__ import annotations

import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import aggregate as A
from tests.helpers import orders_table, people_table, stock_table

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
T = 1024        # rows per tile of k_jt_direct: kJtTile in csvplus_amd/csrc/join_totals.hip (which points back here)
RT = 2048       # rows per tile of the segmented reduce the float Sum route shares with Totals: kResTile, runs_device.hpp
L = N.CPH_CHAIN_AGG_LDS_GROUPS
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
OPS = [A.Sum, A.Min, A.Max]
SORT_ROWS = 1 << 20   # kJtSortRows: joined rows from which a table above the LDS limit is reduced over sorted runs even without a float Sum
ROWS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_floats(got, want):
    """Bit for bit, except that any NaN equals any NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and bits(got[~nan]) == bits(want[~nan])


def exact_floats(rng, n):
    return [float(v) / 1024.0 for v in rng.integers(-(1 << 29), 1 << 29, n)]


def plain_group_by(groups, ngroups, vals, op, is_float):
    """dict of lists, then one plain reduction per group; a group without rows gives 0."""
    d = {}
    for g, v in zip(groups, vals):
        d.setdefault(int(g), []).append(v)
    out = []
    for g in range(ngroups):
        vs = d.get(g)
        if not vs:
            out.append(0.0 if is_float else 0)
        elif op is A.Sum:
            s = math.fsum(vs) if is_float else sum(vs)
            out.append(s if is_float else (s + (1 << 63)) % (1 << 64) - (1 << 63))
        elif is_float and any(v != v for v in vs):
            out.append(math.nan)
        elif is_float and all(v == 0 for v in vs):   # -0 sorts below +0
            neg = any(math.copysign(1.0, v) < 0 for v in vs)
            pos = any(math.copysign(1.0, v) > 0 for v in vs)
            out.append((-0.0 if neg else 0.0) if op is A.Min else (0.0 if pos else -0.0))
        else:
            out.append(min(vs) if op is A.Min else max(vs))
    return [len(d.get(g, ())) for g in range(ngroups)], out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_join_totals_model_against_a_dict_of_lists():
    rng = np.random.default_rng(7)
    for _ in range(200):
        n, ng = int(rng.integers(0, 60)), int(rng.integers(1, 12))
        groups = [int(g) for g in rng.integers(0, ng, n)]
        if ng > 2:
            groups = [g for g in groups if g != 1]   # an empty group among the others
            n = len(groups)
        ints = [int(v) for v in rng.integers(-(1 << 62), 1 << 62, n)]
        floats = [float(v) / 8.0 for v in rng.integers(-1000, 1000, n)]   # every order of addition is exact
        if n > 3:
            floats[int(rng.integers(0, n))] = [math.nan, math.inf, -math.inf, -0.0, 0.0][int(rng.integers(0, 5))]
        for op in OPS:
            m = A.join_totals_model(groups, ng, [ints, floats], [op(None, "int"), op(None, "float")])
            cnt, wi = plain_group_by(groups, ng, ints, op, False)
            _, wf = plain_group_by(groups, ng, floats, op, True)
            assert m["ngroups"] == ng and m["count"] == cnt and sum(cnt) == n
            assert m["values"][0] == wi
            if op is A.Sum:   # fsum of a list with a NaN (or inf - inf) is NaN too; -0.0 == 0.0
                assert all((a != a and b != b) or a == b for a, b in zip(m["values"][1], wf))
            else:
                assert same_floats(m["values"][1], wf)
    assert A.join_totals_model([], 0) == {"ngroups": 0, "count": [], "values": []}
    assert A.join_totals_model([], 3, [[]], [A.Sum(None, "float")]) == {"ngroups": 3, "count": [0, 0, 0], "values": [[0.0, 0.0, 0.0]]}
    assert A.join_totals_model([2, 2, 0], 3)["count"] == [1, 0, 2]                     # no specs: counts only
    assert A.join_totals_model([0, 0], 1, [[INT64_MAX, 1]], [(N.CPH_AGG_SUM, N.CPH_NUM_INT64)])["values"] == [[INT64_MIN]]
    assert A.join_totals_model([0, 0], 1, [[INT64_MIN, -1]], [A.Sum(None, "int")])["values"] == [[INT64_MAX]]
    m = A.join_totals_model([0, 0, 1, 1, 2, 2, 3], 5, [[math.inf, math.nan, -0.0, 0.0, 0.0, -0.0, -0.0]] * 3,
                            [A.Min(None, "float"), A.Max(None, "float"), A.Sum(None, "float")])
    assert math.isnan(m["values"][0][0]) and math.isnan(m["values"][1][0])           # NaN beside +inf
    assert bits(m["values"][0][1:]) == bits([-0.0, -0.0, -0.0, 0.0]) and bits(m["values"][1][1:]) == bits([0.0, 0.0, -0.0, 0.0])
    assert bits(m["values"][2][3:]) == bits([-0.0, 0.0])                            # a sum starts from -0.0; an empty group is +0.0
    with pytest.raises(ValueError):
        A.join_totals_model([3], 3)


def test_join_totals_struct_sizes_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    s, f = N.cph_chain_agg_spec, N.cph_chain_aggregated
    sf = ["op", "kind", "numbers", "status", "numbers_mem", "reserved_"]
    ff = ["ngroups", "count", "values", "nspecs", "mem", "positions", "reserved_", "nerrors", "first_error_row", "first_error_kind",
          "first_error_spec"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("sizes %zu %zu\\n", sizeof(cph_chain_agg_spec), sizeof(cph_chain_aggregated));'
                   'printf("spec ' + "%zu " * len(sf) + '\\n", ' + ", ".join(f"offsetof(cph_chain_agg_spec, {x})" for x in sf) + ");"
                   'printf("offs ' + "%zu " * len(ff) + '\\n", ' + ", ".join(f"offsetof(cph_chain_aggregated, {x})" for x in ff) + ");"
                   'printf("lds %d\\n", CPH_CHAIN_AGG_LDS_GROUPS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert out["sizes"].split() == [str(C.sizeof(s)), str(C.sizeof(f))] == ["32", "120"]
    assert out["spec"].split() == [str(getattr(s, x).offset) for x in sf]
    assert out["offs"].split() == [str(getattr(f, x).offset) for x in ff]
    assert out["lds"].split() == [str(L)]


def test_join_totals_symbols_declared_exported_and_bound():
    lib = C.CDLL(str(N.LIB_PATH))
    bound = {p[0] for p in N.PROTOTYPES}
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    for name in ("cph_chain_aggregate", "cph_chain_aggregated_release"):
        assert hasattr(lib, name) and name in bound and re.search(r"CPH_API\s+\w+\s+%s\(" % name, hdr)
    assert "} cph_chain_aggregated;" in hdr and "} cph_chain_agg_spec;" in hdr
    from csvplus_amd import pipeline
    assert callable(A.join_totals) and callable(A.join_totals_model) and callable(pipeline.join_totals_to_csv)
    src = (ROOT / "csvplus_amd" / "csrc" / "join_totals.hip").read_text()
    assert "kJtTile" in src and "kJtRows = 4" in src and "kJtThreads = 256" in src and T == 256 * 4
    assert "kJtSortRows = 1ull << 20" in src and SORT_ROWS == 1 << 20


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def d2h(ptr, count, dtype):
    from tests.test_numeric import d2h as f
    return f(ptr, count, dtype)


def device_tensor(arr, keep):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")
    keep.append(t)
    return t


class Build:
    """A build table of `ng` distinct fixed-width keys in a shuffled row order, and its unique index."""

    def __init__(self, ctx, ng, seed, width=7):
        rng = np.random.default_rng(seed)
        self.ng = ng
        self.order = rng.permutation(ng)                       # order[r] = the number whose key sits in table row r
        self.keys = [b"%0*d" % (width, int(v)) for v in self.order]
        self.row_of = np.empty(ng, np.int64)
        self.row_of[self.order] = np.arange(ng)                # number -> table row; number == sorted position (zero padded)
        self.index = N.DeviceIndex(ctx, [StrCol.from_values(self.keys)], unique=True)
        assert self.index.status == N.CPH_OK
        self.width = width

    def stream(self, numbers):
        return StrCol.from_values([b"%0*d" % (self.width, int(v)) for v in numbers])

    def groups(self, numbers, positions):
        numbers = np.asarray(numbers, dtype=np.int64)
        return numbers if positions else self.row_of[numbers]

    def close(self):
        self.index.close()


def eight_specs(rng, n):
    """Every op x kind in one call (8 specs): values per joined row and the spec objects over them."""
    ints = [np.array([int(v) for v in rng.integers(-(1 << 40), 1 << 40, n)], dtype=np.int64) for _ in range(2)]
    flts = [np.array(exact_floats(rng, n), dtype=np.float64) for _ in range(2)]
    vals = [ints[0], ints[0], ints[0], flts[0], flts[0], flts[0], ints[1], flts[1]]
    mk = [A.Sum, A.Min, A.Max, A.Sum, A.Min, A.Max, A.Max, A.Sum]
    return vals, [c(v) for c, v in zip(mk, vals)]


def check(got, groups, ng, vals, specs, positions=None):
    want = A.join_totals_model(groups, ng, [v.tolist() for v in vals], specs)
    assert got.ngroups == ng == want["ngroups"]
    assert got.count.tolist() == want["count"]
    for s, sp in enumerate(specs):
        if sp.kind == N.CPH_NUM_FLOAT64:
            assert same_floats(got.values[s], want["values"][s]), (s, sp)
        else:
            assert got.values[s].dtype == np.int64 and got.values[s].tolist() == want["values"][s], (s, sp)
    if positions is not None:
        assert got.positions == positions


def numbers_for(rng, kind, n, ng):
    if kind == "one":            # every row hits one group: the contention extreme
        return np.full(n, ng // 2, dtype=np.int64)
    if kind == "half_empty":
        return 2 * rng.integers(0, max(ng // 2, 1), n)
    return rng.integers(0, ng, n)


@pytest.mark.gpu
@pytest.mark.parametrize("ng,kind", [(1, "one"), (3, "random"), (L - 1, "random"), (L, "random"), (L + 1, "random"), (L + 1, "one"),
                                     (2 * L, "one"), (L, "half_empty"), (8192, "random"), (8193, "half_empty")])
def test_gpu_rows_and_groups(ctx, ng, kind):
    """Row counts around the wave and the tile of the direct kernel x group tables on both sides of the LDS limit; ngroups at a
    power of two and one above it (the key bits of the sort route)."""
    rng = np.random.default_rng(ng * 31 + len(kind))
    b = Build(ctx, ng, seed=ng)
    try:
        for n in ROWS:
            positions = bool(n & 1)
            if n == 0:   # one stream row whose key the index lacks: no joined rows
                ch = N.join_chain(ctx, [(b.index, [StrCol.from_values([b"9999999"])])], out_mem=DEVICE, positions=positions)
                nums = np.zeros(0, np.int64)
            else:
                nums = numbers_for(rng, kind, n, ng)
                ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=positions)
            assert ch.nrows == n
            vals, specs = eight_specs(rng, n)
            got = A.join_totals(ch, 0, b.index, specs)
            check(got, b.groups(nums, positions), ng, vals, specs, positions)
            ch.release()
    finally:
        b.close()


def order_free_specs(rng, n):
    """No float Sum: below SORT_ROWS rows such a call goes through the atomics on every table size."""
    ints = np.array([int(v) for v in rng.integers(-(1 << 40), 1 << 40, n)], dtype=np.int64)
    flts = np.array(exact_floats(rng, n), dtype=np.float64)
    vals = [ints, ints, ints, flts, flts]
    return vals, [c(v) for c, v in zip([A.Sum, A.Min, A.Max, A.Min, A.Max], vals)]


@pytest.mark.gpu
@pytest.mark.parametrize("ng,kind", [(L + 1, "one"), (L + 1, "random"), (8193, "half_empty")])
def test_gpu_global_atomics_route(ctx, ng, kind):
    """Above the LDS limit without a float Sum: device-scope atomics on the table itself, the one-group extreme included."""
    rng = np.random.default_rng(ng * 17 + len(kind))
    b = Build(ctx, ng, seed=ng + 3)
    try:
        for n in ROWS[1:]:
            positions = not (n & 1)
            nums = numbers_for(rng, kind, n, ng)
            ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=positions)
            vals, specs = order_free_specs(rng, n)
            check(A.join_totals(ch, 0, b.index, specs), b.groups(nums, positions), ng, vals, specs, positions)
            check(A.join_totals(ch, 0, b.index), b.groups(nums, positions), ng, [], [], positions)
            ch.release()
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [SORT_ROWS - 1, SORT_ROWS])
def test_gpu_rows_at_the_sort_threshold_without_a_float_sum(ctx, n):
    """One row below kJtSortRows the atomics, at it the sorted runs — for Count, an int Sum and a float Max alike."""
    rng = np.random.default_rng(n)
    ng = L + 1
    b = Build(ctx, ng, seed=77)
    nums = rng.integers(0, ng, n)
    nums[nums == 9] = 10                                     # an empty group
    ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=True)
    assert ch.nrows == n
    vals = [rng.integers(-(1 << 40), 1 << 40, n), rng.integers(-(1 << 29), 1 << 29, n) / 1024.0]
    specs = [A.Sum(vals[0]), A.Max(vals[1])]
    got = A.join_totals(ch, 0, b.index, specs)
    check(got, nums, ng, vals, specs, True)
    assert int(got.count[9]) == 0 and int(got.values[0][9]) == 0 and bits([got.values[1][9]]) == bits([0.0])
    ch.release()
    b.close()


@pytest.mark.gpu
def test_gpu_every_group_exactly_one_row_and_no_specs(ctx):
    for ng in (1, 65, T + 1, L + 5):
        b = Build(ctx, ng, seed=ng + 1)
        nums = np.random.default_rng(ng).permutation(ng)
        ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE)
        vals, specs = eight_specs(np.random.default_rng(ng + 2), ng)
        check(A.join_totals(ch, 0, b.index, specs), b.groups(nums, False), ng, vals, specs, False)
        got = A.join_totals(ch, 0, b.index)                   # nspecs == 0: the counts only
        assert got.values == [] and got.count.tolist() == [1] * ng
        ch.release()
        b.close()


@pytest.mark.gpu
def test_gpu_a_run_across_the_tiles_of_the_segmented_reduce(ctx):
    """Sorted by group, group 5 covers more than three tiles of the reduce, between short groups on both sides."""
    rng = np.random.default_rng(11)
    ng = 40
    b = Build(ctx, ng, seed=3)
    n = 4 * RT + 321
    nums = rng.integers(0, ng, n)
    nums[rng.permutation(n)[:3 * RT + 100]] = 5
    ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=True)
    vals, specs = eight_specs(rng, n)
    got = A.join_totals(ch, 0, b.index, specs)
    check(got, b.groups(nums, True), ng, vals, specs, True)
    assert int(got.count[5]) > 3 * RT
    ch.release()
    b.close()


@pytest.mark.gpu
def test_gpu_two_step_chain_host_chain_numbers_and_out_mem(ctx):
    """Step 0 and step 1 of a fused two-step chain; the chain in host and in device memory; numbers on host and on device;
    out_mem host and device with identical bits."""
    rng = np.random.default_rng(21)
    b0, b1 = Build(ctx, 300, seed=5), Build(ctx, L + 77, seed=6, width=6)
    n = 2 * T + 99
    n0, n1 = rng.integers(0, b0.ng, n), rng.integers(0, b1.ng, n)
    vals, specs = eight_specs(rng, n)
    keep = []
    dev_specs = [type(sp)(device_tensor(v, keep), sp.kind_name) for sp, v in zip(specs, vals)]
    for positions in (False, True):
        results = []
        for mem in (HOST, DEVICE):
            ch = N.join_chain(ctx, [(b0.index, [b0.stream(n0)]), (b1.index, [b1.stream(n1)])], out_mem=mem, positions=positions)
            assert ch.nrows == n and ch.identity and ch.mem == mem            # stream_row == NULL: the identity
            for step, b, nums in ((0, b0, n0), (1, b1, n1)):
                g = b.groups(nums, positions)
                got = A.join_totals(ch, step, b.index, specs)
                check(got, g, b.ng, vals, specs, positions)
                same = A.join_totals(ch, step, b.index, dev_specs)
                dev = A.join_totals(ch, step, b.index, specs, out_mem=DEVICE)
                assert d2h(dev.count[0], b.ng, np.uint64).tolist() == got.count.tolist() == same.count.tolist()
                for s, sp in enumerate(specs):
                    dt = np.float64 if sp.kind == N.CPH_NUM_FLOAT64 else np.int64
                    assert d2h(dev.values[s][0], b.ng, dt).view(np.uint64).tolist() == got.values[s].view(np.uint64).tolist()
                    assert same.values[s].view(np.uint64).tolist() == got.values[s].view(np.uint64).tolist()
                dev.release()
                results.append(got)
            ch.release()
        for a, c in zip(results[:2], results[2:]):                            # host chain == device chain
            assert a.count.tolist() == c.count.tolist()
            assert all(x.view(np.uint64).tolist() == y.view(np.uint64).tolist() for x, y in zip(a.values, c.values))
    b0.close()
    b1.close()


@pytest.mark.gpu
def test_gpu_duplicate_key_index_and_unmatched_rows(ctx):
    """The general chain (stream_row set): an index with duplicate keys — a group is a BUILD ROW, every row of a run gets the
    stream rows of its key — and stream rows without a match."""
    rng = np.random.default_rng(31)
    nb = 500
    bkeys = [b"%03d" % int(v) for v in rng.integers(0, 120, nb)]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(bkeys)])
    order = sorted(range(nb), key=lambda r: (bkeys[r], r))   # the index's rows: key order, input order inside a run
    by_key = {}
    for p, r in enumerate(order):
        by_key.setdefault(bkeys[r], []).append((p, r))
    ns = T + 300
    skeys = [b"%03d" % int(v) for v in rng.integers(0, 140, ns)]   # 120..139: no match
    for positions in (False, True):
        ch = N.join_chain(ctx, [(ix, [StrCol.from_values(skeys)])], out_mem=DEVICE, positions=positions)
        groups = [pr[0 if positions else 1] for k in skeys for pr in by_key.get(k, ())]
        assert ch.nrows == len(groups) and not ch.identity
        vals, specs = eight_specs(rng, len(groups))
        check(A.join_totals(ch, 0, ix, specs), groups, nb, vals, specs, positions)
        ch.release()
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [6, L + 6])
def test_gpu_special_values(ctx, ng):
    """NaN beside +inf, -0 / +0 for Min and Max, an int Sum that wraps — on the LDS and on the global route."""
    nan, inf = math.nan, math.inf
    b = Build(ctx, ng, seed=9)
    per_group = [[inf, nan], [-0.0, 0.0], [0.0, -0.0, 0.0], [nan, -inf, 3.0], [-0.0, -0.0], [2.5]]
    ints_per = [[INT64_MAX, 1], [INT64_MIN, -1], [INT64_MAX, INT64_MAX, 2], [INT64_MIN, INT64_MAX, 0], [-1, 1], [7]]
    nums, fl, it = [], [], []
    assert [len(x) for x in per_group] == [len(x) for x in ints_per]
    for g, (fs, is_) in enumerate(zip(per_group, ints_per)):
        for f, i in zip(fs, is_):
            nums.append(g)
            fl.append(f)
            it.append(i)
    order = np.random.default_rng(2).permutation(len(nums))
    nums, fl, it = np.array(nums)[order], np.array(fl, np.float64)[order], np.array(it, np.int64)[order]
    ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=True)
    specs = [A.Min(fl), A.Max(fl), A.Sum(it), A.Min(it), A.Max(it)]
    got = A.join_totals(ch, 0, b.index, specs)
    check(got, nums, ng, [fl, fl, it, it, it], specs, True)
    assert bits(got.values[0][[0, 3]]) == bits(got.values[1][[0, 3]]) == [0x7FF8000000000001] * 2   # Go's math.NaN()
    assert bits(got.values[0][[1, 2, 4]]) == bits([-0.0] * 3) and bits(got.values[1][[1, 2, 4]]) == bits([0.0, 0.0, -0.0])
    assert got.values[2][:3].tolist() == [INT64_MIN, INT64_MAX, 0]
    ch.release()
    b.close()


def raw(ctx, chain_ptr, step, ix, arr, nspecs, out_mem=HOST):
    out = C.POINTER(N.cph_chain_aggregated)()
    rc = ctx.lib.cph_chain_aggregate(ctx.handle, chain_ptr, step, ix.handle if ix is not None else None, arr, nspecs, out_mem, C.byref(out))
    return rc, out


def raw_specs(pairs, keep, status=None):
    arr = (N.cph_chain_agg_spec * max(1, len(pairs)))()
    for i, (op, v) in enumerate(pairs):
        v = np.ascontiguousarray(v)
        keep.append(v)
        arr[i].op, arr[i].kind = op, N.CPH_NUM_FLOAT64 if v.dtype == np.float64 else N.CPH_NUM_INT64
        arr[i].numbers, arr[i].numbers_mem = v.ctypes.data, HOST
        if status is not None and status[i] is not None:
            keep.append(status[i])
            arr[i].status = status[i].ctypes.data
    return arr


@pytest.mark.gpu
def test_gpu_status_errors_are_data(ctx):
    b = Build(ctx, 50, seed=13)
    n = T + 40
    rng = np.random.default_rng(14)
    nums = rng.integers(0, 50, n)
    ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE)
    keep = []
    st0, st1, st2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    st0[T + 3] = N.CPH_NUM_ERR_RANGE
    st2[77] = N.CPH_NUM_ERR_DIV_ZERO
    st2[T + 3] = N.CPH_NUM_ERR_SYNTAX
    v = np.arange(n, dtype=np.int64)
    arr = raw_specs([(N.CPH_AGG_SUM, v), (N.CPH_AGG_MIN, v.astype(np.float64)), (N.CPH_AGG_SUM, v.astype(np.float64))], keep, [st0, st1, st2])
    for out_mem in (HOST, DEVICE):
        rc, out = raw(ctx, ch.ptr, 0, b.index, arr, 3, out_mem)
        r = out.contents
        assert rc == N.CPH_OK and r.nerrors == 3 and r.ngroups == 0 and not r.count and not any(r.values[i] for i in range(8))
        assert (r.first_error_row, r.first_error_kind, r.first_error_spec) == (77, N.CPH_NUM_ERR_DIV_ZERO, 2)
        ctx.lib.cph_chain_aggregated_release(out)
    st2[77] = 0                                              # now row T + 3 fails in specs 0 and 2: the lowest spec is named
    rc, out = raw(ctx, ch.ptr, 0, b.index, arr, 3)
    r = out.contents
    assert rc == N.CPH_OK and r.nerrors == 2 and (r.first_error_row, r.first_error_kind, r.first_error_spec) == (T + 3, N.CPH_NUM_ERR_RANGE, 0)
    ctx.lib.cph_chain_aggregated_release(out)
    st0[:] = 0
    st2[:] = 0
    rc, out = raw(ctx, ch.ptr, 0, b.index, arr, 3)           # all valid: the arrays are there
    r = out.contents
    assert rc == N.CPH_OK and r.nerrors == 0 and r.ngroups == 50 and r.first_error_row == 0xFFFFFFFFFFFFFFFF and r.nspecs == 3
    assert N._ptr_array(r.count, 50, np.uint64).tolist() == np.bincount(b.groups(nums, False), minlength=50).tolist()
    ctx.lib.cph_chain_aggregated_release(out)
    # the wrapper: a NumCol whose status is handed through
    from csvplus_amd.materialize import eval_number
    from csvplus_amd import expr as E
    den = np.ones(n, np.int64)
    den[5] = 0
    nc = eval_number(ctx, {}, E.IntArr(v) / E.IntArr(den), nrows=n, out_mem=DEVICE)
    with pytest.raises(A.TotalsError) as ei:
        A.join_totals(ch, 0, b.index, [A.Sum(nc, "int")])
    assert (ei.value.row, ei.value.kind, ei.value.spec, ei.value.nerrors) == (5, N.CPH_NUM_ERR_DIV_ZERO, 0, 1)
    nc.release()
    ch.release()
    b.close()


@pytest.mark.gpu
def test_gpu_invalid_arguments(ctx):
    b, small = Build(ctx, 50, seed=15), Build(ctx, 20, seed=16)
    n = 100
    nums = np.arange(n) % 50
    ch = N.join_chain(ctx, [(b.index, [b.stream(nums)])], out_mem=DEVICE, positions=True)
    keep = []
    v = np.arange(n, dtype=np.int64)
    ok = raw_specs([(N.CPH_AGG_SUM, v)], keep)

    def spec(**kw):
        a = raw_specs([(N.CPH_AGG_SUM, v)], keep)
        for k, x in kw.items():
            setattr(a[0], k, x)
        return a

    big = N.cph_chain()
    C.memmove(C.byref(big), ch.ptr, C.sizeof(big))
    big.nrows = 1 << 32
    cases = {
        "null chain": dict(chain=None), "null index": dict(ix=None), "step -1": dict(step=-1), "step nsteps": dict(step=1),
        "another index (fewer rows)": dict(ix=small.index), "nspecs -1": dict(nspecs=-1), "nspecs 9": dict(nspecs=N.CPH_AGG_MAX_SPECS + 1),
        "null specs": dict(arr=None), "op": dict(arr=spec(op=7)), "kind": dict(arr=spec(kind=3)), "numbers_mem": dict(arr=spec(numbers_mem=5)),
        "null numbers": dict(arr=spec(numbers=None)), "out_mem": dict(out_mem=9), "2^32 rows": dict(chain=C.pointer(big)),
    }
    for name, kw in cases.items():
        args = dict(chain=ch.ptr, step=0, ix=b.index, arr=ok, nspecs=1, out_mem=HOST)
        args.update(kw)
        rc, out = raw(ctx, args["chain"], args["step"], args["ix"], args["arr"], args["nspecs"], args["out_mem"])
        assert rc == N.CPH_ERR_INVALID and not out, name
        assert ctx.last_error(), name
    out = C.POINTER(N.cph_chain_aggregated)()
    assert ctx.lib.cph_chain_aggregate(None, ch.ptr, 0, b.index.handle, ok, 1, HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_chain_aggregate(ctx.handle, ch.ptr, 0, b.index.handle, ok, 1, HOST, None) == N.CPH_ERR_INVALID
    assert ctx.last_error()
    rc, out = raw(ctx, ch.ptr, 0, b.index, ok, 1)             # and the call still works afterwards
    assert rc == N.CPH_OK and out.contents.ngroups == 50
    ctx.lib.cph_chain_aggregated_release(out)
    one = Build(ctx, 1, seed=17)                              # an index of 1 row
    c1 = N.join_chain(ctx, [(one.index, [one.stream([0, 0, 0])])], out_mem=HOST)
    got = A.join_totals(c1, 0, one.index, [A.Sum(np.array([1.5, 2.5, -8.0]))])
    assert got.count.tolist() == [3] and got.values[0].tolist() == [-4.0]
    for x in (c1, ch):
        x.release()
    for x in (one, b, small):
        x.close()


@pytest.mark.gpu
def test_gpu_float_sums_on_inexact_data_are_within_the_summation_bound_and_reproducible(ctx):
    """The inputs of tests/test_totals.py::test_gpu_float_sums_are_within_the_summation_bound_and_reproducible, grouped by a
    Join instead of an index; its bound: (m - 1) * 2^-52 * sum|x| against math.fsum (any order of m - 1 additions, a factor 2
    of slack)."""
    rng = np.random.default_rng(53)
    n = 4 * RT + 321
    ids = rng.integers(0, 60, n)
    ids[100:100 + 3 * RT] = 7777
    vals = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).astype(np.float64)
    distinct = sorted(set(int(v) for v in ids))
    bkeys = [b"%04d" % v for v in distinct]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(bkeys)], unique=True)
    ng = len(distinct)
    groups = np.searchsorted(np.array(distinct), ids)          # table row == sorted position here
    ch = N.join_chain(ctx, [(ix, [StrCol.from_values([b"%04d" % int(v) for v in ids])])], out_mem=DEVICE)
    specs = [A.Sum(vals, "float"), A.Min(vals, "float"), A.Max(vals, "float")]
    got = A.join_totals(ch, 0, ix, specs)
    worst = 0.0
    for g in range(ng):
        run = vals[groups == g]
        m = len(run)
        assert int(got.count[g]) == m
        exact = math.fsum(run.tolist())
        bound = (m - 1) * 2.0 ** -52 * math.fsum(np.abs(run).tolist())
        err = abs(float(got.values[0][g]) - exact)
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (g, m, err, bound)
        assert float(got.values[1][g]) == run.min() and float(got.values[2][g]) == run.max()
    print(f"largest error / bound over {ng} groups: {worst:.3g}")
    assert int(got.count.max()) >= 3 * RT
    again = A.join_totals(ch, 0, ix, specs)
    assert all(bits(a) == bits(b) for a, b in zip(got.values, again.values))      # two calls: bit-identical
    dev = A.join_totals(ch, 0, ix, specs, out_mem=DEVICE)
    assert all(bits(d2h(p, c, np.float64)) == bits(b) for (p, c), b in zip(dev.values, got.values))   # and for every out_mem
    dev.release()
    keep = []
    same = A.join_totals(ch, 0, ix, [A.Sum(device_tensor(vals, keep), "float")])  # and wherever the numbers lie
    assert bits(same.values[0]) == bits(got.values[0])
    ch.release()
    ix.close()


def csv_text(table):
    names = list(table)
    return (",".join(names) + "\n" + "".join(",".join(r) + "\n" for r in zip(*[table[c] for c in names]))).encode()


@pytest.mark.gpu
def test_gpu_transformed_source_program(ctx):
    """TestTransformedSource at fixture size: orders joined with people and with the stock, amount = price * float64(qty),
    custAmounts[cust] += amount — one chain, the expression over the joined rows, totals per row of the people index.
    price * qty is not exact in binary, so the sums are compared with the model's left-to-right sums under the summation
    bound: both orders of m - 1 additions lie within (m - 1) * 2^-53 * sum|x| of the exact sum, hence within (m - 1) * 2^-52 *
    sum|x| of each other; the int Sum of qty and the counts are exact."""
    from csvplus_amd import expr as E

    people, stock, orders = people_table(), stock_table(), orders_table(n=3000)
    pix = N.DeviceIndex(ctx, [StrCol.from_values([s.encode() for s in people["id"]])], unique=True)
    six = N.DeviceIndex(ctx, [StrCol.from_values([s.encode() for s in stock["prod_id"]])], unique=True)
    col = lambda vs: StrCol.from_values([s.encode() for s in vs])   # noqa: E731
    ch = N.join_chain(ctx, [(pix, [col(orders["cust_id"])]), (six, [col(orders["prod_id"])])], out_mem=HOST)
    assert ch.nrows == 3000
    specs = [A.Sum(E.FloatCol("price") * E.ToFloat(E.IntCol("qty"))), A.Sum(E.IntCol("qty")), A.Max(E.FloatCol("price"))]
    got = A.join_totals(ch, 0, pix, specs, columns={"price": (col(stock["price"]), 1), "qty": col(orders["qty"])})
    ng = len(people["id"])
    groups = [int(c) for c in orders["cust_id"]]              # people ids are 0..119 in table order: the row IS the id
    price = [float(stock["price"][int(p)]) for p in orders["prod_id"]]
    qty = [int(q) for q in orders["qty"]]
    amount = [p * float(q) for p, q in zip(price, qty)]
    want = A.join_totals_model(groups, ng, [amount, qty, price], specs)
    assert got.count.tolist() == want["count"] and got.values[1].tolist() == want["values"][1]
    assert bits(got.values[2]) == bits(want["values"][2])
    for g in range(ng):
        run = [a for a, gg in zip(amount, groups) if gg == g]
        bound = (len(run) - 1) * 2.0 ** -52 * math.fsum(run)
        assert abs(float(got.values[0][g]) - want["values"][0][g]) <= bound, (g, len(run))
    ch.release()
    pix.close()
    six.close()


@pytest.mark.gpu
def test_gpu_join_totals_to_csv(ctx):
    """pipeline.join_totals_to_csv against the text built on the host from the model; qty / 4 is exact, so the float column
    compares as text too.  People 100..119 get no orders: matched_only drops them."""
    from csvplus_amd import expr as E
    from csvplus_amd import mapping as M
    from csvplus_amd import pipeline

    people, orders = people_table(), orders_table(n=2000)
    orders["cust_id"] = [str(int(c) % 100) for c in orders["cust_id"]]
    pt, ot = pipeline.read_table(ctx, csv_text(people)), pipeline.read_table(ctx, csv_text(orders))
    specs = [A.Sum(E.IntCol("qty")), A.Sum(E.ToFloat(E.IntCol("qty")) * 0.25), A.Max(E.IntCol("qty"))]
    ng = len(people["id"])
    groups = [int(c) for c in orders["cust_id"]]
    qty = [int(q) for q in orders["qty"]]
    want = A.join_totals_model(groups, ng, [qty, [q * 0.25 for q in qty], qty], specs)
    names = list(people)
    for matched_only in (False, True):
        lines = [",".join(names + ["orders", "qty", "quarter", "most"])]
        for r in sorted(range(ng), key=lambda r: people["id"][r].encode()):   # key order: strings.Compare on the ids
            if matched_only and want["count"][r] == 0:
                continue
            lines.append(",".join([people[c][r] for c in names] + [str(want["count"][r]), M.itoa(want["values"][0][r]).decode(),
                                                                  M.ftoa(want["values"][1][r], 2).decode(), str(want["values"][2][r])]))
        text = pipeline.join_totals_to_csv(ctx, ot, pt, ("id", "cust_id"), specs, names=["orders", "qty", "quarter", "most"],
                                           matched_only=matched_only, prec=2)
        assert text.decode().splitlines() == lines
        assert len(lines) == 1 + (100 if matched_only else 120)
    dev = pipeline.join_totals_to_csv(ctx, ot, pt, ("id", "cust_id"), specs, out_mem=DEVICE)
    assert dev.size > 0
    dev.release()
    pt.release()
    ot.release()


@pytest.mark.gpu
def test_gpu_a_device_result_is_a_child_of_its_ctx():
    """A device-resident JoinTotals is released with its ctx; afterwards release() does not call into the library."""
    own = N.Context(0)   # closed below: not the session's
    ix = N.DeviceIndex(own, [StrCol.from_values([b"a", b"b", b"c"])], unique=True)
    ch = N.join_chain(own, [(ix, [StrCol.from_values([b"b", b"a", b"b", b"c", b"b"])])], out_mem=DEVICE)
    specs = [A.Sum(np.arange(5, dtype=np.int64), "int")]
    t = A.join_totals(ch, 0, ix, specs, out_mem=DEVICE)
    assert t.ngroups == 3 and t.ptr and t in own._children
    host = A.join_totals(ch, 0, ix, specs)
    assert host.ptr is None and host.count.tolist() == [1, 3, 1] and host.values[0].tolist() == [1, 6, 3]
    own.close()
    assert t.ptr is None and ch.ptr is None and own.handle is None
    t.lib = None   # a call into the library would fail on this
    t.release()
    t.close()
