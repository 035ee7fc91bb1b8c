"""Totals: Count / Sum / Min / Max per key of an index on the device (cph_index_aggregate, csvplus_amd.aggregate.totals,
pipeline.totals_to_csv) against aggregate.totals_model — the contract in pure Python — over index.perm(), never against the
code under test."""
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
from oracle import orc
from tests.helpers import orders_table, random_keys, stock_table

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
T = 2048   # rows per tile of k_agg_heads / k_agg_reduce: kResTile in csvplus_amd/csrc/runs_device.hpp (which points back here)
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
OPS = [A.Sum, A.Min, A.Max]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_floats(got, want):
    """Bit for bit, except that any NaN equals any NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and bits(got[~nan]) == bits(want[~nan])


def plain_group_by(keys, vals, op, is_float):
    """dict of lists, then one plain reduction per key: first-seen order == key order for sorted keys."""
    groups = {}
    for k, v in zip(keys, vals):
        groups.setdefault(k, []).append(v)
    out = []
    for vs in groups.values():
        if op is A.Sum:
            s = math.fsum(vs) if is_float else sum(vs)
            out.append(s if is_float else (s + (1 << 63)) % (1 << 64) - (1 << 63))
        elif is_float and any(v != v for v in vs):
            out.append(math.nan)
        else:
            out.append(min(vs) if op is A.Min else max(vs))
    return list(groups), [len(v) for v in groups.values()], out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_totals_model_against_a_dict_of_lists():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(0, 50))
        keys = sorted(int(k) for k in rng.integers(0, 8, n))
        ints = [int(v) for v in rng.integers(-(1 << 62), 1 << 62, n)]
        floats = [float(v) / 8.0 for v in rng.integers(-1000, 1000, n)]   # every order of addition is exact
        if n > 3 and rng.integers(0, 2):
            floats[int(rng.integers(0, n))] = math.nan
        for op in OPS:
            m = A.totals_model(keys, [ints, floats], [op(None, "int"), op(None, "float")])
            ks, cnt, wi = plain_group_by(keys, ints, op, False)
            _, _, wf = plain_group_by(keys, floats, op, True)
            assert m["ngroups"] == len(ks) and m["count"] == cnt
            assert [keys[p] for p in m["first_position"]] == ks and all(p == 0 or keys[p - 1] != keys[p] for p in m["first_position"])
            assert m["values"][0] == wi
            if op is A.Sum:   # fsum of a list with a NaN is NaN too
                assert all((a != a and b != b) or a == b for a, b in zip(m["values"][1], wf))
            else:
                assert same_floats(m["values"][1], wf)
    m = A.totals_model([], [], [])
    assert m == {"ngroups": 0, "first_position": [], "count": [], "values": []}
    assert A.totals_model("aab")["count"] == [2, 1]                                   # no specs: keys and frequencies
    assert A.totals_model("aa", [[INT64_MAX, 1]], [(N.CPH_AGG_SUM, N.CPH_NUM_INT64)])["values"] == [[INT64_MIN]]


def test_go_min_max_pins():
    nan, inf = math.nan, math.inf
    assert bits([A.go_min(-0.0, 0.0), A.go_min(0.0, -0.0)]) == bits([-0.0, -0.0])
    assert bits([A.go_max(-0.0, 0.0), A.go_max(0.0, -0.0)]) == bits([0.0, 0.0])
    assert math.isnan(A.go_min(nan, 1.0)) and math.isnan(A.go_max(1.0, nan)) and math.isnan(A.go_min(-inf, nan)) and math.isnan(A.go_max(nan, inf))
    assert A.go_min(-inf, 3.0) == -inf and A.go_max(inf, 3.0) == inf and A.go_min(2.0, 3.0) == 2.0 and A.go_max(2.0, 3.0) == 3.0
    s = A.totals_model("aabbc", [[inf, -inf, nan, 1.0, -0.0]], [A.Sum(None, "float")])["values"][0]
    assert math.isnan(s[0]) and math.isnan(s[1]) and bits([s[2]]) == bits([-0.0])
    with pytest.raises(ValueError):
        A.Sum(None, "decimal")
    with pytest.raises(ValueError):
        A.Max(StrCol.from_values([b"1"]))          # a string column needs a kind
    assert A.Sum(np.zeros(2), None).kind == N.CPH_NUM_FLOAT64 and A.Min(np.zeros(2, np.int32)).kind == N.CPH_NUM_INT64


def test_totals_struct_sizes_and_enums_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("sizes %zu %zu\\n", sizeof(cph_agg_spec), sizeof(cph_aggregated));'
                   'printf("spec %zu %zu %zu %zu %zu\\n", offsetof(cph_agg_spec, op), offsetof(cph_agg_spec, kind), offsetof(cph_agg_spec, col), '
                   "offsetof(cph_agg_spec, numbers), offsetof(cph_agg_spec, numbers_mem));"
                   'printf("offs %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", offsetof(cph_aggregated, ngroups), '
                   "offsetof(cph_aggregated, first_position), offsetof(cph_aggregated, first_row), offsetof(cph_aggregated, count), "
                   "offsetof(cph_aggregated, values), offsetof(cph_aggregated, nspecs), offsetof(cph_aggregated, mem), "
                   "offsetof(cph_aggregated, nerrors), offsetof(cph_aggregated, first_error_position), offsetof(cph_aggregated, first_error_row), "
                   "offsetof(cph_aggregated, first_error_kind), offsetof(cph_aggregated, first_error_spec), offsetof(cph_aggregated, host_rows));"
                   'printf("enums %d %d %d %d\\n", CPH_AGG_SUM, CPH_AGG_MIN, CPH_AGG_MAX, CPH_AGG_MAX_SPECS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert out["sizes"].split() == [str(C.sizeof(N.cph_agg_spec)), str(C.sizeof(N.cph_aggregated))] == ["32", "144"]
    s, f = N.cph_agg_spec, N.cph_aggregated
    assert out["spec"].split() == [str(v.offset) for v in (s.op, s.kind, s.col, s.numbers, s.numbers_mem)]
    assert out["offs"].split() == [str(v.offset) for v in (f.ngroups, f.first_position, f.first_row, f.count, f.values, f.nspecs, f.mem,
                                                           f.nerrors, f.first_error_position, f.first_error_row, f.first_error_kind,
                                                           f.first_error_spec, f.host_rows)]
    assert out["enums"].split() == [str(v) for v in (N.CPH_AGG_SUM, N.CPH_AGG_MIN, N.CPH_AGG_MAX, N.CPH_AGG_MAX_SPECS)] == ["1", "2", "3", "8"]
    assert [c.op for c in OPS] == [1, 2, 3]


def test_totals_symbols_declared_exported_and_bound():
    lib = C.CDLL(str(N.LIB_PATH))
    bound = {p[0] for p in N.PROTOTYPES}
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    for name in ("cph_index_aggregate", "cph_aggregated_release"):
        assert hasattr(lib, name) and name in bound and re.search(r"CPH_API\s+\w+\s+%s\(" % name, hdr)
    assert "} cph_aggregated;" in hdr and "} cph_agg_spec;" in hdr
    from csvplus_amd import pipeline
    assert callable(A.totals) and callable(A.totals_model) and callable(pipeline.totals_to_csv) and issubclass(A.TotalsError, ValueError)
    assert "kResTile" in (ROOT / "csvplus_amd" / "csrc" / "runs_device.hpp").read_text()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def text_col(texts, device=False, layout="auto"):
    """layout: "auto" (fixed width when every value has one length), "o32" / "o64" (offsets of that width)."""
    sc = StrCol.from_values(texts) if layout == "auto" else StrCol.from_values(texts, offset_bits=int(layout[1:]), fixed_width=0)
    return sc.to_device() if device else sc


def ftext(v):
    """A decimal text the device converts to exactly v (v a multiple of 2**-10 of modest size)."""
    s = b"%.10f" % v
    assert float(s) == v
    return s


def check(ix, keycols, sources):
    """sources: [(spec, values by TABLE row as Python numbers)].  Device == model over index.perm(); returns the Totals."""
    perm = ix.perm()
    keys = [tuple(col[int(r)] for col in keycols) for r in perm]
    specs = [s for s, _ in sources]
    model = A.totals_model(keys, [[vals[int(r)] for r in perm] for _, vals in sources], specs)
    got = A.totals(ix, specs)
    assert got.ngroups == model["ngroups"]
    assert got.first_position.dtype == np.uint64 and got.first_position.tolist() == model["first_position"]
    assert got.first_row.dtype == np.uint32 and got.first_row.tolist() == [int(perm[p]) for p in model["first_position"]]
    assert got.count.dtype == np.uint64 and got.count.tolist() == model["count"]
    assert len(got.values) == len(specs)
    for i, sp in enumerate(specs):
        if sp.kind == N.CPH_NUM_INT64:
            assert got.values[i].dtype == np.int64 and got.values[i].tolist() == model["values"][i], (i, sp)
        else:
            assert got.values[i].dtype == np.float64 and same_floats(got.values[i], model["values"][i]), (i, sp)
    return got


def six_sources(rng, n, numbers=False, device=False, layout="auto"):
    """Every op x kind.  Ints of modest size; floats multiples of 2**-10 below 2**20: every order of addition is exact."""
    ints = [int(v) for v in rng.integers(-100000, 100000, n)]
    floats = [float(v) / 1024.0 for v in rng.integers(-(1 << 29), 1 << 29, n)]
    if numbers:
        si, sf = np.asarray(ints, np.int64), np.asarray(floats, np.float64)
    else:
        si, sf = text_col([b"%d" % v for v in ints], device, layout), text_col([ftext(v) for v in floats], device, layout)
    return [(op(si, "int"), ints) for op in OPS] + [(op(sf, "float"), floats) for op in OPS]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, T - 1, T, T + 1])
def test_gpu_sizes_around_the_wave_and_the_tile(ctx, n):
    rng = np.random.default_rng(200 + n)
    keys = sorted(b"%05d" % int(v) for v in rng.integers(0, max(1, n // 3) + 1, n))
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    check(ix, [keys], six_sources(rng, n))
    check(ix, [keys], six_sources(rng, n, numbers=True))
    got = check(ix, [keys], [])                                  # nspecs == 0: the distinct keys and their frequencies
    assert got.values == [] and int(got.count.sum()) == n and got.ngroups == len(set(keys))
    ix.close()


LONG = (T - 3, 3 * T + 2)   # a run of 2T+5 rows over four tiles: 3 rows, two whole tiles, 2 rows
LAYOUTS = {                 # tests/test_resolve.py::LAYOUTS without the winners: (rows, runs of equal keys)
    "run_across_the_tile_edge": (T + 10, [(T - 1, T + 1)]),
    "run_ends_at_the_tile_edge": (T + 10, [(T - 5, T)]),
    "run_starts_at_the_tile_edge": (T + 10, [(T, T + 4)]),
    "long_run_over_four_tiles": (3 * T + 10, [LONG]),
    "one_run_is_the_whole_index": (3 * T + 1, [(0, 3 * T + 1)]),
    "one_run_of_exactly_four_tiles": (4 * T, [(0, 4 * T)]),
    "all_keys_distinct": (T + 5, []),
    "last_row_inside_the_last_run": (T + 9, [(5, 9), (T + 6, T + 9)]),
    "last_row_outside_the_last_run": (T + 9, [(5, 9), (T + 5, T + 8)]),
    "runs_back_to_back_over_the_edge": (2 * T + 3, [(T - 4, T), (T, T + 3), (T + 3, 2 * T + 1)]),
    "long_runs_back_to_back": (5 * T, [(3, 2 * T), (2 * T, 4 * T + 1), (4 * T + 1, 5 * T)]),
}


def keys_with_runs(n, runs):
    """n ascending keys, all distinct except that the positions of every run [lo, hi) share one."""
    ids = np.arange(n)
    for lo, hi in runs:
        ids[lo:hi] = lo
    return [b"%07d" % int(i) for i in ids]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_gpu_run_layouts(ctx, name):
    n, runs = LAYOUTS[name]
    keys = keys_with_runs(n, runs)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    assert ix.perm().tolist() == list(range(n))   # sorted input, stable order: position p reads row p
    # a different value at every position: a dropped or doubled row changes the sum, a wrong row the minimum / maximum
    ints = [1000003 * p + 17 for p in range(n)]
    down = [5 * n - 3 * p for p in range(n)]
    floats = [1.0 + p / 1024.0 for p in range(n)]
    icol, fcol = text_col([b"%d" % v for v in ints]), text_col([ftext(v) for v in floats])
    sources = [(A.Sum(icol, "int"), ints), (A.Min(icol, "int"), ints), (A.Max(np.asarray(down), "int"), down),
               (A.Max(np.asarray(ints), "int"), ints), (A.Min(np.asarray(down), "int"), down),
               (A.Sum(np.asarray(floats), "float"), floats), (A.Min(fcol, "float"), floats), (A.Max(fcol, "float"), floats)]
    got = check(ix, [keys], sources)              # 8 specs in one call
    for lo, hi in runs:                           # and spelled out for the runs
        g = got.first_position.tolist().index(lo)
        assert int(got.count[g]) == hi - lo and int(got.values[0][g]) == sum(ints[lo:hi]) and int(got.values[1][g]) == ints[lo]
        assert int(got.values[2][g]) == down[lo] and int(got.values[3][g]) == ints[hi - 1] and float(got.values[7][g]) == floats[hi - 1]
    ix.close()


def shaped_keys(rng, shape, n):
    if shape == "key32":
        return [random_keys(rng, n, 0, 3, alphabet=np.frombuffer(b"abc", np.uint8))]
    if shape == "one_word":
        return [random_keys(rng, n, 3, 9, alphabet=np.frombuffer(b"0123456789", np.uint8), distinct=max(1, n // 3))]
    if shape == "multi_word":
        return [random_keys(rng, n, 10, 40, distinct=max(1, n // 4))]
    return [random_keys(rng, n, 0, 2, alphabet=np.frombuffer(b"xy", np.uint8)),
            random_keys(rng, n, 0, 2, alphabet=np.frombuffer(b"pq", np.uint8))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["key32", "one_word", "multi_word", "two_cols"])
def test_gpu_key_shapes_and_a_selected_index(ctx, shape):
    rng = np.random.default_rng(23)
    n = 3000
    keycols = shaped_keys(rng, shape, n)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(v) for v in keycols])
    check(ix, keycols, six_sources(rng, n))
    check(ix, keycols, six_sources(rng, n, numbers=True))
    # an index out of cph_index_select: its perm still names rows of the ORIGINAL table, and so do the value sources
    pos = np.flatnonzero(rng.integers(0, 3, n) > 0).astype(np.uint64)
    sub = ix.select(pos)
    assert sub.nrows == len(pos) < n
    check(sub, keycols, six_sources(rng, n))
    got = check(sub, keycols, six_sources(rng, n, numbers=True))
    uniq = sub.select(got.first_position)          # first_position is what cph_index_select takes: the distinct keys
    assert uniq.nrows == got.ngroups and uniq.perm().tolist() == got.first_row.tolist() and uniq.dup_groups()[0].size == 0
    for x in (uniq, sub, ix):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["auto", "o32", "o64"])
def test_gpu_value_columns_of_every_layout(ctx, device, layout):
    rng = np.random.default_rng(31)
    n = T + 300
    keys = [b"%03d" % int(v) for v in rng.integers(0, 400, n)]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    if layout == "auto":   # one length for every value: a fixed-width column
        ints = [int(v) for v in rng.integers(10000, 99999, n)]
        col = text_col([b"%d" % v for v in ints], device, layout)
        assert col.fixed_width == 5
        check(ix, [keys], [(op(col, "int"), ints) for op in OPS] + [(op(col, "float"), [float(v) for v in ints]) for op in OPS])
    else:
        src = six_sources(rng, n, device=device, layout=layout)
        assert not src[0][0].source.fixed_width
        assert check(ix, [keys], src).host_rows == 0
    ix.close()


def device_tensor(arr, keep):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")
    keep.append(t)
    return t


@pytest.mark.gpu
def test_gpu_numbers_on_host_and_device(ctx):
    rng = np.random.default_rng(41)
    n = 2 * T + 77
    keys = [b"%04d" % int(v) for v in rng.integers(0, 700, n)]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    ints = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, n)]
    floats = [float(v) / 1024.0 for v in rng.integers(-(1 << 29), 1 << 29, n)]
    keep = []
    ti, tf = device_tensor(np.asarray(ints, np.int64), keep), device_tensor(np.asarray(floats, np.float64), keep)
    host = check(ix, [keys], [(A.Sum(np.asarray(ints), "int"), ints), (A.Min(np.asarray(floats), "float"), floats)])
    dev = check(ix, [keys], [(A.Sum(ti, "int"), ints), (A.Min((tf.data_ptr(), n), "float"), floats),    # a tensor, a raw pointer
                             (A.Max(ti, "int"), ints), (A.Sum(tf, "float"), floats)])
    assert dev.values[0].tolist() == host.values[0].tolist() and bits(dev.values[1]) == bits(host.values[1])
    with pytest.raises(ValueError):
        A.totals(ix, [A.Sum(ti, "float")])          # an int64 tensor read as doubles
    ix.close()


@pytest.mark.gpu
def test_gpu_int_wrap_around_and_extremes(ctx):
    #        rows:  0     1     2     3     4     5     6
    keys = [b"b", b"a", b"b", b"a", b"c", b"b", b"c"]
    ints = [INT64_MAX, INT64_MIN, 1, -1, INT64_MIN, 5, INT64_MAX]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    assert ix.perm().tolist() == [1, 3, 0, 2, 5, 4, 6]
    for src in (text_col([b"%d" % v for v in ints]), np.asarray(ints, np.int64)):
        got = check(ix, [keys], [(op(src, "int"), ints) for op in OPS])
        assert got.values[0].tolist() == [INT64_MAX, INT64_MIN + 5, -1]          # a: MIN + -1 wraps; b: MAX + 1 + 5 wraps; c: MIN + MAX
        assert got.values[1].tolist() == [INT64_MIN, 1, INT64_MIN] and got.values[2].tolist() == [-1, INT64_MAX, INT64_MAX]
    # the wrap inside one run that spans tiles: T+5 times INT64_MAX
    n = T + 5
    one = N.DeviceIndex(ctx, [StrCol.from_values([b"k"] * n)])
    got = check(one, [[b"k"] * n], [(A.Sum(np.full(n, INT64_MAX, np.int64), "int"), [INT64_MAX] * n)])
    assert got.values[0].tolist() == [((n * INT64_MAX) + (1 << 63)) % (1 << 64) - (1 << 63)]
    one.close()
    ix.close()


@pytest.mark.gpu
def test_gpu_float_sums_are_within_the_summation_bound_and_reproducible(ctx):
    rng = np.random.default_rng(53)
    n = 4 * T + 321
    ids = rng.integers(0, 60, n)
    ids[100:100 + 3 * T] = 7777                       # one run over more than three tiles among the short ones
    keys = [b"%04d" % int(v) for v in ids]
    vals = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).astype(np.float64)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    perm = ix.perm()
    specs = [A.Sum(vals, "float"), A.Min(vals, "float"), A.Max(vals, "float")]
    got = A.totals(ix, specs)
    sv = vals[perm]
    worst = 0.0
    for g in range(got.ngroups):
        lo, m = int(got.first_position[g]), int(got.count[g])
        run = sv[lo:lo + m]
        exact = math.fsum(run.tolist())
        bound = (m - 1) * 2.0 ** -52 * math.fsum(np.abs(run).tolist())   # any order of m-1 additions, factor 2 of slack
        err = abs(float(got.values[0][g]) - exact)
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (g, m, err, bound)
        assert float(got.values[1][g]) == run.min() and float(got.values[2][g]) == run.max()
    print(f"largest error / bound over {got.ngroups} runs: {worst:.3g}")
    assert got.ngroups == len(set(keys)) and int(got.count.max()) >= 3 * T
    again = A.totals(ix, specs)
    assert all(bits(a) == bits(b) for a, b in zip(got.values, again.values))      # two calls: bit-identical
    from tests.test_numeric import d2h
    dev = A.totals(ix, specs, out_mem=DEVICE)
    assert all(bits(d2h(p, c, np.float64)) == bits(b) for (p, c), b in zip(dev.values, got.values))   # and for every out_mem
    dev.release()
    keep = []
    same = A.totals(ix, [A.Sum(device_tensor(vals, keep), "float")])              # and wherever the numbers lie
    assert bits(same.values[0]) == bits(got.values[0])
    ix.close()


@pytest.mark.gpu
def test_gpu_float_special_values(ctx):
    nan, inf = math.nan, math.inf
    runs = [[inf, -inf], [nan, 1.0], [1.0, nan, -inf], [inf, 1.0, nan], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [0.0, 0.0, 0.0],
            [inf, inf], [-inf, 5.0], [1.5], [nan], [-0.0], [3.0, -inf, inf], [2.0, -2.0], [1e308, 1e308], [-1e308, -1e308, 1.0]]
    texts = {"inf": b"inf", "-inf": b"-Inf", "nan": b"NaN"}
    keys, vals = [], []
    for k, run in enumerate(runs):
        keys += [b"%02d" % k] * len(run)
        vals += run
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    col = text_col([texts.get(repr(v), repr(v).encode()) for v in vals])
    for src in (col, np.asarray(vals, np.float64)):
        got = check(ix, [keys], [(op(src, "float"), vals) for op in OPS])
        s, lo, hi = (got.values[i].tolist() for i in range(3))
        assert math.isnan(s[0]) and math.isnan(s[1]) and math.isnan(s[2]) and math.isnan(s[3])      # inf - inf, NaN propagate
        assert bits(s[4:8]) == bits([0.0, 0.0, -0.0, 0.0]) and s[8] == inf and s[9] == -inf and s[15] == inf and s[16] == -inf
        assert math.isnan(s[13]) and s[14] == 0.0
        assert math.isnan(lo[1]) and math.isnan(lo[2]) and math.isnan(lo[3]) and math.isnan(lo[11])   # a NaN in the run gives NaN
        assert math.isnan(hi[1]) and math.isnan(hi[2]) and math.isnan(hi[3]) and math.isnan(hi[11])
        assert bits(lo[4:8]) == bits([-0.0, -0.0, -0.0, 0.0]) and bits(hi[4:8]) == bits([0.0, 0.0, -0.0, 0.0])
        assert (lo[0], hi[0], lo[9], hi[9], lo[13], hi[13]) == (-inf, inf, -inf, 5.0, -inf, inf)
        assert bits([lo[12], hi[12]]) == bits([-0.0, -0.0]) and (lo[10], hi[10]) == (1.5, 1.5)
    # the same special values at the tile edge: a NaN in the first tile of a run that ends in the third
    n = 2 * T + 9
    big = [1.0] * n
    big[T - 1], big[T + 1] = nan, -0.0
    keys2 = [b"k"] * n
    one = N.DeviceIndex(ctx, [StrCol.from_values(keys2)])
    got = check(one, [keys2], [(op(np.asarray(big), "float"), big) for op in OPS])
    assert all(math.isnan(float(v[0])) for v in got.values)
    one.close()
    ix.close()


@pytest.mark.gpu
def test_gpu_a_deferred_float_is_finished_on_the_host(ctx):
    keys = [b"a", b"b", b"a", b"b", b"a"]
    texts = [b"0.5", b"1.7976931348623157e308", b"0.25", b"1", b"123456789012345678901234"]
    vals = [float(t) for t in texts]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    got = check(ix, [keys], [(A.Max(text_col(texts), "float"), vals), (A.Min(text_col(texts), "float"), vals)])
    assert got.host_rows == 4 and got.values[0].tolist() == [vals[4], vals[1]] and vals[4] > 1e23   # 2 deferred rows x 2 specs
    assert check(ix, [keys], [(A.Sum(text_col([b"1"] * 5), "float"), [1.0] * 5)]).host_rows == 0
    ix.close()


def raw_aggregate(ctx, ix, specs, nspecs, out_mem=HOST):
    out = C.POINTER(N.cph_aggregated)()
    rc = ctx.lib.cph_index_aggregate(ctx.handle, ix.handle if ix else None, specs, nspecs, out_mem, C.byref(out))
    return rc, out


def raw_spec(op, kind, col=None, numbers=None, mem=HOST):
    s = N.cph_agg_spec()
    s.op, s.kind, s.numbers_mem = op, kind, mem
    if col is not None:
        s.col = C.pointer(col)
    if numbers is not None:
        s.numbers = numbers.ctypes.data
    return s


@pytest.mark.gpu
def test_gpu_conversion_errors_are_data(ctx):
    #        rows:  0     1      2                        3     4     5     6
    keys = [b"c", b"c", b"b", b"b", b"a", b"a", b"d"]
    texts = [b"1", b"zz", b"99999999999999999999", b"3", b"5", b"6", b"x"]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    assert ix.perm().tolist() == [4, 5, 2, 3, 0, 1, 6]
    good = np.arange(7, dtype=np.int64)
    # three bad values: the lowest bad position (2: the range error of row 2) is reported; the single row "d" is a group too
    with pytest.raises(A.TotalsError) as e:
        A.totals(ix, [A.Sum(good, "int"), A.Sum(text_col(texts), "int")])
    assert (e.value.position, e.value.row, e.value.kind, e.value.nerrors, e.value.spec) == (2, 2, N.CPH_NUM_ERR_RANGE, 3, 1)
    sc, keep = text_col(texts).as_c()
    arr = (N.cph_agg_spec * 2)(raw_spec(N.CPH_AGG_MAX, N.CPH_NUM_FLOAT64, col=sc), raw_spec(N.CPH_AGG_MIN, N.CPH_NUM_INT64, col=sc))
    rc, out = raw_aggregate(ctx, ix, arr, 2)
    r = out.contents
    assert rc == N.CPH_OK and r.ngroups == 0 and not r.first_position and not r.first_row and not r.count
    assert not any(r.values[i] for i in range(N.CPH_AGG_MAX_SPECS))
    # as floats "zz" (position 5) and "x" (6) fail, as ints also position 2: 5 values; position 2 belongs to spec 1
    assert (r.nerrors, r.first_error_position, r.first_error_row, r.first_error_kind, r.first_error_spec) == (5, 2, 2, N.CPH_NUM_ERR_RANGE, 1)
    ctx.lib.cph_aggregated_release(out)
    with pytest.raises(A.TotalsError) as e:
        A.totals(ix, [A.Min(text_col(texts, device=True), "float")])
    assert (e.value.position, e.value.row, e.value.kind, e.value.nerrors, e.value.spec) == (5, 1, N.CPH_NUM_ERR_SYNTAX, 2, 0)
    # the same input as numbers cannot fail
    got = check(ix, [keys], [(A.Sum(good, "int"), good.tolist())])
    assert got.values[0].tolist() == [9, 5, 1, 6] and got.count.tolist() == [2, 2, 2, 1]
    del keep
    ix.close()


@pytest.mark.gpu
def test_gpu_argument_errors_have_a_status_and_a_message(ctx):
    keys = [b"a", b"a", b"b"]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    sc, keep = text_col([b"1", b"2", b"3"]).as_c()
    short, keep2 = text_col([b"1", b"2"]).as_c()
    nums = np.arange(3, dtype=np.int64)
    one = lambda s: (N.cph_agg_spec * 1)(s)   # noqa: E731
    ok = one(raw_spec(N.CPH_AGG_SUM, N.CPH_NUM_INT64, col=sc))
    rc, out = raw_aggregate(ctx, ix, ok, 1)
    assert rc == N.CPH_OK and out.contents.ngroups == 2 and N._ptr_array(out.contents.values[0], 2, np.int64).tolist() == [3, 3]
    ctx.lib.cph_aggregated_release(out)
    rc, out = raw_aggregate(ctx, ix, None, 0)                                        # no specs: specs may be NULL
    assert rc == N.CPH_OK and N._ptr_array(out.contents.count, 2, np.uint64).tolist() == [2, 1] and out.contents.nspecs == 0
    ctx.lib.cph_aggregated_release(out)
    both = raw_spec(N.CPH_AGG_SUM, N.CPH_NUM_INT64, col=sc, numbers=nums)
    bad = [
        (dict(ix=None), "index"),
        (dict(nspecs=-1), "nspecs"),
        (dict(nspecs=9, specs=(N.cph_agg_spec * 9)(*[raw_spec(N.CPH_AGG_SUM, N.CPH_NUM_INT64, col=sc)] * 9)), "nspecs"),
        (dict(specs=None), "specs"),
        (dict(specs=one(raw_spec(0, N.CPH_NUM_INT64, col=sc))), "op"),
        (dict(specs=one(raw_spec(4, N.CPH_NUM_INT64, col=sc))), "op"),
        (dict(specs=one(raw_spec(N.CPH_AGG_MIN, 0, col=sc))), "kind"),
        (dict(specs=one(raw_spec(N.CPH_AGG_MIN, N.CPH_ORDER_BYTES, col=sc))), "kind"),
        (dict(specs=one(raw_spec(N.CPH_AGG_MAX, N.CPH_NUM_INT64, numbers=nums, mem=5))), "numbers_mem"),
        (dict(specs=one(both)), "exactly one"),
        (dict(specs=one(raw_spec(N.CPH_AGG_MAX, N.CPH_NUM_INT64))), "exactly one"),
        (dict(specs=one(raw_spec(N.CPH_AGG_MAX, N.CPH_NUM_INT64, col=short))), "fewer rows"),
        (dict(out_mem=7), "out_mem"),
    ]
    for kw, word in bad:
        args = dict(ix=ix, specs=ok, nspecs=1, out_mem=HOST)
        args.update(kw)
        rc, out = raw_aggregate(ctx, args["ix"], args["specs"], args["nspecs"], args["out_mem"])
        assert rc == N.CPH_ERR_INVALID and not out, kw
        assert word in ctx.last_error(), (kw, ctx.last_error())
    out = C.POINTER(N.cph_aggregated)()
    assert ctx.lib.cph_index_aggregate(None, ix.handle, ok, 1, HOST, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_index_aggregate(ctx.handle, ix.handle, ok, 1, HOST, None) == N.CPH_ERR_INVALID
    with pytest.raises(TypeError):
        A.totals(ix, [lambda rows: 0])
    with pytest.raises(N.CphError):
        A.totals(ix, [A.Sum(text_col([b"1", b"2"]), "int")])
    del keep, keep2
    ix.close()


@pytest.mark.gpu
def test_gpu_device_results(ctx):
    from tests.test_numeric import d2h
    keys = keys_with_runs(T + 9, [(5, 9), (T - 2, T + 3)])
    n = len(keys)
    ints = np.arange(n, dtype=np.int64) * 3 - 100
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    specs = [A.Sum(ints, "int"), A.Max(text_col([b"%d.5" % v for v in range(n)], device=True), "float")]
    want = A.totals(ix, specs)
    got = A.totals(ix, specs, out_mem=DEVICE)
    assert got.ngroups == want.ngroups == n - 3 - 4
    for (ptr, count), w in zip([got.first_position, got.first_row, got.count] + got.values,
                               [want.first_position, want.first_row, want.count] + want.values):
        assert count == want.ngroups and ptr and d2h(ptr, count, w.dtype).tolist() == w.tolist()
    got.release()
    got.release()   # idempotent
    empty = N.DeviceIndex(ctx, [StrCol.from_values([])])
    t = A.totals(empty, [A.Sum(np.zeros(0, np.int64), "int")], out_mem=DEVICE)
    assert t.ngroups == 0 and t.count == (0, 0) and t.values == [(0, 0)]
    t.release()
    empty.close()
    ix.close()


@pytest.mark.gpu
def test_gpu_simple_totals_end_to_end(ctx):
    """The reference's TestSimpleTotals (csvplus_test.go:516-571) at fixture size, the sum the comment above it promises:
    orders JOIN products, qty * price on the device, IndexOn(cust_id), Sum per customer; its own 1e-6 relative check."""
    import torch
    from csvplus_amd.materialize import to_float, to_int
    from tests.test_numeric import _hip

    orders, stock = orders_table(), stock_table()
    n = len(orders["qty"])
    prod_ix = N.DeviceIndex(ctx, [StrCol.from_values(stock["prod_id"])], unique=True)
    m = prod_ix.probe([StrCol.from_values(orders["prod_id"])])
    assert m.nmatches == n and m.probe_idx.tolist() == list(range(n))                 # every order has its product
    price = to_float(ctx, StrCol.from_values(stock["price"]), row_ids=np.asarray(m.build_row, dtype=np.uint32), out_mem=DEVICE)
    qty = to_int(ctx, StrCol.from_values(orders["qty"]), out_mem=DEVICE)
    assert price.nerrors == 0 and qty.nerrors == 0 and price.values[1] == qty.values[1] == n
    tq, tp = torch.empty(n, dtype=torch.int64, device="cuda:0"), torch.empty(n, dtype=torch.float64, device="cuda:0")
    for dst, src in ((tq, qty), (tp, price)):
        assert _hip().hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.values[0]), C.c_size_t(8 * n), 3) == 0   # device to device
    amount = tq.to(torch.float64) * tp
    torch.cuda.synchronize()
    cust_ix = N.DeviceIndex(ctx, [StrCol.from_values(orders["cust_id"])])
    got = A.totals(cust_ix, [A.Sum(amount, "float"), A.Sum(tq, "int")])
    cust = np.asarray([int(c) for c in orders["cust_id"]])
    price_of = {p: float(v) for p, v in zip(stock["prod_id"], stock["price"])}
    want = np.zeros(cust.max() + 1)
    np.add.at(want, cust, np.asarray([price_of[p] * int(q) for p, q in zip(orders["prod_id"], orders["qty"])]))
    want_qty = np.bincount(cust, weights=np.asarray([int(q) for q in orders["qty"]]))
    ids = [int(orders["cust_id"][int(r)]) for r in got.first_row]
    assert sorted(ids) == sorted(set(cust.tolist())) and got.ngroups == len(ids)
    assert got.count.tolist() == [int((cust == i).sum()) for i in ids]
    for g, i in enumerate(ids):
        total = float(got.values[0][g])
        assert abs((total - want[i]) / total) <= 1e-6, (i, total, want[i])            # csvplus_test.go:566
        assert int(got.values[1][g]) == int(want_qty[i])
    for x in (price, qty, m, cust_ix, prod_ix):
        x.release() if hasattr(x, "release") else x.close()


@pytest.mark.gpu
def test_gpu_totals_to_csv(ctx):
    from csvplus_amd import pipeline
    from csvplus_amd.mapping import MissingColumn

    orders = orders_table(n=3000)
    names = ["order_id", "cust_id", "prod_id", "qty"]
    text = (",".join(names) + "\n" + "".join(",".join(orders[c][i] for c in names) + "\n" for i in range(3000))).encode()
    table = pipeline.read_table(ctx, text)

    def model(by):
        order = sorted(range(3000), key=lambda i: tuple(orders[b][i].encode() for b in by))   # stable: input order inside a key
        keys = [tuple(orders[b][i] for b in by) for i in order]
        qty = [int(orders["qty"][i]) for i in order]
        oid = [int(orders["order_id"][i]) for i in order]
        m = A.totals_model(keys, [qty, oid, qty], [A.Sum(None, "int"), A.Min(None, "int"), A.Max(None, "int")])
        cols = [[keys[p][k] for p in m["first_position"]] for k in range(len(by))]
        cols += [[str(v) for v in m["count"]]] + [[str(v) for v in vs] for vs in m["values"]]
        return [StrCol.from_values(c) for c in cols]

    specs = [A.Sum("qty", "int"), A.Min("order_id", "int"), A.Max(table["qty"], "int")]
    got = pipeline.totals_to_csv(ctx, table, by=["cust_id"], specs=specs, names=["orders", "qty", "first_order", "largest"])
    assert got == orc.csv_write(model(["cust_id"]), ["cust_id", "orders", "qty", "first_order", "largest"])
    assert got.count(b"\n") == 1 + len(set(orders["cust_id"]))
    got = pipeline.totals_to_csv(ctx, table, by=["prod_id", "cust_id"], specs=specs)
    assert got == orc.csv_write(model(["prod_id", "cust_id"]), ["prod_id", "cust_id", "count", "sum0", "min1", "max2"])
    assert pipeline.totals_to_csv(ctx, table, by=["prod_id"], specs=[]) == orc.csv_write(model(["prod_id"])[:2], ["prod_id", "count"])
    dev = pipeline.totals_to_csv(ctx, table, by=["cust_id"], specs=specs[:1], out_mem=DEVICE)
    assert len(dev) == len(orc.csv_write(model(["cust_id"])[:3], ["cust_id", "count", "sum0"]))
    dev.release()
    with pytest.raises(ValueError, match="float64"):
        pipeline.totals_to_csv(ctx, table, by=["cust_id"], specs=[A.Sum("qty", "float")])
    with pytest.raises(MissingColumn):
        pipeline.totals_to_csv(ctx, table, by=["cust_id"], specs=[A.Sum("price", "int")])
    with pytest.raises(MissingColumn):
        pipeline.totals_to_csv(ctx, table, by=["customer"], specs=[])
    with pytest.raises(ValueError, match="names"):
        pipeline.totals_to_csv(ctx, table, by=["cust_id"], specs=specs, names=["n"])
    table.release()


@pytest.mark.gpu
def test_gpu_a_device_result_is_a_child_of_its_ctx():
    """A device-resident Totals is released with its ctx (the library wants its results released first); afterwards
    release() does not call into the library."""
    own = N.Context(0)   # closed below: not the session's
    ix = N.DeviceIndex(own, [StrCol.from_values([b"a", b"b", b"a", b"c", b"b"])])
    t = A.totals(ix, [A.Sum(np.arange(5, dtype=np.int64), "int")], out_mem=DEVICE)
    assert t.ngroups == 3 and t.ptr and t in own._children
    host = A.totals(ix, [A.Sum(np.arange(5, dtype=np.int64), "int")])
    assert host.ptr is None and host.count.tolist() == [2, 2, 1] and host.values[0].tolist() == [2, 5, 3]   # released before it came back
    own.close()
    assert t.ptr is None and ix.handle is None and own.handle is None
    t.lib = None   # a call into the library would fail on this
    t.release()
    t.close()
