"""Index.ResolveDuplicates with a NAMED rule on the device (cph_index_resolve, csvplus_amd.dedup.resolve_duplicates_device)
against the callback route stating the same rule (dedup.rule_pick + resolve_duplicates) and against the oracle's literal
restatement of dedup (csvplus.go:810-867)."""
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
from csvplus_amd import dedup as D
from oracle import orc
from tests.helpers import random_keys

ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
T = 2048   # rows per tile of k_resolve_tile: kResTile in csvplus_amd/csrc/resolve.hip (which points back here)

RULES = [(D.First(), None), (D.Last(), None), (D.DropAll(), None), (D.MinBy(), "int"), (D.MaxBy(), "int"),
         (D.MinBy(), "float"), (D.MaxBy(), "float"), (D.MinBy(), "bytes"), (D.MaxBy(), "bytes")]
RULE_IDS = [f"{type(r).__name__}-{k}" if k else type(r).__name__ for r, k in RULES]

INT_POOL = [b"007", b"+5", b"-0", b"0", b"5", b"-3", b"12", b"9223372036854775807", b"-9223372036854775808", b"41", b"-41"]
FLOAT_POOL = [b"nan", b"NaN", b"inf", b"-inf", b"-0", b"0", b"0.1", b"2.5", b"-2.5", b"1e3", b"+Inf", b"0.25", b"7"]
BYTES_POOL = [b"ab", b"abc", b"b", b"", b"\x80", b"a", b"zz", b"abcdefghij", b"abcdefghik", b"abcdefgh", b"\xff\x00", b"~"]
POOLS = {"int": INT_POOL, "float": FLOAT_POOL, "bytes": BYTES_POOL, None: [b"x"]}


def parse(kind, text):
    """The order value of a well-formed text as the rule's kind reads it."""
    if kind == "int":
        return int(text)
    if kind == "float":
        return float(text)
    return bytes(text)


def groups_of(keys):
    """(lower, upper) of every maximal run of >= 2 equal adjacent keys."""
    lower, upper, i, n = [], [], 0, len(keys)
    while i < n:
        j = i
        while j + 1 < n and keys[j + 1] == keys[i]:
            j += 1
        if j > i:
            lower.append(i)
            upper.append(j + 1)
        i = j + 1
    return lower, upper


def oracle_resolver(rule, kind):
    """The same rule written independently over the oracle's row dicts (field "v" = the order value's text)."""
    if isinstance(rule, D.First):
        return lambda g: g[0]
    if isinstance(rule, D.Last):
        return lambda g: g[-1]
    if isinstance(rule, D.DropAll):
        return lambda g: {}
    best = min if isinstance(rule, D.MinBy) else max   # both return the FIRST of equal candidates

    def resolve(g):
        if kind == "float":
            cand = [r for r in g if not math.isnan(float(r["v"]))]
            return best(cand, key=lambda r: float(r["v"])) if cand else g[0]
        return best(g, key=lambda r: parse(kind, r["v"]))
    return resolve


def model_positions(keys, rule, values, keep_last_row):
    """The survivors as the header states them: rows outside groups, every group's choice, minus the tail row."""
    lower, upper = groups_of(keys)
    in_group = set()
    for lo, hi in zip(lower, upper):
        in_group.update(range(lo, hi))
    pick = D.rule_pick(rule, values)
    keep = [p for p in range(len(keys)) if p not in in_group]
    keep += [c for c in (pick(lo, hi) for lo, hi in zip(lower, upper)) if c is not None]
    n = len(keys)
    if lower and not keep_last_row and (n - 1) not in in_group:
        keep.remove(n - 1)
    return sorted(keep)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,kind", RULES, ids=RULE_IDS)
def test_rule_pick_and_dedup_positions_match_the_oracle(rule, kind):
    rng = np.random.default_rng(11)
    cases = [list(k) for k in ("AAB", "AABC", "ABB", "ABC", "AABBC", "AABCC", "AAAB")]   # test_oracle_dedup_tail_rule
    for _ in range(300):
        n = int(rng.integers(0, 40))
        cases.append(sorted(random_keys(rng, n, 0, 2, alphabet=np.frombuffer(b"ab", np.uint8))))
    pool = POOLS[kind]
    for keys in cases:
        n = len(keys)
        texts = [pool[i] for i in rng.integers(0, len(pool), n)]
        values = [parse(kind, t) for t in texts] if kind else None
        rows = [{"k": k, "id": str(i), "v": texts[i]} for i, k in enumerate(keys)]
        lower, upper = groups_of(keys)
        pick = D.rule_pick(rule, values)
        got = D.dedup_positions(n, lower, upper, pick).tolist()
        want = [int(r["id"]) for r in orc.dedup_rows(rows, ["k"], oracle_resolver(rule, kind))]
        assert got == want == model_positions(keys, rule, values, False), (keys, texts)
        got = D.dedup_positions(n, lower, upper, pick, keep_last_row=True).tolist()
        assert got == model_positions(keys, rule, values, True), (keys, texts)


def test_pick_pins():
    nan, inf = math.nan, math.inf
    for rule in (D.MinBy(), D.MaxBy()):
        assert D.rule_pick(rule, [nan, 1.0, nan])(0, 3) == 1                    # a NaN loses under MIN and under MAX
        assert D.rule_pick(rule, [nan, nan, nan])(0, 3) == 0                    # only NaNs: the first row
        assert D.rule_pick(rule, [nan, nan, nan])(1, 3) == 1
        assert D.rule_pick(rule, [-0.0, 0.0])(0, 2) == 0 and D.rule_pick(rule, [0.0, -0.0])(0, 2) == 0   # -0 and +0 tie
        assert D.rule_pick(rule, [3, 7, 7, 3, 7, 3])(0, 6) == (0 if isinstance(rule, D.MinBy) else 1)   # ties: the lowest position
    assert D.rule_pick(D.MaxBy(), [nan, -inf, nan])(0, 3) == 1 and D.rule_pick(D.MinBy(), [nan, inf])(0, 2) == 1
    vals = [b"b", b"abc", b"ab", b"\x80", b"a~"]
    assert D.rule_pick(D.MinBy(), vals)(0, 3) == 2 and D.rule_pick(D.MaxBy(), vals)(0, 3) == 0   # b"ab" < b"abc" < b"b"
    assert D.rule_pick(D.MaxBy(), vals)(0, 5) == 3 and D.rule_pick(D.MinBy(), vals)(3, 5) == 4   # 0x80 ranks above ASCII
    assert D.rule_pick(D.First())(4, 9) == 4 and D.rule_pick(D.Last())(4, 9) == 8 and D.rule_pick(D.DropAll())(4, 9) is None
    with pytest.raises(ValueError):
        D.rule_pick(D.MaxBy())
    with pytest.raises(TypeError):
        D.rule_pick(object())


def test_resolve_struct_sizes_and_enums_against_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("sizes %zu %zu\\n", sizeof(cph_resolve_opts), sizeof(cph_resolved));'
                   'printf("offs %zu %zu %zu %zu %zu %zu %zu %zu\\n", offsetof(cph_resolved, positions), offsetof(cph_resolved, mem), '
                   "offsetof(cph_resolved, ngroups), offsetof(cph_resolved, nerrors), offsetof(cph_resolved, first_error_position), "
                   "offsetof(cph_resolved, first_error_row), offsetof(cph_resolved, first_error_kind), offsetof(cph_resolved, host_rows));"
                   'printf("rules %d %d %d %d %d %d\\n", CPH_RESOLVE_FIRST, CPH_RESOLVE_LAST, CPH_RESOLVE_DROP, CPH_RESOLVE_MIN, '
                   "CPH_RESOLVE_MAX, CPH_ORDER_BYTES);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert out["sizes"].split() == [str(C.sizeof(N.cph_resolve_opts)), str(C.sizeof(N.cph_resolved))] == ["16", "80"]
    f = N.cph_resolved
    assert out["offs"].split() == [str(v.offset) for v in (f.positions, f.mem, f.ngroups, f.nerrors, f.first_error_position,
                                                           f.first_error_row, f.first_error_kind, f.host_rows)]
    assert out["rules"].split() == [str(v) for v in (N.CPH_RESOLVE_FIRST, N.CPH_RESOLVE_LAST, N.CPH_RESOLVE_DROP, N.CPH_RESOLVE_MIN,
                                                     N.CPH_RESOLVE_MAX, N.CPH_ORDER_BYTES)] == ["1", "2", "3", "4", "5", "3"]
    assert [r.code for r in (D.First(), D.Last(), D.DropAll(), D.MinBy(), D.MaxBy())] == [1, 2, 3, 4, 5]


def test_resolve_symbols_declared_exported_and_bound():
    lib = C.CDLL(str(N.LIB_PATH))
    bound = {p[0] for p in N.PROTOTYPES}
    hdr = (ROOT / "include" / "csvplus_hip.h").read_text()
    for name in ("cph_index_resolve", "cph_resolved_release"):
        assert hasattr(lib, name) and name in bound and re.search(r"CPH_API\s+\w+\s+%s\(" % name, hdr)
    assert "} cph_resolved;" in hdr and "} cph_resolve_opts;" in hdr
    assert callable(D.resolve_duplicates_device) and callable(D.rule_pick) and issubclass(D.ResolveError, ValueError)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def order_col(texts, device=False, layout="auto"):
    """layout: "auto" (fixed width when every value has one length), "o32" / "o64" (offsets of that width)."""
    if layout == "auto":
        sc = StrCol.from_values(texts)
    else:
        sc = StrCol.from_values(texts, offset_bits=int(layout[1:]), fixed_width=0)
    return sc.to_device() if device else sc


def check(ctx, keycols, rule, kind, texts, keep_last_row=False, device=False, layout="auto", oracle=False, probe=False, ix=None):
    """Device route == callback route (== oracle) for one index; returns the device route's result."""
    own = ix is None
    if own:
        ix = N.DeviceIndex(ctx, [StrCol.from_values(v) for v in keycols])
    n = ix.nrows
    perm = ix.perm()
    values = [parse(kind, texts[int(r)]) for r in perm] if kind else None
    pick = D.rule_pick(rule, values)
    lower, upper = ix.dup_groups()
    want_pos = D.dedup_positions(n, lower, upper, pick, keep_last_row)
    want_ix = D.resolve_duplicates(ix, pick, keep_last_row)
    want_perm = want_ix.perm().tolist()
    want_ix.close()
    got = D.resolve_duplicates_device(ix, rule, order=order_col(texts, device, layout) if kind else None, kind=kind,
                                      keep_last_row=keep_last_row)
    assert got.positions.dtype == np.uint64 and got.positions.tolist() == want_pos.tolist()
    assert got.index.nrows == len(want_perm) and got.index.perm().tolist() == want_perm
    assert got.ngroups == len(lower) and got.group_rows == int((upper - lower).sum())
    if oracle and not keep_last_row:
        rows = [dict({f"c{c}": keycols[c][int(r)] for c in range(len(keycols))}, id=str(int(r)), v=texts[int(r)]) for r in perm]
        want = [int(r["id"]) for r in orc.dedup_rows(rows, [f"c{c}" for c in range(len(keycols))], oracle_resolver(rule, kind))]
        assert want_perm == want
    if probe and want_perm:   # the compacted index answers probes like a fresh index over the survivors
        sub = [StrCol.from_values([keycols[c][r] for r in want_perm]) for c in range(len(keycols))]
        pr = [StrCol.from_values(v) for v in keycols]
        m = got.index.probe(pr)
        o2 = orc.OracleIndex(sub).join(pr)
        assert m.cnt.tolist() == o2["cnt"].tolist()
        assert m.probe_idx.tolist() == o2["probe_idx"].tolist()
        assert m.build_row.tolist() == [want_perm[int(b)] for b in o2["build_row"]]
    got.index.close()
    if own:
        ix.close()
    return got


def keys_with_runs(n, runs):
    """n ascending keys, all distinct except that the positions of every run [lo, hi) share one."""
    ids = np.arange(n)
    for lo, hi in runs:
        ids[lo:hi] = lo
    return [b"%07d" % int(i) for i in ids]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, T - 1, T, T + 1])
def test_gpu_sizes_around_the_wave_and_the_tile(ctx, n):
    rng = np.random.default_rng(100 + n)
    keys = sorted(b"%05d" % int(v) for v in rng.integers(0, max(1, n // 3) + 1, n))
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    for rule, kind in RULES:
        pool = POOLS[kind]
        texts = [pool[i] for i in rng.integers(0, len(pool), n)]
        for keep_last in (False, True):
            check(ctx, [keys], rule, kind, texts, keep_last_row=keep_last, ix=ix, oracle=True)
    ix.close()


LONG = (T - 3, 3 * T + 2)   # a run of 2T+5 rows over four tiles: 3 rows, two whole tiles, 2 rows
LAYOUTS = {
    "run_across_the_tile_edge": (T + 10, [(T - 1, T + 1)], [T - 1, T]),
    "run_ends_at_the_tile_edge": (T + 10, [(T - 5, T)], [T - 5, T - 1]),
    "run_starts_at_the_tile_edge": (T + 10, [(T, T + 4)], [T, T + 3]),
    "long_run_winner_in_its_first_tile": (3 * T + 10, [LONG], [T - 2]),
    "long_run_winner_in_a_middle_tile": (3 * T + 10, [LONG], [2 * T + 5]),
    "long_run_winner_in_its_last_tile": (3 * T + 10, [LONG], [3 * T + 1]),
    "long_run_tied_across_tiles": (3 * T + 10, [LONG], [T - 1, T + 7, 2 * T + 9, 3 * T + 1]),
    "one_run_is_the_whole_index": (3 * T + 1, [(0, 3 * T + 1)], [2 * T + 11, 3 * T]),
    "all_keys_distinct": (T + 5, [], []),
    "last_row_inside_the_last_run": (T + 9, [(5, 9), (T + 6, T + 9)], [7, T + 7]),
    "last_row_outside_the_last_run": (T + 9, [(5, 9), (T + 5, T + 8)], [7, T + 6]),
    "runs_back_to_back_over_the_edge": (2 * T + 3, [(T - 4, T), (T, T + 3), (T + 3, 2 * T + 1)], [T - 2, T + 1, 2 * T]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_gpu_run_layouts(ctx, name):
    n, runs, winners = LAYOUTS[name]
    keys = keys_with_runs(n, runs)
    rng = np.random.default_rng(7)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    assert ix.perm().tolist() == list(range(n))   # sorted input, stable order: position p reads row p
    base = rng.integers(10, 20, n)
    for keep_last in (False, True):
        for rule in (D.First(), D.Last(), D.DropAll()):
            check(ctx, [keys], rule, None, None, keep_last_row=keep_last, ix=ix)
        for rule, kind, win in ((D.MaxBy(), "int", 99), (D.MinBy(), "int", -99), (D.MaxBy(), "float", 99), (D.MinBy(), "bytes", 0)):
            vals = base.copy()
            vals[np.asarray(winners, dtype=np.int64)] = win
            texts = [b"%d" % int(v) for v in vals]
            got = check(ctx, [keys], rule, kind, texts, keep_last_row=keep_last, ix=ix)
            for lo, hi in runs:   # the winner placed in the run survives: of tied winners the lowest position
                inside = [w for w in winners if lo <= w < hi]
                assert min(inside) in got.positions.tolist()
                assert sum(lo <= p < hi for p in got.positions.tolist()) == 1
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
def test_gpu_key_shapes_match_callback_route_and_oracle(ctx, shape):
    rng = np.random.default_rng(23)
    n = 3000
    keycols = shaped_keys(rng, shape, n)
    ix = N.DeviceIndex(ctx, [StrCol.from_values(v) for v in keycols])
    for rule, kind in RULES:
        pool = POOLS[kind]
        texts = [pool[i] for i in rng.integers(0, len(pool), n)]
        check(ctx, keycols, rule, kind, texts, ix=ix, oracle=True, probe=isinstance(rule, (D.First, D.MaxBy)))
    check(ctx, keycols, D.MaxBy(), "int", [b"%d" % int(v) for v in rng.integers(-50, 50, n)], keep_last_row=True, ix=ix)
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["auto", "o32", "o64"])
def test_gpu_order_columns_of_every_layout(ctx, device, layout):
    rng = np.random.default_rng(31)
    n = T + 300
    keys = [b"%03d" % int(v) for v in rng.integers(0, 400, n)]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    fixed_ints = [b"+9223372036854775807", b"-9223372036854775808", b"00000000000000000007", b"+0000000000000000005",
                  b"-0000000000000000000", b"00000000000000000041"]
    pools = {"int": fixed_ints if layout == "auto" else INT_POOL, "float": FLOAT_POOL,
             "bytes": [b"abcdefgh", b"abcdefgi", b"\x80bcdefgh", b"abcdefg\xff", b"ABCDEFGH"] if layout == "auto" else BYTES_POOL}
    for kind, pool in pools.items():
        texts = [pool[i] for i in rng.integers(0, len(pool), n)]
        col = order_col(texts, device, layout)
        assert bool(col.fixed_width) == (layout == "auto" and kind != "float")
        for rule in (D.MinBy(), D.MaxBy()):
            got = check(ctx, [keys], rule, kind, texts, device=device, layout=layout, ix=ix)
            assert got.host_rows == 0
    ix.close()


@pytest.mark.gpu
def test_gpu_exact_and_deferred_floats(ctx):
    rng = np.random.default_rng(37)
    n = 500
    keys = [b"%02d" % int(v) for v in rng.integers(0, 60, n)]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    exact = [b"0.1", b"0.3", b"12.75", b"1e22", b"-0.1", b"5."]
    texts = [exact[i] for i in rng.integers(0, len(exact), n)]
    for rule in (D.MinBy(), D.MaxBy()):
        assert check(ctx, [keys], rule, "float", texts, ix=ix).host_rows == 0     # the device decides every one of them
    deferred = [b"1.7976931348623157e308", b"123456789012345678901234"]
    where = rng.integers(0, n, 40)
    for i in where:
        texts[int(i)] = deferred[int(i) % 2]
    for rule in (D.MinBy(), D.MaxBy()):
        got = check(ctx, [keys], rule, "float", texts, ix=ix)
        assert got.host_rows == len(set(int(i) for i in where)) > 0
    ix.close()


@pytest.mark.gpu
def test_gpu_device_positions(ctx):
    from tests.test_numeric import d2h
    keys = keys_with_runs(T + 9, [(5, 9), (T - 2, T + 3)])
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    want = D.resolve_duplicates_device(ix, D.Last())
    got = D.resolve_duplicates_device(ix, D.Last(), out_mem=DEVICE)
    ptr, count = got.positions
    assert count == len(want.positions) and d2h(ptr, count, np.uint64).tolist() == want.positions.tolist()
    assert got.index.perm().tolist() == want.index.perm().tolist()
    got.release()


def raw_resolve(ctx, ix, opts, col, out_mem=HOST, want_index=True):
    h = N._P()
    out = C.POINTER(N.cph_resolved)()
    rc = ctx.lib.cph_index_resolve(ctx.handle, ix.handle if ix else None, C.byref(opts) if opts else None, col, out_mem,
                                   C.byref(h) if want_index else None, C.byref(out))
    return rc, h, out


@pytest.mark.gpu
def test_gpu_conversion_errors_are_data(ctx):
    #        rows:  0     1      2                        3     4     5     6
    keys = [b"c", b"c", b"b", b"b", b"a", b"a", b"d"]
    texts = [b"1", b"zz", b"99999999999999999999", b"3", b"5", b"6", b"x"]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    assert ix.perm().tolist() == [4, 5, 2, 3, 0, 1, 6]
    # two bad groups: the lowest bad position (2: the range error of row 2) is reported, not the syntax error at position 5
    with pytest.raises(D.ResolveError) as e:
        D.resolve_duplicates_device(ix, D.MaxBy(), order=order_col(texts), kind="int")
    assert (e.value.position, e.value.row, e.value.kind, e.value.nerrors) == (2, 2, N.CPH_NUM_ERR_RANGE, 2)
    sc, keep = order_col(texts).as_c()
    rc, h, out = raw_resolve(ctx, ix, N.cph_resolve_opts(N.CPH_RESOLVE_MIN, N.CPH_NUM_INT64, 0, 0), C.pointer(sc))
    r = out.contents
    assert rc == N.CPH_OK and not h.value and r.nrows == 0 and not r.positions and r.nerrors == 2 and r.ngroups == 3
    assert (r.first_error_position, r.first_error_row, r.first_error_kind) == (2, 2, N.CPH_NUM_ERR_RANGE)
    ctx.lib.cph_resolved_release(out)
    # as floats only "zz" fails: position 5, row 1
    with pytest.raises(D.ResolveError) as e:
        D.resolve_duplicates_device(ix, D.MinBy(), order=order_col(texts), kind="float")
    assert (e.value.position, e.value.row, e.value.kind, e.value.nerrors) == (5, 1, N.CPH_NUM_ERR_SYNTAX, 1)
    # the non-numeric value of row 6 lies outside every group: the callback never sees it, the call does not fail
    texts[1], texts[2] = b"2", b"4"
    got = check(ctx, [keys], D.MaxBy(), "bytes", texts, ix=ix)
    got = D.resolve_duplicates_device(ix, D.MaxBy(), order=order_col(texts), kind="int", keep_last_row=True)
    assert got.index.perm().tolist() == [5, 2, 1, 6] and got.positions.tolist() == [1, 2, 5, 6]
    # rules without an order never look at a column
    assert D.resolve_duplicates_device(ix, D.DropAll()).positions.tolist() == []
    ix.close()


@pytest.mark.gpu
def test_gpu_argument_errors_have_a_status_and_a_message(ctx):
    keys = [b"a", b"a", b"b"]
    ix = N.DeviceIndex(ctx, [StrCol.from_values(keys)])
    sc, keep = order_col([b"1", b"2", b"3"]).as_c()
    short, keep2 = order_col([b"1", b"2"]).as_c()
    ok = N.cph_resolve_opts(N.CPH_RESOLVE_MAX, N.CPH_NUM_INT64, 0, 0)
    rc, h, out = raw_resolve(ctx, ix, ok, C.pointer(sc))
    assert rc == N.CPH_OK and out.contents.nrows == 1
    ctx.lib.cph_resolved_release(out)
    ctx.lib.cph_index_destroy(h)
    rc, h, out = raw_resolve(ctx, ix, ok, C.pointer(sc), want_index=False)      # out_index may be NULL
    assert rc == N.CPH_OK and N._ptr_array(out.contents.positions, 1, np.uint64).tolist() == [1]
    ctx.lib.cph_resolved_release(out)
    rc, h, out = raw_resolve(ctx, ix, N.cph_resolve_opts(N.CPH_RESOLVE_FIRST, 77, 0, 0), None)   # order kind and column ignored
    assert rc == N.CPH_OK
    ctx.lib.cph_resolved_release(out)
    ctx.lib.cph_index_destroy(h)
    bad = [
        (dict(ix=None), "index"),
        (dict(opts=None), "opts"),
        (dict(opts=N.cph_resolve_opts(0, N.CPH_NUM_INT64, 0, 0)), "rule"),
        (dict(opts=N.cph_resolve_opts(6, N.CPH_NUM_INT64, 0, 0)), "rule"),
        (dict(opts=N.cph_resolve_opts(N.CPH_RESOLVE_MAX, 0, 0, 0)), "order_kind"),
        (dict(opts=N.cph_resolve_opts(N.CPH_RESOLVE_MIN, 4, 0, 0)), "order_kind"),
        (dict(out_mem=7), "out_mem"),
        (dict(col=None), "order column"),
        (dict(col=C.pointer(short)), "fewer rows"),
    ]
    for kw, word in bad:
        args = dict(ix=ix, opts=ok, col=C.pointer(sc), out_mem=HOST)
        args.update(kw)
        rc, h, out = raw_resolve(ctx, args["ix"], args["opts"], args["col"], args["out_mem"])
        assert rc == N.CPH_ERR_INVALID and not h.value and not out, kw
        assert word in ctx.last_error(), (kw, ctx.last_error())
    assert ctx.lib.cph_index_resolve(None, ix.handle, C.byref(ok), C.pointer(sc), HOST, None, C.byref(out)) == N.CPH_ERR_INVALID
    assert ctx.lib.cph_index_resolve(ctx.handle, ix.handle, C.byref(ok), C.pointer(sc), HOST, None, None) == N.CPH_ERR_INVALID
    with pytest.raises(ValueError):
        D.resolve_duplicates_device(ix, D.MaxBy())
    with pytest.raises(ValueError):
        D.resolve_duplicates_device(ix, D.MaxBy(), order=order_col([b"1", b"2", b"3"]), kind="decimal")
    with pytest.raises(TypeError):
        D.resolve_duplicates_device(ix, lambda lo, hi: lo)
    del keep, keep2
    ix.close()


@pytest.mark.gpu
def test_gpu_a_device_result_is_a_child_of_its_ctx():
    """A device-resident Resolved is released with its ctx; afterwards release() does not call into the library."""
    own = N.Context(0)   # closed below: not the session's
    ix = N.DeviceIndex(own, [StrCol.from_values([b"a", b"b", b"a", b"c", b"b"])])
    r = D.resolve_duplicates_device(ix, D.First(), keep_last_row=True, out_mem=DEVICE)
    assert r.positions[1] == 3 and r.ptr and r in own._children
    host = D.resolve_duplicates_device(ix, D.First(), keep_last_row=True)
    assert host.ptr is None and host.positions.tolist() == [0, 2, 4]   # sorted a a b b c: the first of each run
    own.close()
    assert r.ptr is None and r.index.handle is None and own.handle is None
    r.lib = None   # a call into the library would fail on this
    r.release()
    r.close()
