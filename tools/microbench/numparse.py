#!/usr/bin/env python3
"""cph_col_to_number and the numeric compare predicates at scale, device-resident columns with 32-bit offsets:

    to_int               over `rows` values of 1-7 decimal digits
    to_float             over `rows` price-like values ("%d.%02d", integer part < 100 000)
    to_time              over `rows` RFC 3339 stamps of 25 bytes ("YYYY-MM-DDTHH:MM:SS+HH:MM", three zone offsets); its yardstick
                         is the to_int line of the same run: the same kernel geometry over 8-byte values
    filter_rows(IntCmp)  WHERE v > median over the integer column
    filter_rows(Like)    WHERE v == one of its values over the same column — the yardstick: it reads the same bytes
                         through the same evaluation kernel (it runs without this feature too: measure it at the parent
                         commit for the comparison; `like` alone as the third argument skips the rest)

    `float` as the third argument measures only the float conversion, over three columns and under both settings of
    cph_ctx_set_option "float_device" (a library without the option runs setting 0 alone: the parent commit's build, named by
    CSVPLUS_HIP_LIB, gives the baseline rows):
        prices       the price column of the to_float line
        deferred     repr of random doubles in -1e6..1e6 with 17 significant digits: every value outside Clinger's cases
        mixed        prices with 1 % of the rows replaced by such values
    (`prices` has `rows` rows, the other two at most 4e6: their texts are made value by value.)
    The cases are measured round-robin, `rounds` (fourth argument, default 3) times each, so that drift hits all alike.

Per case: warm-up, then REPS synchronised calls with the profiler off (wall time per call), and a second pass with
cph_ctx_profile on for the kernel times.  Next to it cph_calibrate kind 0, this box's streaming-copy rate.

    python tools/microbench/numparse.py [rows=1e8] [reps=20] [like]
    python tools/microbench/numparse.py 4e6 5 float [rounds=3]
"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, StrCol, _native as N  # noqa: E402
from csvplus_amd.materialize import filter_rows  # noqa: E402
from csvplus_amd.predicates import Like  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
LIKE_ONLY = len(sys.argv) > 3 and sys.argv[3] == "like"
FLOAT_ONLY = len(sys.argv) > 3 and sys.argv[3] == "float"
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
SLOW_ROWS = 4_000_000   # rows of the float mode's `deferred` and `mixed` columns (at most `rows`)
ctx = Context(0)


def sync():
    ctx.synchronize()
    torch.cuda.synchronize()


def timed(fn, reps):
    fn()   # warm-up
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def decimal_column(v, frac=None):
    """The decimal text of the non-negative integers v (and, with frac, of "v.ff") as a StrCol, built with numpy."""
    nd = np.ones(len(v), dtype=np.int64)
    for k in range(1, 10):
        nd += v >= 10 ** k
    lens = nd + (3 if frac is not None else 0)
    offs = np.zeros(len(v) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = np.empty(int(offs[-1]), dtype=np.uint8)
    end = offs[1:].astype(np.int64)
    if frac is not None:
        data[end - 1] = 0x30 + frac % 10
        data[end - 2] = 0x30 + frac // 10
        data[end - 3] = 0x2E
        end = end - 3
    w = v.copy()
    for k in range(int(nd.max())):
        live = nd > k
        data[end[live] - 1 - k] = 0x30 + w[live] % 10
        w //= 10
    return StrCol(data, offs.astype(np.uint32), len(v), 32)


def two_digits(out, at, v):
    out[:, at] = 0x30 + v // 10
    out[:, at + 1] = 0x30 + v % 10


def stamp_column(n, rng):
    """n stamps "2016-MM-DDTHH:MM:SS+HH:MM" (25 bytes each, variable-length layout with 32-bit offsets), built with numpy."""
    out = np.empty((n, 25), dtype=np.uint8)
    out[:] = np.frombuffer(b"2016-00-00T00:00:00+00:00", dtype=np.uint8)
    two_digits(out, 5, rng.integers(1, 13, n))
    two_digits(out, 8, rng.integers(1, 29, n))
    two_digits(out, 11, rng.integers(0, 24, n))
    two_digits(out, 14, rng.integers(0, 60, n))
    two_digits(out, 17, rng.integers(0, 60, n))
    zone = rng.integers(0, 3, n)
    out[:, 19] = np.array([0x2B, 0x2B, 0x2D], dtype=np.uint8)[zone]
    two_digits(out, 20, np.array([0, 2, 5])[zone])
    two_digits(out, 23, np.array([0, 0, 30])[zone])
    return StrCol(out.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * 25).astype(np.uint32), n, 32, fixed_width=0)


def profiled(fn):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(3):
        fn()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    return ", ".join(f"{k}={v['total_ms'] / 3:.3f} ms" for k, v in st.items())


copy_bytes = 1 << 30
copy_ms = ctx.calibrate("copy", copy_bytes, reps=10)
copy_rate = 2 * copy_bytes / (copy_ms * 1e-3)
print(f"rows {M}, reps {REPS}; streaming copy (cph_calibrate kind 0): {copy_rate / 1e9:.0f} GB/s", flush=True)



def report(label, wall, bytes_moved, extra):
    print(f"{label:22s}: call {wall * 1e3:8.3f} ms  {bytes_moved / wall / 1e9:7.1f} GB/s by the model ({100 * bytes_moved / wall / copy_rate:4.1f} % of copy) | {extra}",
          flush=True)


def text_column(values):
    """A StrCol (32-bit offsets) over a list of bytes."""
    offs = np.zeros(len(values) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(v) for v in values), dtype=np.uint64, count=len(values)), out=offs[1:])
    return StrCol(np.frombuffer(b"".join(values), dtype=np.uint8).copy(), offs.astype(np.uint32), len(values), 32)


def deferred_texts(n, rng):
    """repr of random doubles, those with 17 significant digits: a mantissa >= 10^16 > 2^53 is outside Clinger's cases."""
    out = []
    while len(out) < n:
        for x in rng.uniform(-1e6, 1e6, n - len(out) + 1024).tolist():
            t = repr(x).encode()
            if b"e" not in t and len(t.lstrip(b"-").replace(b".", b"").lstrip(b"0")) >= 17 and len(out) < n:
                out.append(t)
    return out


def float_columns():
    from csvplus_amd.materialize import to_float

    rng = np.random.default_rng(2)
    whole, cents = rng.integers(0, 100000, M), rng.integers(0, 100, M)
    prices = decimal_column(whole.copy(), cents)
    S = min(M, SLOW_ROWS)   # the columns built value by value in Python
    slow = deferred_texts(S, rng)
    mixed = [b"%d.%02d" % (a, b) for a, b in zip(whole[:S].tolist(), cents[:S].tolist())]
    for i in rng.choice(S, S // 100, replace=False).tolist():
        mixed[i] = slow[i]
    cols = {"prices": prices, "deferred": text_column(slow), "mixed": text_column(mixed)}
    del mixed, slow
    dev = {k: c.to_device() for k, c in cols.items()}
    try:
        ctx.set_option("float_device", 1)
        ctx.set_option("float_device", 0)
        settings = (0, 1)
    except N.CphError:
        settings = (0,)   # a library from before the option
    print(f"library {os.environ.get('CSVPLUS_HIP_LIB', N.LIB_PATH)}; float_device settings {settings}; {ROUNDS} rounds of up to {REPS} calls per case "
          f"(fewer where a call takes long: about 2 s per case); rows: " + ", ".join(f"{k} {c.nrows}" for k, c in cols.items()), flush=True)
    for rnd in range(ROUNDS):
        for name, col in dev.items():
            for opt in settings:
                if len(settings) > 1:
                    ctx.set_option("float_device", opt)
                f = lambda: to_float(ctx, col, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
                r = to_float(ctx, col, out_mem=N.CPH_MEM_DEVICE)
                host_rows, nerr = r.host_rows, r.nerrors
                r.release()
                sync()
                t0 = time.perf_counter()
                f()
                sync()
                reps = max(1, min(REPS, int(2.0 / (time.perf_counter() - t0))))
                wall = timed(f, reps)
                report(f"{name} opt {opt} round {rnd}", wall, cols[name].nbytes_values() + cols[name].nbytes_offsets() + 9 * cols[name].nrows,
                       f"{reps} calls | host_rows {host_rows} nerrors {nerr} | " + profiled(f))
    if len(settings) > 1:
        ctx.set_option("float_device", 0)


if FLOAT_ONLY:
    float_columns()
    ctx.close()
    sys.exit(0)

rng = np.random.default_rng(1)
digits = rng.integers(1, 8, M)
ints = (rng.random(M) * 10.0 ** digits).astype(np.int64)
hint = decimal_column(ints)
dint = hint.to_device()
in_bytes = hint.nbytes_values() + hint.nbytes_offsets()
cols = {"v": dint}
like = Like(v=hint.value(0))


f = lambda: filter_rows(ctx, cols, like, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
rl = filter_rows(ctx, cols, like, out_mem=N.CPH_MEM_DEVICE)
kept = len(rl)
rl.release()
report("filter_rows(Like)", timed(f, REPS), in_bytes + 2 * M / 8 + 4 * kept, f"kept {kept} | " + profiled(f))
if not LIKE_ONLY:
    from csvplus_amd.materialize import to_float, to_int
    from csvplus_amd.predicates import IntCmp

    pred = IntCmp("v", ">", int(np.median(ints)))
    f = lambda: filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
    rl = filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE)
    kept = len(rl)
    rl.release()
    assert kept == int((ints > int(np.median(ints))).sum())
    report("filter_rows(IntCmp)", timed(f, REPS), in_bytes + 2 * M / 8 + 4 * kept, f"kept {kept} | " + profiled(f))
    f = lambda: to_int(ctx, dint, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
    r = to_int(ctx, dint, out_mem=N.CPH_MEM_DEVICE)
    assert r.nerrors == 0
    r.release()
    report("to_int", timed(f, REPS), in_bytes + 9 * M, profiled(f))
    del dint, cols
    torch.cuda.empty_cache()
    hflt = decimal_column(rng.integers(0, 100000, M), rng.integers(0, 100, M))
    dflt = hflt.to_device()
    f = lambda: to_float(ctx, dflt, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
    r = to_float(ctx, dflt, out_mem=N.CPH_MEM_DEVICE)
    assert r.nerrors == 0
    host_rows = r.host_rows
    r.release()
    report("to_float", timed(f, REPS), hflt.nbytes_values() + hflt.nbytes_offsets() + 9 * M, f"host_rows {host_rows} | " + profiled(f))
    del dflt, hflt
    torch.cuda.empty_cache()
    from csvplus_amd.materialize import to_time

    htim = stamp_column(M, rng)
    dtim = htim.to_device()
    f = lambda: to_time(ctx, dtim, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
    r = to_time(ctx, dtim, out_mem=N.CPH_MEM_DEVICE)
    assert r.nerrors == 0
    r.release()
    report("to_time", timed(f, REPS), htim.nbytes_values() + htim.nbytes_offsets() + 9 * M, profiled(f))
ctx.close()
