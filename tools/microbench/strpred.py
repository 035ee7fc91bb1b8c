#!/usr/bin/env python3
"""The string conditions at scale: `rows` device-resident RFC3339 timestamps (25 bytes each, 32-bit offsets, the `ts`
column of the orders fixture) through cph_filter_rows in WHERE mode:

    filter_rows(Like)        ts == one of its values — the yardstick: the same bytes through the same kernel
    filter_rows(StrCmp)      ts >= "2016-09-14"
    filter_rows(HasPrefix)   ts starts with "2016-09-14"
    filter_rows(HasSuffix)   ts ends with ":00+01:00"
    filter_rows(Contains)    "T08:" in ts (a match ends the search early), and ":61+" in ts (never there: every row is
                             searched to its end)

Per case: warm-up, then REPS synchronised calls with the profiler off (wall time per call), a second pass with
cph_ctx_profile on for the kernel times, and both as a ratio to the yardstick's.  Next to it cph_calibrate kind 0, this
box's streaming-copy rate.  Every count is checked against numpy before it is timed.

    python tools/microbench/strpred.py [rows=1e8] [reps=10]
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, StrCol, _native as N  # noqa: E402
from csvplus_amd.materialize import filter_rows  # noqa: E402
from csvplus_amd.predicates import Contains, HasPrefix, HasSuffix, Like, StrCmp  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
W = 25
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


def profiled(fn):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(3):
        fn()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    return {k: v["total_ms"] / 3 for k, v in st.items()}


def ts_block(n, rng):
    """n timestamps 2016-09-DDThh:mm:ss+01:00 as an (n, 25) byte matrix."""
    a = np.tile(np.frombuffer(b"2016-09-14T08:48:22+01:00", dtype=np.uint8), (n, 1))
    for at, hi in ((8, 28), (11, 24), (14, 60), (17, 60)):
        v = rng.integers(1 if at == 8 else 0, hi + (1 if at == 8 else 0), n)
        a[:, at], a[:, at + 1] = 0x30 + v // 10, 0x30 + v % 10
    return a


copy_bytes = 1 << 30
copy_ms = ctx.calibrate("copy", copy_bytes, reps=10)
copy_rate = 2 * copy_bytes / (copy_ms * 1e-3)
print(f"rows {M}, reps {REPS}; streaming copy (cph_calibrate kind 0): {copy_rate / 1e9:.0f} GB/s", flush=True)

rng = np.random.default_rng(14)
block = ts_block(min(M, 1 << 20), rng)
mat = np.resize(block, (M, W))   # the block repeated: the kernels' work per row does not depend on which rows repeat
offs = (np.arange(M + 1, dtype=np.uint64) * W).astype(np.uint32)
hcol = StrCol(mat.reshape(-1), offs, M, 32, fixed_width=0)   # offsets, as a CSV reader hands the column over
dcol = hcol.to_device()
cols = {"ts": dcol}
in_bytes = M * W + 4 * M


def count(fn_rows):
    """rows of the block that hold, scaled to M rows (the block divides into M exactly or the tail is counted too)"""
    flags = fn_rows(block)
    reps, tail = divmod(M, len(block))
    return int(flags.sum()) * reps + int(flags[:tail].sum())


def has_at(a, at, lit):
    return np.all(a[:, at:at + len(lit)] == np.frombuffer(lit, dtype=np.uint8), axis=1)


def contains(a, lit):
    f = np.zeros(len(a), dtype=bool)
    for at in range(W - len(lit) + 1):
        f |= has_at(a, at, lit)
    return f


def lex_ge(a, lit):
    """value >= lit for lit shorter than every value: decided by the first len(lit) bytes (equal there: the value is longer)"""
    key = a[:, :len(lit)]
    ref = np.frombuffer(lit, dtype=np.uint8)
    diff = key != ref
    first = np.where(diff.any(axis=1), diff.argmax(axis=1), 0)
    rows = np.arange(len(a))
    return ~diff.any(axis=1) | (key[rows, first] > ref[first])


first_value = hcol.value(0)
cases = [
    ("filter_rows(Like)", Like(ts=first_value), lambda a: has_at(a, 0, first_value)),
    ("filter_rows(StrCmp >=)", StrCmp("ts", ">=", b"2016-09-14"), lambda a: lex_ge(a, b"2016-09-14")),
    ("filter_rows(HasPrefix)", HasPrefix("ts", b"2016-09-14"), lambda a: has_at(a, 0, b"2016-09-14")),
    ("filter_rows(HasSuffix)", HasSuffix("ts", b":00+01:00"), lambda a: has_at(a, W - 9, b":00+01:00")),
    ("filter_rows(Contains hit)", Contains("ts", b"T08:"), lambda a: contains(a, b"T08:")),
    ("filter_rows(Contains miss)", Contains("ts", b":61+"), lambda a: contains(a, b":61+")),
]
base_wall = base_kernel = None
for label, pred, model in cases:
    f = lambda: filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE).release()   # noqa: E731
    rl = filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE)
    kept = len(rl)
    rl.release()
    assert kept == count(model), (label, kept, count(model))
    wall = timed(f, REPS)
    kern = profiled(f)
    ev = sum(v for k, v in kern.items() if k.startswith("k_pred_eval"))
    if base_wall is None:
        base_wall, base_kernel = wall, ev
    moved = in_bytes + 2 * M / 8 + 4 * kept
    print(f"{label:27s}: call {wall * 1e3:8.3f} ms ({wall / base_wall:5.2f} x Like)  eval kernel {ev:8.3f} ms ({ev / base_kernel:5.2f} x Like)  "
          f"{moved / wall / 1e9:7.1f} GB/s by the model ({100 * moved / wall / copy_rate:4.1f} % of copy) | kept {kept} | "
          + ", ".join(f"{k}={v:.3f} ms" for k, v in kern.items()), flush=True)
ctx.close()
