#!/usr/bin/env python3
"""The SPAN piece at scale: `rows` device-resident order keys " ORD-0001234-42 " (16 bytes each, 32-bit offsets) through
cph_map_format into device memory:

    Format(Col("x"))                 the whole value: 16 bytes a row — the floor of a template that moves every byte
    Format(Col("x")[1:-1])           a slice: 14 bytes a row — the floor of the two below, which move the same or fewer bytes
    Format(Col("x").trim_space())    strings.TrimSpace: the same 14 bytes, found by looking at the value
    Format(Col("x").field(b"-", 1))  strings.Split(x, "-")[1]: 7 bytes a row
    Format(Col("x")[:10]), Format(Float.shortest(v))   two more templates WITHOUT a span piece

Mode "kernels" (default): per template a check of the first rows against mapping.render, a warm-up, then REPS calls with
cph_ctx_profile on: the kernel times per call, and the span templates as ratios to the slice's.  Mode "plain": the same calls
with the library's profiler off and nothing printed but the wall time per call — the mode to run under
`rocprofv3 --kernel-trace --stats`.  Mode "old": only the templates without a span piece, one line of kernel times: what a
library from before the SPAN piece can run too (CSVPLUS_HIP_LIB selects the library), for an A/B of unchanged templates.

    python tools/microbench/map_span.py [rows=1e7] [reps=10] [kernels|plain|old]
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, StrCol, _native as N  # noqa: E402
from csvplus_amd import mapping as M  # noqa: E402
from csvplus_amd.mapping import Col, Float, Format  # noqa: E402
from csvplus_amd.materialize import map_column  # noqa: E402

ROWS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
MODE = sys.argv[3] if len(sys.argv) > 3 else "kernels"
W = 16
ctx = Context(0)


def sync():
    ctx.synchronize()
    torch.cuda.synchronize()


rng = np.random.default_rng(14)
block_rows = min(ROWS, 1 << 20)
block = np.tile(np.frombuffer(b" ORD-0000000-00 ", dtype=np.uint8), (block_rows, 1))
ids, qty = rng.integers(0, 10_000_000, block_rows), rng.integers(0, 100, block_rows)
for k in range(7):
    block[:, 5 + k] = 0x30 + (ids // 10 ** (6 - k)) % 10
block[:, 13], block[:, 14] = 0x30 + qty // 10, 0x30 + qty % 10
mat = np.resize(block, (ROWS, W))
offs = (np.arange(ROWS + 1, dtype=np.uint64) * W).astype(np.uint32)
hcol = StrCol(mat.reshape(-1), offs, ROWS, 32, fixed_width=0)
cols = {"x": hcol.to_device()}
floats = torch.from_numpy(rng.random(ROWS) * 1000.0).to("cuda:0")
X = Col("x")

OLD = [("Format(x)", Format(X), 16), ("Format(x[:10])", Format(X[:10]), 10),
       ("Format(Float.shortest)", Format(Float.shortest_on_device(floats.data_ptr(), ROWS, "g")), None)]
NEW = [("Format(x[1:-1])", Format(X[1:-1]), 14), ("Format(x.trim_space())", Format(X.trim_space()), 14),
       ("Format(x.field('-', 1))", Format(X.field(b"-", 1)), 7)] if MODE != "old" else []


def call(template):
    map_column(ctx, cols, template, out_mem=N.CPH_MEM_DEVICE).release()


def kernel_times(template):
    call(template)   # warm-up
    sync()
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(REPS):
        call(template)
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    return {k: v["total_ms"] / REPS for k, v in st.items() if k.startswith("k_map")}


def wall_time(template):
    call(template)
    sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        call(template)
    sync()
    return (time.perf_counter() - t0) / REPS


# the first rows of every string template against the host model
head = {"x": StrCol(mat[:1000].reshape(-1).copy(), offs[:1001].copy(), 1000, 32, fixed_width=0)}
for label, t, width in OLD[:2] + NEW:
    cb = map_column(ctx, head, t, out_mem=N.CPH_MEM_HOST)
    got = cb.to_strcol().values()
    cb.release()
    assert got == [M.render(t, {"x": hcol.value(i)}) for i in range(1000)] and all(len(g) == width for g in got), label

if MODE == "old":
    parts = []
    for label, t, _ in OLD:
        kt = kernel_times(t)
        parts.append(f"{label}: " + " ".join(f"{k}={v:.4f}" for k, v in sorted(kt.items())) + f" sum={sum(kt.values()):.4f}")
    print("; ".join(parts), flush=True)
elif MODE == "plain":
    for label, t, _ in OLD + NEW:
        print(f"{label:26s}: {wall_time(t) * 1e3:8.3f} ms per call", flush=True)
else:
    print(f"rows {ROWS}, reps {REPS}, {W} bytes a value", flush=True)
    floor = None
    for label, t, width in OLD + NEW:
        kt = kernel_times(t)
        total = sum(kt.values())
        if label == "Format(x[1:-1])":
            floor = total
        ratio = f"  {total / floor:5.2f} x the slice" if floor and label != "Format(x[1:-1])" else ""
        print(f"{label:26s}: kernels {total:7.4f} ms  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(kt.items())) + ratio, flush=True)
ctx.close()
