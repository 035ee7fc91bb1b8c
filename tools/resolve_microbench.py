#!/usr/bin/env python3
"""cph_index_resolve over the bench's own `orders` table: a device-resident index over cust_id (8-byte fixed width) with about
10 rows per key, resolved with MaxBy(prod_id, "int") (prod_id: decimal, variable length, 32-bit offsets) and with First().

First the positions are VERIFIED at full size against the route without the feature, vectorised with numpy: dup_groups ->
the pick per group with np.maximum.reduceat / np.minimum.reduceat over the order values in sorted order -> select.  Then both
routes are timed in the same process, alternating them (the order values of the host route are converted once, outside its
timed part: they are an input of that route, not its work).  A second pass with cph_ctx_profile on gives the kernel times
and the achieved bytes per second by the kernels' byte models, next to cph_calibrate kind 0 (this box's
streaming-copy rate).

    python tools/resolve_microbench.py [rows=1e8] [reps=10]      (rocprofv3 --kernel-trace --stats -- python tools/... 2e7 3)
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, DeviceIndex, _native as N, datagen as dg  # noqa: E402
from csvplus_amd import dedup as D  # noqa: E402
from csvplus_amd.materialize import to_int  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ctx = Context(0)


def sync():
    ctx.synchronize()
    torch.cuda.synchronize()


copy_bytes = 1 << 30
copy_ms = ctx.calibrate("copy", copy_bytes, reps=10)
copy_rate = 2 * copy_bytes / (copy_ms * 1e-3)
print(f"rows {M}, reps {REPS}; streaming copy (cph_calibrate kind 0): {copy_rate / 1e9:.0f} GB/s", flush=True)

o = dg.orders(M, max(1, M // 10), 1000)
cust, prod = o["cust_id"].to_device(), o["prod_id"].to_device()
ix = DeviceIndex(ctx, [cust])
nc = to_int(ctx, prod)
assert nc.nerrors == 0
prod_sorted = nc.values[ix.perm_host_view()]   # the host route's input: the order value per sorted position
nc.release()
n = ix.nrows


def host_route(rule):
    """dup_groups -> vectorised pick -> select: what a caller without cph_index_resolve can do best."""
    lower, upper = ix.dup_groups()
    lower, upper = lower.astype(np.int64), upper.astype(np.int64)
    keep = np.ones(n, dtype=bool)
    if len(lower):
        lens = upper - lower
        gstart = np.cumsum(lens) - lens
        pos = np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(lower - gstart, lens)
        keep[pos] = False
        if isinstance(rule, D.First):
            choice = lower
        else:
            v = prod_sorted[pos]
            mx = np.maximum.reduceat(v, gstart)
            choice = np.minimum.reduceat(np.where(v == np.repeat(mx, lens), pos, np.int64(n)), gstart)   # ties: the lowest position
        keep[choice] = True
        if upper[-1] != n:
            keep[n - 1] = False   # the reference's tail rule
    positions = np.flatnonzero(keep).astype(np.uint64)
    return positions, ix.select(positions)


def device_route(rule, out_mem=N.CPH_MEM_HOST):
    return D.resolve_duplicates_device(ix, rule, order=prod if rule.ordered else None, kind="int" if rule.ordered else None,
                                       out_mem=out_mem)


for label, rule in (("MaxBy(prod_id, int)", D.MaxBy()), ("First()", D.First())):
    want_pos, want_ix = host_route(rule)
    got = device_route(rule)
    assert np.array_equal(got.positions, want_pos), f"{label}: positions differ from the host route"
    assert np.array_equal(got.index.perm_host_view(), want_ix.perm_host_view()), f"{label}: compacted index differs"
    ngroups, group_rows, kept = got.ngroups, got.group_rows, len(want_pos)
    got.index.close()
    want_ix.close()
    del got, want_pos
    print(f"{label}: verified at {n} rows: {ngroups} groups of {group_rows} rows, {kept} survivors", flush=True)

    def dev():
        r = device_route(rule, N.CPH_MEM_DEVICE)
        r.index.close()
        r.release()

    def host():
        _, nx = host_route(rule)
        nx.close()

    dev()
    sync()
    td, th = [], []
    host_reps = max(1, min(REPS, 2 if M > 20_000_000 else 5))
    for k in range(REPS):   # alternating: both routes see the same box in the same minutes
        t0 = time.perf_counter()
        dev()
        sync()
        td.append(time.perf_counter() - t0)
        if k < host_reps:
            t0 = time.perf_counter()
            host()
            sync()
            th.append(time.perf_counter() - t0)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(3):
        dev()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    kernel_ms = sum(v["total_ms"] for v in st.values()) / 3
    model = sum(v["algo_bytes"] for v in st.values()) / 3
    ks = ", ".join(f"{k}={v['total_ms'] / 3:.3f} ms" for k, v in st.items())
    dmed, hmed = float(np.median(td)), float(np.median(th))
    print(f"{label}: device route {dmed * 1e3:.3f} ms (min {min(td) * 1e3:.3f}, max {max(td) * 1e3:.3f}, {REPS} calls) | "
          f"host route {hmed * 1e3:.0f} ms ({len(th)} calls) = x{hmed / dmed:.0f} | kernels {kernel_ms:.3f} ms, "
          f"{model / 1e9:.2f} GB by the byte models = {model / (kernel_ms * 1e-3) / 1e9:.0f} GB/s "
          f"({100 * model / (kernel_ms * 1e-3) / copy_rate:.1f} % of copy) | {ks}", flush=True)
    assert dmed < hmed, f"{label}: the device route is not faster than the vectorised host route"
ix.close()
ctx.close()
