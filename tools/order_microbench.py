#!/usr/bin/env python3
"""cph_order_rows (OrderBy with Top-N select) on one GPU: what profiles/order_rows.txt records.

  full sort     one int64 key, and an int64 + a float64 key, at every size of `sizes`
  top-k         one int64 key, k of `ks`, with the select (order_select = 2: whatever the gate says) and without it
                (order_select = 0): where the two routes cross is where the gate belongs (kSelectGate, order.hip)
  old route     what a caller had before the feature, at the first size: the values copied to the host and
                numpy.argsort(kind="stable"), copy included

The keys are random 64-bit values in device memory, the ids stay on the device.  Per case: warmed, CALLS timed calls (a host
clock around calls that each end in a stream synchronisation), then as many with cph_ctx_profile on for the per-kernel times
(HIP events) and their byte models.  Every route's first ids are compared with numpy's at the first size.

    python tools/order_microbench.py [sizes=1e7,1e8] [calls=5] [ks=10,1e4,1e6]
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, _native as N  # noqa: E402
from csvplus_amd import ordering as O  # noqa: E402
from csvplus_amd.materialize import order_rows  # noqa: E402

DEVICE = N.CPH_MEM_DEVICE
SIZES = [int(float(s)) for s in (sys.argv[1] if len(sys.argv) > 1 else "1e7,1e8").split(",")]
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
KS = [int(float(k)) for k in (sys.argv[3] if len(sys.argv) > 3 else "10,1e4,1e6").split(",")]


def d2h(ptr, count, dtype):
    import ctypes as C
    with open("/proc/self/maps") as f:   # the HIP runtime torch loaded: one runtime per process
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64.so" in line))
    out = np.empty(count, dtype=dtype)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


def timed(ctx, fn):
    """(wall ms per call, {kernel: (ms per call, launches per call, model MB per call)}, the last call's Ordered facts)"""
    facts = None
    for _ in range(2):
        fn().release()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        r = fn()
        facts = (r.select_used, r.candidates, len(r))
        r.release()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / CALLS * 1e3
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(CALLS):
        fn().release()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile(False)
    kernels = {k: (v["total_ms"] / CALLS, v["launches"] / CALLS, v["algo_bytes"] / CALLS / 1e6) for k, v in prof.items()}
    return wall, kernels, facts


def show(title, wall, kernels, facts):
    total = sum(ms for ms, _, _ in kernels.values())
    print(f"\n== {title}: {wall:.3f} ms per call (kernels {total:.3f} ms); select_used={int(facts[0])} candidates={facts[1]} rows out={facts[2]} ==")
    print(f"{'kernel':28s}{'ms':>9s}{'launches':>10s}{'model MB':>12s}{'TB/s':>8s}")
    for name, (ms, launches, mb) in sorted(kernels.items(), key=lambda kv: -kv[1][0]):
        rate = f"{mb / 1e6 / (ms / 1e3):8.2f}" if ms > 0 and mb > 0 else ""
        print(f"{name:28s}{ms:9.3f}{launches:10.1f}{mb:12.1f}{rate}")


def main():
    ctx = Context(0)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(794)
    print(f"cph_order_rows microbenchmark: sizes {SIZES}, {CALLS} timed calls per case, k in {KS}")
    try:
        print(f"copy rate of this box (cph_calibrate kind copy, 1 GiB): {2 * (1 << 30) / ctx.calibrate('copy', 1 << 30) / 1e9:.2f} TB/s")
    except Exception as e:   # noqa: BLE001 — the rate is context, not a result
        print(f"copy rate: not measured ({e})")
    summary = []
    for si, n in enumerate(SIZES):
        ints = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda:0", generator=gen)
        flts = torch.rand((n,), dtype=torch.float64, device="cuda:0", generator=gen)
        few = torch.randint(0, 1000, (n,), dtype=torch.int64, device="cuda:0", generator=gen)
        torch.cuda.synchronize()
        if si == 0:   # the old route, and the answer every route is compared with
            t0 = time.perf_counter()
            host = ints.cpu().numpy()
            t1 = time.perf_counter()
            want = np.argsort(host, kind="stable")
            t2 = time.perf_counter()
            print(f"\nold route at {n:.0e} rows: copy to the host {(t1 - t0) * 1e3:.1f} ms + numpy.argsort(kind='stable') {(t2 - t1) * 1e3:.1f} ms "
                  f"= {(t2 - t0) * 1e3:.1f} ms (one run, host clock)")
            summary.append((f"{n:.0e} old route (copy + numpy stable argsort)", (t2 - t0) * 1e3))
        one = [O.Asc(ints, "int")]
        two = [O.Asc(few, "int"), O.Desc(flts, "float")]
        ctx.set_option("order_select", 1)
        w, k, f = timed(ctx, lambda: order_rows(ctx, one, n, out_mem=DEVICE))
        show(f"full sort, one int64 key, {n:.0e} rows", w, k, f)
        summary.append((f"{n:.0e} full sort, one int64 key", w))
        if si == 0:
            r = order_rows(ctx, one, n, out_mem=DEVICE)
            assert (d2h(r.ids_ptr, n, np.uint32) == want).all(), "the full sort differs from numpy's stable argsort"
            r.release()
        w, k, f = timed(ctx, lambda: order_rows(ctx, two, n, out_mem=DEVICE))
        show(f"full sort, int64 key (1000 values) then float64 key descending, {n:.0e} rows", w, k, f)
        summary.append((f"{n:.0e} full sort, two keys", w))
        for kk in KS:
            if kk > n:
                continue
            for mode, label in ((2, "select"), (0, "full sort")):
                ctx.set_option("order_select", mode)
                w, k, f = timed(ctx, lambda: order_rows(ctx, one, n, limit=kk, out_mem=DEVICE))
                show(f"top-{kk:.0e}, {label}, one int64 key, {n:.0e} rows", w, k, f)
                summary.append((f"{n:.0e} top-{kk:.0e} {label}", w))
                if si == 0:
                    r = order_rows(ctx, one, n, limit=kk, out_mem=DEVICE)
                    assert (d2h(r.ids_ptr, kk, np.uint32) == want[:kk]).all(), f"top-{kk} ({label}) differs from numpy's stable argsort"
                    r.release()
        ctx.set_option("order_select", 1)
        del ints, flts, few, one, two
        torch.cuda.empty_cache()
    print("\n== summary: ms per call ==")
    for name, ms in summary:
        print(f"{name:52s}{ms:12.3f}")
    ctx.close()


if __name__ == "__main__":
    main()
