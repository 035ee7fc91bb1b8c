#!/usr/bin/env python3
"""cph_chain_aggregate (Totals over a Join) against the route without it, on the bench's own tables: `rows` orders joined with a
customers table of G rows (8-byte fixed-width ids, unique index, chain of sorted positions in device memory), then per customer
Count + one int64 Sum + one float64 Sum over device arrays with one value per joined row.  G = 1e7, 1e5 and 3 by default.

new route   aggregate.join_totals(chain, 0, index, [Sum(int), Sum(float)]): grouped by build_row[0], no second index.
old route   what a caller had before: the key column gathered through the chain (cph_gather_rows over the customers' ids in
            index order), IndexOn over the gathered column, cph_index_aggregate with the same two arrays as `numbers`.  It
            uses nothing this feature adds, so it is measured here, in the same process on the same tables.

Per route: warmed, CALLS timed calls (wall clock, results left on the device and released), then as many with cph_ctx_profile
on for the per-kernel times and their byte models.  "Algorithmic bytes" of the new route: 4 B of build_row per pass (Count, int
Sum, sort keys) + 8 B per value and spec + 8 B per group and column.  The sums of the two routes are compared at full size
(ints exactly; floats are multiples of 1/8, exact in every order).

    python tools/join_totals_microbench.py [rows=1e8] [calls=10] [json path] [groups,comma,separated]
"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, DeviceIndex, _native as N, datagen as dg  # noqa: E402
from csvplus_amd import aggregate as A  # noqa: E402
from csvplus_amd.materialize import gather_rows, permute_col  # noqa: E402

DEVICE = N.CPH_MEM_DEVICE
M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
GROUPS = [int(float(g)) for g in sys.argv[4].split(",")] if len(sys.argv) > 4 else [10_000_000, 100_000, 3]


def d2h(ptr, count, dtype):
    import ctypes as C
    with open("/proc/self/maps") as f:   # the HIP runtime torch loaded: one runtime per process
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64.so" in line))
    out = np.empty(count, dtype=dtype)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


def timed(ctx, fn):
    for _ in range(2):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / CALLS * 1e3
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(CALLS):
        fn()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile(False)
    kern = {}
    for name, st in prof.items():
        ms = st["total_ms"] / CALLS
        b = st["algo_bytes"] / CALLS
        kern[name] = {"ms_per_call": round(ms, 4), "launches_per_call": st["launches"] / CALLS, "algo_MB_per_call": round(b / 1e6, 2),
                      "TBps": round(b / (ms / 1e3) / 1e12, 3) if ms > 0 else None}
    return wall, kern


def main():
    ctx = Context(0)
    c_bytes = 1 << 30
    c_ms = ctx.calibrate("copy", c_bytes, 0, 5)
    copy_tbps = 2 * c_bytes / (c_ms / 1e3) / 1e12
    res = {"rows": M, "calls": CALLS, "copy_TBps": round(copy_tbps, 3), "lds_groups": N.CPH_CHAIN_AGG_LDS_GROUPS, "configs": []}
    print("copy_TBps", copy_tbps, flush=True)
    ints = torch.randint(-1000, 1000, (M,), dtype=torch.int64, device="cuda:0")
    flts = torch.randint(-8000, 8000, (M,), dtype=torch.int64, device="cuda:0").to(torch.float64) / 8.0
    torch.cuda.synchronize()
    for G in GROUPS:
        t0 = time.perf_counter()
        ids = dg.customers(G)["id"].to_device()
        cust = dg.column(dg.UNIFORM, M, G, encoding=dg.FIXED8, seed=dg.SEED + 3).to_device()
        ix = DeviceIndex(ctx, [ids], unique=True)
        ch = N.join_chain(ctx, [(ix, [cust])], out_mem=DEVICE, positions=True)
        n = ch.nrows
        sorted_ids = permute_col(ctx, ix, ids)
        rows = (ch.device_ptrs()["build_row"][0], 32, n)
        print(f"G={G}: generated, indexed and joined in {time.perf_counter() - t0:.1f}s, {n} joined rows", flush=True)
        assert n == M
        specs = [A.Sum(ints, "int"), A.Sum(flts, "float")]
        cfg = {"groups": G, "joined_rows": n}

        def new_route():
            A.join_totals(ch, 0, ix, specs, out_mem=DEVICE).release()

        def old_route():
            keys = gather_rows(ctx, sorted_ids.as_device_strcol(), rows, out_mem=DEVICE)
            ix2 = DeviceIndex(ctx, [keys.as_device_strcol()])
            A.totals(ix2, specs, out_mem=DEVICE).release()
            ix2.close()
            keys.release()

        for label, fn in (("new", new_route), ("old", old_route)):
            wall, kern = timed(ctx, fn)
            run = {"call_wall_ms": round(wall, 3), "kernels_ms_sum": round(sum(k["ms_per_call"] for k in kern.values()), 3), "kernels": kern}
            if label == "new":
                algo = n * (3 * 4 + 2 * 8) + G * 3 * 8
                run.update(algorithmic_bytes=algo, bytes_over_wall_TBps=round(algo / (wall / 1e3) / 1e12, 3))
            else:   # the same information by the old route's own model: keys gathered (8 B read + written), then the new route's bytes
                algo = n * (4 + 16 + 3 * 4 + 2 * 8) + G * 3 * 8
                run.update(algorithmic_bytes=algo, bytes_over_wall_TBps=round(algo / (wall / 1e3) / 1e12, 3))
            cfg[label] = run
            print(label, json.dumps(run), flush=True)
        cfg["speedup"] = round(cfg["old"]["call_wall_ms"] / cfg["new"]["call_wall_ms"], 2)
        # the two routes agree: the old route's groups are the customers that have orders, in key order
        t = A.join_totals(ch, 0, ix, specs, out_mem=DEVICE)
        cnt = d2h(t.count[0], G, np.int64)
        si, sf = d2h(t.values[0][0], G, np.int64), d2h(t.values[1][0], G, np.float64)
        t.release()
        keys = gather_rows(ctx, sorted_ids.as_device_strcol(), rows, out_mem=DEVICE)
        ix2 = DeviceIndex(ctx, [keys.as_device_strcol()])
        o = A.totals(ix2, specs)
        have = cnt > 0
        assert o.ngroups == int(have.sum()) and (o.count.astype(np.int64) == cnt[have]).all()
        assert (o.values[0] == si[have]).all() and (o.values[1] == sf[have]).all()
        cfg["routes_agree"] = True
        print(f"G={G}: speedup {cfg['speedup']}x, routes agree over {o.ngroups} groups", flush=True)
        ix2.close()
        keys.release()
        res["configs"].append(cfg)
        sorted_ids.release()
        ch.release()
        ix.close()
        del ids, cust
        torch.cuda.empty_cache()
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(json.dumps(res, indent=1))


main()
