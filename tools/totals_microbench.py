#!/usr/bin/env python3
"""cph_index_aggregate over the bench's own `orders` table: a device-resident index over cust_id (8-byte fixed-width ids) of `rows`
rows with rows/10 and rows/1000 distinct keys; one int64 SUM from `numbers` (a device array, gathered through perm), one from a
`col` (qty: decimal text, converted through perm), and the groups alone (no spec).

Per configuration: warmed, CALLS timed calls for the call's total (wall clock around the calls, results left on the device), then
as many with cph_ctx_profile on for the per-kernel times and the achieved bytes per second by the kernels' byte models
(DESIGN.md §9), next to cph_calibrate kind 0 (this box's streaming-copy rate) and to the algorithmic bytes of the whole call:
codes once, 8 B + 1 B per row and spec, 4 B of perm per row for `numbers`, 20 B + 8 B x nspecs per group.  Last the host route,
the only way to the same sums without the feature: index.perm() and the typed column downloaded, numpy.add.reduceat (the run
starts are handed to it for free), checked against the device's sums at full size.

    python tools/totals_microbench.py [rows=1e8] [calls=20] [json path]
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
from csvplus_amd.materialize import to_int  # noqa: E402

DEVICE = N.CPH_MEM_DEVICE
M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def main():
    ctx = Context(0)
    c_bytes = 1 << 30
    c_ms = ctx.calibrate("copy", c_bytes, 0, 5)
    copy_tbps = 2 * c_bytes / (c_ms / 1e3) / 1e12
    res = {"rows": M, "copy_TBps": round(copy_tbps, 3), "configs": []}
    print("copy_TBps", copy_tbps, flush=True)
    for ngroups_asked in (M // 10, M // 1000):
        t0 = time.perf_counter()
        ords = dg.orders(M, ngroups_asked, 100)
        cust, qty = ords["cust_id"].to_device(), ords["qty"].to_device()
        ix = DeviceIndex(ctx, [cust])
        info = ix.info()
        code_bytes = info["key_bytes"] * info["code_words"]
        print(f"generated + indexed in {time.perf_counter() - t0:.1f}s, info {info}", flush=True)
        nums = torch.randint(-1000, 1000, (M,), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        cfg = {"groups_asked": ngroups_asked, "code_bytes_per_row": code_bytes, "runs": {}}
        for label, specs in (("sum_numbers", [A.Sum(nums, "int")]), ("sum_col", [A.Sum(qty, "int")]), ("count_only", [])):
            ng = 0
            for _ in range(3):
                t = A.totals(ix, specs, out_mem=DEVICE)
                ng = t.ngroups
                t.release()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                A.totals(ix, specs, out_mem=DEVICE).release()
            ctx.synchronize()
            wall = (time.perf_counter() - t0) / CALLS * 1e3
            ctx.profile(True)
            ctx.profile_read(reset=True)
            for _ in range(CALLS):
                A.totals(ix, specs, out_mem=DEVICE).release()
            ctx.synchronize()
            prof = ctx.profile_read()
            ctx.profile(False)
            kern = {}
            for name, st in prof.items():
                ms = st["total_ms"] / max(1, st["launches"])
                b = st["algo_bytes"] / max(1, st["launches"])
                kern[name] = {"ms": round(ms, 4), "launches_per_call": st["launches"] / CALLS, "algo_MB": round(b / 1e6, 2),
                              "TBps": round(b / (ms / 1e3) / 1e12, 3) if ms > 0 else None,
                              "frac_of_copy": round(b / (ms / 1e3) / 1e12 / copy_tbps, 3) if ms > 0 else None}
            nspecs = len(specs)
            algo = M * code_bytes + M * 9 * nspecs + (4 * M if label == "sum_numbers" else 0) + ng * (20 + 8 * nspecs)
            run = {"ngroups": ng, "call_wall_ms": round(wall, 3), "kernels_ms_sum": round(sum(k["ms"] * k["launches_per_call"] for k in kern.values()), 3),
                   "algorithmic_bytes": algo, "bytes_over_wall_TBps": round(algo / (wall / 1e3) / 1e12, 3),
                   "frac_of_copy": round(algo / (wall / 1e3) / 1e12 / copy_tbps, 3), "kernels": kern}
            cfg["runs"][label] = run
            print(label, json.dumps(run), flush=True)
        # the host route of the parent commit: perm and the typed column downloaded, numpy.add.reduceat (run starts given for free)
        t = A.totals(ix, [])
        starts = t.first_position.astype(np.int64)
        want = A.totals(ix, [A.Sum(qty, "int")]).values[0]
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            perm = ix.perm_host_view()
            col = to_int(ctx, qty)
            sums = np.add.reduceat(col.values[perm], starts)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        assert (sums == want).all()
        cfg["host_route_ms"] = round(best, 1)
        print("host_route_ms", best, flush=True)
        res["configs"].append(cfg)
        ix.close()
        del nums, cust, qty, ords
        torch.cuda.empty_cache()
    if len(sys.argv) > 3:
        Path(sys.argv[3]).write_text(json.dumps(res, indent=1))


main()
