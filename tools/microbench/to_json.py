#!/usr/bin/env python3
"""ToJSON of the README chain's joined rows (orders JOIN customers JOIN products, 6 output columns, device-resident, sorted
positions) against the two-pass ToCsv (csv_onepass = 0) on the same rows, in one process: warm-up, then alternating repeats.
Prints wall time, output GB and GB/s per writer, and the ctx.profile attribution of k_json_lens / k_json_copy."""
import sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import torch
from csvplus_amd import _native as N, datagen as dg
from csvplus_amd.engine import Engine
from csvplus_amd.materialize import csv_write, json_write, permute_col

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 50_000_000
REPS = 3
NC, NP = 10_000_000, 100_000
eng = Engine(0); ctx = eng.ctx; dev = eng.device
cust = dg.customers(NC); prod = dg.products(NP); ords = dg.orders(M, NC, NP)
d = {k: v.to_device(dev) for k, v in {"cid": cust["id"], "name": cust["name"], "surname": cust["surname"], "pid": prod["prod_id"],
                                       "product": prod["product"], "price": prod["price"], "o_cid": ords["cust_id"],
                                       "o_pid": ords["prod_id"], "o_qty": ords["qty"]}.items()}
ia = N.DeviceIndex(ctx, [d["cid"]], unique=True); ib = N.DeviceIndex(ctx, [d["pid"]], unique=True)
ch = N.join_chain(ctx, [(ia, [d["o_cid"]]), (ib, [d["o_pid"]])], out_mem=N.CPH_MEM_DEVICE, positions=True)
ptrs = ch.device_ptrs(); n = ch.nrows
keep = [permute_col(ctx, ia, d["name"]), permute_col(ctx, ia, d["surname"]), permute_col(ctx, ib, d["product"]), permute_col(ctx, ib, d["price"])]
cols = [d["o_cid"], d["o_qty"]] + [k.as_device_strcol() for k in keep]
ids = [None, None] + [(ptrs["build_row"][0], 32, n)] * 2 + [(ptrs["build_row"][1], 32, n)] * 2
names = ["cust_id", "qty", "name", "surname", "product", "price"]
ctx.set_option("csv_onepass", 0)
writers = {"ToJSON": lambda: json_write(ctx, cols, names, out_mem=N.CPH_MEM_DEVICE, row_ids=ids, nrows=n),
           "ToCsv(2-pass)": lambda: csv_write(ctx, cols, names, out_mem=N.CPH_MEM_DEVICE, row_ids=ids, nrows=n)}
size, wall, prof = {}, {k: 0.0 for k in writers}, {k: {} for k in writers}
for k, w in writers.items():   # warm-up
    t = w(); size[k] = len(t); t.release()
for _ in range(REPS):
    for k, w in writers.items():   # alternating
        ctx.profile(True); ctx.profile_read(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        w().release()
        torch.cuda.synchronize(); wall[k] += time.perf_counter() - t0
        for kn, v in ctx.profile_read(reset=True).items():
            prof[k][kn] = prof[k].get(kn, 0.0) + v["total_ms"]
        ctx.profile(False)
print(f"rows {n} (of {M} orders), 6 columns, device-resident, positions", flush=True)
for k in writers:
    dt = wall[k] / REPS
    ks = ", ".join(f"{kn}={v / REPS:.3f} ms" for kn, v in sorted(prof[k].items(), key=lambda kv: -kv[1])[:5])
    print(f"{k:14s}: wall {dt * 1e3:8.3f} ms  {size[k] / 1e9:6.3f} GB  {size[k] / dt / 1e9:7.1f} GB/s  ({size[k] / n:.1f} B/row) | {ks}", flush=True)
