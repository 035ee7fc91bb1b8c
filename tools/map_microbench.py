#!/usr/bin/env python3
"""cph_map_format over the bench's own `orders` columns, device-resident: a two-column template — cust_id (8 bytes, fixed
width) followed by prod_id (decimal, 32-bit offsets) — against the SUM of two cph_gather_rows calls over the same two
columns, which move the same value bytes into new columns and are the closest thing the library had before Map.

Two cases: the columns' own rows (identity), and both columns read through one array of random 32-bit row ids (what a
template over joined rows does).  Per case and route: warm-up, then REPS rounds in which the two routes ALTERNATE, each
call synchronised, wall time per call; reported as median and min..max over the rounds (the run-to-run spread), with the
byte model of DESIGN.md (value bytes read + written, offsets and row ids read, 8 bytes of offsets written per row) over the
median.  A second pass with cph_ctx_profile on gives the kernels' own times.  Results also go to a JSON file when a path
is given.

    python tools/map_microbench.py [rows=1e7] [reps=15] [out.json]
"""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, _native as N, datagen as dg  # noqa: E402
from csvplus_amd.mapping import Col, Format  # noqa: E402
from csvplus_amd.materialize import gather_rows, map_column  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
OUT = sys.argv[3] if len(sys.argv) > 3 else None
ctx = Context(0)


def sync():
    ctx.synchronize()
    torch.cuda.synchronize()


def once(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


copy_bytes = 1 << 30
copy_ms = ctx.calibrate("copy", copy_bytes, reps=10)
copy_rate = 2 * copy_bytes / (copy_ms * 1e-3)
print(f"rows {M}, reps {REPS}; streaming copy (cph_calibrate kind 0): {copy_rate / 1e9:.0f} GB/s", flush=True)

o = dg.orders(M, 1_000_000, 1000)
host = {"cust_id": o["cust_id"], "prod_id": o["prod_id"]}
dev = {k: c.to_device() for k, c in host.items()}
template = Format(Col("cust_id"), Col("prod_id"))
value_bytes = sum(c.nbytes_values() for c in host.values())
offset_bytes = sum(c.nbytes_offsets() for c in host.values())
perm = torch.from_numpy(np.random.default_rng(1).permutation(M).astype(np.uint32).view(np.uint8)).to("cuda:0")
results = {"rows": M, "reps": REPS, "copy_GBps": copy_rate / 1e9, "cases": {}}

for label, ids in (("identity", None), ("row ids (random, 32-bit)", (perm.data_ptr(), 32, M))):
    row_ids = None if ids is None else {"cust_id": ids, "prod_id": ids}

    def run_map():
        map_column(ctx, dev, template, row_ids=row_ids, out_mem=N.CPH_MEM_DEVICE).release()

    def run_gathers():
        for c in dev.values():
            gather_rows(ctx, c, ids, out_mem=N.CPH_MEM_DEVICE).release()

    cb = map_column(ctx, dev, template, row_ids=row_ids, out_mem=N.CPH_MEM_DEVICE)
    assert cb.nrows == M and cb.nbytes == value_bytes
    cb.release()
    run_gathers()
    t_map, t_gat = [], []
    for _ in range(REPS):
        t_map.append(once(run_map))
        t_gat.append(once(run_gathers))
    id_bytes = 0 if ids is None else 4 * M
    model_map = 2 * value_bytes + offset_bytes + id_bytes + 8 * M          # one offsets array written
    model_gat = 2 * value_bytes + offset_bytes + 2 * id_bytes + 2 * 8 * M   # two of them, the ids read twice
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(3):
        run_map()
        run_gathers()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    ks = {k: v["total_ms"] / 3 for k, v in st.items()}
    case = {}
    for name, ts, model in (("cph_map_format", t_map, model_map), ("2 x cph_gather_rows", t_gat, model_gat)):
        med = statistics.median(ts)
        case[name] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "model_bytes": model, "model_GBps": model / med / 1e6}
        print(f"{label:26s} {name:20s}: median {med:8.3f} ms  (min {min(ts):8.3f}, max {max(ts):8.3f})  {model / med / 1e6:7.1f} GB/s by the model"
              f" ({100 * model / (med * 1e-3) / copy_rate:4.1f} % of copy)", flush=True)
    case["kernels_ms"] = ks
    print(f"{label:26s} kernels: " + ", ".join(f"{k}={v:.3f} ms" for k, v in ks.items()), flush=True)
    results["cases"][label] = case
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(results, indent=1) + "\n")
ctx.close()
