#!/usr/bin/env python3
"""What a FLOAT64 piece costs: k_map_lens / k_map_copy under cph_ctx_profile for rows of Format(Int(a)) and of
Format(Float(a, 2)), the values of both taken from ONE array of whole numbers below 1e6, device-resident, device result.
Per template: warm-up, then REPS profiled calls; the kernels' mean times, the output bytes per row, and the bytes per row
of k_map_copy's byte model (2 x output bytes + 8 of offsets + 8 of the value) over its time.

    python tools/map_float_microbench.py [rows=1e7] [reps=10] [out.json]
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, _native as N  # noqa: E402
from csvplus_amd.mapping import Float, Format, Int  # noqa: E402
from csvplus_amd.materialize import map_column  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else None
ctx = Context(0)
vals = np.random.default_rng(1).integers(0, 1_000_000, M)
ti = torch.from_numpy(vals.astype(np.int64)).to("cuda:0")
tf = torch.from_numpy(vals.astype(np.float64)).to("cuda:0")
torch.cuda.synchronize()
templates = {"Format(Int)": Format(Int.on_device(ti.data_ptr(), M)), "Format(Float, 2)": Format(Float.on_device(tf.data_ptr(), M, 2))}
results = {"rows": M, "reps": REPS, "templates": {}}
for name, t in templates.items():
    def run():
        cb = map_column(ctx, {}, t, nrows=M, out_mem=N.CPH_MEM_DEVICE)
        nbytes = cb.nbytes
        cb.release()
        return nbytes
    out_bytes = run()
    run()
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(REPS):
        run()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    r = {"out_bytes_per_row": out_bytes / M}
    for k in ("k_map_lens", "k_map_copy"):
        r[k + "_ms"] = st[k]["total_ms"] / st[k]["launches"]
    model = st["k_map_copy"]["algo_bytes"] / st["k_map_copy"]["launches"]
    r["k_map_copy_model_bytes_per_row"] = model / M
    r["k_map_copy_model_GBps"] = model / r["k_map_copy_ms"] / 1e6
    r["k_map_copy_ns_per_row"] = r["k_map_copy_ms"] * 1e6 / M
    results["templates"][name] = r
    print(f"{name:18s}: " + ", ".join(f"{k}={v:.4g}" for k, v in r.items()), flush=True)
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(results, indent=1) + "\n")
ctx.close()
