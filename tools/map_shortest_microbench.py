#!/usr/bin/env python3
"""What a FLOAT64_SHORTEST piece costs: k_map_lens / k_map_copy under cph_ctx_profile for rows of Format(Float.shortest(a, fmt)),
fmt = 'e', 'f', 'g', and of Format(Float(a, 2)) over the SAME array: random 64-bit patterns read as doubles, kept when finite
and below 2^128 in magnitude (what the fixed-precision piece accepts), device-resident, device result.  Per template: two
warm-up calls, then REPS profiled calls; the kernels' mean times, the output bytes per row and the output bytes per second of
the two passes together.

    python tools/map_shortest_microbench.py [rows=1e7] [reps=10] [out.json] [fixed]

With a fourth argument only Format(Float(a, 2)) is timed: a library without the piece kind (CSVPLUS_HIP_LIB) runs that one.
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, _native as N  # noqa: E402
from csvplus_amd.mapping import Float, Format  # noqa: E402
from csvplus_amd.materialize import map_column  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None
FIXED_ONLY = len(sys.argv) > 4
ctx = Context(0)
rng = np.random.default_rng(1)
vals = np.empty(0, dtype=np.float64)
while len(vals) < M:
    v = rng.integers(0, 2 ** 64, M, dtype=np.uint64).view(np.float64)
    vals = np.concatenate([vals, v[np.isfinite(v) & (np.abs(v) < 2.0 ** 128)]])[:M]
tf = torch.from_numpy(vals).to("cuda:0")
torch.cuda.synchronize()
templates = {"Format(Float, 2)": Format(Float.on_device(tf.data_ptr(), M, 2))}
if not FIXED_ONLY:
    for fmt in "efg":
        templates[f"Format(shortest '{fmt}')"] = Format(Float.shortest_on_device(tf.data_ptr(), M, fmt))
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
    both = r["k_map_lens_ms"] + r["k_map_copy_ms"]
    r["both_ns_per_row"] = both * 1e6 / M
    r["out_GBps"] = out_bytes / both / 1e6
    r["rows_per_us"] = M / both / 1e3
    results["templates"][name] = r
    print(f"{name:22s}: " + ", ".join(f"{k}={v:.4g}" for k, v in r.items()), flush=True)
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(results, indent=1) + "\n")
ctx.close()
