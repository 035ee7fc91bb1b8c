#!/usr/bin/env python3
"""cph_filter_rows over the bench's own `orders` columns, device-resident: an 8-byte fixed-width id column (cust_id) and a
variable-length one (prod_id, decimal, 32-bit offsets), WHERE mode, at selectivities of about 0.1 %, 50 % and 100 %.

Per case: warm-up, then REPS synchronised calls with the profiler off (wall time per call), achieved bytes/s by the byte
model of DESIGN.md (the column's value and offset bytes + 2 x n/8 bitmap bytes + out_bits/8 per kept row), and — in a
second pass with cph_ctx_profile on — the times of k_pred_eval / the scan / k_pred_emit.  Next to it, measured in the same
process on the same box: cph_calibrate kind 0 (this box's streaming-copy rate) and the only route without the feature (the
column brought to the host with an identity gather_rows, compared there with numpy).

    python tools/filter_microbench.py [rows=1e8] [reps=20]        (rocprofv3 --kernel-trace --stats -- python tools/... 2e7 5)

--expr instead measures the condition `price * float64(qty) >= 100` over a 5-byte price column ("dd.dd") and a 2-byte qty column,
both fixed-width and device-resident: k_expr_cmp (filter_rows with one ExprCmp: one kernel, one bit per row), k_expr_eval for the
same left side (eval_number: the same reads, 9 bytes per row written), and the route without the feature — eval_number, the
values written back as shortest text by a Map, FloatCmp on that text — call by call.

    python tools/filter_microbench.py --expr [rows=1e8] [reps=10]
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from csvplus_amd import Context, _native as N, datagen as dg  # noqa: E402
from csvplus_amd.materialize import filter_rows, gather_rows  # noqa: E402
from csvplus_amd.predicates import Like, Not  # noqa: E402

EXPR = "--expr" in sys.argv
if EXPR:
    sys.argv.remove("--expr")
M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else (10 if EXPR else 20)
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


copy_bytes = 1 << 30
copy_ms = ctx.calibrate("copy", copy_bytes, reps=10)
copy_rate = 2 * copy_bytes / (copy_ms * 1e-3)
print(f"rows {M}, reps {REPS}; streaming copy (cph_calibrate kind 0): {copy_rate / 1e9:.0f} GB/s", flush=True)



def expr_case():
    from csvplus_amd import StrCol
    from csvplus_amd import mapping as MP
    from csvplus_amd.expr import FloatCol, IntCol, ToFloat
    from csvplus_amd.materialize import eval_number, map_column
    from csvplus_amd.predicates import ExprCmp, FloatCmp

    rng = np.random.default_rng(1)
    cents = rng.integers(0, 10000, M)
    qty = rng.integers(0, 100, M)
    price = np.empty((M, 5), dtype=np.uint8)   # "dd.dd"
    for k, div in ((0, 1000), (1, 100), (3, 10), (4, 1)):
        price[:, k] = 0x30 + (cents // div) % 10
    price[:, 2] = 0x2E
    qtxt = np.empty((M, 2), dtype=np.uint8)
    qtxt[:, 0], qtxt[:, 1] = 0x30 + qty // 10, 0x30 + qty % 10
    cols = {"price": StrCol(price.reshape(-1), None, M, 32, N.CPH_MEM_HOST, fixed_width=5).to_device(),
            "qty": StrCol(qtxt.reshape(-1), None, M, 32, N.CPH_MEM_HOST, fixed_width=2).to_device()}
    amount = FloatCol("price") * ToFloat(IntCol("qty"))
    pred = ExprCmp(amount, ">=", 100.0)
    want = int(np.count_nonzero(cents / 100.0 * qty >= 100.0))   # the same IEEE operations: a division, a product

    def new_route():
        rl = filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE)
        k = len(rl)
        rl.release()
        return k

    def old_route():
        nc = eval_number(ctx, cols, amount, out_mem=N.CPH_MEM_DEVICE)
        text = map_column(ctx, {}, MP.Format(MP.Float.shortest_on_device(nc.values[0], M, "g")), nrows=M, out_mem=N.CPH_MEM_DEVICE)
        rl = filter_rows(ctx, {"amount": text.as_device_strcol()}, FloatCmp("amount", ">=", 100.0), out_mem=N.CPH_MEM_DEVICE)
        k = len(rl)
        rl.release()
        text.release()
        nc.release()
        return k

    def eval_only():
        eval_number(ctx, cols, amount, out_mem=N.CPH_MEM_DEVICE).release()

    kept = new_route()
    assert kept == want == old_route(), (kept, want)
    walls = {name: timed(fn, REPS) for name, fn in (("ExprCmp", new_route), ("eval_number", eval_only), ("three calls", old_route))}
    stats = {}
    for name, fn in (("ExprCmp", new_route), ("eval_number", eval_only), ("three calls", old_route)):
        ctx.profile(True)
        ctx.profile_read(reset=True)
        for _ in range(3):
            fn()
        stats[name] = ctx.profile_read(reset=True)
        ctx.profile(False)
    cmp_ms = stats["ExprCmp"]["k_expr_cmp"]["total_ms"] / 3
    eval_ms = stats["eval_number"]["k_expr_eval"]["total_ms"] / 3
    read = 7.0 * M
    print(f"price * float64(qty) >= 100 over {M} rows: kept {kept} ({100.0 * kept / M:.2f} %)")
    print(f"  k_expr_cmp   {cmp_ms:8.3f} ms  {(read + M / 8) / cmp_ms / 1e6:7.0f} GB/s by the model ({100 * (read + M / 8) / (cmp_ms * 1e-3) / copy_rate:4.1f} % of copy)")
    print(f"  k_expr_eval  {eval_ms:8.3f} ms  {(read + 9.0 * M) / eval_ms / 1e6:7.0f} GB/s by the model ({100 * (read + 9.0 * M) / (eval_ms * 1e-3) / copy_rate:4.1f} % of copy)"
          f"   k_expr_cmp / k_expr_eval = {cmp_ms / eval_ms:.3f}")
    for name in ("ExprCmp", "eval_number", "three calls"):
        ks = ", ".join(f"{k}={v['total_ms'] / 3:.3f} ms" for k, v in stats[name].items())
        print(f"  {name:12s} call {walls[name] * 1e3:9.3f} ms | {ks}")
    print(f"  three calls / ExprCmp = {walls['three calls'] / walls['ExprCmp']:.1f}x", flush=True)


if EXPR:
    expr_case()
    ctx.close()
    sys.exit(0)

cases = []   # (label, host column, predicate)
for label, domain in (("0.1 %", 1000), ("50 %", 2)):
    o = dg.orders(M, domain, domain)
    cases.append((f"fixed8 {label}", o["cust_id"], Like(c=o["cust_id"].value(0))))
    cases.append((f"varlen {label}", o["prod_id"], Like(c=o["prod_id"].value(0))))
    if domain == 2:
        cases.append(("fixed8 100 %", o["cust_id"], Not(Like(c=b"zzzzzzzz"))))
        cases.append(("varlen 100 %", o["prod_id"], Not(Like(c=b"zzz"))))

for label, hcol, pred in cases:
    dcol = hcol.to_device()
    cols = {"c": dcol}
    rl = filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE)
    kept = len(rl)
    rl.release()
    wall = timed(lambda: filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE).release(), REPS)
    model = hcol.nbytes_values() + hcol.nbytes_offsets() + 2 * M / 8 + 4 * kept
    ctx.profile(True)
    ctx.profile_read(reset=True)
    for _ in range(3):
        filter_rows(ctx, cols, pred, out_mem=N.CPH_MEM_DEVICE).release()
    st = ctx.profile_read(reset=True)
    ctx.profile(False)
    ks = ", ".join(f"{k}={v['total_ms'] / 3:.3f} ms" for k, v in st.items())
    ev = st["k_pred_eval"]["total_ms"] / 3
    ev_bytes = hcol.nbytes_values() + hcol.nbytes_offsets() + M / 8
    # the route without the feature: the column to the host (identity gather), compared there
    reps_old = 1 if M > 20_000_000 else 3
    lit = pred.items[0][1] if isinstance(pred, Like) else pred.pred.items[0][1]

    def old_route():
        h = gather_rows(ctx, dcol, out_mem=N.CPH_MEM_HOST)
        offs = h.offsets.astype(np.int64)
        lens = np.diff(offs)
        idx = np.flatnonzero(lens == len(lit))
        if len(lit) and len(idx):
            eq = np.ones(len(idx), dtype=bool)
            for j, b in enumerate(lit):
                eq &= h.data[offs[idx] + j] == b
            idx = idx[eq]
        return idx

    old = timed(old_route, reps_old) if reps_old > 1 else None
    if old is None:
        t0 = time.perf_counter()
        old_route()
        old = time.perf_counter() - t0
    print(f"{label:13s}: kept {kept:>10d} ({100.0 * kept / M:7.3f} %)  call {wall * 1e3:8.3f} ms  {model / wall / 1e9:7.1f} GB/s by the model"
          f" ({100 * model / wall / copy_rate:4.1f} % of copy) | k_pred_eval {ev:.3f} ms = {ev_bytes / ev / 1e6:.0f} GB/s"
          f" ({100 * ev_bytes / (ev * 1e-3) / copy_rate:4.1f} % of copy) | {ks} | host route {old * 1e3:.0f} ms", flush=True)
    del dcol, cols
    torch.cuda.empty_cache()
ctx.close()
