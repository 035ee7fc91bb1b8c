#!/usr/bin/env python3
"""cph_csv_parse_lazy against cph_csv_parse on device-resident text, from the library's own HIP-event profile (cph_ctx_profile):
  (a) the orders file of bench.py / tools/microbench/csv_ingest.py (no quote anywhere: both calls take k_csv_fast)
  (b) a strictly valid text of fixed-width records with the middle field of 30 % of the records quoted (10 % of the fields):
      the classic record-parallel passes on both sides, the separator stage is what differs
  (c) the per-kernel split of (b)
Calls alternate strict / lazy; per call the sum of the kernels' event times and the wall time around a synchronise; medians of
REPS warm calls.  Usage: csv_lazy_microbench.py [rows, default 4e7] [reps, default 11]"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from csvplus_amd import _native as N, datagen as dg, ingest  # noqa: E402
from csvplus_amd.engine import Engine  # noqa: E402

M = int(float(sys.argv[1])) if len(sys.argv) > 1 else 40_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
eng = Engine(0)
ctx, dev = eng.ctx, eng.device


def orders_text():
    ords = dg.orders(M, 10_000_000, 100_000)
    names = ["cust_id", "prod_id", "qty"]
    cols = [ords[n].to_device(dev) for n in names]
    arr, keep = (N.cph_strcol * 3)(), []
    for i, c in enumerate(cols):
        arr[i], k = c.as_c()
        keep.append(k)
    hv, hk = (N.cph_strval * 3)(), []
    for i, h in enumerate(names):
        b = (C.c_uint8 * len(h)).from_buffer_copy(h.encode())
        hk.append(b)
        hv[i].data, hv[i].len = C.cast(b, C.c_void_p).value, len(h)
    out = C.POINTER(N.cph_bytes)()
    ctx._check(ctx.lib.cph_csv_write(ctx.handle, arr, 3, hv, N.CPH_MEM_DEVICE, C.byref(out)))
    return int(out.contents.data), int(out.contents.size), M + 1, out


def quoted_text():
    """ddddddd,ddddddd,ddd\\n or ddddddd,"ddddd",ddd\\n: 20 bytes per record, strictly valid."""
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.randint(48, 58, (M, 20), dtype=torch.uint8, device="cuda", generator=g)
    t[:, 7] = t[:, 15] = 44
    t[:, 19] = 10
    q = torch.rand(M, device="cuda", generator=g) < 0.3
    t[q, 8] = 34
    t[q, 14] = 34
    t = t.reshape(-1)
    return t.data_ptr(), t.numel(), M, t


def measure(label, ptr, size, nrec, skip):
    calls = {"strict": lambda: ingest.csv_parse(ctx, None, [0, 1, 2], fields_per_record=3, skip_records=skip, out_mem=N.CPH_MEM_DEVICE,
                                                device_ptr=ptr, size=size),
             "lazy": lambda: ingest.csv_parse_lazy(ctx, None, [0, 1, 2], fields_per_record=3, skip_records=skip, out_mem=N.CPH_MEM_DEVICE,
                                                   device_ptr=ptr, size=size)}
    for fn in calls.values():   # warm: code objects, pool
        for _ in range(2):
            fn().release()
    ev, wall, split = {k: [] for k in calls}, {k: [] for k in calls}, {k: {} for k in calls}
    ctx.profile(True)
    for _ in range(REPS):
        for k, fn in calls.items():
            ctx.profile_read(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            assert r.error_kind == 0 and r.nrecords == nrec - skip, (k, r.error_kind, r.error_record, r.nrecords)
            r.release()
            p = ctx.profile_read(reset=True)
            ev[k].append(sum(v["total_ms"] for v in p.values()))
            for name, v in p.items():
                split[k].setdefault(name, []).append(v["total_ms"])
    ctx.profile(False)
    print(f"== {label}: {size / 1e9:.3f} GB, {nrec} records, medians of {REPS} warm calls, strict and lazy alternating")
    for k in calls:
        med = statistics.median(ev[k])
        print(f"  {k:6s} kernels {med:7.3f} ms (min {min(ev[k]):.3f} max {max(ev[k]):.3f})  {size / med / 1e6:7.1f} GB/s   wall {statistics.median(wall[k]):7.3f} ms")
    print(f"  lazy / strict (kernel time) = {statistics.median(ev['lazy']) / statistics.median(ev['strict']):.3f}")
    for k in calls:
        print(f"  -- {k}: per kernel, median ms")
        for name, v in sorted(split[k].items(), key=lambda kv: -statistics.median(kv[1])):
            print(f"     {name:28s} {statistics.median(v):7.3f}")
    sys.stdout.flush()


ptr, size, nrec, keep_a = orders_text()
measure("(a) orders file, no quotes", ptr, size, nrec, 1)
del keep_a
ptr, size, nrec, keep_b = quoted_text()
measure("(b)+(c) 10 % of the fields quoted", ptr, size, nrec, 0)
