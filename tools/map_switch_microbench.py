"""k_map_copy against k_switch_copy on rows of the people shape: cph_map_format over Format(name, " ", surname) and cph_map_switch over
a When whose predicate holds for half the rows and whose two alternatives are that same template (profiles/map_switch.txt).
Device events of cph_ctx_profile, the two entry points alternating.  Usage: map_switch_microbench.py [rows [reps]]; needs a GPU."""
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from csvplus_amd import Context, StrCol, _native as N   # noqa: E402
from csvplus_amd import predicates as P   # noqa: E402
from csvplus_amd.mapping import Col, Format, When   # noqa: E402
from csvplus_amd.materialize import map_column, map_switch   # noqa: E402
from helpers import PEOPLE_NAMES, PEOPLE_SURNAMES   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
rng = np.random.default_rng(1)


def column(words):
    idx = rng.integers(0, len(words), n)
    lens = np.array([len(w) for w in words], dtype=np.uint64)[idx]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = np.frombuffer(b"".join(map([w.encode() for w in words].__getitem__, idx.tolist())), dtype=np.uint8).copy()
    return StrCol(data, offs, n, 64), idx


name, name_idx = column(PEOPLE_NAMES)
surname, _ = column(PEOPLE_SURNAMES)
ctx = Context(0)
cols = {"name": name.to_device(), "surname": surname.to_device()}
tmpl = Format(Col("name"), " ", Col("surname"))
half = P.Any(*[P.Like(name=w) for w in PEOPLE_NAMES[:5]])
sw = When(half, tmpl, tmpl)
share = float((name_idx < 5).mean())


def fmt():
    cb = map_column(ctx, cols, tmpl, out_mem=N.CPH_MEM_DEVICE)
    nb = cb.nbytes
    cb.release()
    return nb


def switch():
    cb, _ = map_switch(ctx, cols, sw, out_mem=N.CPH_MEM_DEVICE)
    nb = cb.nbytes
    cb.release()
    return nb


assert fmt() == switch()   # warm-up, and the same bytes
ctx.profile(True)
ctx.profile_read()
res = {}
for _ in range(reps):
    for fn in (fmt, switch):
        fn()
        for k, v in ctx.profile_read().items():
            res.setdefault(k, []).append((v["total_ms"], v["algo_bytes"], v["launches"]))
ctx.profile(False)
lines = [f"rows {n}, reps {reps} (alternating), predicate holds for {share:.3f} of the rows; median [min .. max] of the device-event times"]
med = {}
for k in sorted(res):
    ms = [x[0] for x in res[k]]
    med[k] = statistics.median(ms)
    gb = res[k][0][1] / 1e9
    lines.append(f"{k:16s} {med[k]:8.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]  launches/call {res[k][0][2]}  model {gb:.4f} GB"
                 + (f"  {gb / med[k] * 1e3:7.1f} GB/s" if gb else ""))
lines.append(f"k_switch_copy / k_map_copy = {med['k_switch_copy'] / med['k_map_copy']:.3f}")
lines.append(f"k_switch_lens / k_map_lens = {med['k_switch_lens'] / med['k_map_lens']:.3f}")
print("\n".join(lines))
