"""Runs tests/cpp/test_orderkey: OrderBy's value maps (csvplus_amd/csrc/order_device.hpp) compiled for the host by g++ and
compared with Go's cmp.Compare on int64 / float64 — every pair of the edge values (INT64_MIN..INT64_MAX; +-0, denormals,
+-DBL_MIN, +-DBL_MAX, +-Inf, NaNs of several payloads and signs), ascending and descending, and more than a million random
bit patterns.  CPU only."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_orderkey"


def test_order_key_maps_on_the_host_against_cmp_compare():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_orderkey"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"(\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 1_000_000
