"""The error report's packing (csvplus_amd/csrc/num_report.hpp) on the host (CPU only): tests/cpp/test_num_report compiles the
header with g++ and round-trips err_pack / err_row / err_tag / err_kind at row 0, 2^32 - 1, 2^32 and 2^48 - 1 with tag and kind
0 and 255, checks that packed words order by (row, tag, kind), and that err_unpack reads a device accumulator as the host
code of the typed-value passes does."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_num_report"


def test_err_pack_round_trip_and_order_on_the_host():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_num_report"], stdout=subprocess.DEVNULL)
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=60)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "125 triples" in r.stdout and "test_num_report: OK" in r.stdout
