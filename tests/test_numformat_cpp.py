"""Runs tests/cpp/test_numformat: the Map kernels' fixed-precision float formatter (csvplus_amd/csrc/numformat_device.hpp)
compiled for the host by g++ and compared with glibc's exact "%.*f" — every prec 0..22 on the edge table and on more than a
million random bit patterns below 2^128, the reported length against the bytes produced, the values it refuses.  CPU only."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_numformat"


def test_device_formatter_on_the_host_against_glibc():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_numformat"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"(\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 1_000_000
