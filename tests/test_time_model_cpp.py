"""Runs tests/cpp/test_timeparse: the RFC 3339 routines of csvplus_amd/csrc/timeparse_device.hpp (the code k_num_parse and
the Map kernels run per value) compiled for the host by g++ — days from the civil date and back over every day of years
0000..9999 against a running counter, the formatter and the parser against gmtime_r / timegm and each other, the
classification table of the header, one wrong byte at a time over the 25-byte form.  CPU only."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_timeparse"


def test_device_time_routines_on_the_host():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_timeparse"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert "test_timeparse: OK" in r.stdout
