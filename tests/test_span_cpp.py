"""Runs tests/cpp/test_span: the span operations of a CPH_MAP_SPAN piece (csvplus_amd/csrc/span_device.hpp, the code the
Map kernels run per value) compiled for the host by g++ and compared with a per-byte reference written from Go's definitions:
every byte string up to length 6 over a space alphabet, value lengths around the 8-byte chunk at every start alignment,
separators of 1, 2, 8 and 9 bytes at every position, with every touched word checked against load_value_chunk's contract.
CPU only."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_span"


def test_device_span_routines_on_the_host_against_go_definitions():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_span"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 2_500_000
