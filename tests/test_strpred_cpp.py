"""Runs tests/cpp/test_strpred: the string conditions' per-value routines (csvplus_amd/csrc/strpred_device.hpp, the code
k_pred_eval runs) compiled for the host by g++ and compared with std::string's compare / find, every length 0..26 at every
start alignment, with every touched word checked against load_value_chunk's contract.  CPU only."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_strpred"


def test_device_string_routines_on_the_host_against_std_string():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_strpred"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 250_000
