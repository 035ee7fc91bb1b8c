"""Runs the C++ facade's string-condition tests (tests/cpp/test_strpred_facade.cpp): StrCmp / HasPrefix / HasSuffix / Contains
as Filter, TakeWhile / DropWhile and Switch conditions and Substr as a Map part, over the people / orders fixtures with an
RFC3339 `ts` column, against csvplus_amd/host/csvplus.hpp (cph_filter_rows ops 32..37 / 40..42, CPH_MAP_SLICE)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_strpred_facade"
TESTS = ("TestFilters", "TestMissingColumn", "TestWhile", "TestSubstr", "TestSwitchAndTotalsPerDay")


def test_strpred_facade_binary_builds():
    """CPU: the facade's string predicates and Substr compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_strpred_facade"])
    assert BIN.exists()


def test_strpred_facade_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_strpred_facade"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "no usable GPU" in r.stdout + r.stderr


@pytest.mark.gpu
def test_string_conditions_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_strpred_facade"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert f"0 of {len(TESTS)} string predicate tests failed" in r.stdout
    for name in TESTS:
        assert f"PASS {name}" in r.stdout
