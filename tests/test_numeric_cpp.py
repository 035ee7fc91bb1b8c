"""Runs the C++ facade's typed-value tests (tests/cpp/test_numeric.cpp): Filter(IntCmp("born", GT, 1970)) — the reference's
flagship filter (csvplus_test.go:272-281) —, DataSource::ColumnAsInt / ColumnAsFloat64 and the error of
TestNumericalConversions (:911-958), against csvplus_amd/host/csvplus.hpp (cph_filter_rows, cph_col_to_number)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_numeric"


def test_numeric_binary_builds():
    """CPU: IntCmp / FloatCmp / ColumnAsInt compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_numeric"])
    assert BIN.exists()


@pytest.mark.gpu
def test_typed_values_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_numeric"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 3 numeric tests failed" in r.stdout
    for name in ("TestFilterIntCmp", "TestColumnAsNumber", "TestConversionError"):
        assert f"PASS {name}" in r.stdout
