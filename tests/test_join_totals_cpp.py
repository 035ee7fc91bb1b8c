"""Runs the C++ facade's join totals tests (tests/cpp/test_join_totals.cpp): Join(...).Join(...).TotalsBy(step, {SumInt("qty"),
SumFloat(AsFloat64(Col("price")) * Float64(AsInt(Col("qty")))), ...}) in the shape of the reference's TestTransformedSource
(csvplus_test.go:754-806) against a std::map group-by computed in the program, the missing-column and conversion errors and
the edges, over csvplus_amd/host/csvplus.hpp (cph_chain_aggregate)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_join_totals"


def test_join_totals_binary_builds():
    """CPU: DataSource::TotalsBy compiles and links against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_join_totals"])
    assert BIN.exists()


@pytest.mark.gpu
def test_join_totals_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_join_totals"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 2 join totals tests failed" in r.stdout
    for name in ("TestAmountPerCustomer", "TestErrorsAndEdges"):
        assert f"PASS {name}" in r.stdout
