"""Runs the C++ facade's Totals tests (tests/cpp/test_totals.cpp): Index::Totals({SumInt("qty"), MaxFloat("price"), ...}) over the
people / orders fixtures in the shape of the reference's TestSimpleTotals (csvplus_test.go:516-571) against a std::map
group-by, the missing-column error and the conversion error's message (csvplus.go:176 / :198), over
csvplus_amd/host/csvplus.hpp (cph_index_aggregate)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_totals"


def test_totals_binary_builds():
    """CPU: Index::Totals compiles and links against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_totals"])
    assert BIN.exists()


@pytest.mark.gpu
def test_totals_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_totals"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 4 totals tests failed" in r.stdout
    for name in ("TestCountPerName", "TestSumPerCustomer", "TestMissingColumn", "TestConversionError"):
        assert f"PASS {name}" in r.stdout
