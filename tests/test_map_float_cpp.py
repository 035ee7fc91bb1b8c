"""Runs the C++ facade's Fixed tests (tests/cpp/test_map_float.cpp): Map(Set("price", Fixed(Col("price"), 2))) over the stock
rows and over joined rows against Format::render, and a value that does not parse ending the iteration with
ValueAsFloat64's error at its row (csvplus_amd/host/csvplus.hpp: cph_col_to_number, then a FLOAT64 piece of cph_map_format)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_map_float"


@pytest.mark.gpu
def test_fixed_parts_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_map_float"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 3 map-float tests failed" in r.stdout
    for name in ("TestFixedHostModel", "TestMapFixed", "TestMapFixedErrors"):
        assert f"PASS {name}" in r.stdout
