"""Runs the C++ facade's OrderBy tests (tests/cpp/test_order.cpp): DataSource::OrderBy({Desc(IntKey("qty")), ...}) with Top / Drop
behind it over the people / orders fixtures against std::stable_sort, the missing-column error and the conversion error's
message (csvplus.go:176 / :198), over csvplus_amd/host/csvplus.hpp (cph_order_rows)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_order"


def test_order_binary_builds():
    """CPU: DataSource::OrderBy compiles and links against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_order"])
    assert BIN.exists()


@pytest.mark.gpu
def test_order_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_order"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 4 order tests failed" in r.stdout
    for name in ("TestTopFiveByQty", "TestMixedThreeKeys", "TestMissingColumn", "TestConversionError"):
        assert f"PASS {name}" in r.stdout
