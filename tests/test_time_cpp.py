"""Runs the C++ facade's time tests (tests/cpp/test_time.cpp): DataSource::ColumnAsTime / ColumnAsTimeNano, Filter(TimeCmp(...))
and Map(Set(..., Rfc3339(...))) over a dozen rows whose stamps mix zone offsets, against csvplus_amd/host/csvplus.hpp
(cph_col_to_number, cph_filter_rows, cph_map_format / cph_map_switch)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_time"


def test_time_binary_builds():
    """CPU: TimeCmp / ColumnAsTime / Rfc3339 compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_time"])
    assert BIN.exists()


@pytest.mark.gpu
def test_time_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_time"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 3 time tests failed" in r.stdout
    for name in ("TestColumnAsTime", "TestFilterTimeCmp", "TestMapRfc3339"):
        assert f"PASS {name}" in r.stdout
