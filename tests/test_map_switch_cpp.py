"""Runs the C++ facade's conditional Map tests (tests/cpp/test_map_switch.cpp): TestLongChain's Map (csvplus_test.go:283-288,
`if row["name"] == "Amelia" { row["name"] = "Julia" }`) as Map(Set("name", When(...))) over joined rows, a multi-case Switch with
IntCmp cases and a Fixed(Expr) part that fails only in rows of the other branch, against csvplus_amd/host/csvplus.hpp
(cph_map_switch)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_map_switch"


def test_map_switch_binary_builds():
    """CPU: Case / Switch / When / Set(name, Switch) compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_map_switch"])
    assert BIN.exists()


@pytest.mark.gpu
def test_map_switch_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_map_switch"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 3 map switch tests failed" in r.stdout
    for name in ("TestLongChainMap", "TestSwitchCases", "TestSwitchFixedExpr"):
        assert f"PASS {name}" in r.stdout
