"""Runs the C++ facade's tests of the conditions that compare two expressions or two columns (tests/cpp/test_expr_cond.cpp):
ExprCmp and ColCmp as Filter, TakeWhile / DropWhile, Validate and Switch conditions — `price * float64(qty) >= 100`, `qty > 0 &&
price * float64(qty) == amount`, `ship != bill`, the gold / silver tiers — against the facade's own host evaluation
(csvplus_amd/host/csvplus.hpp: cph_filter_rows ops 56..61 and 72..77, cph_map_switch)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_expr_cond"


@pytest.mark.gpu
def test_expression_conditions_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_expr_cond"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 5 expression condition tests failed" in r.stdout
    for name in ("TestHostModel", "TestFilters", "TestMissingColumn", "TestWhileAndValidate", "TestSwitchTiers"):
        assert f"PASS {name}" in r.stdout
