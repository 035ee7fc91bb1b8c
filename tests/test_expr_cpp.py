"""Runs the C++ facade's expression tests (tests/cpp/test_expr.cpp): the reference's amounts table and TestSimpleTotals as one
chain each — Map(Set("amount", Fixed(AsFloat64(Col("price")) * Float64(AsInt(Col("qty"))), 2))) and Totals with SumFloat of the
same product — against Expr::eval and a host loop, and a zero divisor or a value that does not parse ending the iteration at
its row (csvplus_amd/host/csvplus.hpp: cph_num_eval feeding cph_map_format and cph_index_aggregate)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_expr"


@pytest.mark.gpu
def test_expressions_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_expr"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 4 expr tests failed" in r.stdout
    for name in ("TestExprHostModel", "TestAmountsTable", "TestSimpleTotalsExpr", "TestExprErrors"):
        assert f"PASS {name}" in r.stdout
