"""Runs the C++ facade's named-resolver tests (tests/cpp/test_resolve.cpp): Index::ResolveDuplicates(KeepFirst() / KeepMaxInt("id")
/ DropDuplicates() / ...) in the shape of the reference's TestResolver (csvplus_test.go:695-752) against the callback overload,
the conversion error's message (csvplus.go:176 / :198) and the missing-column fallback, over csvplus_amd/host/csvplus.hpp
(cph_index_resolve)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_resolve"


def test_resolve_binary_builds():
    """CPU: the Resolver overload compiles and links against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_resolve"])
    assert BIN.exists()


@pytest.mark.gpu
def test_named_resolvers_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_resolve"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 of 4 resolve tests failed" in r.stdout
    for name in ("TestNamedResolvers", "TestTailRule", "TestConversionError", "TestMissingColumnFallback"):
        assert f"PASS {name}" in r.stdout
