"""Runs the C++ facade's span tests (tests/cpp/test_span_facade.cpp): TrimSpace / TrimLeft / TrimRight / Trim / TrimPrefix /
TrimSuffix / Field / Before / After as Map parts, nested with Substr, inside Switch alternatives and over a Join, against
csvplus_amd/host/csvplus.hpp (CPH_MAP_SPAN) and its host row model, which runs csrc/span_device.hpp on the host."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_span_facade"
TESTS = ("TestHostModel", "TestForms", "TestNested", "TestSwitch", "TestOverAJoin")


def test_span_facade_binary_builds():
    """CPU: the facade's span forms compile and link against the C ABI (g++, no GPU needed)."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_span_facade"])
    assert BIN.exists()


def test_span_facade_host_model_passes_and_the_rest_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_span_facade"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "PASS TestHostModel" in r.stdout            # the host row model needs no device
    assert "no usable GPU" in r.stdout + r.stderr


@pytest.mark.gpu
def test_spans_through_cpp_facade():
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_span_facade"])
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    assert f"0 of {len(TESTS)} span tests failed" in r.stdout
    for name in TESTS:
        assert f"PASS {name}" in r.stdout
