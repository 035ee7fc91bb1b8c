"""The shortest float formatter of csvplus_amd/csrc/shortfmt_device.hpp on the host (CPU only).

  * tests/cpp/test_shortfmt: the header compiled by g++; digits, exponent and the 'e' text against std::to_chars, the other
    layouts against Go's rules written over std::string, the length function against the bytes put, for every power of two with
    its neighbours, the subnormal binades, the powers of ten, integers, short decimals and 1e5 seeded random bit patterns per
    class; the per-format maximum lengths reached and never exceeded;
  * the same stand-alone program under the address and undefined-behaviour sanitizers, with a tenth of the random values."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_shortfmt"
SAN = ROOT / "oracle" / "_build" / "shortfmt_asan"


def _run(target, exe, *args):
    subprocess.check_call(["make", "-C", str(ROOT), target], stdout=subprocess.DEVNULL)
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "test_shortfmt: OK" in r.stdout and "FAIL" not in r.stdout
    return r.stdout


def _classes(out):
    return {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^(.+?)\s+(\d+) values$", out, re.M)}


def test_shortest_digits_against_to_chars_on_the_host():
    out = _run("tests/cpp/test_shortfmt", BIN)
    got = _classes(out)
    assert got["powers of two and neighbours"] >= 2 * 3 * 2098 - 8
    assert got["powers of ten and neighbours"] >= 2 * 3 * 632 - 8
    assert got["subnormal binades"] >= 52 * 2000
    for name in ("integers", "short decimals k / 10^j", "random finite bit patterns", "random subnormals", "random values of 2^-30 .. 2^60",
                 "random values near 1e-300"):
        assert got[name] >= 100000, (name, got[name])
    assert "longest: 'e' 24 (constant 24), 'f' 327 (constant 327), 'g' 24 (constant 24)" in out


def test_shortest_digits_under_the_sanitizers():
    out = _run("oracle/_build/shortfmt_asan", SAN, "10")   # every power of two and of ten, a tenth of the random values
    assert _classes(out)["powers of two and neighbours"] >= 2 * 3 * 2098 - 8
