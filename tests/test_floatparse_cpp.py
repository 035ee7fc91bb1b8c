"""The Eisel-Lemire float conversion of csvplus_amd/csrc/floatparse_device.hpp on the host (CPU only).

  * tests/cpp/test_floatparse: the header compiled by g++, every decided value bit for bit against glibc's strtod (1e5 seeded
    values per class, a literal list; no undecided value where no digit was dropped, at most 1 % where some were);
  * the same stand-alone program under the address and undefined-behaviour sanitizers;
  * csvplus_amd/csrc/pow5_table.inc entry by entry against the formulas of the table, recomputed here."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tests" / "cpp" / "test_floatparse"
SAN = ROOT / "oracle" / "_build" / "floatparse_asan"
TABLE = ROOT / "csvplus_amd" / "csrc" / "pow5_table.inc"


def _run(target, exe):
    subprocess.check_call(["make", "-C", str(ROOT), target], stdout=subprocess.DEVNULL)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "test_floatparse: OK" in r.stdout
    return r.stdout


def _classes(out):
    got = {}
    for m in re.finditer(r"^(.+?)\s+(\d+) values,\s+(\d+) undecided \([\d.]+ %\), (\d+) wrong$", out, re.M):
        got[m.group(1).strip()] = tuple(int(m.group(k)) for k in (2, 3, 4))
    return got


def test_eisel_lemire_against_strtod_on_the_host():
    got = _classes(_run("tests/cpp/test_floatparse", BIN))
    assert set(got) == {"%.17g of random doubles", "subnormals", "19-digit mantissas", "truncated, 25 digits", "truncated, 40 digits", "literals"}
    for name, (n, undecided, wrong) in got.items():
        assert wrong == 0, name
        assert n >= (100000 if name != "literals" else 12), (name, n)
        if name.startswith("truncated"):
            assert undecided * 100 <= n, (name, undecided, n)
        else:
            assert undecided == 0, (name, undecided)


def test_eisel_lemire_under_the_sanitizers():
    out = _run("oracle/_build/floatparse_asan", SAN)
    assert all(wrong == 0 for _, _, wrong in _classes(out).values())


def test_pow5_table_entry_by_entry():
    """The committed table against the formulas, restated: 5^q scaled into [2^127, 2^128) and truncated for q >= 0; for q < 0,
    with z the smallest integer with 2^z >= 5^-q, 2^(z+127) // 5^-q + 1 down to q = -27 and 2^(2z+128) // 5^-q + 1, halved
    until it is below 2^128, beyond."""
    pairs = re.findall(r"^\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\},$", TABLE.read_text(), re.M)
    assert len(pairs) == 651
    body = [ln for ln in TABLE.read_text().splitlines() if ln and not ln.startswith("//")]
    assert len(body) == 651   # nothing but entries and comments
    for q, (hi, lo) in zip(range(-342, 309), pairs):
        have = (int(hi, 16) << 64) | int(lo, 16)
        if q >= 0:
            p = 5 ** q
            want = p << (128 - p.bit_length()) if p.bit_length() <= 128 else p >> (p.bit_length() - 128)
        else:
            p = 5 ** -q
            z = 0
            while (1 << z) < p:
                z += 1
            if q >= -27:
                want = (1 << (z + 127)) // p + 1
            else:
                want = (1 << (2 * z + 128)) // p + 1
                while want >= 1 << 128:
                    want >>= 1
        assert have == want, q
        assert 1 << 127 <= have < 1 << 128, q
