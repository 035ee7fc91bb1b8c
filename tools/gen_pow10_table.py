#!/usr/bin/env python3
"""Writes csvplus_amd/csrc/pow10_table.inc: the 128-bit powers of ten of the shortest float formatter (shortfmt_device.hpp,
Schubfach), one {hi, lo} pair per decimal exponent e = -292..324, from exact Python integers.

  g(e) = ceil(10^e * 2^(127 - floor(log2(10^e))))      in [2^127, 2^128)

that is 10^e scaled by a power of two into [2^127, 2^128) and rounded UP where it is not exact (exact for 0 <= e <= 55).
Schubfach needs an over-estimate of at most one unit; the Eisel-Lemire table (pow5_table.inc) truncates for q >= 0 and is
therefore a different table.

tests/test_map_shortest.py recomputes every entry from this formula and compares it with the committed file.

    python tools/gen_pow10_table.py            # rewrites the file
    python tools/gen_pow10_table.py --check    # exit status 1 when the committed file differs
"""
import sys
from pathlib import Path

EMIN, EMAX = -292, 324
OUT = Path(__file__).resolve().parent.parent / "csvplus_amd" / "csrc" / "pow10_table.inc"


def entry(e):
    """The 128-bit table value of 10^e."""
    if e >= 0:
        p = 10 ** e
        b = p.bit_length()
        c = p << (128 - b) if b <= 128 else -((-p) >> (b - 128))   # ceil
    else:
        p = 10 ** -e
        b = p.bit_length()                       # 2^(b-1) <= p < 2^b, and p is no power of two
        c = -((-(1 << (127 + b))) // p)          # ceil(2^(127+b) / p): 2^127 < . < 2^128
    assert 1 << 127 <= c < 1 << 128, e
    return c


def render():
    lines = ["// pow10_table.inc — written by tools/gen_pow10_table.py, not by hand: {hi, lo} of the 128-bit power of ten, rounded",
             "// up, for e = %d..%d, one entry per line (shortfmt_device.hpp indexes it with e + %d)." % (EMIN, EMAX, -EMIN)]
    for e in range(EMIN, EMAX + 1):
        c = entry(e)
        lines.append("{0x%016xull, 0x%016xull}," % (c >> 64, c & ((1 << 64) - 1)))
    return "\n".join(lines) + "\n"


def main(argv):
    text = render()
    if "--check" in argv:
        same = OUT.exists() and OUT.read_text() == text
        print("%s: %s" % (OUT.name, "up to date" if same else "DIFFERS from the generator"))
        return 0 if same else 1
    OUT.write_text(text)
    print("wrote %s (%d entries)" % (OUT, EMAX - EMIN + 1))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
