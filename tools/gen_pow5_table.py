#!/usr/bin/env python3
"""Writes csvplus_amd/csrc/pow5_table.inc: the 128-bit powers of five of the Eisel-Lemire float conversion
(floatparse_device.hpp), one {hi, lo} pair per decimal exponent q = -342..308, from exact Python integers.

  q >= 0   5^q scaled by a power of two into [2^127, 2^128), truncated
  q <  0   z = the smallest integer with 2^z >= 5^-q;
           q >= -27: c = 2^(z+127) // 5^-q + 1
           q <  -27: c = 2^(2z+128) // 5^-q + 1, halved until c < 2^128

tests/test_floatparse_cpp.py recomputes every entry from these formulas and compares it with the committed file.

    python tools/gen_pow5_table.py            # rewrites the file
    python tools/gen_pow5_table.py --check    # exit status 1 when the committed file differs
"""
import sys
from pathlib import Path

QMIN, QMAX = -342, 308
OUT = Path(__file__).resolve().parent.parent / "csvplus_amd" / "csrc" / "pow5_table.inc"


def entry(q):
    """The 128-bit table value of 10^q's power of five."""
    if q >= 0:
        p = 5 ** q
        b = p.bit_length()
        c = p << (128 - b) if b <= 128 else p >> (b - 128)
    else:
        p = 5 ** -q
        z = (p - 1).bit_length()          # the smallest z with 2^z >= p
        if q >= -27:
            c = (1 << (z + 127)) // p + 1
        else:
            c = (1 << (2 * z + 128)) // p + 1
            while c >= 1 << 128:
                c //= 2
    assert 1 << 127 <= c < 1 << 128, q
    return c


def render():
    lines = ["// pow5_table.inc — written by tools/gen_pow5_table.py, not by hand: {hi, lo} of the 128-bit power of five for",
             "// q = %d..%d, one entry per line (floatparse_device.hpp indexes it with q + %d)." % (QMIN, QMAX, -QMIN)]
    for q in range(QMIN, QMAX + 1):
        c = entry(q)
        lines.append("{0x%016xull, 0x%016xull}," % (c >> 64, c & ((1 << 64) - 1)))
    return "\n".join(lines) + "\n"


def main(argv):
    text = render()
    if "--check" in argv:
        same = OUT.exists() and OUT.read_text() == text
        print("%s: %s" % (OUT.name, "up to date" if same else "DIFFERS from the generator"))
        return 0 if same else 1
    OUT.write_text(text)
    print("wrote %s (%d entries)" % (OUT, QMAX - QMIN + 1))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
