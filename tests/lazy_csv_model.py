"""Go's encoding/csv Reader.readRecord restated line by line, with LazyQuotes — the expectation of the device's lazy CSV
reader (cph_csv_parse_lazy) — and, as a second function, the seven-state byte automaton the device finds record
separators with (csvplus_amd/csrc/csv_lazy_device.hpp).

encoding/csv is not part of the reference tree and Go is not run by these tests: the model restates the stdlib's rules.  Its
strict mode is tied to the pinned oracle (orc.csv_parse) and to tests/golden/go_csv_reader_cases.py by tests/test_csv_lazy.py;
its lazy mode equals its strict mode wherever strict reports no error, and is pinned by tests/golden/go_csv_lazy_cases.py.
"""
from __future__ import annotations

BARE, QUOTE, FIELDS = 1, 2, 3

_GO_SPACES = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | set(
    range(0x2000, 0x200B))


def _trim_left(line: bytes) -> bytes:
    """bytes.TrimLeftFunc(line, unicode.IsSpace) on UTF-8 (an invalid byte is RuneError: no space)."""
    i, n = 0, len(line)
    while i < n:
        b0 = line[i]
        if b0 < 0x80:
            cp, w = b0, 1
        else:
            w = 2 if b0 >> 5 == 0b110 else 3 if b0 >> 4 == 0b1110 else 4 if b0 >> 3 == 0b11110 else 0
            try:
                cp = ord(line[i:i + w].decode("utf-8")) if w else -1
            except UnicodeDecodeError:
                cp = -1
        if cp not in _GO_SPACES:
            break
        i += w
    return line[i:]


def _nl(line: bytes) -> int:
    return 1 if line.endswith(b"\n") else 0


def read_all(text: bytes, *, lazy=False, comma=b",", comment=None, trim=False, fpr=0):
    """Reader.ReadAll the way csvplus consumes it: (records, error_kind, error_record, starts).  records = the records in
    front of the first error (lists of bytes), error_kind 0 or BARE / QUOTE / FIELDS with the 0-based index of the record it
    happened in, starts[r] = offset of the line record r begins with."""
    n, pos = len(text), 0
    sep = comma[0]
    cmt = comment[0] if comment else None

    def read_line():
        nonlocal pos
        if pos >= n:
            return None
        end = text.find(b"\n", pos)
        if end < 0:
            line, pos = text[pos:], n
            if line.endswith(b"\r"):
                line = line[:-1]                    # a "\r" in front of EOF is dropped
        else:
            line, pos = text[pos:end + 1], end + 1
            if line.endswith(b"\r\n"):
                line = line[:-2] + b"\n"
        return line

    records, starts = [], []
    expected = fpr
    while True:
        # ---- readRecord: skip comment and empty lines
        while True:
            start = pos
            line = read_line()
            if line is None:
                return records, 0, 0, starts
            if cmt is not None and line[:1] and line[0] == cmt:
                continue
            if len(line) == _nl(line):
                continue
            break
        fields, err = [], 0
        while True:                                   # parseField
            if trim:
                line = _trim_left(line)
            if not line or line[0] != 0x22:           # unquoted field
                i = line.find(comma)
                field = line[:i] if i >= 0 else line[:len(line) - _nl(line)]
                if not lazy and b'"' in field:
                    err = BARE
                    break
                fields.append(field)
                if i >= 0:
                    line = line[i + 1:]
                    continue
                break
            line = line[1:]                           # quoted field
            buf = bytearray()
            done = False
            while True:
                i = line.find(b'"')
                if i >= 0:
                    buf += line[:i]
                    line = line[i + 1:]
                    if line[:1] == b'"':              # "" -> one quote
                        buf += b'"'
                        line = line[1:]
                    elif line[:1] and line[0] == sep:  # the field ends
                        line = line[1:]
                        fields.append(bytes(buf))
                        break
                    elif len(line) == _nl(line):      # the field and the record end
                        fields.append(bytes(buf))
                        done = True
                        break
                    elif lazy:                        # a literal quote, the field stays quoted
                        buf += b'"'
                    else:
                        err = QUOTE
                        break
                elif line:                            # the field continues on the next line
                    buf += line
                    line = read_line() or b""
                else:                                 # EOF inside the quotes
                    if not lazy:
                        err = QUOTE
                        break
                    fields.append(bytes(buf))
                    done = True
                    break
            if err or done:
                break
        if err:
            return records, err, len(records), starts
        if expected > 0:
            if len(fields) != expected:
                return records, FIELDS, len(records), starts
        elif expected == 0:
            expected = len(fields)
        records.append(fields)
        starts.append(start)


# ---- the byte automaton -----------------------------------------------------------------------------------------------
RS, FS, UQ, QD, QS, QC, CM = range(7)
STATE_NAMES = ["RS", "FS", "UQ", "QD", "QS", "QC", "CM"]
_ASCII_SPACES = frozenset(b" \t\v\f")


def automaton_step(state: int, c: int, sep: int, cmt, trim: bool) -> int:
    """One byte.  Class precedence: newline, quote, Comma, '\\r', comment character, space."""
    if c == 0x0A:
        return QD if state == QD else RS
    if state in (RS, FS):
        if c == 0x22:
            return QD
        if c == sep:
            return FS
        if c == 0x0D or c in _ASCII_SPACES:
            return FS if trim else UQ
        if state == RS and cmt is not None and c == cmt:
            return CM
        return UQ
    if state == UQ:
        return FS if c == sep else UQ
    if state == QD:
        return QS if c == 0x22 else QD
    if state == QS:
        if c == 0x22:
            return QD
        if c == sep:
            return FS
        if c == 0x0D:
            return QC
        return QD
    if state == QC:
        return QS if c == 0x22 else QD
    return CM


def automaton_trace(text: bytes, *, comma=b",", comment=None, trim=False):
    """The state in front of every byte, and behind the last one: len(text) + 1 entries, RS first."""
    sep, cmt = comma[0], (comment[0] if comment else None)
    out = [RS]
    s = RS
    for c in text:
        s = automaton_step(s, c, sep, cmt, trim)
        out.append(s)
    return out


def automaton_record_starts(text: bytes, *, comma=b",", comment=None, trim=False):
    """Record starts as the device derives them: a '\\n' is a separator iff the state in front of it is not QD; a segment
    between separators that is empty (a '\\r' in front of its end dropped) or begins with the comment character is no
    record."""
    tr = automaton_trace(text, comma=comma, comment=comment, trim=trim)
    cmt = comment[0] if comment else None
    starts, b = [], 0
    bounds = [i for i, c in enumerate(text) if c == 0x0A and tr[i] != QD] + [len(text)]
    for e in bounds:
        end = e - 1 if e > b and text[e - 1] == 0x0D else e
        if end > b and not (cmt is not None and text[b] == cmt):
            starts.append(b)
        b = e + 1
    return starts
