"""The Span part as plain data (no GPU): Span.apply — the host model of a CPH_MAP_SPAN piece — against independent
formulations (bytes.split / strip, a byte-at-a-time TrimSpace over Go's utf8 decoding rules written here, Go's documented
results by hand), exhaustively over a small alphabet that holds pieces of the space sequences; then `compile` and `render`
for Span parts, for defaults over a missing column, and the piece and operation limits."""
import itertools

import pytest

from csvplus_amd import mapping as M
from csvplus_amd.mapping import Col, Format, Span, Switch
from csvplus_amd import predicates as P

X = Col("x")


# ---- an independent TrimSpace: utf8.DecodeRune / DecodeLastRune and unicode.IsSpace, a byte at a time -----------------------

SPACES = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | set(range(0x2000, 0x200B))


def decode_rune(p: bytes):
    """(rune, size) as utf8.DecodeRune: an invalid or short encoding is (0xFFFD, 1)."""
    b0 = p[0]
    if b0 < 0x80:
        return b0, 1
    if 0xC2 <= b0 <= 0xDF:
        need, lo, hi, v = 2, 0x80, 0xBF, b0 & 0x1F
    elif 0xE0 <= b0 <= 0xEF:
        need, lo, hi, v = 3, 0xA0 if b0 == 0xE0 else 0x80, 0x9F if b0 == 0xED else 0xBF, b0 & 0x0F
    elif 0xF0 <= b0 <= 0xF4:
        need, lo, hi, v = 4, 0x90 if b0 == 0xF0 else 0x80, 0x8F if b0 == 0xF4 else 0xBF, b0 & 0x07
    else:
        return 0xFFFD, 1
    if len(p) < need:
        return 0xFFFD, 1
    for k in range(1, need):
        c = p[k]
        if not ((lo if k == 1 else 0x80) <= c <= (hi if k == 1 else 0xBF)):
            return 0xFFFD, 1
        v = (v << 6) | (c & 0x3F)
    return v, need


def decode_last_rune(p: bytes):
    end = len(p)
    start = end - 1
    if p[start] < 0x80:
        return p[start], 1
    lim = max(end - 4, 0)
    start -= 1
    while start >= lim:
        if p[start] & 0xC0 != 0x80:
            break
        start -= 1
    start = max(start, lim)
    r, size = decode_rune(p[start:end])
    return (r, size) if start + size == end else (0xFFFD, 1)


def go_trim_left(s: bytes) -> bytes:
    while s:
        r, n = decode_rune(s)
        if r not in SPACES:
            break
        s = s[n:]
    return s


def go_trim_right(s: bytes) -> bytes:
    i = len(s)
    while i > 0:   # strings.lastIndexFunc(s, unicode.IsSpace, false)
        r, n = decode_last_rune(s[:i])
        i -= n
        if r not in SPACES:
            return s[:i + (decode_rune(s[i:])[1] if s[i] >= 0x80 else 1)]
    return b""


def test_trim_space_exhaustively_over_a_space_alphabet():
    """Every byte string of length <= 5 over {20, 61, 2C, C2, 85, E2, 80}, the three modes."""
    count = 0
    for n in range(6):
        for t in itertools.product(b"\x20\x61\x2c\xc2\x85\xe2\x80", repeat=n):
            v = bytes(t)
            assert X.trim_left_space().apply(v) == go_trim_left(v), v
            assert X.trim_right_space().apply(v) == go_trim_right(v), v
            assert X.trim_space().apply(v) == go_trim_right(go_trim_left(v)), v
            count += 1
    assert count == sum(7 ** n for n in range(6))


def test_trim_space_all_25_sequences_and_the_tail_cases():
    assert len(M.SPACE_SEQUENCES) == 25 and {decode_rune(s)[0] for s in M.SPACE_SEQUENCES} == SPACES
    for s in M.SPACE_SEQUENCES:
        assert decode_rune(s) == (decode_rune(s)[0], len(s))
        assert X.trim_space().apply(s + b"a" + s) == b"a"
        assert X.trim_left_space().apply(s + b"a" + s) == b"a" + s
        assert X.trim_right_space().apply(s + b"a" + s) == s + b"a"
    assert X.trim_space().apply(b" \t\n Hello, Gophers \n\t\r\n") == b"Hello, Gophers"
    assert X.trim_right_space().apply(b"\xe2\x80\x80\x80") == b"\xe2\x80\x80\x80"      # the sequence does not END the value
    assert X.trim_right_space().apply(b"\xe2\xc2\x85") == b"\xe2"
    assert X.trim_space().apply(b"a\x85") == b"a\x85" and X.trim_space().apply(b"\x80") == b"\x80"   # lone continuation bytes
    assert X.trim_space().apply(b"".join(M.SPACE_SEQUENCES)) == b""                   # all spaces
    assert X.trim_space().apply(b"") == b""
    # not Python's idea of a space: \x1c..\x1f are str.isspace() / bytes.strip() material only in part, never Go's
    assert X.trim_space().apply(b"\x1c a \x1f") == b"\x1c a \x1f"


def test_cutset_trims_against_bytes_strip():
    values = [b"", b"xx", b"--a--", b"-+-a+b-+", b"a", b"+", b"\xc2\x85-a-\xc2\x85", b" a ", b"-\x00-"]
    for cutset in (b"", b"-", b"-+", b"+-\x00", bytes(range(32, 64))):
        for v in values:
            # bytes.strip(b"") would strip whitespace: the empty cutset changes nothing
            assert X.trim(cutset).apply(v) == (v.strip(cutset) if cutset else v)
            assert X.trim_left(cutset).apply(v) == (v.lstrip(cutset) if cutset else v)
            assert X.trim_right(cutset).apply(v) == (v.rstrip(cutset) if cutset else v)
    with pytest.raises(ValueError, match="0x80"):
        X.trim(b"\xc2\xa0")
    with pytest.raises(ValueError, match="more than 32"):
        X.trim(bytes(range(33)))
    assert X.trim(bytes(range(32))).ops[0][4] == bytes(range(32))


def test_field_against_bytes_split():
    values = [b"", b",", b"a", b"a,b", b"a,b,c,d", b",a,,b,", b",,,,", b"aaa", b"aaaa", b"a man a plan a canal panama", b"ab,ab"]
    for sep in (b",", b"aa", b"a ", b"ab,"):
        for v in values:
            for limit in (-1, 1, 2, 3, 4):
                parts = v.split(sep) if limit < 0 else v.split(sep, limit - 1)
                for k in range(-4, 5):
                    want = parts[k] if -len(parts) <= k < len(parts) else b""
                    assert X.field(sep, k, limit).apply(v) == want, (v, sep, k, limit)


def test_go_documented_results():
    split = lambda v, sep, n=-1: [X.field(sep, k, n).apply(v) for k in range(len(v.split(sep) if n < 0 else v.split(sep, n - 1)))]   # noqa: E731
    assert split(b"a,b,c,d", b",", 2) == [b"a", b"b,c,d"]
    assert split(b"a man a plan a canal panama", b"a ") == [b"", b"man ", b"plan ", b"canal panama"]
    assert split(b"", b"x") == [b""]
    assert split(b"aaa", b"aa") == [b"", b"a"]
    hello = "¡¡¡Hello".encode()
    assert X.trim_prefix(hello).apply(hello) == b""
    assert X.trim_prefix("¡¡¡").apply(hello) == b"Hello"
    assert X.trim_prefix(b"Hello").apply(hello) == hello            # only at the head
    assert X.trim_suffix(b"absent").apply(b"value") == b"value"    # an absent literal: the identity
    assert X.trim_suffix(b".go").apply(b"main.go.go") == b"main.go"  # once
    assert X.trim_prefix(b"").apply(b"a") == b"a" and X.trim_suffix(b"").apply(b"") == b""
    # strings.Cut's documented cases: (before, after); found is `sep in s`
    for s, sep, before, after in [(b"Gopher", b"Go", b"", b"pher"), (b"Gopher", b"ph", b"Go", b"er"), (b"Gopher", b"er", b"Goph", b""),
                                  (b"Gopher", b"Badger", b"Gopher", b"")]:
        assert (X.before(sep).apply(s), X.after(sep).apply(s)) == (before, after)
    assert X.before(b"@").apply(b"ann@example.com") == b"ann" and X.after(b"@").apply(b"ann@b@c") == b"b@c"
    with pytest.raises(ValueError, match="empty separator"):
        X.field(b"", 0)
    for limit in (0, -2):
        with pytest.raises(ValueError, match="limit"):
            X.field(b",", 0, limit)
    with pytest.raises(ValueError, match="more than 255"):
        X.trim_prefix(b"x" * 256)
    assert X.field(b"s" * 255, 0).ops[0][4] == b"s" * 255


def test_programs_chain_and_slice():
    p = X.trim_space().trim_prefix(b"id:").field(b";", -1)[:8]
    assert isinstance(p, Span) and len(p.ops) == 4 and p.name == "x"
    assert p.apply(b"  id:a;b;0123456789  ") == b"01234567"
    assert X.trim_space()[:10].apply(b"  2016-09-14T10:00:00Z ") == b"2016-09-14"
    assert X.trim_space()[-3:].apply(b" abcdef ") == b"def" and X.trim_space()[4:2].apply(b" abcdef ") == b""
    assert X.trim_space()[1:-1][1:-1].apply(b" abcdef ") == b"cd"
    assert isinstance(X[0:10], M.Slice) and not isinstance(X[0:10], Span)   # Col[a:b] stays a Slice
    assert X.trim_space().ops == ((M.SPAN_TRIM_SPACE, 3, 0, 0, b""),) and X.trim_left_space().ops[0][1] == 1 and X.trim_right_space().ops[0][1] == 2
    assert X.before(b"@").ops == ((M.SPAN_FIELD, 2, 0, 0, b"@"),) and X.after(b"@").ops == ((M.SPAN_FIELD, 2, 1, 0, b"@"),)
    with pytest.raises(ValueError, match="1..4 operations"):
        p.trim_space()
    with pytest.raises(TypeError):
        X.trim_space()[::2]
    with pytest.raises(TypeError):
        X.trim_space()[0]
    assert "trim_space()" in repr(p) and "field" in repr(p)


def test_compile_and_render_span_parts():
    t = Format("<", X.trim_space(), "|", Col("y").field(b"-", 1), "|", X[1:3], X.trim(b"_")[:2], ">")
    names, pieces = M.compile(t, ["y", "x", "z"])
    assert names == ["x", "y"]
    assert [p[0] for p in pieces] == [M.LITERAL, M.SPAN, M.LITERAL, M.SPAN, M.LITERAL, M.SLICE, M.SPAN, M.LITERAL]
    assert pieces[1] == (M.SPAN, 0, ((M.SPAN_TRIM_SPACE, 3, 0, 0, b""),))
    assert pieces[3] == (M.SPAN, 1, ((M.SPAN_FIELD, -1, 1, 0, b"-"),))
    assert pieces[6] == (M.SPAN, 0, ((M.SPAN_TRIM_CUTSET, 3, 0, 0, b"_"), (M.SPAN_SLICE, 0, 0, 2, b"")))
    assert M.columns(t) == ["x", "y"]
    assert M.render(t, {"x": b" _ab_ ", "y": b"k-v-w"}) == b"<_ab_|v|_a _>"
    assert M.render(t, {b"x": " _ab_ ", b"y": "k-v-w"}) == b"<_ab_|v|_a _>"
    # a default over a missing column: the program runs on the default and the piece is a literal
    d = Format("[", Col("gone", default=b"  id:7;8 ").trim_space().trim_prefix(b"id:").after(b";"), "]")
    assert M.compile(d, ["x"]) == ([], [(M.LITERAL, 0, b"[8]")])
    assert M.render(d, {"x": b""}) == b"[8]" and M.render(d, {"gone": b"id:1;2"}) == b"[2]"
    with pytest.raises(M.MissingColumn):
        M.compile(Col("gone").trim_space(), ["x"])
    with pytest.raises(M.MissingColumn):
        M.render(Col("gone").trim_space(), {"x": b""})
    # a bare Span is a template, and an alternative of a Switch
    assert M.compile(X.trim_space(), ["x"])[1] == [(M.SPAN, 0, ((M.SPAN_TRIM_SPACE, 3, 0, 0, b""),))]
    sw = Switch((P.HasPrefix("y", b"k"), Col("y").after(b"-")), otherwise=X.trim_space())
    names, cases, otherwise = M.compile_switch(sw, ["x", "y"])
    assert names == ["y", "x"] and cases[0][1][0][:2] == (M.SPAN, 0) and otherwise[0][:2] == (M.SPAN, 1)
    assert M.render(sw, {"x": b" a ", "y": b"k-v"}) == b"v" and M.render(sw, {"x": b" a ", "y": b"q-v"}) == b"a"
    assert M.columns(sw) == ["y", "x"]


def test_piece_and_operation_limits():
    four = X.trim_space().trim_prefix(b"a").trim_suffix(b"b")[1:]
    assert M.compile(Format(four, four, four, four), ["x"])[1][3][0] == M.SPAN          # 16 operations: the limit
    with pytest.raises(ValueError, match="17 span operations"):
        M.compile(Format(four, four, four, four, X.trim_space()), ["x"])
    with pytest.raises(ValueError, match="17 pieces"):
        M.compile(Format(*[p for _ in range(8) for p in (X.trim_space(), "-")], X), ["x"])
    sw = Switch((P.HasPrefix("x", b"a"), Format(four, four)), (P.HasPrefix("x", b"b"), Format(four, four)), otherwise=X.trim_space())
    with pytest.raises(ValueError, match="17 span operations in all"):
        M.compile_switch(sw, ["x"])
    with pytest.raises(TypeError):
        Span("x", ((M.SPAN_TRIM_SPACE, 3, 0, 0, b""),))
    with pytest.raises(TypeError):
        X.field(b",", "0")
