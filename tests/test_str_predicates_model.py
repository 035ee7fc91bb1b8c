"""The string conditions and the Slice part as plain data (no GPU): `compile` emits the ABI's op codes and piece kind,
`matches` / `run_ops` / `render` agree with Python's bytes operations — the exact model of Go's strings.Compare, HasPrefix,
HasSuffix, Contains and s[a:b], which are byte operations."""
import pytest

from csvplus_amd import mapping as M
from csvplus_amd import predicates as P

RELS = {"<": lambda a, b: a < b, "<=": lambda a, b: a <= b, "==": lambda a, b: a == b, "!=": lambda a, b: a != b,
        ">=": lambda a, b: a >= b, ">": lambda a, b: a > b}

# (value, literal): ties on the common prefix, the sign bit, empties, a literal longer than the value
PAIRS = [
    (b"a", b"a\0"), (b"a\0", b"a"), (b"a", b"a"),
    (b"\x7f", b"\x80"), (b"\x80", b"\x7f"), (b"\xff", b"\x00"),
    (b"10", b"9"), (b"9", b"10"),
    (b"", b""), (b"", b"a"), (b"a", b""), (b"\0", b""),
    (b"abc", b"abcd"), (b"abcd", b"abc"), (b"abcd", b"bcd"), (b"abcd", b"bc"), (b"abcd", b"abd"),
    (b"2016-09-14T08:48:22+01:00", b"2016-09"), (b"2016-09-14T08:48:22+01:00", b"+01:00"), (b"2016-08-31T23:59:59+01:00", b"2016-09"),
    (b"aaaaaaaaaaaaaaaaaaaaaaaaa", b"aaaaaaaab"), (b"aaaaaaaaaaaaaaaaaaaaaaaab", b"aaaaaaaab"),
    (b"Smithson", b"Smith"), (b"Goldsmith", b"Smith"), (b"xxSmithxx", b"Smith"),
]


def all_nine(column, literal):
    """(predicate, op code, oracle on a present value) for each of the nine ops"""
    out = [(P.StrCmp(column, rel, literal), 32 + k, (lambda v, f=RELS[rel]: f(v, literal))) for k, rel in enumerate(P.RELS)]
    out.append((P.HasPrefix(column, literal), 40, lambda v: v.startswith(literal)))
    out.append((P.HasSuffix(column, literal), 41, lambda v: v.endswith(literal)))
    out.append((P.Contains(column, literal), 42, lambda v: literal in v))
    return out


def test_op_codes():
    assert (P.STR_LT, P.HAS_PREFIX, P.HAS_SUFFIX, P.CONTAINS) == (32, 40, 41, 42)
    assert P.RELS == ("<", "<=", "==", "!=", ">=", ">")
    for pred, code, _ in all_nine("ts", b"2016"):
        names, ops = P.compile(pred, ["id", "ts"])
        assert names == ["ts"] and ops == [(code, 0, b"2016")]
        names, ops = P.compile(pred, ["id"])
        assert names == [] and ops == [(code, -1, b"2016")]
    names, ops = P.compile(P.All(P.StrCmp("ts", ">=", "2016-09"), P.Not(P.HasPrefix("ts", "2016-09-14")), P.Contains("name", "x")), ["name", "ts"])
    assert names == ["ts", "name"]
    assert ops == [(36, 0, b"2016-09"), (40, 0, b"2016-09-14"), (P.NOT, 0, None), (42, 1, b"x"), (P.ALL, 3, None)]


@pytest.mark.parametrize("value,literal", PAIRS)
def test_matches_agrees_with_bytes(value, literal):
    for pred, _, oracle in all_nine("c", literal):
        want = oracle(value)
        assert P.matches(pred, {"c": value}) is want, (pred, value)
        assert P.matches(pred, {b"c": value}) is want
        names, ops = P.compile(pred, ["c"])
        assert P.run_ops(ops, [value]) is want
        assert P.matches(P.Not(pred), {"c": value}) is (not want)


def test_the_table_has_both_outcomes_for_every_op():
    for k in range(9):
        seen = {all_nine("c", lit)[k][2](val) for val, lit in PAIRS}
        assert seen == {True, False}, k


def test_missing_column_is_false_under_all_nine():
    for literal in (b"", b"a"):
        for pred, code, _ in all_nine("gone", literal):
            assert P.matches(pred, {"c": b"a"}) is False, pred
            names, ops = P.compile(pred, ["c"])
            assert ops == [(code, -1, literal)] and P.run_ops(ops, []) is False


def test_str_and_bytes_literals_and_repr():
    assert P.StrCmp("c", "<", "é").literal == "é".encode("utf-8")
    assert P.matches(P.HasPrefix("c", "é"), {"c": "één"})
    assert repr(P.StrCmp("ts", ">=", b"2016")) == "StrCmp('ts', '>=', b'2016')"
    assert repr(P.HasPrefix("ts", b"x")) == "HasPrefix('ts', b'x')"
    assert repr(P.HasSuffix("ts", b"x")) == "HasSuffix('ts', b'x')"
    assert repr(P.Contains("ts", b"x")) == "Contains('ts', b'x')"
    with pytest.raises(ValueError):
        P.StrCmp("c", "=~", b"x")
    with pytest.raises(TypeError, match="StrCmp / HasPrefix / HasSuffix / Contains"):
        P.All(lambda row: True)


def test_term_limit_counts_the_new_terms():
    terms = [P.HasPrefix("c", b"x")] * 16 + [P.StrCmp("c", "<", b"y")] * 16
    P.compile(P.Any(*terms), ["c"])
    with pytest.raises(ValueError, match="more than 32"):
        P.compile(P.Any(P.Any(*terms), P.Contains("c", b"z")), ["c"])


# ---- Slice ----------------------------------------------------------------------------------------------------------------

VALUES = [b"", b"a", b"2016-09-14T08:48:22+01:00", b"\x00\xff\x80", b"abcdefgh", b"abcdefghi"]
ENDS = [None, 0, 1, 3, 8, 9, 10, 24, 25, 26, 1000, -1, -3, -6, -25, -26, -1000, M.INT64_MAX, M.INT64_MIN]


def test_slice_compiles_to_piece_kind_8():
    assert M.SLICE == 8
    names, pieces = M.compile(M.Format("d=", M.Col("ts")[0:10], M.Col("ts")[-6:], M.Col("id")), ["id", "ts"])
    assert names == ["ts", "id"]
    assert pieces == [(M.LITERAL, 0, b"d="), (M.SLICE, 0, (0, 10)), (M.SLICE, 0, (-6, M.INT64_MAX)), (M.COLUMN, 1, None)]
    assert M.columns(M.Format(M.Col("ts")[:4], M.Col("ts"))) == ["ts"]
    assert repr(M.Col("ts")[:10]) == "Col('ts')[:10]" and repr(M.Col("ts")[-6:]) == "Col('ts')[-6:]"


def test_slice_table_against_bytes_slicing():
    for v in VALUES:
        for a in ENDS:
            for b in ENDS:
                part = M.Col("c")[a:b]
                lo = None if a is None else a
                hi = None if b is None or b == M.INT64_MAX else b
                assert M.render(part, {"c": v}) == v[lo:hi], (v, a, b)
                assert M.render(M.Format("<", part, ">"), {b"c": v}) == b"<" + v[lo:hi] + b">"


def test_slice_of_a_default_is_cut_on_the_host():
    part = M.Col("gone", default=b"2016-09-14")[5:7]
    assert M.compile(M.Format("m", part), ["c"]) == ([], [(M.LITERAL, 0, b"m09")])
    assert M.render(part, {"c": b"x"}) == b"09"
    with pytest.raises(M.MissingColumn):
        M.compile(M.Col("gone")[1:2], ["c"])
    with pytest.raises(M.MissingColumn):
        M.render(M.Col("gone")[1:2], {"c": b"x"})


def test_only_plain_slices():
    for key in (3, slice(0, 10, 2), slice(0, 10, 1), "a", slice("a", None), slice(None, 1.5), slice(1 << 63, None)):
        with pytest.raises(TypeError):
            M.Col("c")[key]


def test_switch_shares_columns_with_slices_and_string_conditions():
    sw = M.When(P.HasPrefix("ts", "2016-09"), M.Col("ts")[:10], M.Format(M.Col("id"), "/", M.Col("ts")[11:19]))
    names, cases, otherwise = M.compile_switch(sw, ["id", "ts"])
    assert names == ["ts", "id"]
    assert cases == [([(40, 0, b"2016-09")], [(M.SLICE, 0, (0, 10))])]
    assert otherwise == [(M.COLUMN, 1, None), (M.LITERAL, 0, b"/"), (M.SLICE, 0, (11, 19))]
    assert M.columns(sw) == ["ts", "id"]
    row = {"id": b"7", "ts": b"2016-09-14T08:48:22+01:00"}
    assert M.render(sw, row) == b"2016-09-14" and M.which_of(sw, row) == 0
    row["ts"] = b"2016-10-01T00:00:01+01:00"
    assert M.render(sw, row) == b"7/00:00:01" and M.which_of(sw, row) == 1
