"""cph_csv_parse_lazy (Reader.LazyQuotes) on the device against the line model of Go's readRecord (tests/lazy_csv_model.py):
records, error kind and error record, on known answers, arbitrary and well-formed random text, with every automaton state
carried across every boundary of the separator scan (chunk, wave, round, tile, scan step), and end to end through read_csv."""
from __future__ import annotations

import hashlib
import io

import numpy as np
import pytest

from oracle import orc
from tests import lazy_csv_model as M
from tests.golden.go_csv_lazy_cases import LAZY_CASES
from tests.golden.go_csv_reader_cases import CASES
from tests.helpers import spliced as _spliced

pytestmark = pytest.mark.gpu

WIDTH = 6
TILE = 16384                # csv_ingest.hip: kCsvTile
SCAN_STEP_TILES = 1024      # csv_ingest.hip: kLazyScanStep, the tiles one step of k_csv_lazy_tile_entry takes


def _pad(recs, width):
    return [r[:width] + [b""] * (width - len(r)) for r in recs]


def model_records(text, opts, width=WIDTH, skip=0):
    recs, ek, er, _ = M.read_all(text, lazy=True, comma=opts.get("comma", b","), comment=opts.get("comment"),
                                 trim=opts.get("trim", False), fpr=opts.get("fpr", 0))
    return _pad(recs, width)[skip:], ek, er if ek else 0


def gpu_records(ctx, text, opts, width=WIDTH, skip=0):
    from csvplus_amd import ingest
    t = ingest.csv_parse_lazy(ctx, text, list(range(width)), comma=opts.get("comma", b","), comment=opts.get("comment"),
                              trim_leading_space=opts.get("trim", False), fields_per_record=opts.get("fpr", 0), skip_records=skip)
    cols = [t.columns[c].values() for c in range(width)]
    return [[cols[c][r] for c in range(width)] for r in range(t.nrecords)], t.error_kind, t.error_record if t.error_kind else 0


# ---- 1. known answers -------------------------------------------------------------------------------------------------
_KNOWN = list(LAZY_CASES) + [c for c in CASES if c[4] is None]


@pytest.mark.parametrize("case", _KNOWN, ids=[("lazy-" if i < len(LAZY_CASES) else "strict-") + c[0] for i, c in enumerate(_KNOWN)])
def test_known_answers(ctx, case):
    _, text, opts, want, err = case
    got, ek, er = gpu_records(ctx, text, opts)
    assert got == _pad(want, WIDTH)
    assert (ek, er) == (err if err else (0, 0))


# ---- 2. random text -----------------------------------------------------------------------------------------------------
def _gen_wellformed(rng, nrec, nfields, alphabet, crlf=False, quote_prob=0.3):
    recs, out = [], io.BytesIO()
    for _ in range(nrec):
        rec = []
        for f in range(nfields):
            ln = int(rng.integers(0, 7))
            rec.append(bytes(alphabet[rng.integers(0, len(alphabet), ln)]))
        if nfields == 1 and rec[0] == b"":
            rec[0] = b"x"   # a lone empty field is an empty line (skipped)
        recs.append(rec)
        parts = []
        for v in rec:
            needs = any(ch in v for ch in b',"\n\r') or v[:1] in (b" ", b"#") or rng.random() < quote_prob
            parts.append(b'"' + v.replace(b'"', b'""') + b'"' if needs else v)
        out.write(b",".join(parts) + (b"\r\n" if crlf else b"\n"))
    return recs, out.getvalue()


def test_random_arbitrary_text_matches_the_model(ctx):
    """Arbitrary, not well-formed text.  The first four option sets run with FieldsPerRecord < 0 (with 0 nearly every such text
    ends at its second record); the fifth is FieldsPerRecord = 0."""
    rng = np.random.default_rng(211)
    alphabet = np.frombuffer(b'ab ,"\n\r#\t', dtype=np.uint8)
    sets = ({"fpr": -1}, {"fpr": -1, "trim": True}, {"fpr": -1, "comment": b"#"}, {"fpr": -1, "comment": b"#", "trim": True}, {"fpr": 0})
    nerr = 0
    for it in range(320):
        text = alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 4001)))].tobytes()
        opts, skip = sets[it % 5], int(rng.integers(0, 3))
        want = model_records(text, opts, skip=skip)
        nerr += want[1] != 0
        assert gpu_records(ctx, text, opts, skip=skip) == want, (it, opts, skip, text[:200])
    assert nerr > 30   # the field count errors of the fifth set


def test_random_wellformed_text_matches_model_and_oracle(ctx):
    rng = np.random.default_rng(223)
    alphabet = np.frombuffer(b'ab ,"\n\rz#\t', dtype=np.uint8)
    for it in range(40):
        nf = int(rng.integers(1, 6))
        nrec = int(rng.integers(0, 4000 if it % 10 == 0 else 60))
        _, text = _gen_wellformed(rng, nrec, nf, alphabet, crlf=bool(it & 1))
        for opts in ({"fpr": -1}, {"fpr": 0, "trim": True}, {"fpr": nf, "comment": b"#"}):
            skip = int(rng.integers(0, 3))
            got = gpu_records(ctx, text, opts, skip=skip)
            assert got == model_records(text, opts, skip=skip), (it, opts)
            cols, ek, er = orc.csv_parse(text, list(range(WIDTH)), comment=opts.get("comment"), trim_leading_space=opts.get("trim", False),
                                         fields_per_record=opts["fpr"], skip_records=skip)
            assert got == ([[cols[c].value(r) for c in range(WIDTH)] for r in range(cols[0].nrows)], ek, er if ek else 0), (it, opts)


# ---- 3. every state carried across every boundary of the scan -----------------------------------------------------------
# (bytes in front of the boundary, bytes behind it, the state in front of the first byte behind it)
_HAZARDS = {
    "FS_quote_opens": (b"k,", b'"x\ny",z\n', M.FS),
    "UQ_quote_is_a_byte": (b"k,a", b'"b,"c\nq,r\n', M.UQ),
    "QD_newline_is_content": (b'k,"x', b'\ny",z\n', M.QD),
    "QS_crlf_ends_record": (b'k,"x"', b"\r\nq,r\n", M.QS),
    "QC_newline_ends_record": (b'k,"x"\r', b"\nq,r\n", M.QC),
    "QC_quote_stays_quoted": (b'k,"x"\r', b'"y",z\n', M.QC),
    "QS_quote_is_escaped": (b'k,"x"', b'"y",z\n', M.QS),
    "QS_comma_ends_field": (b'k,"x"', b",z\n", M.QS),
    "QS_letter_stays_quoted": (b'k,"x"', b'y\nw",z\n', M.QS),
    "CM_quote_in_comment": (b'#c "', b'd" e\nq,r\n', M.CM),
}
_BOUNDARIES = [b + d for b in (16, 1024, 4096, TILE, 2 * TILE) for d in (0, 1)]


@pytest.mark.parametrize("name", list(_HAZARDS))
def test_state_carried_across_scan_boundaries(ctx, name):
    pre, post, state = _HAZARDS[name]
    opts = {"fpr": -1, "comment": b"#"}
    for boundary in _BOUNDARIES:
        text = _spliced(pre, post, boundary)
        assert M.automaton_trace(text, comment=b"#")[boundary] == state
        assert gpu_records(ctx, text, opts, width=4) == model_records(text, opts, width=4), (name, boundary)


# ---- 4. whole tiles inside one field ------------------------------------------------------------------------------------
def test_whole_tiles_inside_one_quoted_field(ctx):
    piece = b'line\nq"uote"\rxy, '   # a newline, a lone quote in front of a letter, a quote + '\r' in front of a letter; 17 bytes: it drifts through the chunks
    bodies = [(piece * 5000)[:size] + b"z" for size in (40 * 1024, 70 * 1024)]
    plain = lambda tag, n: b"".join(b"%s%04d,abc,xyz\n" % (tag, i) for i in range(n))   # noqa: E731
    text = plain(b"a", 700) + b'id7,"' + bodies[0] + b'",end\n' + plain(b"b", 300) + b'id8,"' + bodies[1] + b'",end\r\n' + plain(b"c", 50)
    want = ([[b"a%04d" % i, b"abc", b"xyz"] for i in range(700)] + [[b"id7", bodies[0], b"end"]] +
            [[b"b%04d" % i, b"abc", b"xyz"] for i in range(300)] + [[b"id8", bodies[1], b"end"]] +
            [[b"c%04d" % i, b"abc", b"xyz"] for i in range(50)])
    tr = M.automaton_trace(text)
    first = len(plain(b"a", 700))
    inside = [t for t in range(first // TILE + 1, (first + 40 * 1024) // TILE)]
    assert len(inside) >= 2 and all(tr[t * TILE] in (M.QD, M.QS, M.QC) for t in inside)   # tiles entered inside the field
    assert model_records(text, {"fpr": 3}, width=3) == (want, 0, 0)
    assert gpu_records(ctx, text, {"fpr": 3}, width=3) == (want, 0, 0)


# ---- 5. more tiles than one step of the tile-map scan takes ---------------------------------------------------------------
def test_more_tiles_than_one_scan_step(ctx):
    from csvplus_amd import ingest
    block = (b'1,plain,x\n2,5" nail,y\r\n3,"He said "hi" there",z\n4,"multi\nline",w\n5,"a""b",v\r\n6,a""b,"u"\n'
             b'7,"q"\r"r",t\n8,,"open"x\ny"\n')
    recs, ek, _, _ = M.read_all(block, lazy=True, fpr=3)
    assert ek == 0 and len(recs) == 8 and M.automaton_trace(block)[-1] == M.RS
    big = b'9,"' + (b'big\n"x"\ry, ' * 9000)[:100 * 1024] + b'z",end\n'
    big_rec = M.read_all(big, lazy=True, fpr=3)[0]
    assert len(big_rec) == 1
    n1 = (SCAN_STEP_TILES * TILE // 2) // len(block)
    n2 = (SCAN_STEP_TILES * TILE + 3 * TILE) // len(block) - n1
    text = block * n1 + big + block * n2
    assert SCAN_STEP_TILES * TILE < len(text) <= 32 << 20     # two steps of the scan
    t = ingest.csv_parse_lazy(ctx, text, [0, 1, 2], fields_per_record=3)
    assert (t.error_kind, t.nrecords) == (0, 8 * (n1 + n2) + 1)
    for c in range(3):
        bvals = [r[c] for r in recs]
        want_data = b"".join(bvals) * n1 + big_rec[0][c] + b"".join(bvals) * n2
        lens = np.concatenate([np.tile([len(v) for v in bvals], n1), [len(big_rec[0][c])], np.tile([len(v) for v in bvals], n2)])
        offs = np.asarray(t.columns[c].offsets).astype(np.int64)
        assert np.array_equal(np.diff(offs), lens)
        got = np.asarray(t.columns[c].data).tobytes()
        assert hashlib.sha256(got).digest() == hashlib.sha256(want_data).digest()


# ---- 6. device-resident input, device output, 64-bit offsets ------------------------------------------------------------
def _gen_lazy(rng, nrec):
    forms = [b"plain", b'5" nail', b'"He said "hi" there"', b'"multi\nline"', b'"esc""aped"', b'a""b', b"", b'"x"\r"y"', b' "sp"']
    return b"".join(b",".join(forms[int(i)] for i in rng.integers(0, len(forms), 3)) + (b"\r\n" if rng.random() < 0.5 else b"\n")
                    for _ in range(nrec))


def test_device_resident_text_and_output_with_64bit_offsets(ctx, monkeypatch):
    import torch
    from csvplus_amd import ingest, materialize
    from csvplus_amd import _native as N
    monkeypatch.setenv("CPH_CSV_OFFSETS64", "1")
    rng = np.random.default_rng(227)
    _, well = _gen_wellformed(rng, 3000, 3, np.frombuffer(b'ab ,"\n\rz', dtype=np.uint8), crlf=True)
    for text in (well, _gen_lazy(rng, 3000)):
        dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        t = ingest.csv_parse_lazy(ctx, None, [2, 0], fields_per_record=3, skip_records=1, out_mem=N.CPH_MEM_DEVICE,
                                  device_ptr=dev.data_ptr(), size=len(text))
        recs, ek, _, _ = M.read_all(text, lazy=True, fpr=3)
        assert ek == 0 and (t.error_kind, t.nrecords) == (0, len(recs) - 1) and t.columns[0].offset_bits == 64
        for k, c in enumerate((2, 0)):
            assert list(materialize.gather_rows(ctx, t.columns[k]).values()) == [r[c] for r in recs[1:]]
        t.release()
    cols, ek, _ = orc.csv_parse(well, [0, 1, 2], fields_per_record=3)
    assert ek == 0 and [[cols[c].value(r) for c in range(3)] for r in range(cols[0].nrows)] == M.read_all(well, lazy=True, fpr=3)[0]


# ---- 7. a text without quotes: the same result as strict -----------------------------------------------------------------
def test_text_without_quotes_equals_strict(ctx):
    from csvplus_amd import ingest
    text = b"id,name,qty\n" + b"".join(b"%d,n%d,%d\n" % (i, i % 97, i % 13) for i in range(20_000))

    def run(fn):
        ctx.profile(True)
        ctx.profile_read(reset=True)
        t = fn(ctx, text, [0, 1, 2], skip_records=1)
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert (t.error_kind, t.nrecords) == (0, 20_000)
        return [(np.asarray(c.data).tobytes(), np.asarray(c.offsets).tobytes()) for c in t.columns], prof
    try:
        for fast in (1, 0):
            ctx.set_option("csv_fast", fast)
            lazy, lprof = run(ingest.csv_parse_lazy)
            strict, sprof = run(ingest.csv_parse)
            assert lazy == strict
            assert ("k_csv_fast_copy" in lprof) == bool(fast) and ("k_csv_lazy_marks" in lprof) == (not fast), sorted(lprof)
            assert "k_csv_lazy_marks" not in sprof
    finally:
        ctx.set_option("csv_fast", 1)


# ---- 8. the one limit: TrimLeadingSpace, a non-ASCII space in front of an opening quote ----------------------------------
def test_non_ascii_space_in_front_of_a_quote_is_refused(ctx):
    from csvplus_amd import _native as N
    opts = {"trim": True, "fpr": -1}
    with pytest.raises(N.CphError) as e:
        gpu_records(ctx, b'x,\xc2\xa0"a",y\n', opts)
    assert e.value.code == N.CPH_ERR_INVALID and "non-ASCII Unicode space in front of an opening quote" in str(e.value)
    with pytest.raises(N.CphError):   # the earliest occurrence is seen also behind thousands of records
        gpu_records(ctx, b"a,b,c\n" * 5000 + b'x, \xe2\x80\x83 "a\nb",y\n' + b"a,b,c\n" * 50, opts)
    for text in (b"x,\xc2\xa0a,y\n", b'x, "a",y\n', b'x,\xc2\xa0a"b,y\n'):
        assert gpu_records(ctx, text, opts) == model_records(text, opts)
    assert gpu_records(ctx, b'x, "a",y\n', opts)[0] == [[b"x", b"a", b"y", b"", b"", b""]]


# ---- 9. read_csv(lazy_quotes=True) end to end ----------------------------------------------------------------------------
def test_read_csv_lazy_header_modes_and_pipeline(ctx):
    from csvplus_amd import StrCol, ingest, pipeline
    from csvplus_amd.predicates import Like
    rows = [(b"%d" % i, b'%d" nail' % (i % 7), b"%d" % (i % 5)) for i in range(200)]
    body = b"".join(b",".join(r) + b"\n" for r in rows)
    text = b'id,"na"me",qty\n' + body
    t = ingest.read_csv(ctx, text, lazy_quotes=True)
    assert t.names == [b"id", b'na"me', b"qty"] and (t.nrecords, t.error_kind) == (200, 0)
    assert t.columns[1].values() == [r[1] for r in rows]
    t = ingest.read_csv(ctx, text, select=['na"me', "id"], lazy_quotes=True)
    assert t.columns[t.names.index(b'na"me')].values() == [r[1] for r in rows]
    t = ingest.read_csv(ctx, text, expect_header={'na"me': 1, "qty": -1}, lazy_quotes=True)
    assert t.columns[t.names.index(b"qty")].values() == [r[2] for r in rows]
    with pytest.raises(KeyError):
        ingest.read_csv(ctx, text, expect_header={'na"me': 2}, lazy_quotes=True)
    t = ingest.read_csv(ctx, body, assume_header={"id": 0, "name": 1}, lazy_quotes=True)
    assert t.nrecords == 200 and t.columns[t.names.index(b"name")].values() == [r[1] for r in rows]
    # NumFields: the mismatch is reported at its record, the rows before it are delivered
    t = ingest.read_csv(ctx, text + b'1,2" x\n' + body, lazy_quotes=True)
    assert (t.error_kind, t.error_record, t.nrecords) == (3, 201, 200)
    t = ingest.read_csv(ctx, text, num_fields=3, lazy_quotes=True)
    assert (t.error_kind, t.nrecords) == (0, 200)
    # Filter(Like) | ToCsv over a lazily read table
    ptext = b"id,name,qty\n" + body
    tab = pipeline.read_table(ctx, ptext, lazy_quotes=True)
    try:
        got = pipeline.filter_to_csv(ctx, tab, Like(qty="3"), ["id", "name"])
    finally:
        tab.release()
    mrecs = M.read_all(ptext, lazy=True)[0][1:]
    kept = [r for r in mrecs if r[2] == b"3"]
    assert len(kept) == 40
    assert got == orc.csv_write([StrCol.from_values([r[0] for r in kept]), StrCol.from_values([r[1] for r in kept])], ["id", "name"])


# ---- 10. the contract of the two entry points ----------------------------------------------------------------------------
def test_lazy_entry_point_requires_lazy_quotes(ctx):
    from csvplus_amd import ingest
    from csvplus_amd import _native as N
    with pytest.raises(N.CphError) as e:
        ingest.csv_parse(ctx, b"a,b\n", [0], lazy_quotes=False, _entry="lazy")
    assert e.value.code == N.CPH_ERR_INVALID
    with pytest.raises(N.CphError) as e:   # cph_csv_parse keeps refusing it
        ingest.csv_parse(ctx, b"a,b\n", [0], lazy_quotes=True)
    assert e.value.code == N.CPH_ERR_INVALID
    assert gpu_records(ctx, b"", {}) == ([], 0, 0)
