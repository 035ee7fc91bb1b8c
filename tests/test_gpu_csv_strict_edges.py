"""cph_csv_parse (the strict reader of csv_ingest.hip) with every hazard PLACED on an edge of its four code paths, byte-exact
against the line model of Go's readRecord (tests/lazy_csv_model.read_all(lazy=False), tied to the pinned oracle and the Go known
answers by tests/test_csv_lazy.py): records in front of the first error, error kind, error record.

  1. the separator passes (k_csv_tile_stats, k_csv_pick_counts, k_csv_separators): quote parity carried across chunk, wave, round
     and tile boundaries, whole tiles inside one quoted field, the ends of the text
  2. the record-parallel kernels at their LDS stage edge (a 256-record tile of stage_bytes - 1, stage_bytes, stage_bytes + 1 bytes)
  3. k_csv_copy_fields falling back to global destinations where k_csv_fields staged (one field wanted by several columns)
  4. record counts, skipped records (pad, lead, T0, nout == 0) and the first error at a pad-aligned tile edge
  5. more 256-record tiles than the grid has workgroups (the grid-stride loops with their one-tile-ahead prefetch)
  6. the fast path's 20 KiB window edge, the 16 KiB tile seam and a thread's 64-byte chunk edge

Every text builder asserts on the CPU, ahead of the device call, that the byte it places is where it claims: a test cannot pass
by missing its target.  The unmarked tests run the builders and their placement checks against the model only."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

from tests import lazy_csv_model as M
from tests.helpers import spliced

gpu = pytest.mark.gpu

# ---- the host's constants and formulas, mirrored (csv_ingest.hip points back here) --------------------------------------------
TILE = 16384                      # kCsvTile: text bytes per workgroup of the separator passes and of the fast path
REC_TILE = 256                    # kCsvThreads: records per tile of k_csv_fields / k_csv_copy_fields
STAGE_MIN, STAGE_MAX = 8192, 32768   # kCsvStageMin, kCsvStageMax
MAX_KEY_COLS = 16                 # CPH_MAX_KEY_COLS
K_PRE = 4                         # k_csv_copy_fields: kPre, the columns whose lengths and bases are prefetched
GRID_CAP = 8192                   # grid_for_items' cap (cph_internal.hpp)
FT_STAGE = 20480                  # kFtStage: the fast path's staged window per 16 KiB tile


def stage_bytes(size, nrec):
    """The smallest power of two in [8 KiB, 32 KiB] that is >= 1.5 * 256 * size / nrec (csv_parse_any)."""
    s = STAGE_MIN
    while s < STAGE_MAX and s < 1.5 * 256.0 * size / nrec:
        s *= 2
    return s


def pad_of(skip, nrec):
    return (REC_TILE - min(skip, nrec) % REC_TILE) % REC_TILE


def out_cap(stage):
    return stage + 32 * MAX_KEY_COLS


def rounded(span):
    return (span + 31) & ~15


def copy_fits(text_span, col_spans, stage):
    """k_csv_copy_fields' `fits`: the tile's text is staged and every column's bytes find room in the output stage."""
    if text_span > stage:
        return False
    pos = 0
    for span in col_spans:
        if span > out_cap(stage) or pos + rounded(span) > out_cap(stage):
            return False
        pos += rounded(span)
    return True


def tile_span(text, starts, first, last):
    """ge - gb of the tile holding the records first .. last: the first record's start rounded down to 16, up to the last
    record's separator (the newline that ends it)."""
    end = starts[last + 1] - 1 if last + 1 < len(starts) else len(text) - 1
    assert text[end:end + 1] == b"\n"
    return end - (starts[first] & ~15)


# ---- model and device ---------------------------------------------------------------------------------------------------------
def model(text, cols, opts, skip=0):
    recs, ek, er, starts = M.read_all(text, lazy=False, comma=opts.get("comma", b","), comment=opts.get("comment"),
                                      trim=opts.get("trim", False), fpr=opts.get("fpr", 0))
    rows = [[r[c] if c < len(r) else b"" for c in cols] for r in recs]
    return rows[skip:], ek, (er if ek else 0), starts


def device(ctx, text, cols, opts, skip=0):
    """cph_csv_parse.  A text without any quote would take the fast path (k_csv_fast): it is switched off for such a text, so
    that the strict separator passes and the record-parallel kernels run — and the kernels that ran are checked (t.kernels)."""
    from csvplus_amd import ingest
    plain = b'"' not in text
    if plain:
        ctx.set_option("csv_fast", 0)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        t = ingest.csv_parse(ctx, text, cols, comma=opts.get("comma", b","), comment=opts.get("comment"),
                             trim_leading_space=opts.get("trim", False), fields_per_record=opts.get("fpr", 0), skip_records=skip)
        t.kernels = set(ctx.profile_read(reset=True))
    finally:
        ctx.profile(False)
        if plain:
            ctx.set_option("csv_fast", 1)
    assert {"k_csv_tile_stats", "k_csv_separators", "k_csv_fields"} <= t.kernels and "k_csv_fast_copy" not in t.kernels, sorted(t.kernels)
    assert ("k_csv_copy_fields" in t.kernels) == (t.nrecords > 0), sorted(t.kernels)
    return t


def check(ctx, text, cols, opts, skip=0, bits=32, tag=None):
    """Byte-exact: error kind and record, record count, and per column offsets[nout] == len(data), diff(offsets) == the model's
    field lengths, data == the model's values concatenated (together: every value equal)."""
    want, ek, er, _ = model(text, cols, opts, skip)
    t = device(ctx, text, cols, opts, skip)
    assert (t.error_kind, t.error_record if t.error_kind else 0, t.nrecords) == (ek, er, len(want)), tag
    for k in range(len(cols)):
        col = t.columns[k]
        assert col.offset_bits == bits, tag
        offs = np.asarray(col.offsets).astype(np.int64)
        data = np.asarray(col.data).tobytes()
        assert len(offs) == len(want) + 1 and offs[0] == 0 and int(offs[-1]) == len(data), (tag, k)
        lens = np.fromiter((len(r[k]) for r in want), dtype=np.int64, count=len(want))
        if not np.array_equal(np.diff(offs), lens):
            r = int(np.flatnonzero(np.diff(offs) != lens)[0])
            raise AssertionError(f"{tag}: column {k} (field {cols[k]}) record {r + skip}: length {int(offs[r + 1] - offs[r])}, "
                                 f"model {want[r][k]!r}")
        if data != b"".join(r[k] for r in want):
            r = next(i for i in range(len(want)) if data[offs[i]:offs[i + 1]] != want[i][k])
            raise AssertionError(f"{tag}: column {k} (field {cols[k]}) record {r + skip}: {data[offs[r]:offs[r + 1]]!r}, "
                                 f"model {want[r][k]!r}")
    return t


# =================================================================================================================================
# 1. parity carried across every scan boundary
# =================================================================================================================================
# (bytes in front of the boundary, bytes behind it, the records the spliced bytes form)
_HAZARDS = {
    "quote_opens": (b"k,", b'"x\ny",z\n', [[b"k", b"x\ny", b"z"]]),
    "newline_in_quotes_first": (b'k,"x', b'\ny",z\n', [[b"k", b"x\ny", b"z"]]),
    "escaped_quote_split": (b'k,"x"', b'"y",z\n', [[b"k", b'x"y', b"z"]]),
    "closing_quote_then_crlf": (b'k,"x"', b"\r\nq,r\n", [[b"k", b"x"], [b"q", b"r"]]),
    "crlf_split_behind_quote": (b'k,"x"\r', b"\nq,r\n", [[b"k", b"x"], [b"q", b"r"]]),
    "crlf_split_unquoted": (b"k,x\r", b"\nq,r\n", [[b"k", b"x"], [b"q", b"r"]]),
    "crlf_split_in_quotes": (b'k,"x\r', b'\ny",z\n', [[b"k", b"x\ny", b"z"]]),
    "closing_quote_first": (b'k,"x\ny', b'",z\n', [[b"k", b"x\ny", b"z"]]),
    "blank_line": (b"k,v\n", b"\nq,r\n", [[b"k", b"v"], [b"q", b"r"]]),           # the last three: an inner line is dropped,
    "blank_crlf_split": (b"k,v\n\r", b"\nq,r\n", [[b"k", b"v"], [b"q", b"r"]]),   # k_csv_compact runs
    "comment_line": (b"k,v\n", b"#c,d\nq,r\n", [[b"k", b"v"], [b"q", b"r"]]),
}
_ERR_HAZARDS = {
    "bare_quote": (b"k,a", b'"b\nq,r\n', M.BARE),
    "quote_then_letter": (b'k,"x"', b"y,z\n", M.QUOTE),
}
_BOUNDARIES = [b + d for b in (16, 1024, 4096, TILE, 2 * TILE) for d in (0, 1)]   # chunk, wave, round, tile, tile
_OPTS1 = {"fpr": -1, "comment": b"#"}
_COLS1 = [0, 1, 2, 3]


def _placed_hazard(pre, post, boundary):
    """The spliced text, and the index of the record pre + post begins."""
    text = spliced(pre, post, boundary)
    p0 = boundary - len(pre)
    assert 38 * 1024 < len(text) < 42 * 1024
    assert text[p0 - 1:p0] == b"\n" and text[p0:boundary] == pre and text[boundary:boundary + len(post)] == post
    assert text[boundary - 1:boundary + 1] == pre[-1:] + post[:1]
    return text, (p0 - 2) // 15 + 1


def _wellformed_hazard(name, boundary):
    pre, post, want = _HAZARDS[name]
    text, nhead = _placed_hazard(pre, post, boundary)
    recs, ek, _, starts = M.read_all(text, lazy=False, comment=b"#", fpr=-1)
    assert ek == 0 and starts[nhead] == boundary - len(pre) and recs[nhead:nhead + len(want)] == want, (name, boundary)
    assert recs[nhead + len(want)][0] == b"t00000"      # the splice is clean: the tail's records follow
    return text


def _error_hazard(name, boundary):
    pre, post, kind = _ERR_HAZARDS[name]
    text, nhead = _placed_hazard(pre, post, boundary)
    recs, ek, er, _ = M.read_all(text, lazy=False, comment=b"#", fpr=-1)
    assert (ek, er, len(recs)) == (kind, nhead, nhead), (name, boundary)
    return text


def test_section1_builders_place_their_bytes():
    for boundary in _BOUNDARIES:
        for name in _HAZARDS:
            _wellformed_hazard(name, boundary)
        for name in _ERR_HAZARDS:
            _error_hazard(name, boundary)
    _long_field_text()
    assert len(_end_texts()) == 27


@gpu
@pytest.mark.parametrize("name", list(_HAZARDS))
def test_parity_carried_across_scan_boundaries(ctx, name, monkeypatch):
    for boundary in _BOUNDARIES:
        t = check(ctx, _wellformed_hazard(name, boundary), _COLS1, _OPTS1, tag=(name, boundary))
        assert ("k_csv_compact" in t.kernels) == (name in ("blank_line", "blank_crlf_split", "comment_line")), (name, sorted(t.kernels))
    monkeypatch.setenv("CPH_CSV_OFFSETS64", "1")
    for boundary in (TILE, TILE + 1):
        check(ctx, _wellformed_hazard(name, boundary), _COLS1, _OPTS1, bits=64, tag=(name, boundary, 64))


@gpu
@pytest.mark.parametrize("name", list(_ERR_HAZARDS))
def test_first_error_on_a_scan_boundary(ctx, name):
    """Kind, record index and every record in front of it (check compares all three with the model)."""
    for boundary in _BOUNDARIES:
        t = check(ctx, _error_hazard(name, boundary), _COLS1, _OPTS1, tag=(name, boundary))
        assert t.error_kind == _ERR_HAZARDS[name][2]


def _long_field_text():
    """Two quoted fields of ~40 KiB and ~70 KiB whose body holds `""`, "\\r\\n" and "\\n" with a period of 13 bytes (coprime to
    16: it drifts through the chunks), shifted so that a tile lying wholly inside the first field holds an ODD number of quotes
    (a `""` split by its edge): that tile's parity differs at its two ends."""
    piece = b'ab""c\r\nde\nfgh'
    assert len(piece) == 13
    bodies = [piece * (size // 13) for size in (40 * 1024, 70 * 1024)]
    plain = lambda tag, n: b"".join(b"%s%04d,abc,xyz\n" % (tag, i) for i in range(n))   # noqa: E731
    for shift in range(13):
        text = (plain(b"a", 700) + b"s," + b"x" * shift + b",y\n" + b'id7,"' + bodies[0] + b'",end\n' + plain(b"b", 300) +
                b'id8,"' + bodies[1] + b'",end\r\n' + plain(b"c", 50))
        f0 = text.index(b'id7,"') + 5
        whole = list(range(-(-f0 // TILE), (f0 + len(bodies[0])) // TILE))
        odd = [t for t in whole if text[t * TILE:(t + 1) * TILE].count(b'"') & 1]
        if odd:
            break
    assert len(whole) >= 2 and odd and text[f0:f0 + len(bodies[0])] == bodies[0]
    vals = [b.replace(b'""', b'"').replace(b"\r\n", b"\n") for b in bodies]
    want = ([[b"a%04d" % i, b"abc", b"xyz"] for i in range(700)] + [[b"s", b"x" * shift, b"y"], [b"id7", vals[0], b"end"]] +
            [[b"b%04d" % i, b"abc", b"xyz"] for i in range(300)] + [[b"id8", vals[1], b"end"]] +
            [[b"c%04d" % i, b"abc", b"xyz"] for i in range(50)])
    assert model(text, [0, 1, 2], {"fpr": 3})[:3] == (want, 0, 0)
    return text


@gpu
def test_whole_tiles_inside_one_quoted_field(ctx):
    check(ctx, _long_field_text(), [0, 1, 2], {"fpr": 3})


def _sized_text(size, final_nl, quoted):
    """Exactly `size` bytes of records; the last one is padded to the byte, with or without its newline."""
    rec = (lambda i: b'e%05d,"a""b\r\nc",x\n' % i) if quoted else (lambda i: (b"e%05d,abc,xyz\r\n" if i % 3 == 0 else b"e%05d,abc,xyz\n") % i)
    parts, n, i = [], 0, 0
    while n + 64 < size:
        parts.append(rec(i))
        n += len(parts[-1])
        i += 1
    text = b"".join(parts) + b"k," + b"x" * (size - n - 2 - int(final_nl)) + (b"\n" if final_nl else b"")
    assert len(text) == size and (text[-1:] == b"\n") == final_nl
    return text


def _end_texts():
    """(tag, text, error kind)"""
    out = []
    for quoted in (True, False):
        for final_nl in (True, False):
            for size in (4096, 4097, 4111, TILE, 2 * TILE):
                text = _sized_text(size, final_nl, quoted)
                assert len(text) % 16 == {4096: 0, 4097: 1, 4111: 15, TILE: 0, 2 * TILE: 0}[size]
                out.append((("size", size, final_nl, quoted), text, 0))
            text = _sized_text(5000, final_nl, quoted) + b"\r"           # a last line of a lone '\r', or a '\r' in front of EOF
            assert text[-2:] == (b"\n\r" if final_nl else b"x\r")
            out.append((("lone_cr", final_nl, quoted), text, 0))
    tail = b'k,"open\nstill open'
    for size in (5000, TILE, 2 * TILE + 1):
        text = _sized_text(size - len(tail), True, True) + tail
        assert len(text) == size and text.count(b'"') & 1
        out.append((("eof_in_quotes", size), text, M.QUOTE))
    for tag, text, kind in out:
        recs, ek, er, _ = M.read_all(text, lazy=False, fpr=-1)
        assert ek == kind and (not ek or er == len(recs)), tag          # the error, if any, is the last record's
        assert (b'"' in text) == (tag[-1] is True or tag[0] == "eof_in_quotes"), tag
    return out


@gpu
def test_text_ends(ctx):
    for tag, text, kind in _end_texts():
        t = check(ctx, text, [0, 1, 2], {"fpr": -1}, tag=tag)
        assert t.error_kind == kind, tag


# =================================================================================================================================
# 2. the stage edge of the record-parallel kernels
# =================================================================================================================================
_COLS2 = [0, 3, 5]   # the first field, the last field of a four-field record, the last of a six-field one (the others lack it)


def _short_tile(tag, longer=0):
    """256 records of 7 bytes (1792 = 16 * 112 bytes); `longer` more bytes in record 5."""
    return b"".join(b"%s%03d,u%s\n" % (tag, i, b"p" * longer if i == 5 else b"") for i in range(REC_TILE))


def _stage_edge_text(stage, span, mis, kind):
    """Three tiles of 256 records.  Tile 1 begins `mis` bytes behind a 16-byte boundary and spans exactly `span` bytes; the
    short tiles around it make the host choose `stage`."""
    def rec(i):
        end = b"\r\n" if i % 16 == 7 else b"\n"
        if i == 100:
            return None
        if kind == "quoted" and i % 4 == 1:
            return b'q%03d,"b""b","c\r\nc",d%03d' % (i, i) + end
        if kind == "trim":
            return b't%03d,  bb,\t"c c", d%03d' % (i, i) + end
        if i % 8 == 3:
            return b"p%03d,bb,cc,dd,ee,ff%03d" % (i, i) + end
        return b"p%03d,bb,cc,d%03d" % (i, i) + end
    recs = [rec(i) for i in range(REC_TILE)]
    want_len = span + 1 - mis
    fill = want_len - sum(len(r) for r in recs if r) - len(b"f100,,cc,d100\n")
    assert fill > 0
    recs[100] = b"f100," + b"x" * fill + b",cc,d100\n"
    head = _short_tile(b"s", longer=mis)
    text = head + b"".join(recs) + _short_tile(b"z")
    opts = {"fpr": -1, "trim": kind == "trim"}
    starts = M.read_all(text, lazy=False, fpr=-1, trim=opts["trim"])[3]
    assert len(starts) == 3 * REC_TILE and starts[REC_TILE] == len(head) and starts[REC_TILE] % 16 == mis
    assert tile_span(text, starts, REC_TILE, 2 * REC_TILE - 1) == span
    assert stage_bytes(len(text), len(starts)) == stage
    assert tile_span(text, starts, 0, REC_TILE - 1) <= STAGE_MIN and tile_span(text, starts, 2 * REC_TILE, 3 * REC_TILE - 1) <= STAGE_MIN
    assert (b'"' in text) == (kind != "plain")
    return text, opts


def _stage_edge_cases(stage):
    spans = [stage - 1, stage, stage + 1] + ([60000] if stage == STAGE_MAX else [])   # 60000: a whole tile from global memory
    return [(span, mis) for span in spans for mis in (0, 15)]


def test_section2_builders_place_their_tiles():
    for stage in (8192, 16384, 32768):
        for kind in ("plain", "quoted", "trim"):
            for span, mis in _stage_edge_cases(stage):
                text, opts = _stage_edge_text(stage, span, mis, kind)
                assert model(text, _COLS2, opts)[1] == 0


@gpu
@pytest.mark.parametrize("kind", ["plain", "quoted", "trim"])
@pytest.mark.parametrize("stage", [8192, 16384, 32768])
def test_tile_at_the_stage_edge(ctx, stage, kind):
    """Tile 1 at stage_bytes - 1 and stage_bytes is staged in LDS, at stage_bytes + 1 it is parsed from global memory, between
    two staged tiles of the same launch."""
    for span, mis in _stage_edge_cases(stage):
        text, opts = _stage_edge_text(stage, span, mis, kind)
        check(ctx, text, _COLS2, opts, tag=(stage, span, mis, kind))


# =================================================================================================================================
# 3. the copy pass falls back where the length pass staged
# =================================================================================================================================
def _two_field_tile(a_total, b_total):
    """256 records `f0,f1`; the VALUES of field 0 sum to a_total bytes, those of field 1 to b_total; every fourth f1 is quoted
    and holds a quote and a comma."""
    out = []
    for i in range(REC_TILE):
        la = a_total // REC_TILE + (i < a_total % REC_TILE)
        lb = b_total // REC_TILE + (i < b_total % REC_TILE)
        f1 = b"y" * lb
        if i % 4 == 1 and lb >= 2:
            v = b"y" * (lb - 2) + b'",'
            f1 = b'"' + v.replace(b'"', b'""') + b'"'
        out.append(b"k" * la + b"," + f1 + b"\n")
    return b"".join(out)


def _copy_fallback_text(a_total, b_total, cols, expect_fits):
    text = _short_tile(b"s") + _two_field_tile(a_total, b_total) + _short_tile(b"z")
    rows, ek, _, starts = model(text, cols, {"fpr": 2})
    assert ek == 0 and len(starts) == 3 * REC_TILE
    stage = stage_bytes(len(text), len(starts))
    assert stage == STAGE_MIN
    fits = []
    for t in range(3):
        spans = [sum(len(r[k]) for r in rows[t * REC_TILE:(t + 1) * REC_TILE]) for k in range(len(cols))]
        text_span = tile_span(text, starts, t * REC_TILE, (t + 1) * REC_TILE - 1)
        assert text_span <= stage                      # k_csv_fields stages every tile
        fits.append(copy_fits(text_span, spans, stage))
        if t == 1:
            mid = spans
    assert fits == [True, expect_fits, True], fits     # both kinds of tile in one launch
    assert [mid[k] for k in range(len(cols))] == [b_total if c == 1 else a_total for c in cols]
    return text, sum(rounded(s) for s in mid)


# (field-0 bytes, field-1 bytes, columns, the copy pass stages tile 1, sum of the rounded spans or None)
_COPY_CASES = {
    "field_twice": (256, 6656, [1, 1], False, None),
    "field_five_times": (256, 6656, [1, 0, 1, 1, 1, 1], False, None),           # more than kPre columns
    "field_sixteen_times": (256, 6656, [1] * MAX_KEY_COLS, False, None),
    # the cap's edge.  With two columns the text is staged (<= S) and the spans overflow only when both are the same field, so
    # the sum of the rounded spans moves in steps of 32; a third column moves it by 16
    "two_columns_at_the_cap": (256, 4336, [1, 1], True, STAGE_MIN + 512),
    "two_columns_32_over": (256, 4337, [1, 1], False, STAGE_MIN + 512 + 32),
    "three_columns_at_the_cap": (1008, 3824, [1, 1, 0], True, STAGE_MIN + 512),
    "three_columns_16_over": (1009, 3824, [1, 1, 0], False, STAGE_MIN + 512 + 16),
}


def _copy_case(name):
    a, b, cols, fits, total = _COPY_CASES[name]
    assert len(cols) <= MAX_KEY_COLS and (name != "field_five_times" or cols.count(1) == 5 > K_PRE)
    text, rounded_sum = _copy_fallback_text(a, b, cols, fits)
    assert total is None or rounded_sum == total
    assert fits or rounded_sum > out_cap(STAGE_MIN)
    return text, cols


def _distinct_columns_text():
    recs = []
    for i in range(3 * REC_TILE):
        f = [b"%x%x" % (i % 251, j) for j in range(20)]
        if i % 5 == 2:
            f[7] = b'"%x""q\r\n"' % i
        recs.append(b",".join(f) + b"\n")
    text = b"".join(recs)
    cols16 = [0, 19, 3, 7, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14]
    cols5 = [19, 0, 7, 3, 11]
    assert len(set(cols16)) == MAX_KEY_COLS and len(set(cols5)) == 5 > K_PRE
    rows, ek, _, starts = model(text, cols16, {"fpr": 20})
    stage = stage_bytes(len(text), len(starts))
    for t in range(3):   # staged by both passes: LDS destinations with more than kPre columns
        spans = [sum(len(r[k]) for r in rows[t * REC_TILE:(t + 1) * REC_TILE]) for k in range(16)]
        assert ek == 0 and copy_fits(tile_span(text, starts, t * REC_TILE, (t + 1) * REC_TILE - 1), spans, stage)
    return text, cols16, cols5


def test_section3_builders_place_their_spans():
    for name in _COPY_CASES:
        _copy_case(name)
    _distinct_columns_text()


@gpu
@pytest.mark.parametrize("name", list(_COPY_CASES))
def test_copy_pass_falls_back_where_the_length_pass_staged(ctx, name, monkeypatch):
    text, cols = _copy_case(name)
    check(ctx, text, cols, {"fpr": 2}, tag=name)
    check(ctx, text, cols, {"fpr": 2}, skip=3, tag=(name, "skip"))
    monkeypatch.setenv("CPH_CSV_OFFSETS64", "1")
    check(ctx, text, cols, {"fpr": 2}, bits=64, tag=(name, 64))


@gpu
def test_sixteen_distinct_columns(ctx):
    text, cols16, cols5 = _distinct_columns_text()
    check(ctx, text, cols16, {"fpr": 20}, tag=16)
    check(ctx, text, cols5, {"fpr": 20}, tag=5)
    check(ctx, text, cols16, {"fpr": 20}, skip=1, tag=(16, "skip"))


# =================================================================================================================================
# 4. record counts, skipped records, the first error
# =================================================================================================================================
_GOOD = (lambda i: b'r%d,"q""%d",z\n' % (i, i), lambda i: b"r%d,p%d,z\r\n" % (i, i), lambda i: b'r%d,"m\n%d",z\n' % (i, i))
_BAD = {M.BARE: lambda i: b'r%d,a"b,z\n' % i, M.QUOTE: lambda i: b'r%d,"x"y,z\n' % i, M.FIELDS: lambda i: b"r%d,only\n" % i}


def _records_text(nrec, errs=None):
    errs = errs or {}
    return b"".join(_BAD[errs[i]](i) if i in errs else _GOOD[i % 3](i) for i in range(nrec))


_NRECS = (1, 255, 256, 257, 512, 513)


def _skips(nrec):
    return (0, 1, 3, 255, 256, 257, nrec, nrec + 1)


def _count_case(nrec, skip):
    text = _records_text(nrec)
    rows, ek, _, starts = model(text, [0, 1, 2], {"fpr": 3}, skip)
    pad = pad_of(skip, nrec)
    assert ek == 0 and len(starts) == nrec and len(rows) == max(0, nrec - skip)
    assert 0 <= pad < REC_TILE and (min(skip, nrec) + pad) % REC_TILE == 0     # the first returned record starts a tile
    return text


def _error_cases():
    """(tag, text, options, skip, kind, record)"""
    out = []
    for e in (0, 255, 256, 257):
        for skip in (0, 1):   # skip = 1: pad = 255, the tile edges lie behind records 0, 256, ...: e on both sides of one
            for kind, fpr in ((M.BARE, 3), (M.QUOTE, 3), (M.FIELDS, 0), (M.FIELDS, 3)):
                er = 1 if (e, fpr, kind) == (0, 0, M.FIELDS) else e   # FieldsPerRecord = 0: record 0 sets the count, record 1 breaks it
                out.append((("first", e, skip, kind, fpr), _records_text(600, {e: kind}), {"fpr": fpr}, skip, kind, er))
    for skip in (0, 1):
        # two errors: the smallest record index wins, whichever tile (workgroup) reports first
        out.append((("two", 100, 400, skip), _records_text(600, {100: M.FIELDS, 400: M.QUOTE}), {"fpr": 3}, skip, M.FIELDS, 100))
        out.append((("two", 400, 100, skip), _records_text(600, {100: M.QUOTE, 400: M.FIELDS}), {"fpr": 3}, skip, M.QUOTE, 100))
        out.append((("two_in_tile_0", skip), _records_text(600, {10: M.QUOTE, 200: M.FIELDS}), {"fpr": 3}, skip, M.QUOTE, 10))
        out.append((("two_far", skip), _records_text(600, {255: M.FIELDS, 599: M.BARE}), {"fpr": 3}, skip, M.FIELDS, 255))
    out.append((("below_skip",), _records_text(600, {3: M.QUOTE}), {"fpr": 3}, 10, M.QUOTE, 3))
    out.append((("below_skip_at_tile",), _records_text(600, {256: M.FIELDS}), {"fpr": 3}, 300, M.FIELDS, 256))
    for kind in (M.QUOTE, M.FIELDS):   # well-formed records behind the error in the last tile: the columns end at the true size
        for skip in (0, 1):
            out.append((("mid_last_tile", kind, skip), _records_text(600, {560: kind}), {"fpr": 3}, skip, kind, 560))
    for tag, text, opts, skip, kind, er in out:
        rows, ek, mer, _ = model(text, [0, 1, 2], opts, skip)
        assert (ek, mer) == (kind, er) and len(rows) == max(0, er - skip), tag
    return out


def test_section4_builders_and_mirrored_pad():
    for nrec in _NRECS:
        for skip in _skips(nrec):
            _count_case(nrec, skip)
    assert [pad_of(s, 600) for s in (0, 1, 255, 256, 257, 700)] == [0, 255, 1, 0, 255, 168]
    assert len(_error_cases()) == 32 + 8 + 2 + 4


@gpu
@pytest.mark.parametrize("nrec", _NRECS)
def test_record_counts_and_skips(ctx, nrec, monkeypatch):
    for bits in (32, 64):
        if bits == 64:
            monkeypatch.setenv("CPH_CSV_OFFSETS64", "1")
        for skip in _skips(nrec):
            t = check(ctx, _count_case(nrec, skip), [0, 1, 2], {"fpr": 3}, skip=skip, bits=bits, tag=(nrec, skip, bits))
            assert t.nrecords == max(0, nrec - skip)


@gpu
def test_first_error_at_tile_edges(ctx):
    for tag, text, opts, skip, kind, er in _error_cases():
        t = check(ctx, text, [0, 1, 2], opts, skip=skip, tag=tag)
        assert (t.error_kind, t.error_record, t.nrecords) == (kind, er, max(0, er - skip)), tag


# =================================================================================================================================
# 5. more tiles than the grid has workgroups
# =================================================================================================================================
_BLOCK = b'1,a\n2,"b""c"\n3,"d\ne"\n4,f\r\n5,g\n6,"h"\r\n7,i\n8,"j"\n'
_NBLOCKS = (GRID_CAP * REC_TILE + 8 * 1024) // 8     # 2 105 344 records: 33 tiles behind the grid's first round
_LONG = b'9,"' + b'lo""ng\n' * 1700 + b'"\n'       # ~12 KiB: its tile exceeds stage_bytes


def _grid_case(with_long):
    """(text, per column: expected lengths and SHA-256 of the expected bytes, records).  The CPU models ONE block (and the one
    long record), never the whole text."""
    recs, ek, _, _ = M.read_all(_BLOCK, lazy=False, fpr=2)
    assert ek == 0 and len(recs) == 8 and _BLOCK.endswith(b"\n")
    n1, n2 = (_NBLOCKS - 375, 375) if with_long else (_NBLOCKS, 0)      # the long record 3000 records from the end
    long_rec = M.read_all(_LONG, lazy=False, fpr=2)[0]
    assert len(long_rec) == 1 and long_rec[0][1] == b'lo"ng\n' * 1700
    text = _BLOCK * n1 + (_LONG + _BLOCK * n2 if with_long else b"")
    nrec = 8 * _NBLOCKS + int(with_long)
    assert nrec > GRID_CAP * REC_TILE + 300 and len(text) < 16 << 20
    skip, pad = 1, pad_of(1, nrec)
    assert pad == 255
    ntile = (nrec + pad + REC_TILE - 1) // REC_TILE
    assert ntile > GRID_CAP and (nrec - skip + REC_TILE - 1) // REC_TILE > GRID_CAP     # both kernels loop a second time
    stage = stage_bytes(len(text), nrec)
    assert stage == STAGE_MIN
    if with_long:
        r = 8 * n1                                                         # the long record's index
        assert (r + pad) // REC_TILE >= GRID_CAP and (r - skip) // REC_TILE >= GRID_CAP   # in a tile that was prefetched
        assert len(_LONG) > stage > 2 * REC_TILE * len(_BLOCK) // 8        # that one tile is not staged, the others are
    want = []
    for c in range(2):
        vals = [r[c] for r in recs]
        lens = np.tile([len(v) for v in vals], n1)
        data = b"".join(vals) * n1
        if with_long:
            lens = np.concatenate([lens, [len(long_rec[0][c])], np.tile([len(v) for v in vals], n2)])
            data += long_rec[0][c] + b"".join(vals) * n2
        want.append((lens[skip:], hashlib.sha256(data[len(vals[0]):]).digest()))
    return text, want, nrec - skip


def test_section5_builder():
    for with_long in (False, True):
        text, want, nout = _grid_case(with_long)
        assert all(len(lens) == nout for lens, _ in want)


@gpu
@pytest.mark.parametrize("with_long", [False, True])
def test_more_tiles_than_the_grid_has_workgroups(ctx, with_long):
    """More than 8192 * 256 records: 8192 is grid_for_items' cap, so k_csv_fields' bounds(T + gridDim.x) and k_csv_copy_fields'
    prefetch(r0 + gridDim.x * 256) load a second tile.  skip_records = 1 gives pad = 255."""
    text, want, nout = _grid_case(with_long)
    t = device(ctx, text, [0, 1], {"fpr": 2}, skip=1)
    assert (t.error_kind, t.nrecords) == (0, nout)
    for c in range(2):
        offs = np.asarray(t.columns[c].offsets).astype(np.int64)
        data = np.asarray(t.columns[c].data).tobytes()
        assert offs[0] == 0 and int(offs[-1]) == len(data)
        assert np.array_equal(np.diff(offs), want[c][0])
        assert hashlib.sha256(data).digest() == want[c][1]


# =================================================================================================================================
# 6. the fast path's window edge, tile seam and chunk edge
# =================================================================================================================================
_WINDOW_OFFSETS = (20416, 20478, 20479, 20480, 20481)


def _window_text(tile, w):
    """The last record `tile` owns (it begins behind the last newline of the tile's own 16 KiB) ends with its newline at offset
    w of the tile's window.  The fast path takes the text iff that newline lies inside the window's kFtStage bytes."""
    target = tile * TILE + w
    head = b"a,b\n" * (((tile + 1) * TILE - 8) // 4)
    text = head + b"x" * (target - len(head) - 2) + b",y\n" + b"c,d\n" * 10
    assert text[target:target + 1] == b"\n" and b"\n" not in text[len(head):target]
    assert tile * TILE < len(head) <= (tile + 1) * TILE and text[len(head) - 1:len(head)] == b"\n"   # owned by `tile`, and its last
    return text, w < FT_STAGE


def _placed(pos, chunk, prefix=b"k,"):
    """A text of short records with `chunk` at byte `pos`, inside a record that begins with `prefix`."""
    head = b"a,b\n" * (max(0, pos - 8) // 4)
    text = head + prefix + b"x" * (pos - len(head) - len(prefix)) + chunk + b"q,r\n" * 20
    assert text[pos:pos + len(chunk)] == chunk and len(head) + len(prefix) < pos
    return text


def _seam_texts(edge):
    """The five placements at `edge` (the byte at edge - 1 is the last of a tile / chunk, the byte at edge the first of the next)."""
    out = {
        "cr_last_nl_first": _placed(edge - 1, b"\r\n"),
        "nl_last": _placed(edge - 1, b"\n"),
        "nl_first": _placed(edge, b"\n"),
        "delimiter_last": _placed(edge - 1, b",y\n"),
        "delimiter_first": _placed(edge, b",y\n"),
        "record_starts_at_last": _placed(edge - 2, b"\ns,t\n"),
    }
    want = {"cr_last_nl_first": b"\r\n", "nl_last": b"\nq", "nl_first": b"x\n", "delimiter_last": b",y", "delimiter_first": b"x,",
            "record_starts_at_last": b"s,"}
    for name, text in out.items():
        assert text[edge - 1:edge + 1] == want[name], (name, edge)
        assert b'"' not in text and M.read_all(text, lazy=False, fpr=-1)[1] == 0
    assert out["record_starts_at_last"][edge - 2:edge - 1] == b"\n"
    return out


def _three_chunk_field_text():
    text = b"a,b\n" * 24 + b"k," + b"v" * 260 + b",e\n" + b"q,r\n" * 20
    f0 = text.index(b"v")
    assert f0 <= 128 and f0 + 260 >= 320 and text[128:320] == b"v" * 192     # the chunks at 128, 192 and 256 hold nothing else
    return text


def test_section6_builders_place_their_bytes():
    for tile in (0, 1):
        assert [_window_text(tile, w)[1] for w in _WINDOW_OFFSETS] == [True, True, True, False, False]
    for edge in (64, 4096, TILE):
        _seam_texts(edge)
    _three_chunk_field_text()


@gpu
@pytest.mark.parametrize("tile", [0, 1])
def test_fast_path_window_edge(ctx, tile):
    """k_csv_fast: `slow = any && all < own + 1` — the newline that ends the last owned record must be one of the window's
    kFtStage = 20480 bytes: offset 20479 is taken, 20480 goes to the classic kernels."""
    from tests.test_csv_ingest import _fast_vs_classic
    for w in _WINDOW_OFFSETS:
        text, fast = _window_text(tile, w)
        _fast_vs_classic(ctx, text, [0, 1], expect_fast=fast)
        want, ek, er, _ = model(text, [1, 0], {"fpr": 2}, 1)
        got = _fast_vs_classic(ctx, text, [1, 0], expect_fast=fast, fields_per_record=2, skip_records=1)
        assert (got[1], got[2], got[3]) == (len(want), ek, er) and [list(v) for v in zip(*got[0])] == want, (tile, w)


@gpu
@pytest.mark.parametrize("edge", [64, 4096, TILE])
def test_fast_path_tile_seam_and_chunk_edges(ctx, edge):
    """edge 16384: the tile seam; 64: a thread's chunk; 4096: a wave (64 threads x 64 bytes)."""
    from tests.test_csv_ingest import _fast_vs_classic
    for name, text in _seam_texts(edge).items():
        want, ek, er, _ = model(text, [0, 1, 2], {"fpr": -1})
        got = _fast_vs_classic(ctx, text, [0, 1, 2], fields_per_record=-1)
        assert (got[1], got[2], got[3]) == (len(want), ek, er) and [list(v) for v in zip(*got[0])] == want, (name, edge)


@gpu
def test_fast_path_field_spanning_three_chunks(ctx):
    from tests.test_csv_ingest import _fast_vs_classic
    text = _three_chunk_field_text()
    want = model(text, [0, 1, 2], {"fpr": -1})[0]
    got = _fast_vs_classic(ctx, text, [0, 1, 2], fields_per_record=-1)
    assert [list(v) for v in zip(*got[0])] == want
