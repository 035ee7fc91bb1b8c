"""LazyQuotes on the CPU: the line model of Go's readRecord (tests/lazy_csv_model.py) is tied to the pinned oracle in its strict
mode, pinned by known answers in its lazy mode, and equals the seven-state byte automaton (Python, and the device's own chunk code
compiled for the host) on record starts.  ingest.first_record(lazy_quotes=True) — the header line — follows the same rules."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import orc
from tests import lazy_csv_model as M
from tests.golden.go_csv_lazy_cases import LAZY_CASES
from tests.golden.go_csv_reader_cases import CASES

ROOT = Path(__file__).resolve().parent.parent
ALPHABET = np.frombuffer(b'ab ,"\n\r#\t', dtype=np.uint8)
OPTION_SETS = ({}, {"trim": True}, {"comment": b"#"}, {"comment": b"#", "trim": True})
WIDTH = 8


def _kw(opts):
    return dict(comma=opts.get("comma", b","), comment=opts.get("comment"), trim=opts.get("trim", False), fpr=opts.get("fpr", 0))


def _random_texts(seed, n, maxlen):
    rng = np.random.default_rng(seed)
    return [ALPHABET[rng.integers(0, len(ALPHABET), int(rng.integers(0, maxlen)))].tobytes() for _ in range(n)]


def _oracle(text, opts):
    cols, ek, er = orc.csv_parse(text, list(range(WIDTH)), comma=opts.get("comma", b","), comment=opts.get("comment"),
                                 trim_leading_space=opts.get("trim", False), fields_per_record=opts.get("fpr", 0))
    return [[cols[c].value(r) for c in range(WIDTH)] for r in range(cols[0].nrows)], ek, er if ek else 0


def _padded(recs):
    return [r[:WIDTH] + [b""] * (WIDTH - len(r)) for r in recs]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_strict_model_matches_go_known_answers(case):
    _, text, opts, want, err = case
    recs, ek, er, _ = M.read_all(text, **_kw(opts))
    assert recs == want and (ek, er) == (err if err else (0, 0))


def test_strict_model_matches_the_oracle_on_random_text():
    nerr = 0
    for i, text in enumerate(_random_texts(101, 20_000, 36)):
        opts = dict(OPTION_SETS[i % 4], fpr=(-1, 0)[(i // 4) % 2])
        recs, ek, er, _ = M.read_all(text, **_kw(opts))
        assert (_padded(recs), ek, er) == _oracle(text, opts), (text, opts)
        nerr += ek != 0
    assert nerr > 5000   # arbitrary text is mostly malformed


@pytest.mark.parametrize("case", LAZY_CASES, ids=[c[0] for c in LAZY_CASES])
def test_lazy_model_matches_known_answers(case):
    _, text, opts, want, err = case
    recs, ek, er, _ = M.read_all(text, lazy=True, **_kw(opts))
    assert recs == want and (ek, er) == (err if err else (0, 0))


def test_lazy_equals_strict_where_strict_has_no_error():
    nvalid = 0
    texts = _random_texts(103, 30_000, 30) + [c[1] for c in CASES]
    for i, text in enumerate(texts):
        opts = dict(OPTION_SETS[i % 4], fpr=-1)
        strict = M.read_all(text, **_kw(opts))
        if strict[1] == 0:
            nvalid += 1
            assert M.read_all(text, lazy=True, **_kw(opts)) == strict, (text, opts)
    assert nvalid > 5000


def test_automaton_record_starts_equal_the_lazy_model():
    for text in _random_texts(107, 50_000, 28) + [c[1] for c in LAZY_CASES]:
        for opts in OPTION_SETS:
            kw = dict(comment=opts.get("comment"), trim=opts.get("trim", False))
            assert M.automaton_record_starts(text, **kw) == M.read_all(text, lazy=True, fpr=-1, **kw)[3], (text, opts)


def test_device_chunk_code_on_the_host_equals_the_automaton():
    """csv_lazy_device.hpp compiled by g++ (tests/cpp/test_csv_lazy): chunk maps, packed, scanned, walked again for the separators."""
    subprocess.check_call(["make", "-C", str(ROOT), "tests/cpp/test_csv_lazy"])
    texts = _random_texts(109, 4000, 200) + [c[1] for c in LAZY_CASES]
    payload = "\n".join(t.hex() for t in texts) + "\n"
    for opts in OPTION_SETS:
        r = subprocess.run([str(ROOT / "tests/cpp/test_csv_lazy"), "44", str(ord(opts["comment"])) if "comment" in opts else "0",
                            "1" if opts.get("trim") else "0"], input=payload, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(texts)
        for text, line in zip(texts, lines):
            tr = M.automaton_trace(text, comment=opts.get("comment"), trim=opts.get("trim", False))
            assert [int(x) for x in line.split(",") if x] == [i for i, c in enumerate(text) if c == 0x0A and tr[i] != M.QD], (text, opts)


def test_first_record_lazy_follows_the_model():
    from csvplus_amd.ingest import first_record
    for text in _random_texts(113, 6000, 40) + [c[1] for c in LAZY_CASES]:
        for opts in OPTION_SETS:
            recs = M.read_all(text, lazy=True, fpr=-1, comment=opts.get("comment"), trim=opts.get("trim", False))[0]
            got = first_record(text, comment=opts.get("comment"), trim_leading_space=opts.get("trim", False), lazy_quotes=True)
            assert got == (recs[0] if recs else None), (text, opts)
    for _, text, opts, want, _ in LAZY_CASES:
        got = first_record(text, comma=opts.get("comma", b","), comment=opts.get("comment"), trim_leading_space=opts.get("trim", False),
                           lazy_quotes=True)
        assert got == want[0]
