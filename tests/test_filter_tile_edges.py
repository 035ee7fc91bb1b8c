"""cph_filter_rows' WHERE window at the edges of its bitmap tiles (T = 2048 rows, 64 rows per word): k_pred_eval's tile store,
the scan of the tile counts and k_pred_emit's rank walk with its [skip, skip + limit) window, against predicates.select_rows;
and cph_rowsel_take + csv_write as consumers of the emitted row numbers."""
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import StrCol
from csvplus_amd import _native as N
from csvplus_amd import predicates as P
from csvplus_amd.predicates import Like

T = 2048   # rows per tile: kTileRows in csvplus_amd/csrc/tile_bitmap.hpp
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
FIRST = 3   # the non-zero first_row: the tiles start there, not at row 0 of the column
DEVICE = N.CPH_MEM_DEVICE

PATTERNS = {
    "all": lambda i, n: np.ones(n, dtype=bool),
    "none": lambda i, n: np.zeros(n, dtype=bool),
    "every_other": lambda i, n: i % 2 == 0,
    "last_of_each_tile": lambda i, n: (i % T == T - 1) | (i == n - 1),
    "first_of_second_tile": lambda i, n: i == T,
}


def flags_of(pattern, n, first_row):
    """One flag per row of the column: `first_row` kept rows in front of the call's n rows, which follow the pattern."""
    return np.concatenate([np.ones(first_row, dtype=bool), PATTERNS[pattern](np.arange(n), n)])


def windows(flags, n, first_row):
    """(skip, limit): everything | two rows around the first tile boundary | skip == the total | limit 0"""
    total = int(flags[first_row:first_row + n].sum())
    in_tile0 = int(flags[first_row:first_row + min(n, T)].sum())
    return [(0, None), (max(in_tile0 - 1, 0), 2), (total, None), (0, 0)]


def value_col(flags):
    return StrCol.from_values([b"y" if f else b"no" for f in flags])


def test_the_cases_sit_on_the_tile_edges():
    assert "kTileRows" in (Path(__file__).resolve().parent.parent / "csvplus_amd" / "csrc" / "tile_bitmap.hpp").read_text()
    assert SIZES == (1, 63, 64, 65, 2047, 2048, 2049, 4097)
    f = flags_of("last_of_each_tile", 2 * T + 1, 0)
    assert np.flatnonzero(f).tolist() == [T - 1, 2 * T - 1, 2 * T]
    assert windows(f, 2 * T + 1, 0) == [(0, None), (0, 2), (3, None), (0, 0)]
    assert P.select_rows(f, "where", 0, 2 * T + 1, 0, 2) == [T - 1, 2 * T - 1]
    f = flags_of("every_other", T + 1, FIRST)
    assert windows(f, T + 1, FIRST)[1] == (T // 2 - 1, 2)
    assert P.select_rows(f, "where", FIRST, T + 1, T // 2 - 1, 2) == [FIRST + T - 2, FIRST + T]   # one row of each tile
    assert np.flatnonzero(flags_of("first_of_second_tile", T + 1, 0)).tolist() == [T] and not flags_of("first_of_second_tile", T, 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_where_window_against_select_rows(ctx, n):
    from csvplus_amd.materialize import filter_rows
    for pattern in PATTERNS:
        for first_row in (0, FIRST):
            flags = flags_of(pattern, n, first_row)
            cols = {"v": value_col(flags).to_device()}
            for skip, limit in windows(flags, n, first_row):
                want = P.select_rows(flags, "where", first_row, n, skip, limit)
                for bits in (32, 64):
                    got = filter_rows(ctx, cols, Like(v=b"y"), nrows=n, first_row=first_row, skip=skip, limit=limit, out_bits=bits)
                    assert got.dtype == (np.uint32 if bits == 32 else np.uint64)
                    assert got.tolist() == want, (pattern, first_row, skip, limit, bits)


def _device_array(a, keep):
    import torch
    t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
    keep.append(t)
    return t.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_taken_ids_feed_the_csv_writer(ctx, n):
    """The rows read through a Join-like id array (reversed order); the filter's two rows around the first tile boundary, narrowed
    by cph_rowsel_take, are what csv_write prints."""
    from csvplus_amd.materialize import csv_write, filter_rows, take_rows
    sel = np.arange(n, dtype=np.uint32)[::-1].copy()   # joined row i = table row n - 1 - i
    names = ["id", "v"]
    for pattern in PATTERNS:
        flags = flags_of(pattern, n, 0)
        ids_host = [b"%d" % j for j in range(n)]
        table = {"id": ids_host, "v": [b"y" if flags[n - 1 - j] else b"no" for j in range(n)]}   # so that joined row i carries flags[i]
        cols = {k: StrCol.from_values(v).to_device() for k, v in table.items()}
        keep = []
        dev_sel = (_device_array(sel, keep), 32, n)
        skip, limit = windows(flags, n, 0)[1]
        want = P.select_rows(flags, "where", 0, n, skip, limit)
        assert len(want) <= 2
        kept = filter_rows(ctx, cols, Like(v=b"y"), row_ids={"id": dev_sel, "v": dev_sel}, nrows=n, skip=skip, limit=limit, out_mem=DEVICE,
                           as_handle=True)
        taken = take_rows(ctx, dev_sel, kept, out_mem=DEVICE, as_handle=True)
        try:
            assert len(kept) == len(taken) == len(want)
            if not want:   # an empty list is a range: nothing to read through
                continue
            want_cols = [StrCol.from_values([table[k][n - 1 - i] for i in want]) for k in names]
            want_csv = csv_write(ctx, want_cols, names)
            assert want_csv.count(b"\n") == len(want) + 1
            assert csv_write(ctx, [cols[k] for k in names], names, row_ids=[taken.as_row_ids()] * 2, nrows=len(want)) == want_csv, pattern
        finally:
            kept.release()
            taken.release()
        del keep
