"""ordering.order_model — the pure-Python statement of cph_order_rows (slices.SortStableFunc over cmp.Compare per key) —
against hand-written cases, and the ctypes structs against the compiled header.  CPU only."""
from __future__ import annotations

import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from csvplus_amd import _native as N
from csvplus_amd import ordering as O

ROOT = Path(__file__).resolve().parent.parent
NAN = math.nan


def test_descending_keeps_ties_in_input_order():
    v = [2, 1, 2, 1, 3]
    assert O.order_model([O.Asc(v, "int")]) == [1, 3, 0, 2, 4]
    assert O.order_model([O.Desc(v, "int")]) == [4, 0, 2, 1, 3]            # not the reverse of ascending: [4, 2, 0, 3, 1]
    assert O.order_model([O.Desc(v, "int")]) != O.order_model([O.Asc(v, "int")])[::-1]
    assert O.order_model([O.Asc([7, 7, 7], "int")]) == [0, 1, 2] == O.order_model([O.Desc([7, 7, 7], "int")])


def test_nan_is_first_under_asc_and_last_under_desc():
    v = [1.0, NAN, -math.inf, -NAN, 0.0, math.inf]
    assert O.order_model([O.Asc(v, "float")]) == [1, 3, 2, 4, 0, 5]        # the NaNs tie: input order
    assert O.order_model([O.Desc(v, "float")]) == [5, 0, 4, 2, 1, 3]
    z = [0.0, -0.0, 1.0, -0.0, 0.0, -1.0]                                   # -0 == +0: input order decides
    assert O.order_model([O.Asc(z, "float")]) == [5, 0, 1, 3, 4, 2]
    assert O.order_model([O.Desc(z, "float")]) == [2, 0, 1, 3, 4, 5]
    assert O.compare_float(NAN, -math.inf) == -1 and O.compare_float(-math.inf, NAN) == 1 and O.compare_float(NAN, -NAN) == 0
    assert O.compare_float(-0.0, 0.0) == 0 and O.compare_int(-(1 << 63), (1 << 63) - 1) == -1


def test_keys_decide_in_order_then_the_input_order():
    name = [b"b", b"a", b"b", b"a", b"b", b"a"]
    qty = [1, 2, 2, 2, 1, 1]
    price = [0.5, 0.5, 0.25, 0.5, 0.5, NAN]
    # name ascending, qty descending, price ascending
    assert O.order_model([O.Asc(name, "bytes"), O.Desc(qty, "int"), O.Asc(price, "float")]) == [1, 3, 5, 2, 0, 4]
    assert O.order_model([(name, "bytes", False), (qty, N.CPH_NUM_INT64, True), (price, "float", False)]) == [1, 3, 5, 2, 0, 4]
    # strings.Compare, not numbers: "10" < "9"; tuples compare column by column
    assert O.order_model([O.Asc([b"9", b"10", b"1"], "bytes")]) == [2, 1, 0]
    assert O.order_model([O.Asc([(b"a", b"z"), (b"a", b""), (b"", b"zz")], "bytes")]) == [2, 1, 0]


def test_skip_and_limit_beyond_the_ends():
    v = [5, 3, 4, 1, 2]
    full = [3, 4, 1, 2, 0]
    assert O.order_model([O.Asc(v, "int")], 0, None) == full
    assert O.order_model([O.Asc(v, "int")], 2, 2) == full[2:4]
    assert O.order_model([O.Asc(v, "int")], 4, 10) == full[4:]
    assert O.order_model([O.Asc(v, "int")], 5, 1) == [] == O.order_model([O.Asc(v, "int")], 99, None)
    assert O.order_model([O.Asc(v, "int")], 0, 0) == [] and O.order_model([O.Asc(v, "int")], 0, 99) == full
    assert O.order_model([O.Asc([], "int")], 0, 3) == []
    with pytest.raises(ValueError):
        O.order_model([])
    with pytest.raises(ValueError):
        O.order_model([O.Asc([1, 2], "int"), O.Asc([1.0], "float")])


def test_key_kinds():
    assert O.Asc(np.zeros(2)).kind == N.CPH_NUM_FLOAT64 and O.Desc(np.zeros(2, np.int64)).kind == N.CPH_NUM_INT64
    assert O.Desc(None, "bytes").descending and not O.Asc(None, "bytes").descending
    with pytest.raises(ValueError):
        O.Asc([1, 2])            # a list needs a kind
    with pytest.raises(ValueError):
        O.Desc(None, "decimal")
    e = O.OrderError(40, 1, N.CPH_NUM_ERR_SYNTAX, 2)
    assert "row 40" in str(e) and "key 1" in str(e) and "invalid syntax" in str(e) and (e.row, e.key, e.nerrors) == (40, 1, 2)


def test_order_struct_sizes_against_the_compiled_header(tmp_path):
    import ctypes as C

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csvplus_hip.h"\nint main(void){'
                   'printf("sizes %zu %zu %d\\n", sizeof(cph_order_key), sizeof(cph_ordered), CPH_ORDER_MAX_KEYS);'
                   'printf("key %zu %zu %zu %zu %zu %zu\\n", offsetof(cph_order_key, kind), offsetof(cph_order_key, descending), '
                   "offsetof(cph_order_key, values), offsetof(cph_order_key, status), offsetof(cph_order_key, values_mem), offsetof(cph_order_key, index));"
                   'printf("out %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", offsetof(cph_ordered, nrows), offsetof(cph_ordered, ids), '
                   "offsetof(cph_ordered, mem), offsetof(cph_ordered, select_used), offsetof(cph_ordered, candidates), offsetof(cph_ordered, nerrors), "
                   "offsetof(cph_ordered, first_error_row), offsetof(cph_ordered, first_error_kind), offsetof(cph_ordered, first_error_key));"
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    nums = [[int(x) for x in re.findall(r"\d+", line)] for line in out.splitlines()]
    K, R = N.cph_order_key, N.cph_ordered
    assert nums[0] == [C.sizeof(K), C.sizeof(R), N.CPH_ORDER_MAX_KEYS]
    assert nums[1] == [getattr(K, f).offset for f in ("kind", "descending", "values", "status", "values_mem", "index")]
    assert nums[2] == [getattr(R, f).offset for f in ("nrows", "ids", "mem", "select_used", "candidates", "nerrors", "first_error_row",
                                                      "first_error_kind", "first_error_key")]
