"""The Python binding's shared plumbing (csvplus_amd/_native.py), on the CPU: the row-id marshaller fill_rowsel, the
number-array marshaller number_source and the result owner Owned.  Only ctypes structures and a counting stand-in for the
library are used: nothing here loads libcsvplus_hip.so."""
import ctypes as C
import gc
import weakref

import numpy as np
import pytest

from csvplus_amd import _native as N
from csvplus_amd import expr as E
from csvplus_amd import mapping as M
from csvplus_amd.columns import StrCol

HOST, DEVICE = N.CPH_MEM_HOST, N.CPH_MEM_DEVICE
INT, FLT = N.CPH_NUM_INT64, N.CPH_NUM_FLOAT64


def held(keep, address):
    """The numpy array of `keep` that starts at `address`."""
    found = [k for k in keep if isinstance(k, np.ndarray) and k.size and k.ctypes.data == address]
    assert len(found) == 1
    return found[0]


# ---- fill_rowsel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, bits", [(np.uint32, 32), (np.uint64, 64), (np.int64, 32)])
@pytest.mark.parametrize("base", [None, 7])
def test_fill_rowsel_host_forms(dtype, bits, base):
    """numpy ids and (numpy ids, base): uint64 stays, everything else is converted to uint32; the array the structure points
    at is the one `keep` holds."""
    ids = np.array([9, 7, 8], dtype=dtype)
    sel, keep = N.cph_rowsel(), []
    sel.base = 99   # a stale value must not survive
    assert N.fill_rowsel(sel, ids if base is None else (ids, base), keep) == 3
    assert (sel.bits, sel.base) == (bits, base or 0)
    arr = held(keep, sel.ids)
    assert arr.dtype == (np.uint64 if bits == 64 else np.uint32) and arr.tolist() == [9, 7, 8]
    assert arr.flags.c_contiguous


def test_fill_rowsel_takes_a_strided_host_array():
    ids = np.arange(10, dtype=np.uint64)[::3]
    sel, keep = N.cph_rowsel(), []
    assert N.fill_rowsel(sel, ids, keep) == 4
    assert sel.bits == 64 and held(keep, sel.ids).tolist() == [0, 3, 6, 9]


@pytest.mark.parametrize("dtype, bits", [(np.uint32, 32), (np.uint64, 64), (np.int64, 32)])
@pytest.mark.parametrize("base", [None, 5])
def test_fill_rowsel_empty_host_array(dtype, bits, base):
    ids = np.zeros(0, dtype=dtype)
    sel, keep = N.cph_rowsel(), []
    assert N.fill_rowsel(sel, ids if base is None else (ids, base), keep) == 0
    assert sel.ids is None and (sel.bits, sel.base) == (bits, base or 0)
    assert len(keep) == 1 and keep[0].size == 0


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("base", [None, 11])
def test_fill_rowsel_device_form(bits, base):
    """(device_ptr, bits, count[, base]) is passed through; nothing is kept, which is how take_rows tells the forms apart."""
    form = (0x7F0000001000, bits, 42) if base is None else (0x7F0000001000, bits, 42, base)
    sel, keep = N.cph_rowsel(), []
    sel.base = 99
    assert N.fill_rowsel(sel, form, keep) == 42
    assert (sel.ids, sel.bits, sel.base) == (0x7F0000001000, bits, base or 0)
    assert keep == []
    assert N.fill_rowsel(sel, (0, bits, 0), keep) == 0 and sel.ids is None   # a NULL device pointer stays NULL


def test_cols_array_keeps_what_it_points_into():
    cols = [StrCol.from_values([b"a", b"bc"]), StrCol.from_values([b"xyz", b""])]
    keep = []
    arr = N.cols_array(cols, keep)
    assert len(arr) == 2 and [int(arr[i].nrows) for i in range(2)] == [2, 2]
    assert any(k is arr for k in keep)
    for i, c in enumerate(cols):
        assert any(isinstance(k, tuple) and k[0].ctypes.data == arr[i].data for k in keep)
        assert (arr[i].offset_bits, arr[i].mem, arr[i].fixed_width) == (c.offset_bits, HOST, c.fixed_width)
    one, kept = N._cols_array(cols[:1])   # the same with a keep list of its own
    assert len(one) == 1 and one[0].data == arr[0].data and any(k is one for k in kept)


# ---- number_source -------------------------------------------------------------------------------------------------------
class FakeTensor:
    def __init__(self, n, dtype="torch.int64", is_cuda=True, ptr=0x7F0000002000):
        self.n, self.dtype, self.is_cuda, self.ptr = n, dtype, is_cuda, ptr

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


SHORT = "Asc: {count} values for {need} rows"


def test_number_source_host_arrays():
    keep = []
    a = np.array([3, -1, 2], dtype=np.int64)
    ptr, mem = N.number_source(a, INT, 3, SHORT, keep)
    assert mem == HOST and ptr == a.ctypes.data and np.shares_memory(held(keep, ptr), a)   # passed as it is, and held
    ptr, mem = N.number_source([1.5, 2, -0.25], FLT, 2, SHORT, keep)       # a Python list becomes float64
    v = held(keep, ptr)
    assert mem == HOST and v.dtype == np.float64 and v.tolist() == [1.5, 2.0, -0.25]
    ptr, mem = N.number_source(np.arange(6, dtype=np.int32).reshape(2, 3), INT, 6, SHORT, keep)   # converted, flattened
    assert held(keep, ptr).dtype == np.int64 and held(keep, ptr).tolist() == [0, 1, 2, 3, 4, 5]


def test_number_source_empty_host_array_and_its_stand_in():
    keep = []
    assert N.number_source(np.zeros(0, np.int64), INT, 0, SHORT, keep) == (None, HOST)
    ptr, mem = N.number_source(np.zeros(0, np.float64), FLT, 0, SHORT, keep, stand_in=True)
    v = held(keep, ptr)
    assert mem == HOST and v.dtype == np.float64 and v.tolist() == [0.0]
    with pytest.raises(ValueError, match="^Asc: 0 values for 1 rows$"):    # the stand-in does not count as a value
        N.number_source([], INT, 1, SHORT, keep, stand_in=True)
    a = np.array([5], dtype=np.int64)
    assert N.number_source(a, INT, 1, SHORT, keep, stand_in=True) == (a.ctypes.data, HOST)


def test_number_source_device_pair_and_tensor():
    keep = []
    assert N.number_source((0x7F0000003000, 10), FLT, 10, SHORT, keep) == (0x7F0000003000, DEVICE)
    assert N.number_source((0, 0), INT, 0, SHORT, keep) == (None, DEVICE)
    assert keep == []
    t = FakeTensor(4)
    assert N.number_source(t, INT, 4, SHORT, keep) == (t.ptr, DEVICE) and keep == [t]
    assert N.number_source(FakeTensor(2, "torch.float64"), FLT, 2, SHORT, keep)[1] == DEVICE


def test_number_source_tensor_checks():
    """One stand-in tensor per outcome; the caller's name is what stands in front of the colon of `who`."""
    with pytest.raises(ValueError, match="^Sum: the tensor's dtype is torch.int64, the kind wants float64$"):
        N.number_source(FakeTensor(4), FLT, 4, "Sum: {count} values for {need} joined rows", [])
    with pytest.raises(ValueError, match=r"^Desc: a tensor source must live on the device \(pass \.numpy\(\) for host values\)$"):
        N.number_source(FakeTensor(4, is_cuda=False), INT, 4, "Desc: {count} values for {need} rows", [])
    with pytest.raises(ValueError, match="^Asc: 3 values for 4 rows$"):
        N.number_source(FakeTensor(3), INT, 4, SHORT, [])


def test_number_source_objects_of_expr_and_mapping():
    """IntArr / FloatArr / Int / Float stand for their host array or their device pair."""
    keep = []
    a = E.IntArr([1, 2, 3])
    assert N.number_source(a, INT, 3, SHORT, keep) == (a.values.ctypes.data, HOST) and np.shares_memory(keep[-1], a.values)
    f = M.Float([0.5, 1.5], 2)
    assert N.number_source(f, FLT, 2, SHORT, keep) == (f.values.ctypes.data, HOST)
    assert N.number_source(E.FloatArr.on_device(0x7F0000004000, 8), FLT, 8, SHORT, keep) == (0x7F0000004000, DEVICE)
    assert N.number_source(M.Int.on_device(0, 0), INT, 0, SHORT, keep) == (None, DEVICE)
    assert N.number_source(E.IntArr([]), INT, 0, SHORT, keep) == (None, HOST)


@pytest.mark.parametrize("who, text", [
    ("filter_rows: {src!r} has {count} values for positions 0..{last} of the selection",
     "filter_rows: IntArr(<2 values>) has 2 values for positions 0..4 of the selection"),
    ("eval_number: {src!r} has {count} values for {need} rows", "eval_number: IntArr(<2 values>) has 2 values for 5 rows"),
    ("map_column: an Int part has {count} values for {need} rows", "map_column: an Int part has 2 values for 5 rows"),
    ("Asc: {count} values for {need} rows", "Asc: 2 values for 5 rows"),
    ("Max: {count} values for {need} joined rows", "Max: 2 values for 5 joined rows"),
])
def test_number_source_too_short_raises_the_callers_message(who, text):
    with pytest.raises(ValueError) as e:
        N.number_source(E.IntArr([1, 2]), INT, 5, who, [])
    assert str(e.value) == text
    dev = E.IntArr.on_device(0x7F0000005000, 2)
    with pytest.raises(ValueError) as e:
        N.number_source(dev, INT, 5, who, [])
    assert str(e.value) == text.replace("<2 values>", "<2 values on the device>")


# ---- Owned ---------------------------------------------------------------------------------------------------------------
class FakeLib:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def cph_thing_release(self, ptr):
        self.calls.append(ptr)
        if self.fail:
            raise RuntimeError("the library is gone")


class FakeCtx:
    def __init__(self, lib):
        self.lib, self._children = lib, weakref.WeakSet()


class Thing(N.Owned):
    _release_fn = "cph_thing_release"


def test_owned_releases_once_and_leaves_the_ctx():
    lib = FakeLib()
    ctx = FakeCtx(lib)
    ptr = C.pointer(C.c_int(5))
    t = Thing(ctx, ptr)
    assert (t.ctx, t.lib, t.ptr) == (ctx, lib, ptr) and t in ctx._children
    t.release()
    assert lib.calls == [ptr] and t.ptr is None
    t.release()
    t.close()
    assert lib.calls == [ptr]
    assert N.Owned.close is N.Owned.release and Thing.close is N.Owned.release
    del t
    gc.collect()
    assert lib.calls == [ptr] and len(ctx._children) == 0


def test_owned_is_released_by_the_ctx_and_by_its_death():
    lib = FakeLib()
    ctx = FakeCtx(lib)
    a, b = Thing(ctx, C.pointer(C.c_int(1))), Thing(ctx, C.pointer(C.c_int(2)))
    assert set(ctx._children) == {a, b}
    for child in list(ctx._children):   # what Context.close does
        child.close()
    assert len(lib.calls) == 2 and a.ptr is None and b.ptr is None
    a.release()
    assert len(lib.calls) == 2
    c = Thing(ctx, C.pointer(C.c_int(3)))
    del c
    gc.collect()
    assert len(lib.calls) == 3          # the last reference gives the result back


def test_owned_del_swallows_what_the_library_raises():
    lib = FakeLib(fail=True)
    t = Thing(FakeCtx(lib), C.pointer(C.c_int(1)))
    with pytest.raises(RuntimeError):
        t.release()
    assert t.ptr is None and len(lib.calls) == 1     # not tried again
    u = Thing(FakeCtx(lib), C.pointer(C.c_int(2)))
    u.__del__()                                       # nothing propagates
    assert len(lib.calls) == 2 and u.ptr is None
    N.Owned.__del__(Thing.__new__(Thing))             # an owner whose __init__ never ran


def test_owned_without_a_ctx_and_the_host_tail():
    lib = FakeLib()
    t = Thing(None, C.pointer(C.c_int(7)), lib)       # Matches(lib, ptr) without an index
    assert t.ctx is None and t.lib is lib
    assert t.taken(lambda o: o.ptr.contents.value) == 7 and t.ptr is None and len(lib.calls) == 1
    u = Thing(None, C.pointer(C.c_int(8)), lib)
    with pytest.raises(ZeroDivisionError):
        u.taken(lambda o: 1 // 0)
    assert u.ptr is None and len(lib.calls) == 2      # released although the copy failed


def test_every_result_owner_names_a_release_function_of_the_abi():
    from csvplus_amd import aggregate, dedup, ingest, materialize

    names = {name for name, _, _ in N.PROTOTYPES}
    owners = [N.Chain, N.Gathered, N.Matches, materialize.ColBuf, materialize.DeviceBytes, materialize.RowList, materialize.NumCol,
              materialize.Ordered, ingest.CsvTable, aggregate.Totals, aggregate.JoinTotals, dedup.Resolved]
    for cls in owners:
        assert issubclass(cls, N.Owned) and cls._release_fn in names, cls
        assert "release" not in vars(cls) and "close" not in vars(cls) and "__del__" not in vars(cls), cls
    assert len({cls._release_fn for cls in owners}) == len(owners)
