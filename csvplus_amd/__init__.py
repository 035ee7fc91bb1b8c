"""csvplus_amd — MI355X (gfx950) implementation of csvplus's Index-build + Join hot path.

The product is the C-ABI library `lib/libcsvplus_hip.so` (hand-written HIP kernels,
include/csvplus_hip.h).  This package is its Python host side: the ctypes binding,
the SoA column staging and the multi-GPU sharding.  There is no CPU fallback.

Modules: `engine` (one GPU: index_on / join / chained_join on torch device memory), `dist` (probe-row sharding +
allgatherv over RCCL), `streaming` (host -> device pipeline of join chunks), `ingest` (CSV text -> columns),
`materialize` (gather through row ids, ToCsv, ToJSON, Filter / TakeWhile / DropWhile over `predicates`: Like, All, Any,
Not, IntCmp, FloatCmp as plain data; ValueAsInt / ValueAsFloat64 for a whole column: to_int / to_float), `dedup` (ResolveDuplicates over the device index: a callback over the groups, or a named rule — First, Last, DropAll,
MinBy, MaxBy — resolved on the device: resolve_duplicates_device),
`aggregate` (Totals per key of an index on the device — Sum, Min, Max as plain data: totals; the contract in pure Python:
totals_model),
`mapping` (Map as row templates — Format, Col, Int, Float, Const — for computed columns: materialize.map_column; Validate:
materialize.validate_rows),
`expr` (numeric expressions as plain data — IntCol, FloatCol, IntArr, FloatArr, ToFloat, ToInt and + - * / % with Go's
arithmetic — evaluated per row on the device: materialize.eval_number, mapping.Float.of / Int.of, aggregate.Sum(expr)),
`ordering` (OrderBy as plain data — Asc, Desc over int / float / bytes keys — sorted on the device with Top-N select:
materialize.order_rows; the contract in pure Python: order_model),
`pipeline` (CSV -> indices -> chained join -> CSV or JSON, all in HBM), `datagen` (deterministic synthetic tables).
"""
from . import _native as native  # noqa: F401
from ._native import CphError, NativeLibraryMissing, Context, DeviceIndex, Matches, Chain, join_chain  # noqa: F401
from .columns import StrCol  # noqa: F401
from .predicates import Like, All, Any, Not, IntCmp, FloatCmp, TimeCmp, ExprCmp, ColCmp  # noqa: F401

__all__ = ["native", "CphError", "NativeLibraryMissing", "Context", "DeviceIndex", "Matches", "Chain", "join_chain", "StrCol",
           "Like", "All", "Any", "Not", "IntCmp", "FloatCmp", "TimeCmp", "ExprCmp", "ColCmp"]
