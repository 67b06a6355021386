"""Broker-side reduce for the filter -> aggregation / group-by path.

Mirrors the final steps the reference applies after the server-side combine:

* ``AggregationFunction.extractFinalResult`` -- COUNT -> long, SUM/MIN/MAX -> double,
  DISTINCTCOUNTHLL -> ``HyperLogLog.cardinality()`` (DistinctCountHLLAggregationFunction.java:362-364),
  DISTINCTCOUNT -> the value set's size as int (DistinctCountAggregationFunction.java:61-68),
  PERCENTILE -> element (int)(n * p / 100) of the sorted values (PercentileAggregationFunction.java:146-158).
* ``IndexedTable.finish`` / ``GroupByDataTableReducer.reduceAndSetResults`` -- ORDER BY over group-by
  columns and aggregations (ASC/DESC), then LIMIT (core/data/table/IndexedTable.java:148-173,
  core/query/reduce/GroupByDataTableReducer.java:99).
* Aggregation-only queries produce exactly one row (AggregationDataTableReducer).

A group-by query without ORDER BY returns an arbitrary subset in the reference; here groups are
returned in key order so results are deterministic.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import Any, List, Sequence

import numpy as np

from .query import COUNT, DISTINCTCOUNT, DISTINCTCOUNTHLL, MAX, MIN, PERCENTILE, SUM, QueryContext


def _java_round(x: float) -> int:
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return (1 << 63) - 1 if x > 0 else -(1 << 63)
    return int(math.floor(x + 0.5))


def hll_cardinality(registers: np.ndarray, log2m: int) -> int:
    """clearspring HyperLogLog.cardinality() (stream 2.7.0) over raw 1-byte registers."""
    m = 1 << log2m
    reg = np.asarray(registers, dtype=np.int64)
    assert reg.shape[-1] == m
    s = float(np.sum(1.0 / np.left_shift(np.int64(1), reg).astype(np.float64)))
    zeros = float(np.sum(reg == 0))
    if log2m == 4:
        alpha_mm = 0.673 * m * m
    elif log2m == 5:
        alpha_mm = 0.697 * m * m
    elif log2m == 6:
        alpha_mm = 0.709 * m * m
    else:
        alpha_mm = (0.7213 / (1 + 1.079 / m)) * m * m
    estimate = alpha_mm * (1 / s)
    if estimate <= (5.0 / 2.0) * m:
        return _java_round(m * math.log(m / zeros)) if zeros > 0 else (1 << 63) - 1
    return _java_round(estimate)


def hll_serialize(registers: np.ndarray, log2m: int) -> bytes:
    """ObjectSerDeUtils HyperLogLog serializer: int32 BE log2m, int32 BE byte size, then the clearspring
    RegisterSet words (6 x 5-bit registers per int, register i at word i/6, shift 5*(i%6)), BE
    (ObjectSerDeUtils.java:535-560, HyperLogLogUtils.java:28-43)."""
    m = 1 << log2m
    nwords = m // 6 + 1
    regs = np.zeros(nwords * 6, dtype=np.uint32)
    regs[:m] = np.asarray(registers[:m], dtype=np.uint32) & 0x1F
    words = (regs.reshape(nwords, 6) << (5 * np.arange(6, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    return (np.array([log2m, 4 * nwords], dtype=">i4").tobytes() + words.astype(">u4").tobytes())


def set_serialize(values, data_type: str) -> bytes:
    """ObjectSerDeUtils value-set serializers (IntSet / LongSet / FloatSet / DoubleSet / StringSet,
    ObjectSerDeUtils.java:725-891): int32 BE size, then the values big-endian (strings: int32 BE length + UTF-8).
    Values are written ascending; the reference writes its fastutil set's iteration order and its deserializers
    read any order, so this is the same set, not the same bytes."""
    vals = sorted(values)
    head = np.array([len(vals)], dtype=">i4").tobytes()
    if data_type == "STRING":
        enc = [str(v).encode("utf-8") for v in vals]
        return head + b"".join(np.array([len(e)], dtype=">i4").tobytes() + e for e in enc)
    dt = {"INT": ">i4", "LONG": ">i8", "FLOAT": ">f4", "DOUBLE": ">f8"}[data_type]
    return head + np.asarray(vals, dtype=dt).tobytes()


@dataclass(frozen=True, eq=False)
class ValueCounts:
    """A PERCENTILE intermediate result: the reference's DoubleArrayList of matched values
    (PercentileAggregationFunction.java:77-94) as a multiset -- the distinct doubles ascending and how often each
    occurs.  Partial results of different calls have different dictionaries, so they merge by value."""
    values: np.ndarray  # float64, ascending, distinct
    counts: np.ndarray  # int64, the same length

    @staticmethod
    def of(values, counts=None) -> "ValueCounts":
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        c = np.ones(len(v), np.int64) if counts is None else np.asarray(counts, dtype=np.int64).reshape(-1)
        keep = c > 0
        u, inv = np.unique(v[keep], return_inverse=True)
        total = np.zeros(len(u), np.int64)
        np.add.at(total, inv.reshape(-1), c[keep])
        return ValueCounts(u, total)

    def merge(self, other: "ValueCounts") -> "ValueCounts":  # DoubleArrayList.addAll
        return ValueCounts.of(np.concatenate([self.values, other.values]), np.concatenate([self.counts, other.counts]))

    @property
    def size(self) -> int:
        return int(self.counts.sum())

    def sorted_values(self) -> np.ndarray:
        return np.repeat(self.values, self.counts)

    def __eq__(self, other):
        return (isinstance(other, ValueCounts) and np.array_equal(self.values, other.values)
                and np.array_equal(self.counts, other.counts))


def percentile_final(vc: ValueCounts, percentile: float) -> float:
    """PercentileAggregationFunction.extractFinalResult (:146-158): -inf for an empty list; the largest value for
    p = 100; else the element of rank (int)((long) size * p / 100) -- double arithmetic, truncated -- in ascending
    order (clamped to size - 1)."""
    n = vc.size
    if n == 0:
        return float("-inf")
    if percentile == 100:
        return float(vc.values[-1])
    rank = min(n - 1, max(0, int(float(n) * float(percentile) / 100.0)))
    return float(vc.values[int(np.searchsorted(np.cumsum(vc.counts), rank, side="right"))])


def double_list_serialize(vc: ValueCounts) -> bytes:
    """ObjectSerDeUtils DoubleArrayList serializer (ObjectSerDeUtils.java:328-357): int32 BE size, then the doubles
    BE.  Values are written ascending; the reference writes arrival order and sorts at the broker."""
    return np.array([vc.size], dtype=">i4").tobytes() + vc.sorted_values().astype(">f8").tobytes()


def _double_compare_key(x) -> int:
    """An int whose order is Double.compare's (NaN largest, -0.0 < 0.0)."""
    x = float(x)
    if x != x:
        return 0x7FF8000000000000
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFFFFFFFFFF


def math_min(a, b) -> float:
    """Java's Math.min: a NaN operand gives NaN, -0.0 is below 0.0 (Python's min keeps whichever came first)."""
    if a != a or b != b:
        return float("nan")
    return b if _double_compare_key(b) < _double_compare_key(a) else a


def math_max(a, b) -> float:
    if a != a or b != b:
        return float("nan")
    return b if _double_compare_key(b) > _double_compare_key(a) else a


def merge_intermediate(function: str, a, b):
    """AggregationFunction.merge of two intermediate results of one group: COUNT / SUM add, MIN / MAX, HyperLogLog
    registers max, DISTINCTCOUNT value sets union (by value: the partial results' dictionaries may differ)."""
    if function == COUNT:
        return int(a) + int(b)
    if function == SUM:
        # the intermediate result of SUM is a double (SumAggregationFunction.merge); an integer-typed partial (numpy
        # int64) would wrap where the doubles do not: 3 x 2^62 + 2^62 is 2^64, not 0
        return float(a) + float(b)
    if function == MIN:
        return math_min(a, b)
    if function == MAX:
        return math_max(a, b)
    if function == DISTINCTCOUNT:
        return frozenset(a) | frozenset(b)
    if function == PERCENTILE:
        return a.merge(b)
    return np.maximum(a, b)  # HyperLogLog.addAll


@dataclass
class ResultTable:
    columns: List[str]
    rows: List[List[Any]]

    def __repr__(self):
        return f"ResultTable({self.columns}, {self.rows[:5]}{'...' if len(self.rows) > 5 else ''})"


def final_value(spec, value):
    if spec.function == COUNT:
        return int(value)
    if spec.function == DISTINCTCOUNTHLL:
        return hll_cardinality(value, spec.log2m)
    if spec.function == DISTINCTCOUNT:
        return len(value)
    if spec.function == PERCENTILE:
        return percentile_final(value, spec.percentile)
    return float(value)


def reduce_groups(q: QueryContext, keys: Sequence[tuple], aggs: Sequence[Sequence[Any]]) -> ResultTable:
    """keys[i]: tuple of group-by values of group i; aggs[i][k]: intermediate result of
    aggregation k (COUNT int, SUM/MIN/MAX float, HLL register array, DISTINCTCOUNT value set)."""
    finals = [[final_value(q.aggregations[k], a[k]) for k in range(len(q.aggregations))] for a in aggs]
    idx = list(range(len(keys)))
    if q.group_by:
        # deterministic base order: keys ascending
        idx.sort(key=lambda i: keys[i])
        for ob in reversed(q.order_by):
            if ob.kind == "column":
                c = q.group_by.index(ob.ref)
                idx.sort(key=lambda i, c=c: keys[i][c], reverse=not ob.asc)
            else:
                # Double.compare order: a NaN would make Python's comparison sort inconsistent
                idx.sort(key=lambda i, k=ob.ref: (_double_compare_key(finals[i][k]) if isinstance(finals[i][k], float)
                                                   else finals[i][k]), reverse=not ob.asc)
        idx = idx[: q.limit]
    rows = []
    for i in idx:
        row = []
        for s in q.select:
            if s.kind == "column":
                row.append(keys[i][q.group_by.index(s.ref)])
            else:
                row.append(finals[i][s.ref])
        rows.append(row)
    return ResultTable(q.result_columns(), rows)
