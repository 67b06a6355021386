"""Broker-side reduce for the filter -> aggregation / group-by path.

Mirrors the final steps the reference applies after the server-side combine:

* ``AggregationFunction.extractFinalResult`` -- COUNT -> long, SUM/MIN/MAX -> double,
  DISTINCTCOUNTHLL -> ``HyperLogLog.cardinality()`` (DistinctCountHLLAggregationFunction.java:362-364),
  DISTINCTCOUNT -> the value set's size as int (DistinctCountAggregationFunction.java:61-68),
  PERCENTILE -> element (int)(n * p / 100) of the sorted values (PercentileAggregationFunction.java:146-158),
  VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP -> m2 / count or m2 / (count - 1), its square root for STDDEV
  (VarianceAggregationFunction.java:228-248),
  COVARPOP / COVARSAMP -> sumXY / count - sumX sumY / (count count), or its sample form
  (CovarianceAggregationFunction.java:185-201),
  SKEWNESS / KURTOSIS -> commons-math 3's Skewness / Kurtosis over the merged PinotFourthMoment (restated from their
  published form: parity unpinned).
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

from .query import (COUNT, COVARIANCE_AGGREGATIONS, COVARSAMP, DISTINCTCOUNT, DISTINCTCOUNTHLL,
                    FIRSTWITHTIME, FOURTHMOMENT_AGGREGATIONS, HISTOGRAM, LASTWITHTIME, MAX, MIN, PERCENTILE, SKEWNESS,
                    STDDEVPOP, STDDEVSAMP, SUM, VARIANCE_AGGREGATIONS, VARSAMP, WITHTIME_AGGREGATIONS, QueryContext)


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


def variance_merge(a, b) -> tuple:
    """VarianceTuple.apply(VarianceTuple) (VarianceTuple.java:46-55) on (count, sum, m2) tuples, in its order of
    operations: ``b`` merged into ``a``; a zero count on either side adds nothing."""
    (n1, s1, m1), (n2, s2, m2) = a, b
    if n2 == 0:
        return (int(n1), float(s1), float(m1))
    avg = 0.0 if n1 == 0 else float(s1) / float(n1)
    delta = float(s2) / float(n2) - avg
    return (int(n1) + int(n2), float(s1) + float(s2),
            float(m1) + (float(m2) + delta * delta * float(n2) * float(n1) / float(int(n2) + int(n1))))


def variance_final(t, function: str) -> float:
    """VarianceAggregationFunction.extractFinalResult (:228-248): -Infinity for count 0 and for a sample function with
    count 1, else m2 / count (population) or m2 / (count - 1) (sample), its square root for the STDDEV functions."""
    n, _, m2 = t
    sample = function in (VARSAMP, STDDEVSAMP)
    if n == 0 or (sample and n == 1):
        return float("-inf")
    v = float(m2) / float(n - 1 if sample else n)
    return math.sqrt(v) if function in (STDDEVPOP, STDDEVSAMP) else v


def variance_serialize(t) -> bytes:
    """VarianceTuple.toBytes (VarianceTuple.java:69-75): long count, double sum, double m2, big-endian."""
    return struct.pack(">qdd", int(t[0]), float(t[1]), float(t[2]))


def covariance_merge(a, b) -> tuple:
    """CovarianceTuple.apply(CovarianceTuple) on (sum_x, sum_y, sum_xy, count) tuples: the components add."""
    return (float(a[0]) + float(b[0]), float(a[1]) + float(b[1]), float(a[2]) + float(b[2]), int(a[3]) + int(b[3]))


def covariance_final(t, function: str) -> float:
    """CovarianceAggregationFunction.extractFinalResult (:185-201), in its order of operations (the counts multiply as
    integers before they divide): -Infinity for count 0 and for the sample function with count 1."""
    sum_x, sum_y, sum_xy, count = float(t[0]), float(t[1]), float(t[2]), int(t[3])
    if count == 0:
        return float("-inf")
    if function == COVARSAMP:
        if count - 1 == 0:
            return float("-inf")
        return (sum_xy / float(count - 1)) - (sum_x * sum_y) / float(count * (count - 1))
    return (sum_xy / float(count)) - (sum_x * sum_y) / float(count * count)


def covariance_serialize(t) -> bytes:
    """CovarianceTuple.toBytes: double sumX, double sumY, double sumXY, long count, big-endian, 32 bytes."""
    return struct.pack(">dddq", float(t[0]), float(t[1]), float(t[2]), int(t[3]))


def fourthmoment_merge(a, b) -> tuple:
    """PinotFourthMoment.combine (PinotFourthMoment.java:55-97) on (n, m1, m2, m3, m4) tuples, in its order of
    operations (Java multiplies a double by a long in double, left to right; n * n is a long product)."""
    an, am1, am2, am3, am4 = int(a[0]), float(a[1]), float(a[2]), float(a[3]), float(a[4])
    bn, bm1, bm2, bm3, bm4 = int(b[0]), float(b[1]), float(b[2]), float(b[3]), float(b[4])
    if bn == 0:
        return (an, am1, am2, am3, am4)
    if an == 0:
        return (bn, bm1, bm2, bm3, bm4)
    n = an + bn
    fa, fb, fn = float(an), float(bn), float(n)
    m1 = (fa * am1 + fb * bm1) / fn
    delta = bm1 - am1
    delta2 = delta * delta
    m2 = am2 + bm2 + delta2 * fa * fb / fn
    delta3 = delta2 * delta
    m3 = am3 + bm3 + delta3 * fa * fb * float(an - bn) / float(n * n) + 3.0 * delta * (fa * bm2 - fb * am2) / fn
    delta4 = delta3 * delta
    n3 = fn * fn * fn
    m4 = (am4 + bm4 + delta4 * fa * fb * float(an * an - an * bn + bn * bn) / n3
          + 6.0 * delta2 * (float(an * an) * bm2 + float(bn * bn) * am2) / float(n * n)
          + 4.0 * delta * (fa * bm3 - fb * am3) / fn)
    return (n, m1, m2, m3, m4)


def fourthmoment_final(t, function: str) -> float:
    """commons-math 3's Skewness.getResult / Kurtosis.getResult over the moment, restated from their published form:
    with v = m2 / (n - 1), skewness is NaN for n < 3, 0.0 when v < 10E-20, else n m3 / ((n - 1)(n - 2) sqrt(v) v);
    kurtosis is NaN for n <= 3, 0.0 when v < 10E-20, else (n (n + 1) m4 - 3 m2^2 (n - 1)) / ((n - 1)(n - 2)(n - 3) v^2)."""
    n, m2, m3, m4 = int(t[0]), float(t[2]), float(t[3]), float(t[4])
    if n < 3 or (function != SKEWNESS and n <= 3):
        return float("nan")
    n0 = float(n)
    v = m2 / (n0 - 1.0)
    if v < 10E-20:
        return 0.0
    if function == SKEWNESS:
        return (n0 * m3) / ((n0 - 1.0) * (n0 - 2.0) * math.sqrt(v) * v)
    return (n0 * (n0 + 1.0) * m4 - 3.0 * m2 * m2 * (n0 - 1.0)) / ((n0 - 1.0) * (n0 - 2.0) * (n0 - 3.0) * v * v)


def fourthmoment_serialize(t) -> bytes:
    """PinotFourthMoment.serialize (:107-115): long n, double m1, m2, m3, m4, big-endian, 40 bytes."""
    return struct.pack(">qdddd", int(t[0]), float(t[1]), float(t[2]), float(t[3]), float(t[4]))


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
    if function == HISTOGRAM:  # DoubleVectorOpUtils.vectorAdd (HistogramAggregationFunction.merge :174-177)
        return tuple(float(x) + float(y) for x, y in zip(a, b))
    # (value, time) pairs: the first argument is kept on equal times (LastWithTimeAggregationFunction.merge :200-206,
    # FirstWithTimeAggregationFunction.merge :199-205)
    if function == LASTWITHTIME:
        return a if a[1] >= b[1] else b
    if function == FIRSTWITHTIME:
        return a if a[1] <= b[1] else b
    if function in VARIANCE_AGGREGATIONS:
        return variance_merge(a, b)
    if function in COVARIANCE_AGGREGATIONS:
        return covariance_merge(a, b)
    if function in FOURTHMOMENT_AGGREGATIONS:
        return fourthmoment_merge(a, b)
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
    if spec.function == HISTOGRAM:  # DOUBLE_ARRAY: the list of doubles (extractFinalResult returns the list)
        return [float(x) for x in value]
    if spec.function in WITHTIME_AGGREGATIONS:  # extractFinalResult: the pair's value, in the declared type
        return int(value[0]) if spec.data_type in ("INT", "LONG") else float(value[0])
    if spec.function in VARIANCE_AGGREGATIONS:
        return variance_final(value, spec.function)
    if spec.function in COVARIANCE_AGGREGATIONS:
        return covariance_final(value, spec.function)
    if spec.function in FOURTHMOMENT_AGGREGATIONS:
        return fourthmoment_final(value, spec.function)
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
