"""The variance family above the C ABI, no GPU: SQL names, the broker's tuple merge and final results, and the
VarianceTuple payload of the DataTable."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd.datatable import VARIANCE_TUPLE_OBJECT_TYPE, DataTable, reduce_datatables, variance_deserialize
from pinot_amd.query import parse_sql
from pinot_amd.reduce import merge_intermediate, variance_final, variance_serialize
from tests.moments_ref import exact_tuple


@pytest.mark.parametrize("spelling,function,name", [
    ("VAR_POP", "VARPOP", "varpop(x)"), ("VARPOP", "VARPOP", "varpop(x)"), ("var_samp", "VARSAMP", "varsamp(x)"),
    ("StdDev_Pop", "STDDEVPOP", "stddevpop(x)"), ("stddev_samp", "STDDEVSAMP", "stddevsamp(x)")])
def test_sql_names(spelling, function, name):
    q = parse_sql(f"SELECT {spelling}(x), COUNT(*) FROM t WHERE f < 3 GROUP BY g")
    assert [a.function for a in q.aggregations] == [function, "COUNT"]
    assert q.aggregations[0].column == "x" and q.result_columns() == [name, "count(*)"]


def as_tuple(values):
    n, s, m2 = exact_tuple(np.asarray(values, dtype=np.float64))
    return n, float(s), float(m2)


@pytest.mark.parametrize("parts", [
    [[1.0, 2.0, 4.0], [8.0, 16.0]], [[3.5], [3.5, 3.5], [-1.25, 7.0, 9.5]], [[], [5.0, 6.0]], [[5.0, 6.0], []]])
def test_merge_equals_the_tuple_of_the_concatenation(parts):
    got = as_tuple(parts[0])
    for p in parts[1:]:
        got = merge_intermediate("VARPOP", got, as_tuple(p))
    n, s, m2 = exact_tuple(np.asarray([x for p in parts for x in p], dtype=np.float64))
    # (small dyadic values: every step of VarianceTuple.apply is exact or within a few ulps)
    assert got[0] == n and got[1] == float(s) and abs(Fraction(got[2]) - m2) <= Fraction(4, 2 ** 52) * m2


@pytest.mark.parametrize("function,t,want", [
    ("VARPOP", (0, 0.0, 0.0), -math.inf), ("STDDEVSAMP", (0, 0.0, 0.0), -math.inf),
    ("VARPOP", (1, 7.0, 0.0), 0.0), ("STDDEVPOP", (1, 7.0, 0.0), 0.0),
    ("VARSAMP", (1, 7.0, 0.0), -math.inf), ("STDDEVSAMP", (1, 7.0, 0.0), -math.inf),
    ("VARPOP", (4, 10.0, 18.0), 4.5), ("VARSAMP", (4, 10.0, 18.0), 6.0),
    ("STDDEVPOP", (4, 10.0, 18.0), math.sqrt(4.5)), ("STDDEVSAMP", (4, 10.0, 18.0), math.sqrt(6.0))])
def test_final_results(function, t, want):
    assert variance_final(t, function) == want


def test_datatable_payload():
    t = (5, -12.5, 1e-3)
    payload = variance_serialize(t)
    assert struct.pack(">i", VARIANCE_TUPLE_OBJECT_TYPE) + payload == struct.pack(">iqdd", 33, *t)
    assert variance_deserialize(payload) == t
    with pytest.raises(ValueError):
        variance_deserialize(payload[:-1])
    # two servers' tables through the broker merge
    q = parse_sql("SELECT g, VAR_SAMP(x) FROM t GROUP BY g ORDER BY g")
    tabs = [DataTable(["g", "varsamp(x)"], ["INT", "OBJECT"], [[1, (33, variance_serialize(as_tuple(v)))]])
            for v in ([1.0, 2.0], [4.0])]
    assert reduce_datatables(q, tabs).rows == [[1, float(as_tuple([1.0, 2.0, 4.0])[2] / 2)]]
    assert reduce_datatables(parse_sql("SELECT STDDEV_POP(x) FROM t"), []).rows == [[-math.inf]]
