"""COVAR_POP / COVAR_SAMP above the C ABI, no GPU: SQL names, the broker's tuple merge and final results, and the
CovarianceTuple payload of the DataTable."""
import math
import struct

import pytest

from pinot_amd.datatable import COVARIANCE_TUPLE_OBJECT_TYPE, DataTable, covariance_deserialize, reduce_datatables
from pinot_amd.query import SqlParseError, parse_sql
from pinot_amd.reduce import covariance_final, covariance_serialize, merge_intermediate


@pytest.mark.parametrize("spelling,function,name", [
    ("COVAR_POP", "COVARPOP", "covarpop(x,y)"), ("covarpop", "COVARPOP", "covarpop(x,y)"),
    ("CoVar_Samp", "COVARSAMP", "covarsamp(x,y)"), ("COVARSAMP", "COVARSAMP", "covarsamp(x,y)")])
def test_sql_names(spelling, function, name):
    q = parse_sql(f"SELECT {spelling}(x, y), COUNT(*) FROM t WHERE f < 3 GROUP BY g")
    assert [a.function for a in q.aggregations] == [function, "COUNT"]
    a = q.aggregations[0]
    assert (a.column, a.column2, a.op) == ("x", "y", None) and q.result_columns() == [name, "count(*)"]


@pytest.mark.parametrize("call", ["COVAR_POP(x)", "COVAR_SAMP(x, y, z)", "COVAR_POP(x * y, z)", "COVAR_POP(*)"])
def test_argument_count(call):
    with pytest.raises(SqlParseError):
        parse_sql(f"SELECT {call} FROM t")


def test_merge_adds_the_components():
    assert merge_intermediate("COVARPOP", (1.5, -2.0, 8.25, 3), (0.5, 4.0, -0.25, 2)) == (2.0, 2.0, 8.0, 5)
    assert merge_intermediate("COVARSAMP", (0.0, 0.0, 0.0, 0), (7.0, 1.0, 7.0, 1)) == (7.0, 1.0, 7.0, 1)


@pytest.mark.parametrize("function,t,want", [
    ("COVARPOP", (0.0, 0.0, 0.0, 0), -math.inf), ("COVARSAMP", (0.0, 0.0, 0.0, 0), -math.inf),
    ("COVARPOP", (7.0, 3.0, 21.0, 1), 0.0), ("COVARSAMP", (7.0, 3.0, 21.0, 1), -math.inf),
    # the reference's two expressions, written out (CovarianceAggregationFunction.java:199, :201)
    ("COVARPOP", (10.0, 7.0, 33.0, 4), (33.0 / 4) - (10.0 * 7.0) / (4 * 4)),
    ("COVARSAMP", (10.0, 7.0, 33.0, 4), (33.0 / 3) - (10.0 * 7.0) / (4 * 3)),
    ("COVARPOP", (0.1, 0.7, 0.3, 3), (0.3 / 3) - (0.1 * 0.7) / (3 * 3)),
    ("COVARSAMP", (0.1, 0.7, 0.3, 3), (0.3 / 2) - (0.1 * 0.7) / (3 * 2))])
def test_final_results(function, t, want):
    assert covariance_final(t, function) == want


def test_datatable_payload():
    t = (-12.5, 1e-3, 2.0 ** 70, 5)
    payload = covariance_serialize(t)
    assert len(payload) == 32 and COVARIANCE_TUPLE_OBJECT_TYPE == 32
    assert payload == struct.pack(">dddq", *t) and covariance_deserialize(payload) == t
    assert covariance_serialize(covariance_deserialize(payload)) == payload
    with pytest.raises(ValueError):
        covariance_deserialize(payload[:-1])
    # two servers' tables through the broker merge
    q = parse_sql("SELECT g, COVAR_SAMP(x, y) FROM t GROUP BY g ORDER BY g")
    parts = [(3.0, 5.0, 8.0, 2), (4.0, 1.0, 4.0, 1)]
    tabs = [DataTable(["g", "covarsamp(x,y)"], ["INT", "OBJECT"], [[1, (32, covariance_serialize(p))]]) for p in parts]
    assert reduce_datatables(q, tabs).rows == [[1, covariance_final((7.0, 6.0, 12.0, 3), "COVARSAMP")]]
    assert reduce_datatables(parse_sql("SELECT COVAR_POP(x, y) FROM t"), []).rows == [[-math.inf]]
