"""SKEWNESS / KURTOSIS above the C ABI, no GPU: SQL names, the broker's PinotFourthMoment merge and the two finals
against the reference's recorded outputs (tests/golden/fourthmoment_kat.json), and the DataTable payload."""
import json
import math
import os
import struct

import pytest

from pinot_amd.datatable import FOURTHMOMENT_OBJECT_TYPE, DataTable, fourthmoment_deserialize, reduce_datatables
from pinot_amd.query import SqlParseError, parse_sql
from pinot_amd.reduce import fourthmoment_final, fourthmoment_serialize, merge_intermediate
from tests.moments4_ref import exact_tuple

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fourthmoment_kat.json")))
KAT_VALUES = [row[2] for row in KAT["inputs"] if row[0] == "a"]
_, KAT_SKEW, KAT_KURT = KAT["grouped_outputs"][0]


def as_tuple(values):
    t = exact_tuple(values)
    return (t[0],) + tuple(float("nan") if c is None else float(c) for c in t[1:])


@pytest.mark.parametrize("sql,function,name", [
    ("SKEWNESS(x)", "SKEWNESS", "skewness(x)"), ("skewness(x)", "SKEWNESS", "skewness(x)"),
    ("KURTOSIS(x)", "KURTOSIS", "kurtosis(x)")])
def test_sql_names(sql, function, name):
    q = parse_sql(f"SELECT {sql}, COUNT(*) FROM t WHERE f < 3 GROUP BY g")
    assert [a.function for a in q.aggregations] == [function, "COUNT"]
    assert q.aggregations[0].column == "x" and q.result_columns() == [name, "count(*)"]


@pytest.mark.parametrize("sql", ["SKEWNESS(x, 2)", "SKEWNESS(*)", "FOURTHMOMENT(x)"])
def test_sql_rejects(sql):
    with pytest.raises(SqlParseError, match="unsupported function" if sql.startswith("FOURTH") else "SKEWNESS"):
        parse_sql(f"SELECT {sql} FROM t")


@pytest.mark.parametrize("split", [None, 3, 5])
def test_kat_finals(split):
    t = as_tuple(KAT_VALUES)
    if split is not None:  # two servers' tuples through PinotFourthMoment.combine
        t = merge_intermediate("SKEWNESS", as_tuple(KAT_VALUES[:split]), as_tuple(KAT_VALUES[split:]))
    assert t[0] == len(KAT_VALUES)
    assert fourthmoment_final(t, "SKEWNESS") == pytest.approx(KAT_SKEW, rel=1e-12, abs=0)
    assert fourthmoment_final(t, "KURTOSIS") == pytest.approx(KAT_KURT, rel=1e-12, abs=0)


@pytest.mark.parametrize("values,skew_nan,kurt_nan", [
    ([], True, True), ([5], True, True), ([5, 6], True, True), ([5, 6, 8], False, True)])
def test_special_cases(values, skew_nan, kurt_nan):
    t = as_tuple(values)
    assert math.isnan(fourthmoment_final(t, "SKEWNESS")) == skew_nan
    assert math.isnan(fourthmoment_final(t, "KURTOSIS")) == kurt_nan
    both = merge_intermediate("KURTOSIS", as_tuple([]), t)  # an empty side leaves the other as it is
    assert both[0] == t[0] and all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(both[1:], t[1:]))


def test_equal_values_give_zero():
    t = as_tuple([7, 7, 7, 7])
    assert t == (4, 7.0, 0.0, 0.0, 0.0)
    assert fourthmoment_final(t, "SKEWNESS") == 0.0 and fourthmoment_final(t, "KURTOSIS") == 0.0


def test_datatable_payload():
    t = (5, -12.5, 1e-3, -2.5, 1e9)
    payload = fourthmoment_serialize(t)
    assert struct.pack(">i", FOURTHMOMENT_OBJECT_TYPE) + payload == struct.pack(">iqdddd", 34, *t)
    assert fourthmoment_deserialize(payload) == t
    with pytest.raises(ValueError):
        fourthmoment_deserialize(payload[:-1])
    # two servers' tables through the broker merge
    q = parse_sql("SELECT g, SKEWNESS(x), KURTOSIS(x) FROM t GROUP BY g ORDER BY g")
    tabs = [DataTable(["g", "skewness(x)", "kurtosis(x)"], ["INT", "OBJECT", "OBJECT"],
                      [[1, (34, fourthmoment_serialize(as_tuple(v))), (34, fourthmoment_serialize(as_tuple(v)))]])
            for v in (KAT_VALUES[:3], KAT_VALUES[3:])]
    (row,) = reduce_datatables(q, tabs).rows
    assert row[0] == 1 and row[1:] == pytest.approx([KAT_SKEW, KAT_KURT], rel=1e-12, abs=0)
    (row,) = reduce_datatables(parse_sql("SELECT SKEWNESS(x) FROM t"), []).rows
    assert math.isnan(row[0])
