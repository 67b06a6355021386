"""FIRSTWITHTIME / LASTWITHTIME without a GPU: the parser's spellings, result column names and argument errors
(AggregationFunctionFactory.java:201-254), the DataTable pair objects 27-30 against bytes written out by hand from the
toBytes() layouts, and the merge's tie rule."""
import math
import struct

import pytest

from pinot_amd.datatable import pair_deserialize, pair_serialize
from pinot_amd.query import FIRSTWITHTIME, LASTWITHTIME, SqlParseError, parse_sql
from pinot_amd.reduce import final_value, merge_intermediate


@pytest.mark.parametrize("spelling,function", [
    ("LASTWITHTIME", LASTWITHTIME), ("last_with_time", LASTWITHTIME), ("LastWithTime", LASTWITHTIME),
    ("lastWithTime", LASTWITHTIME), ("FIRSTWITHTIME", FIRSTWITHTIME), ("first_with_time", FIRSTWITHTIME),
    ("FirstWithTime", FIRSTWITHTIME), ("FIRST_WITH_TIME", FIRSTWITHTIME)])
@pytest.mark.parametrize("literal,declared", [("'LONG'", "LONG"), ("'double'", "DOUBLE"), ("'Int'", "INT"),
                                              ("'FLOAT'", "FLOAT"), ("'boolean'", "BOOLEAN"), ("'string'", "STRING")])
def test_spellings_and_result_column_names(spelling, function, literal, declared):
    q = parse_sql(f"SELECT {spelling}(x, ts, {literal}), COUNT(*) FROM t GROUP BY g")
    a = q.aggregations[0]
    assert (a.function, a.column, a.column2, a.data_type) == (function, "x", "ts", declared)
    assert q.result_columns()[0] == f"{function.lower()}(x,ts,'{declared}')"


@pytest.mark.parametrize("sql,message", [
    ("SELECT LASTWITHTIME(x, ts) FROM t", "LAST_WITH_TIME expects 3 arguments, got: 2"),
    ("SELECT first_with_time(x) FROM t", "FIRST_WITH_TIME expects 3 arguments, got: 1"),
    ("SELECT LASTWITHTIME(x, ts, 'INT', 4) FROM t", "LAST_WITH_TIME expects 3 arguments, got: 4"),
    ("SELECT LASTWITHTIME(x, ts, y) FROM t", "LAST_WITH_TIME expects the 3rd argument to be literal, got: IDENTIFIER"),
    ("SELECT FIRSTWITHTIME(x, ts, y) FROM t", "firstWithTime\\(dataColumn, timeColumn, 'dataType'\\)"),
    ("SELECT LASTWITHTIME(x, ts, 'BYTES') FROM t", "Unsupported data type for LAST_WITH_TIME: BYTES"),
    ("SELECT LASTWITHTIME(x + y, ts, 'INT') FROM t", "expression argument")])
def test_argument_errors(sql, message):
    with pytest.raises(SqlParseError, match=message):
        parse_sql(sql)


# toBytes(): the value at its own width, then the 8-byte time, big-endian
PAIRS = [
    (27, "INT", (-2, 1 << 40), bytes.fromhex("fffffffe" "0000010000000000")),
    (28, "LONG", (1 << 33, -1), bytes.fromhex("0000000200000000" "ffffffffffffffff")),
    (29, "FLOAT", (1.5, 3), bytes.fromhex("3fc00000" "0000000000000003")),
    (30, "DOUBLE", (-0.25, -(1 << 63)), bytes.fromhex("bfd0000000000000" "8000000000000000"))]


@pytest.mark.parametrize("otype,declared,pair,raw", PAIRS, ids=[p[1] for p in PAIRS])
def test_pair_objects_against_hand_written_bytes(otype, declared, pair, raw):
    assert pair_serialize(declared, pair) == raw
    assert pair_deserialize(otype, raw) == pair
    with pytest.raises(ValueError):
        pair_deserialize(otype, raw + b"\0")


def test_the_float_default_is_nan_on_the_wire():
    assert math.isnan(pair_deserialize(29, struct.pack(">fq", float("nan"), -(1 << 63)))[0])


@pytest.mark.parametrize("function,a,b,kept", [
    (LASTWITHTIME, (1, 5), (2, 5), (1, 5)), (LASTWITHTIME, (1, 4), (2, 5), (2, 5)), (LASTWITHTIME, (1, 6), (2, 5), (1, 6)),
    (FIRSTWITHTIME, (1, 5), (2, 5), (1, 5)), (FIRSTWITHTIME, (1, 4), (2, 5), (1, 4)), (FIRSTWITHTIME, (1, 6), (2, 5), (2, 5))])
def test_merge_keeps_its_first_argument_on_equal_times(function, a, b, kept):
    assert merge_intermediate(function, a, b) == kept


def test_final_is_the_value_in_the_declared_type():
    q = parse_sql("SELECT LASTWITHTIME(x, ts, 'LONG'), FIRSTWITHTIME(y, ts, 'FLOAT') FROM t")
    assert final_value(q.aggregations[0], (1 << 40, 7)) == 1 << 40
    assert final_value(q.aggregations[1], (0.5, 7)) == 0.5
