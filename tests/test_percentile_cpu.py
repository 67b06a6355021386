"""PERCENTILE off the GPU: the SQL subset, the broker reduce (value lists merged by value, the final result element
(int)(n * p / 100) of the sorted list: PercentileAggregationFunction.java:146-158), the DoubleArrayList object
serialisation (ObjectSerDeUtils.java:328-357) and the C-ABI's new symbols in the built library."""
import ctypes
import json
import math
import os
import struct

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import DOUBLE_LIST_OBJECT_TYPE, decode, double_list_deserialize
from pinot_amd.query import PERCENTILE, SUPPORTED_AGGREGATIONS, SqlParseError, parse_sql
from pinot_amd.reduce import (ValueCounts, double_list_serialize, final_value, merge_intermediate, percentile_final,
                              reduce_groups)
from tests import kat_sv

KAT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "percentile_kat.json")


def test_parser_accepts_every_spelling():
    assert PERCENTILE in SUPPORTED_AGGREGATIONS
    q = parse_sql("SELECT g, PERCENTILE(c, 50), percentile(c, 99.9), Percentile(c, '50'), PERCENTILE95(c), "
                  "percentile0(d) AS x, PeRcEnTiLe100(d) FROM t WHERE f > 3 GROUP BY g ORDER BY x DESC")
    got = [(a.function, a.column, a.percentile, a.name_form) for a in q.aggregations]
    # PERCENTILE(c, 50) and PERCENTILE(c, '50') are one aggregation (QueryContext de-duplicates)
    assert got == [(PERCENTILE, "c", 50.0, 0), (PERCENTILE, "c", 99.9, 0), (PERCENTILE, "c", 95.0, 1),
                   (PERCENTILE, "d", 0.0, 1), (PERCENTILE, "d", 100.0, 1)]
    assert [s.ref for s in q.select[1:]] == [0, 1, 0, 2, 3, 4]
    assert q.order_by[0].kind == "aggregation" and q.order_by[0].ref == 3
    # the two spellings of one percentile are two aggregations: their result columns are named differently
    q = parse_sql("SELECT PERCENTILE50(c), PERCENTILE(c, 50) FROM t")
    assert len(q.aggregations) == 2


@pytest.mark.parametrize("sql", [
    "SELECT PERCENTILE(c, 101) FROM t", "SELECT PERCENTILE(c, -1) FROM t", "SELECT PERCENTILE(c, 100.5) FROM t",
    "SELECT PERCENTILE(c, 'x') FROM t", "SELECT PERCENTILE101(c) FROM t", "SELECT PERCENTILE50(c, 50) FROM t",
    "SELECT PERCENTILE(c) FROM t", "SELECT PERCENTILE(*, 50) FROM t", "SELECT PERCENTILE(a * b, 50) FROM t",
    "SELECT PERCENTILE(c, 50, 3) FROM t", "SELECT PERCENTILEEST(c, 50) FROM t", "SELECT PERCENTILETDIGEST95(c) FROM t"])
def test_parser_rejects(sql):
    with pytest.raises(SqlParseError):
        parse_sql(sql)


def test_result_names():
    # PercentileAggregationFunction.getResultColumnName (:60-64): Double.toString of the percentile in the 2-argument form
    names = {"PERCENTILE90(column6)": "percentile90(column6)", "percentile(c, 90)": "percentile(c, 90.0)",
             "PERCENTILE(c, 99.9)": "percentile(c, 99.9)", "PERCENTILE(c, '50')": "percentile(c, 50.0)",
             "PERCENTILE(c, 0)": "percentile(c, 0.0)", "PERCENTILE(c, 0.0001)": "percentile(c, 1.0E-4)",
             "PERCENTILE(c, 12.5)": "percentile(c, 12.5)", "PERCENTILE0(c)": "percentile0(c)"}
    for sql, name in names.items():
        q = parse_sql(f"SELECT {sql} FROM testTable")
        assert q.aggregations[0].result_name() == name
        assert q.result_columns() == [name]


def test_reduce_merges_by_value():
    # two partial results whose dictionaries differ: ids mean different values, the merge is by value
    from pinot_amd.engine import HistogramColumn
    a = HistogramColumn(np.array([[2, 0, 1, 3]], np.uint32), np.array([10, 20, 30, 40], np.int32), np.array([30.0]))
    b = HistogramColumn(np.array([[1, 4, 0]], np.uint32), np.array([20, 25, 50], np.int32), np.array([25.0]))
    va, vb = a.value_counts(0), b.value_counts(0)
    assert va == ValueCounts.of([10, 10, 30, 40, 40, 40]) and vb == ValueCounts.of([20, 25, 25, 25, 25])
    merged = merge_intermediate(PERCENTILE, va, vb)
    assert merged.sorted_values().tolist() == [10, 10, 20, 25, 25, 25, 25, 30, 40, 40, 40] and merged.size == 11
    q = parse_sql("SELECT PERCENTILE50(c), PERCENTILE(c, 90), PERCENTILE100(c) FROM t")
    assert [final_value(s, merged) for s in q.aggregations] == [25.0, 40.0, 40.0]
    assert all(isinstance(final_value(s, merged), float) for s in q.aggregations)
    assert reduce_groups(q, [()], [[merged] * 3]).rows == [[25.0, 40.0, 40.0]]
    q = parse_sql("SELECT g, PERCENTILE50(c) FROM t GROUP BY g ORDER BY PERCENTILE50(c) DESC, g LIMIT 5")
    rows = reduce_groups(q, [("a",), ("b",), ("c",)], [[ValueCounts.of([1])], [ValueCounts.of([1, 2, 3])],
                                                       [ValueCounts.of([5, 6])]]).rows
    assert rows == [["c", 6.0], ["b", 2.0], ["a", 1.0]]


def test_final_value_hand_cases():
    one, two = ValueCounts.of([7]), ValueCounts.of([3, 9])
    for p in (0, 50, 99.9, 100):
        assert percentile_final(one, p) == 7.0
    assert [percentile_final(two, p) for p in (0, 49.9, 50, 99.9, 100)] == [3.0, 3.0, 9.0, 9.0, 9.0]
    four = ValueCounts.of([4, 1, 3, 2])
    assert percentile_final(four, 50) == 3.0  # even n: element n / 2, not an interpolation
    assert percentile_final(four, 0) == 1.0 and percentile_final(four, 100) == 4.0
    assert percentile_final(four, 74.9) == 3.0 and percentile_final(four, 75) == 4.0
    thousand = ValueCounts.of(np.arange(1000))
    assert percentile_final(thousand, 99.9) == 999.0 and percentile_final(thousand, 99.89) == 998.0
    assert percentile_final(ValueCounts.of([]), 50) == -math.inf  # DEFAULT_FINAL_RESULT
    # counts, not only distinct values, decide the rank
    assert percentile_final(ValueCounts.of([1.0, 2.0], [9, 1]), 89.9) == 1.0
    assert percentile_final(ValueCounts.of([1.0, 2.0], [9, 1]), 90) == 2.0
    # a zero count is no value
    assert percentile_final(ValueCounts.of([1.0, 2.0], [3, 0]), 100) == 1.0


@pytest.mark.parametrize("values", [[], [2.5], [3.0, -7.0, 3.0, 1e300, -0.25, 3.0], list(range(100))])
def test_double_list_round_trip(values):
    vc = ValueCounts.of(values)
    b = double_list_serialize(vc)
    assert DOUBLE_LIST_OBJECT_TYPE == 3
    assert int.from_bytes(b[:4], "big") == len(values) and len(b) == 4 + 8 * len(values)
    assert np.frombuffer(b, ">f8", len(values), 4).tolist() == sorted(float(v) for v in values)  # ascending, big-endian
    assert double_list_deserialize(b) == vc
    # a Java reader slices the object to its length: a length that also counts the objectType int, or one cut short,
    # is not the list's serialisation
    for bad in (b + b"\0\0\0\0", b[:-1] if len(b) > 4 else b + b"\0", b"\0\0"):
        with pytest.raises(ValueError):
            double_list_deserialize(bad)


def _datatable_with_object(payload_len_field, payload):
    """A one-row, one-OBJECT-column DataTable V4 whose cell says (offset 0, payload_len_field)."""
    def s(x):
        e = x.encode("utf-8")
        return struct.pack(">i", len(e)) + e
    schema = struct.pack(">i", 1) + s("percentile90(c)") + s("OBJECT")
    fixed = struct.pack(">ii", 0, payload_len_field)
    var = struct.pack(">i", DOUBLE_LIST_OBJECT_TYPE) + payload
    meta = struct.pack(">i", 0)
    head, off, secs = 4 * 13, 0, []
    for body in (b"", b"", schema, fixed, var):
        secs.append((head + off, len(body)))
        off += len(body)
    out = struct.pack(">iii", 4, 1, 1) + b"".join(struct.pack(">ii", *x) for x in secs)
    return out + schema + fixed + var + meta


def test_decode_checks_the_object_framing():
    payload = double_list_serialize(ValueCounts.of([5, 6, 6]))
    dt = decode(_datatable_with_object(len(payload), payload))
    assert dt.object_spans == [(0, len(payload))] and dt.variable_size == 4 + len(payload)
    otype, body = dt.rows[0][0]
    assert otype == DOUBLE_LIST_OBJECT_TYPE and double_list_deserialize(body).sorted_values().tolist() == [5, 6, 6]
    with pytest.raises(ValueError):  # the length counts the objectType int too: 4 bytes past the section
        decode(_datatable_with_object(len(payload) + 4, payload))


def test_native_symbols():
    L = N.lib()
    assert N.PH_AGG_PERCENTILE == 6
    for name in ("ph_result_percentile_dictionary", "ph_result_percentile_values", "ph_result_percentile_final"):
        assert name in N.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    # the two fields appended to ph_aggregation: a double (8-aligned) after expr_op, then an int32
    assert [f[0] for f in N.Aggregation._fields_][-2:] == ["percentile", "percentile_name_form"]
    assert N.Aggregation.percentile.offset == 40 and N.Aggregation.percentile_name_form.offset == 48
    assert ctypes.sizeof(N.Aggregation) == 56
    # not a result: the accessors refuse instead of reading
    assert L.ph_result_percentile_values(None, 0) is None
    assert L.ph_result_percentile_final(None, 0, None) == N.PH_ERR_INVALID_ARGUMENT
    assert L.ph_result_percentile_dictionary(None, 0, None, None, None) == N.PH_ERR_INVALID_ARGUMENT


def test_kat_file_matches_the_data():
    # the recorded answers are reproducible from the golden columns with plain numpy: each matched doc taken four
    # times (one segment queried four times), sorted, element (int)(n * p / 100)
    from oracle import oracle as O
    kats = json.load(open(KAT_FILE))
    cols = kat_sv.load_columns()
    seg = O.build_segment("kat", cols, inverted=kat_sv.INVERTED)
    assert kats["filter"] == kat_sv.FILTER
    assert len(kats["kats"]) == 25  # testPercentile's 16, p50 in two more spellings (8), the column11 group-by
    for k in kats["kats"]:
        q = parse_sql(k["sql"].replace("{FILTER}", kats["filter"]))
        assert all(a.function == PERCENTILE for a in q.aggregations)
        docs, _ = O.filter_docs(q, seg)
        gcols = [cols[g][0][docs] for g in q.group_by]
        keys = list(zip(*[c.tolist() for c in gcols])) if gcols else [()] * int(docs.sum())
        rows_of = {}
        for j, key in enumerate(keys):
            rows_of.setdefault(key, []).append(j)
        ks = list(rows_of)
        finals = []
        for key in ks:
            row = []
            for a in q.aggregations:
                v = np.sort(np.repeat(cols[a.column][0][docs][rows_of[key]], 4)).astype(np.float64)
                row.append(ValueCounts.of(v))
                # the formula restated without ValueCounts
                assert final_value(a, row[-1]) == (v[-1] if a.percentile == 100 else v[int(len(v) * a.percentile / 100)])
            finals.append(row)
        assert reduce_groups(q, ks, finals).rows == k["rows"], k["source"]
        assert 4 * int(docs.sum()) == k["stats"][0]
        ncols = len(set(q.group_by) | {a.column for a in q.aggregations})
        assert k["stats"][2] == k["stats"][0] * ncols and k["stats"][3] == 4 * len(docs)
