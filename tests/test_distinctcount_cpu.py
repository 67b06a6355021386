"""DISTINCTCOUNT off the GPU: the SQL subset, the broker reduce (value sets merged by value, the final result their
size: DistinctCountAggregationFunction.java:61-68), the value-set object serialisation (ObjectSerDeUtils.java:725-891)
and the C-ABI's new symbols in the built library."""
import json
import os

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import SET_OBJECT_TYPES, set_deserialize
from pinot_amd.query import DISTINCTCOUNT, SUPPORTED_AGGREGATIONS, SqlParseError, parse_sql
from pinot_amd.reduce import final_value, merge_intermediate, reduce_groups, set_serialize
from tests import kat_sv

KAT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distinctcount_kat.json")


def test_parser_accepts_distinctcount():
    assert DISTINCTCOUNT in SUPPORTED_AGGREGATIONS
    q = parse_sql("SELECT g, DISTINCTCOUNT(c), DistinctCount(d) AS x FROM t WHERE f > 3 GROUP BY g ORDER BY x DESC")
    assert [(a.function, a.column, a.op, a.column2) for a in q.aggregations] == [
        (DISTINCTCOUNT, "c", None, None), (DISTINCTCOUNT, "d", None, None)]
    assert q.order_by[0].kind == "aggregation" and q.order_by[0].ref == 1
    # the same aggregation twice is one aggregation (QueryContext de-duplicates)
    q = parse_sql("SELECT DISTINCTCOUNT(c), DISTINCTCOUNT(c) FROM t")
    assert len(q.aggregations) == 1 and [s.ref for s in q.select] == [0, 0]


@pytest.mark.parametrize("sql", ["SELECT DISTINCTCOUNT(*) FROM t", "SELECT DISTINCTCOUNT(a*b) FROM t",
                                 "SELECT DISTINCTCOUNT(a + b) FROM t", "SELECT DISTINCTCOUNT(a, 12) FROM t"])
def test_parser_rejects(sql):
    with pytest.raises(SqlParseError):
        parse_sql(sql)


def test_result_name():
    q = parse_sql("SELECT DISTINCTCOUNT(column11) FROM testTable")
    assert q.aggregations[0].result_name() == "distinctcount(column11)"
    assert q.result_columns() == ["distinctcount(column11)"]


def test_reduce_unions_by_value():
    # two partial results whose dictionaries differ: ids mean different values, the merge is by value
    from pinot_amd.engine import DistinctColumn
    a = DistinctColumn(np.array([[0b1011]], np.uint32), np.array([10, 20, 30, 40], np.int32), np.array([3], np.int32))
    b = DistinctColumn(np.array([[0b0111]], np.uint32), np.array([20, 25, 50], np.int32), np.array([3], np.int32))
    sa, sb = a.value_set(0), b.value_set(0)
    assert sa == {10, 20, 40} and sb == {20, 25, 50}
    merged = merge_intermediate(DISTINCTCOUNT, sa, sb)
    assert merged == {10, 20, 25, 40, 50}
    q = parse_sql("SELECT DISTINCTCOUNT(c) FROM t")
    assert final_value(q.aggregations[0], merged) == 5 and isinstance(final_value(q.aggregations[0], merged), int)
    assert reduce_groups(q, [()], [[merged]]).rows == [[5]]
    # strings, a bitset wider than one word, and ORDER BY on the set size
    s = DistinctColumn(np.array([[1, 1 << 1], [0, 0]], np.uint32), [f"v{i:02d}" for i in range(40)],
                       np.array([2, 0], np.int32))
    assert s.value_set(0) == {"v00", "v33"} and s.value_set(1) == frozenset()
    q = parse_sql("SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g ORDER BY DISTINCTCOUNT(c) DESC, g LIMIT 5")
    rows = reduce_groups(q, [("a",), ("b",), ("c",)], [[{1}], [{1, 2, 3}], [{5, 6}]]).rows
    assert rows == [["b", 3], ["c", 2], ["a", 1]]


@pytest.mark.parametrize("data_type,values", [
    ("INT", [3, -7, 2147483647, 0]), ("LONG", [1 << 40, -(1 << 50), 5]), ("FLOAT", [1.5, -0.25, 3.0e10]),
    ("DOUBLE", [1e-300, 2.5, -1e300]), ("STRING", ["b", "", "naïve", "日本"]),
    ("INT", []), ("LONG", []), ("FLOAT", []), ("DOUBLE", []), ("STRING", [])])
def test_set_round_trip(data_type, values):
    otype = {v: k for k, v in SET_OBJECT_TYPES.items()}[data_type]
    assert sorted(SET_OBJECT_TYPES) == [9, 15, 16, 17, 18]
    b = set_serialize(values, data_type)
    assert int.from_bytes(b[:4], "big") == len(values)
    got = set_deserialize(otype, b)
    if data_type == "FLOAT":
        values = np.asarray(values, np.float32).tolist()
    assert got == frozenset(values) and len(got) == len(values)
    width = {"INT": 4, "LONG": 8, "FLOAT": 4, "DOUBLE": 8}.get(data_type)
    if width:
        assert len(b) == 4 + width * len(values)
    else:
        assert len(b) == 4 + sum(4 + len(v.encode("utf-8")) for v in values)
        if values:  # ascending, length-prefixed UTF-8
            assert b[4:8] == (0).to_bytes(4, "big")


@pytest.mark.parametrize("data_type,values", [("INT", [1, 2, 3]), ("LONG", [7]), ("DOUBLE", []), ("STRING", ["a", "日本"])])
def test_set_deserialize_consumes_the_object_exactly(data_type, values):
    # a Java reader slices the object to its length: a length that also counts the objectType int (4 more bytes), or
    # one cut short, is not the set's serialisation
    otype = {v: k for k, v in SET_OBJECT_TYPES.items()}[data_type]
    b = set_serialize(values, data_type)
    for bad in (b + b"\0\0\0\0", b[:-1] if len(b) > 4 else b + b"\0"):
        with pytest.raises(ValueError):
            set_deserialize(otype, bad)


def _datatable_with_object(payload_len_field, payload):
    """A one-row, one-OBJECT-column DataTable V4 whose cell says (offset 0, payload_len_field)."""
    import struct
    def s(x):
        e = x.encode("utf-8")
        return struct.pack(">i", len(e)) + e
    schema = struct.pack(">i", 1) + s("distinctcount(c)") + s("OBJECT")
    fixed = struct.pack(">ii", 0, payload_len_field)
    var = struct.pack(">i", 9) + payload
    meta = struct.pack(">i", 0)
    head, off, secs = 4 * 13, 0, []
    for body in (b"", b"", schema, fixed, var):
        secs.append((head + off, len(body)))
        off += len(body)
    out = struct.pack(">iii", 4, 1, 1) + b"".join(struct.pack(">ii", *x) for x in secs)
    return out + schema + fixed + var + meta


def test_decode_checks_the_object_framing():
    from pinot_amd.datatable import decode
    payload = set_serialize([5, 6], "INT")
    dt = decode(_datatable_with_object(len(payload), payload))
    assert dt.object_spans == [(0, len(payload))] and dt.variable_size == 4 + len(payload)
    assert set_deserialize(*dt.rows[0][0]) == {5, 6}
    with pytest.raises(ValueError):  # the length counts the objectType int too: 4 bytes past the section
        decode(_datatable_with_object(len(payload) + 4, payload))


def test_native_symbols():
    L = N.lib()
    assert N.PH_AGG_DISTINCTCOUNT == 5
    for name in ("ph_result_distinct_dictionary", "ph_result_distinct_values", "ph_result_distinct_words",
                 "ph_result_distinct_counts"):
        assert name in N.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    # not a result: the accessors refuse instead of reading
    assert L.ph_result_distinct_words(None, 0) == -1
    assert L.ph_result_distinct_values(None, 0) is None
    assert L.ph_result_distinct_counts(None, 0, None) == N.PH_ERR_INVALID_ARGUMENT


def test_kat_file_matches_the_data():
    # the recorded answers are reproducible from the golden columns with plain numpy (one segment queried four times)
    from oracle import oracle as O
    kats = json.load(open(KAT_FILE))
    cols = kat_sv.load_columns()
    seg = O.build_segment("kat", cols, inverted=kat_sv.INVERTED)
    assert kats["filter"] == kat_sv.FILTER
    for k in kats["kats"]:
        q = parse_sql(k["sql"].replace("{FILTER}", kats["filter"]))
        docs, _ = O.filter_docs(q, seg)
        groups = {}
        gcols = [cols[g][0] for g in q.group_by]
        keys = list(zip(*[c[docs].tolist() for c in gcols])) if gcols else [()] * int(docs.sum())
        for a in q.aggregations:
            vals = cols[a.column][0][docs]
            for key in set(keys):
                sel = np.array([x == key for x in keys], bool) if gcols else np.ones(len(vals), bool)
                groups.setdefault(key, []).append(frozenset(np.unique(vals[sel]).tolist()))
        ks = list(groups)
        assert reduce_groups(q, ks, [groups[x] for x in ks]).rows == k["rows"], k["source"]
        assert 4 * int(docs.sum()) == k["stats"][0]
