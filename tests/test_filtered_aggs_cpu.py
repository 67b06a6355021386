"""CPU: the host side of filtered aggregations (agg(...) FILTER(WHERE ...)): the parser, the result column names
against the literal strings of the reference's FilteredAggregationsTest.java, (function, filter) dedup, the ph_query
packing and the host-only refusals."""
import ctypes

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.query import (COUNT, MAX, SUM, EqPredicate, FilterContext, InPredicate, NotEqPredicate, NotInPredicate,
                             RangePredicate, parse_sql)


def test_parser_round_trip():
    q = parse_sql("SELECT region, COUNT(*), COUNT(*) FILTER(WHERE status = 'error'), "
                  "SUM(bytes) FILTER(WHERE status = 'ok' AND tier IN ('a','b')) AS ok_bytes, "
                  "MAX(latency) FILTER(WHERE dc <> 'x') FROM t WHERE day BETWEEN 10 AND 20 GROUP BY region")
    a = q.aggregations
    assert [x.function for x in a] == [COUNT, COUNT, SUM, MAX]
    assert a[0].filter is None
    assert a[1].filter == FilterContext.pred(EqPredicate("status", "error"))
    assert a[2].filter == FilterContext.and_(FilterContext.pred(EqPredicate("status", "ok")),
                                             FilterContext.pred(InPredicate("tier", ("a", "b"))))
    assert a[3].filter == FilterContext.pred(NotEqPredicate("dc", "x"))
    assert q.filter == FilterContext.pred(RangePredicate("day", "10", "20", True, True))
    assert q.result_columns() == ["region", "count(*)", "count(*) FILTER(WHERE status = 'error')", "ok_bytes",
                                  "max(latency) FILTER(WHERE dc != 'x')"]
    # the alias without AS, as the reference's test queries write it (FilteredAggregationsTest.java:165): accepted
    # after a FILTER clause only
    with pytest.raises(Exception):
        parse_sql("SELECT SUM(INT_COL) sum1 FROM MyTable")
    q = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999) sum1 FROM MyTable WHERE INT_COL < 1000000")
    assert q.result_columns() == ["sum1"] and q.aggregations[0].filter is not None
    # ORDER BY on a filtered aggregation refers to the same (function, filter) pair
    q = parse_sql("SELECT g, SUM(m) FILTER(WHERE f < 3) FROM t GROUP BY g ORDER BY SUM(m) FILTER(WHERE f < 3) DESC")
    assert len(q.aggregations) == 1 and q.order_by[0].ref == 0 and not q.order_by[0].asc


def test_result_names_are_the_reference_tests_literals():
    # FilteredAggregationsTest.java:217-243
    q = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999) FROM MyTable WHERE INT_COL < 1000000 "
                  "GROUP BY BOOLEAN_COL")
    assert q.aggregations[0].result_name() == "sum(INT_COL) FILTER(WHERE INT_COL > '9999')"
    q = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999 AND INT_COL < 1000000) FROM MyTable")
    assert q.aggregations[0].result_name() == "sum(INT_COL) FILTER(WHERE (INT_COL > '9999' AND INT_COL < '1000000'))"


def test_to_string_of_every_predicate():
    p = FilterContext.pred
    assert p(EqPredicate("c", "4")).to_string() == "c = '4'"
    assert p(NotEqPredicate("c", "x")).to_string() == "c != 'x'"
    assert p(InPredicate("c", ("a", "b"))).to_string() == "c IN ('a','b')"
    assert p(NotInPredicate("c", ("a",))).to_string() == "c NOT IN ('a')"
    assert p(RangePredicate("c", "1", "*", True, False)).to_string() == "c >= '1'"
    assert p(RangePredicate("c", "*", "9", False, True)).to_string() == "c <= '9'"
    assert p(RangePredicate("c", "1", "9", True, True)).to_string() == "c BETWEEN '1' AND '9'"
    assert p(RangePredicate("c", "1", "9", False, True)).to_string() == "(c > '1' AND c <= '9')"
    f = FilterContext.or_(p(EqPredicate("a", "1")), FilterContext.not_(p(EqPredicate("b", "2"))))
    assert f.to_string() == "(a = '1' OR (NOT b = '2'))"


def test_function_filter_pairs_stay_distinct():
    q = parse_sql("SELECT SUM(m), SUM(m) FILTER(WHERE f < 3), SUM(m) FILTER(WHERE f < 4), SUM(m) FILTER(WHERE f < 3) "
                  "FROM t")
    assert len(q.aggregations) == 3
    assert [s.ref for s in q.select] == [0, 1, 2, 1]


def test_struct_layout_and_packing():
    # the new field sits in what was ph_aggregation's tail padding: both layouts are the header's 56 bytes
    assert N.FilteredAggregation.filter.offset == 52
    assert ctypes.sizeof(N.FilteredAggregation) == ctypes.sizeof(N.Aggregation) == 56
    assert N.PH_KERNEL_SCAN_FILTERED == 20
    from pinot_amd.engine import _QueryStruct
    q = parse_sql("SELECT COUNT(*), SUM(m) FILTER(WHERE f < 3 AND g = 1), MAX(m) FILTER(WHERE f < 3 AND g = 1) "
                  "FROM t WHERE h > 0")
    s = _QueryStruct(q).struct
    aggs = ctypes.cast(s.aggregations, ctypes.POINTER(N.FilteredAggregation))
    assert aggs[0].filter == 0
    # main: one predicate node; each FILTER tree is packed under its own root (two leaves, then the AND)
    assert s.filter_root == 0 and s.num_filter_nodes == 7 and s.num_predicates == 5
    assert [aggs[1].filter, aggs[2].filter] == [4, 7]
    for k in (1, 2):
        root = s.filter_nodes[aggs[k].filter - 1]
        assert root.type == N.PH_FILTER_AND and root.num_children == 2
        assert [s.predicates[s.filter_nodes[root.children[i]].predicate].column for i in range(2)] == [b"f", b"g"]


def test_host_only_refusals():
    L = N.lib()
    from pinot_amd.engine import _QueryStruct
    qs = _QueryStruct(parse_sql("SELECT SUM(m) FILTER(WHERE f < 3) FROM t"))
    aggs = ctypes.cast(qs.struct.aggregations, ctypes.POINTER(N.FilteredAggregation))
    size = ctypes.c_uint64()
    # ph_result_datatable names a filtered column from the query: without a result it refuses before reading it
    assert L.ph_result_datatable(None, ctypes.byref(qs.struct), None, 0, None, 0, ctypes.byref(size)) == \
        N.PH_ERR_INVALID_ARGUMENT
    # ph_query_dense_layout judges the query's shape before it asks for a context, so a null one serves: a bad index is
    # an argument error with its own message, a good one the shape's refusal (were the order to change, the null
    # context's "null argument" would fail the message checks below)
    lay = N.DenseLayout()
    h = None
    aggs[0].filter = 99
    assert L.ph_query_dense_layout(h, ctypes.byref(qs.struct), None, 0, ctypes.byref(lay)) == N.PH_ERR_INVALID_ARGUMENT
    assert b"filter index" in L.ph_last_error()
    aggs[0].filter = -1
    assert L.ph_query_dense_layout(h, ctypes.byref(qs.struct), None, 0, ctypes.byref(lay)) == N.PH_ERR_INVALID_ARGUMENT
    assert b"filter index" in L.ph_last_error()
    aggs[0].filter = 1
    assert L.ph_query_dense_layout(h, ctypes.byref(qs.struct), None, 0, ctypes.byref(lay)) == N.PH_ERR_UNSUPPORTED
    assert b"dense partials" in L.ph_last_error()
    # a FILTER tree whose nodes form a cycle: the AND's child is the AND itself
    qs = _QueryStruct(parse_sql("SELECT SUM(m) FILTER(WHERE f < 3 AND g = 1) FROM t"))
    aggs = ctypes.cast(qs.struct.aggregations, ctypes.POINTER(N.FilteredAggregation))
    root = qs.struct.filter_nodes[aggs[0].filter - 1]
    root.children[1] = aggs[0].filter - 1
    assert L.ph_query_dense_layout(h, ctypes.byref(qs.struct), None, 0, ctypes.byref(lay)) == N.PH_ERR_INVALID_ARGUMENT
    assert b"cycle" in L.ph_last_error()
    # refused function shapes, each with its own message
    for sql, word in (("SELECT DISTINCTCOUNT(m) FILTER(WHERE f < 3) FROM t", b"DISTINCTCOUNT with a FILTER"),
                      ("SELECT DISTINCTCOUNTHLL(m) FILTER(WHERE f < 3) FROM t", b"DISTINCTCOUNTHLL with a FILTER"),
                      ("SELECT PERCENTILE(m, 50) FILTER(WHERE f < 3) FROM t", b"PERCENTILE with a FILTER"),
                      ("SELECT SUM(m * n) FILTER(WHERE f < 3) FROM t", b"2-operand")):
        qs = _QueryStruct(parse_sql(sql))
        assert L.ph_query_dense_layout(h, ctypes.byref(qs.struct), None, 0, ctypes.byref(lay)) == N.PH_ERR_UNSUPPORTED
        assert word in L.ph_last_error(), (sql, L.ph_last_error())


def test_reference_defaults_and_union_rows():
    # the numpy reference itself on a tiny table: a group seen only through one sub-filter is a row, its other cells
    # hold the defaults; a group main matches but no pipeline does is absent
    from oracle import oracle as O
    from tests import filtered_ref as F
    t = {"g": np.array([0, 0, 1, 2, 2], np.int32), "f": np.array([1, 5, 5, 9, 0], np.int32),
         "m": np.array([10, 20, 30, 40, 50], np.int32)}
    seg = O.build_segment("s", {c: (v, "INT") for c, v in t.items()})
    q = parse_sql("SELECT g, SUM(m) FILTER(WHERE f < 3), MIN(m) FILTER(WHERE f = 5), COUNT(*) FILTER(WHERE f = 5) "
                  "FROM t WHERE f < 9 GROUP BY g")
    rows, stats = F.reference(q, [seg], [t])
    assert rows == {(0,): [("exact", 10.0), ("exact", 20.0), ("exact", 1)],
                    (1,): [("exact", 0.0), ("exact", 30.0), ("exact", 1)],
                    (2,): [("exact", 50.0), ("exact", float("inf")), ("exact", 0)]}
    # two pipelines under a scan main filter: 2 + 2 docs, projected columns {g, m}; each single scan leaf scans
    # |docs(main)| = 4 entries
    assert stats == {"docs": 4, "post_filter": 8, "in_filter": 8}
