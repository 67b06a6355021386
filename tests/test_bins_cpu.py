"""CPU: HISTOGRAM's host side -- ph_histogram_bin_ids against tests/bins_ref.py (equality, no tolerance), the SQL parse
of both spellings and of the reference's bad-argument cases, the broker merge, and the known answers of
HistogramQueriesTest (tests/golden/histogram_kat.json) on the bin table plus numpy counting."""
import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.query import HISTOGRAM, SqlParseError, parse_sql
from pinot_amd.reduce import final_value, merge_intermediate
from tests.bins_ref import DTYPES, KAT, OUT_OF_BOUNDS, bin_ids, counts, kat_column

INF = float("inf")


def native_bin_ids(values, edges, equal_bins=0):
    values = np.ascontiguousarray(values)
    dt = {v: k for k, v in DTYPES.items()}[values.dtype.type]
    e = np.ascontiguousarray(edges, np.float64)
    out = np.full(len(values), -9, np.int32)
    rc = N.lib().ph_histogram_bin_ids(e.ctypes.data, len(e), equal_bins, N.DATA_TYPES[dt], values.ctypes.data,
                                      len(values), out.ctypes.data)
    return rc, out


CASES = [  # (edges, equal_bins)
    ([-8.0, -0.5, 0.0, 3.0, 1024.0], 0), ([-INF, -0.5, 0.0, 3.0, INF], 0), ([5.0, 6.0], 0),
    ([0.0, 1.0], 10), ([-8.0, 1024.0], 7), ([0.0, 1000.0], 1024)]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("edges,equal", CASES)
def test_bin_ids_match_the_reference(dt, edges, equal):
    t = DTYPES[dt]
    lo, hi = (e if np.isfinite(e) else np.sign(e) * 1e6 for e in (edges[0], edges[-1]))
    if dt in ("FLOAT", "DOUBLE"):  # every edge, one ulp inside and outside of each; k/10, where the floor is decided
        vals = [np.nextafter(t(e), t(d)) for e in edges if np.isfinite(e) for d in (-INF, e, INF)]  # by rounding
        vals += [k / 10 for k in range(11)]
        vals += [lo - 1, hi + 1, 0.0, -0.0, INF, -INF] + np.linspace(lo, hi, 97).tolist()
    else:
        vals = [int(e) + d for e in edges if np.isfinite(e) for d in (-1, 0, 1)] + [int(lo) - 5, int(hi) + 5]
        vals += np.linspace(lo, hi, 97).astype(np.int64).tolist()
    vals = np.array(vals).astype(t)
    exp = bin_ids(vals, edges, equal)
    ok = exp != OUT_OF_BOUNDS  # (an equal-length id that reaches B: its own test below)
    rc, got = native_bin_ids(vals[ok], edges, equal)
    assert rc == N.PH_OK and got.tolist() == exp[ok].tolist()


def test_long_values_round_to_double_first():
    big = np.array([2 ** 53 + 1, 2 ** 62 + 12345, 2 ** 53, 2 ** 62], np.int64)
    for v in big[:2].tolist():  # an edge at the value's rounded double: the value equals the edge, not one above it
        e = float(v)
        edges = [0.0, e, 2.0 ** 63]
        rc, got = native_bin_ids(big, edges)
        assert rc == N.PH_OK and got.tolist() == bin_ids(big, edges).tolist()
        assert got[big.tolist().index(v)] == 1
        rc, got = native_bin_ids(big, [0.0, e])  # ... and as `upper` it is inside, in the last bin
        assert got[big.tolist().index(v)] == 0


def test_nan_and_ids_that_reach_the_number_of_bins():
    L = N.lib()
    nan = np.array([1.0, np.nan], np.float64)
    rc, got = native_bin_ids(nan, [0.0, 2.0], 4)  # (int) NaN is 0
    assert rc == N.PH_OK and got.tolist() == [2, 0] == bin_ids(nan, [0.0, 2.0], 4).tolist()
    rc, _ = native_bin_ids(nan, [0.0, 1.0, 2.0])  # the binary search ends at the last edge: index B
    assert rc == N.PH_ERR_UNSUPPORTED and b"out of bounds" in L.ph_last_error()
    assert bin_ids(nan, [0.0, 1.0, 2.0])[1] == OUT_OF_BOUNDS
    # the value just below upper = 1 over three bins: its quotient by the rounded 1/3 rounds up to 3.0
    lower, upper, bins = 0.0, 1.0, 3
    v = np.nextafter(upper, -INF)
    assert np.floor((v - lower) / ((upper - lower) / bins)) == bins, "the case no longer reaches B"
    rc, _ = native_bin_ids(np.array([v]), [lower, upper], bins)
    assert rc == N.PH_ERR_UNSUPPORTED and bin_ids([v], [lower, upper], bins)[0] == OUT_OF_BOUNDS


def test_malformed_edges_are_bad_queries():
    for edges, equal in (([0.0], 0), ([0.0, 0.0, 1.0], 0), ([1.0, 0.0], 0), ([0.0, np.nan], 0), ([1000.0, 1000.0], 10),
                         ([0.0, 1000.0], -1), ([0.0, 1.0, 2.0], 2)):
        assert native_bin_ids(np.zeros(1), edges, equal)[0] == N.PH_ERR_BAD_QUERY, (edges, equal)


def test_sql_parse():
    q = parse_sql('SELECT histogram(x, ARRAY["-Infinity", 0, 1.5, "Infinity"]), HISTOGRAM(x, 0, 1000, 10), COUNT(*) '
                  "FROM t WHERE y < 3 GROUP BY g")
    a, b, _ = q.aggregations
    assert (a.function, a.column, a.edges, a.equal_bins, a.num_bins) == (HISTOGRAM, "x", (-INF, 0.0, 1.5, INF), 0, 3)
    assert (b.edges, b.equal_bins, b.num_bins) == ((0.0, 1000.0), 10, 10)
    # BaseSingleInputAggregationFunction.getResultColumnName (:43-45): the edges are not part of the name
    assert q.result_columns()[:2] == ["histogram(x)", "histogram(x)"] and len(q.aggregations) == 3
    # HistogramQueriesTest.testInvalidInput (:283-345)
    for sql in ("HISTOGRAM(intColumn,1000,1000,10)", "HISTOGRAM(intColumn,0,1000,-1)", "HISTOGRAM(intColumn,ARRAY[0])",
                "HISTOGRAM(intColumn,FUNCTION[0, 10, 20])", "HISTOGRAM(intColumn,ARRAY[0, 0, 1, 2])",
                "HISTOGRAM(intColumn)", 'HISTOGRAM(intColumn,0,1000,"Infinity")', "HISTOGRAM(intColumn,0,1000,'NaN')"):
        with pytest.raises(SqlParseError):
            parse_sql(f"SELECT {sql} FROM testTable")


def test_broker_merge_and_final_type():
    spec = parse_sql("SELECT HISTOGRAM(x, 0, 3, 3) FROM t").aggregations[0]
    merged = merge_intermediate(HISTOGRAM, (1.0, 0.0, 5.0), (2.0, 0.0, 2.0 ** 40))
    assert merged == (3.0, 0.0, 2.0 ** 40 + 5)
    assert final_value(spec, merged) == [3.0, 0.0, 2.0 ** 40 + 5] and type(final_value(spec, merged)[0]) is float


@pytest.mark.parametrize("case", KAT["cases"], ids=lambda c: c["sql"][7:60])
def test_known_answers_of_the_reference_test(case):
    vals = kat_column(case["column"])
    keep = kat_column("intColumn") >= (case["min_int"] or 0)
    edges = [float(e) for e in case["edges"]]
    spec = parse_sql(case["sql"]).aggregations[0]
    assert (list(spec.edges), spec.equal_bins) == (edges, case["equal_bins"])
    rc, ids = native_bin_ids(vals, edges, case["equal_bins"])
    assert rc == N.PH_OK and int(keep.sum()) == case["docs"]
    got = np.bincount(ids[keep & (ids >= 0)], minlength=spec.num_bins)
    assert got.tolist() == case["expected"] == counts(vals[keep], edges, case["equal_bins"]).tolist()
