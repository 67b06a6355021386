"""GPU: filtered aggregations (agg(...) FILTER(WHERE ...)) through ctx.execute, against tests/filtered_ref.py -- the
reference's own test method (FilteredAggregationsTest.testQuery :151-161): the filtered query equals numpy aggregates
over the oracle's doc masks of the equivalent unfiltered filters.

Segments of 4 099 + 193 docs (a partial last mask word, more than one chunk's tile) plus 1-, 63-, 64- and 65-doc
segments for the mask-word edges.  Every served case asserts scan_kernel == 20 and its plan_mode, the rows, and the
three statistics (``in_filter`` on the closed forms).  Tolerances: COUNT, MIN, MAX and integer SUM exact; a real SUM
within n * 2^-52 * sum|x| of the exact sum (tests/float_ref.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.native import BadQueryError, PinotHipError, UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.segment import SegmentBuffers, create_column, create_column_from_dict_ids, create_segment
from tests import filtered_ref as F
from tests import float_ref as R

pytestmark = pytest.mark.gpu

K_FILTERED = 20
MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
INVERTED, RANGE_INDEX = ("inv",), ("rng",)
TYPES = {"g": "INT", "g2": "INT", "h": "INT", "f": "INT", "inv": "INT", "srt": "INT", "rng": "INT", "part": "INT",
         "i": "INT", "l": "LONG", "fl": "FLOAT", "d": "DOUBLE", "u1": "INT", "u2": "INT", "u3": "INT", "u4": "INT"}


def make_table(n, si):
    rng = np.random.default_rng(77 + si)
    doc = np.arange(n)
    t = {"g": (doc % 12).astype(np.int32), "g2": rng.integers(0, 3, n).astype(np.int32),
         "f": rng.integers(0, 10, n).astype(np.int32), "inv": rng.integers(0, 4, n).astype(np.int32),
         "srt": (doc * 5 // max(n, 1)).astype(np.int32), "rng": rng.integers(0, 20, n).astype(np.int32),
         "part": np.full(n, si, np.int32), "i": rng.integers(-1000, 1000, n).astype(np.int32),
         "l": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
         "fl": (rng.integers(-4000, 4000, n) * 0.25).astype(np.float32), "d": np.round(rng.normal(0, 100, n), 2)}
    t["h"] = t["g"].copy()
    for k in range(4):
        t[f"u{k + 1}"] = rng.permutation(n).astype(np.int32)
    return t


def both(name, t, raw=()):
    cols = {c: (v, TYPES[c]) for c, v in t.items()}
    return (create_segment(name, cols, inverted=INVERTED, range_index=RANGE_INDEX, raw=raw),
            O.build_segment(name, cols, inverted=INVERTED, range_index=RANGE_INDEX))


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base(ctx):
    tables = [make_table(4099, 0), make_table(193, 1)]
    made = [both(f"fa_{i}", t) for i, t in enumerate(tables)]
    segs = [ctx.pin(b) for b, _ in made]
    yield segs, [o for _, o in made], tables
    for s in segs:
        s.unpin()


def run(ctx, sql, segs, osegs, tables, mode, in_filter_known=True):
    q = parse_sql(sql)
    r = ctx.execute(q, segs)
    rows, stats = F.reference(q, osegs, tables)
    print(sql, "->", r.num_groups, "rows; stats", r.stats.num_docs_scanned, r.stats.num_entries_scanned_in_filter,
          r.stats.num_entries_scanned_post_filter, "expected", stats)
    assert r.stats.scan_kernel == K_FILTERED and r.stats.mode == mode, (sql, r.stats.scan_kernel, r.stats.mode)
    F.compare(dict(zip(r.keys, r.aggs)), rows, sql)
    assert r.stats.num_docs_scanned == stats["docs"], sql
    assert r.stats.num_entries_scanned_post_filter == stats["post_filter"], sql
    if in_filter_known:
        assert stats["in_filter"] is not None and r.stats.num_entries_scanned_in_filter == stats["in_filter"], sql
    assert r.stats.num_total_docs == sum(len(t["g"]) for t in tables)
    return r


# the reference test's queries on this table (FilteredAggregationsTest.java:165-199, :217-241, :279-311; INT_COL has an
# inverted and a range index there, NO_INDEX_COL none: inv / rng and f here)
REFERENCE_QUERIES = [
    "SELECT SUM(i) FILTER(WHERE rng > 9) sum1 FROM t WHERE rng < 15",
    "SELECT SUM(i) FILTER(WHERE rng < 3) sum1 FROM t WHERE rng > 1",
    "SELECT COUNT(*) FILTER(WHERE inv = 2) count1 FROM t",
    "SELECT SUM(i) FILTER(WHERE rng > 8) sum1 FROM t",
    "SELECT SUM(i) FILTER(WHERE f <= 1) sum1 FROM t WHERE rng > 1",
    "SELECT MIN(i) FILTER(WHERE f > 7) min1, MAX(i) FILTER(WHERE rng > 17) max1 FROM t",
    "SELECT SUM(i) FILTER(WHERE rng > 9 AND rng < 15) FROM t",
    "SELECT SUM(i) FILTER(WHERE rng > 3) AS s1, SUM(i) FILTER(WHERE rng < 4) AS s2 FROM t WHERE rng > 2",
    "SELECT SUM(i) FILTER(WHERE rng > 12) AS s1, SUM(i) FILTER(WHERE rng < 19) AS s2, "
    "MIN(i) FILTER(WHERE rng > 5) AS m FROM t WHERE rng > 1",
    "SELECT SUM(i) FILTER(WHERE f > 6) AS s1, SUM(i) FILTER(WHERE f < 9) AS s2, MIN(i) FILTER(WHERE f > 2) AS m "
    "FROM t WHERE rng > 1",
    "SELECT SUM(i) FILTER(WHERE rng > 12) AS s1, SUM(l) FILTER(WHERE rng < 19) AS s2, MIN(i) FILTER(WHERE rng > 5) "
    "AS m FROM t WHERE rng < 18 AND f > 3",
]


@pytest.mark.parametrize("sql", REFERENCE_QUERIES)
def test_reference_test_queries(ctx, base, sql):
    run(ctx, sql, *base, MODE_AGG)


def test_reference_group_by_names(ctx, base):
    # :217-228: the group-by forms, and the column names the DataTable carries
    segs, osegs, tables = base
    for sql, name in (("SELECT SUM(i) FILTER(WHERE rng > 9) FROM t WHERE rng < 15 GROUP BY g2",
                       "sum(i) FILTER(WHERE rng > '9')"),
                      ("SELECT SUM(i) FILTER(WHERE rng > 9 AND rng < 15) FROM t GROUP BY g2",
                       "sum(i) FILTER(WHERE (rng > '9' AND rng < '15'))")):
        run(ctx, sql, segs, osegs, tables, MODE_LDS)
        from pinot_amd.datatable import decode
        dt = decode(ctx.execute_datatable(parse_sql(sql), segs))
        assert dt.column_names == ["g2", name], dt.column_names


AGG_ONLY = {
    1: "SELECT COUNT(*), SUM(d) FILTER(WHERE f < 3) FROM t",
    3: "SELECT SUM(i) FILTER(WHERE f < 3), MIN(l) FILTER(WHERE inv = 1), MAX(fl) FILTER(WHERE srt = 2), SUM(fl) FROM t",
    8: "SELECT " + ", ".join(f"SUM(i) FILTER(WHERE f = {k})" for k in range(8)) + " FROM t",
}
MAINS = {"none": "", "scan": " WHERE f < 8", "sorted": " WHERE srt BETWEEN 1 AND 3", "inverted": " WHERE inv = 1",
         "range": " WHERE rng BETWEEN 3 AND 10", "conj": " WHERE f < 8 AND inv IN (1, 2)"}


@pytest.mark.parametrize("k", sorted(AGG_ONLY))
@pytest.mark.parametrize("main", sorted(MAINS))
def test_aggregation_only(ctx, base, k, main):
    run(ctx, AGG_ONLY[k] + MAINS[main], *base, MODE_AGG)


GROUP_QUERIES = [
    # a mix with unfiltered functions, two aggregations sharing one filter (equal trees at different node indices)
    "SELECT g, COUNT(*), SUM(i) FILTER(WHERE f < 3), MAX(i) FILTER(WHERE f < 3), MIN(d) FILTER(WHERE inv = 2), "
    "SUM(l) FROM t{main} GROUP BY g",
    # a sub-filter matching all, one empty
    "SELECT g, SUM(i) FILTER(WHERE f >= 0), COUNT(*) FILTER(WHERE f > 100), MIN(fl) FILTER(WHERE rng < 5) "
    "FROM t{main} GROUP BY g",
    # groups present only through one sub-filter; the groups main matches but no pipeline does are absent
    "SELECT g, SUM(i) FILTER(WHERE h = 3), COUNT(*) FILTER(WHERE h IN (3, 5)) FROM t{main} GROUP BY g",
    "SELECT g, g2, SUM(d) FILTER(WHERE srt = 1), COUNT(*) FILTER(WHERE inv != 0) FROM t{main} GROUP BY g, g2",
]


@pytest.mark.parametrize("hbm", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("main", sorted(MAINS))
@pytest.mark.parametrize("qi", range(len(GROUP_QUERIES)))
def test_group_by(ctx, base, monkeypatch, qi, main, hbm):
    if hbm:
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    run(ctx, GROUP_QUERIES[qi].format(main=MAINS[main]), *base, MODE_HBM if hbm else MODE_LDS)


def test_absent_groups(ctx, base):
    segs, osegs, tables = base
    r = run(ctx, GROUP_QUERIES[2].format(main=" WHERE f < 8"), segs, osegs, tables, MODE_LDS)
    assert sorted(r.keys) == [(3,), (5,)]
    row = dict(zip(r.keys, r.aggs))[(5,)]
    assert row[0] == 0.0 and row[1] > 0  # SUM's default beside a pipeline that saw the group


def test_main_empty_on_one_segment(ctx, base):
    # part = 0: matches all of segment 0 (one dictionary value), nothing of segment 1
    segs, osegs, tables = base
    r = run(ctx, "SELECT g, COUNT(*), SUM(i) FILTER(WHERE f < 3) FROM t WHERE part = 0 GROUP BY g", segs, osegs, tables,
            MODE_LDS)
    assert r.stats.num_segments_matched == 1
    run(ctx, "SELECT COUNT(*) FILTER(WHERE f > 4), SUM(i) FILTER(WHERE f < 3) FROM t WHERE part = 1 AND f < 8", segs, osegs,
        tables, MODE_AGG)
    run(ctx, "SELECT SUM(i) FILTER(WHERE f < 3) FROM t WHERE part = 7", segs, osegs, tables, MODE_AGG)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_mask_word_edges(ctx, n):
    t = make_table(n, 0)
    b, o = both(f"fa_edge_{n}", t)
    seg = ctx.pin(b)
    try:
        run(ctx, "SELECT COUNT(*), SUM(i) FILTER(WHERE f < 5), MAX(l) FILTER(WHERE f >= 5) FROM t", [seg], [o], [t], MODE_AGG)
        run(ctx, "SELECT g2, COUNT(*) FILTER(WHERE f < 5), MIN(d) FILTER(WHERE inv > 0) FROM t WHERE rng < 15 GROUP BY g2",
            [seg], [o], [t], MODE_LDS)
    finally:
        seg.unpin()


def test_segment_pinned_twice_and_raw_value_column(ctx, base):
    segs, osegs, tables = base
    b, o = both("fa_again", tables[1])
    braw, oraw = both("fa_raw", tables[1], raw=("i", "d"))
    extra = [ctx.pin(b), ctx.pin(braw)]
    try:
        run(ctx, "SELECT g, SUM(i) FILTER(WHERE f < 3), MIN(d) FILTER(WHERE inv = 2), COUNT(*) FROM t WHERE rng < 15 "
                 "GROUP BY g", segs + extra, osegs + [o, oraw], tables + [tables[1], tables[1]], MODE_LDS)
    finally:
        for s in extra:
            s.unpin()


def test_datatable_and_broker_reduce(ctx, base):
    from pinot_amd.datatable import decode, reduce_datatables
    from pinot_amd.reduce import reduce_groups
    segs, osegs, tables = base
    sql = ("SELECT g, COUNT(*), SUM(i) FILTER(WHERE f < 3), MAX(i) FILTER(WHERE inv = 2) FROM t WHERE rng < 15 "
           "GROUP BY g ORDER BY g LIMIT 100")
    q = parse_sql(sql)
    tabs = [decode(ctx.execute_datatable(q, [s])) for s in segs]  # two calls, merged by the broker
    assert tabs[0].column_names == ["g", "count(*)", "sum(i) FILTER(WHERE f < '3')", "max(i) FILTER(WHERE inv = '2')"]
    got = reduce_datatables(q, tabs)
    r = ctx.execute(q, segs)
    want = reduce_groups(q, r.keys, r.aggs)
    assert got.columns == want.columns and got.rows == want.rows
    rows, _ = F.reference(q, osegs, tables)
    F.compare({(row[0],): row[1:] for row in got.rows}, rows, sql)


def test_sum_at_the_precision_flag(ctx):
    n = 70
    t = {"g": (np.arange(n) % 2).astype(np.int32), "f": (np.arange(n) % 10).astype(np.int32),
         "l": np.where(np.arange(n) % 10 < 5, 1 << 52, 3).astype(np.int64)}
    cols = {"g": (t["g"], "INT"), "f": (t["f"], "INT"), "l": (t["l"], "LONG")}
    seg = ctx.pin(create_segment("fa_flag", cols))
    o = O.build_segment("fa_flag", cols)
    try:
        r = run(ctx, "SELECT SUM(l) FILTER(WHERE f < 5), SUM(l) FILTER(WHERE f >= 5) FROM t", [seg], [o], [t], MODE_AGG)
        assert r.stats.sum_precision_flag and r.aggs[0][0] == float(35 * (1 << 52)) and r.aggs[0][1] == 105.0
        r = run(ctx, "SELECT SUM(l) FILTER(WHERE f >= 5), COUNT(*) FROM t", [seg], [o], [t], MODE_AGG)
        assert not r.stats.sum_precision_flag
        r = run(ctx, "SELECT g, SUM(l) FILTER(WHERE f < 5) FROM t GROUP BY g", [seg], [o], [t], MODE_LDS)
        assert r.stats.sum_precision_flag
    finally:
        seg.unpin()


def test_sum_widened_to_double(ctx, monkeypatch):
    # |term| x the call's docs reaches 2^63 (2^62 x 70): the term is summed in double, as the reference sums, on every
    # kernel form; the bar is float_ref's for n double additions (n * 2^-52 * sum|x|), and the flag reports >= 2^53
    n = 70
    doc = np.arange(n)
    big = (1 << 62) - 7 * doc.astype(np.int64)
    t = {"g": (doc % 2).astype(np.int32), "f": (doc % 10).astype(np.int32),
         "l": np.where(doc % 10 < 5, big, np.where(doc % 4 == 0, -big, big)).astype(np.int64)}
    cols = {"g": (t["g"], "INT"), "f": (t["f"], "INT"), "l": (t["l"], "LONG")}
    seg = ctx.pin(create_segment("fa_wide", cols))
    o = O.build_segment("fa_wide", cols)
    try:
        sql = "SELECT {k}SUM(l) FILTER(WHERE f < 5), SUM(l) FILTER(WHERE f >= 5), SUM(l), MAX(l) FILTER(WHERE f < 5) FROM t{g}"
        r = run(ctx, sql.format(k="", g=""), [seg], [o], [t], MODE_AGG)
        assert r.stats.sum_precision_flag and r.aggs[0][0] > 2.0 ** 66 and r.aggs[0][3] == float(1 << 62)
        r = run(ctx, sql.format(k="g, ", g=" GROUP BY g"), [seg], [o], [t], MODE_LDS)
        assert r.stats.sum_precision_flag
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
        r = run(ctx, sql.format(k="g, ", g=" GROUP BY g"), [seg], [o], [t], MODE_HBM)
        assert r.stats.sum_precision_flag
    finally:
        seg.unpin()


def test_min_max_nan_and_signed_zero(ctx, monkeypatch):
    n = 130
    doc = np.arange(n)
    d = np.where(doc % 3 == 0, -0.0, 0.0)
    d[doc % 13 == 5] = np.nan  # f = doc % 10: NaN docs have f in {5, 8, 1, 4, ...}
    d[100:] = 2.5
    t = {"g": (doc % 4).astype(np.int32), "f": (doc % 10).astype(np.int32), "d": d, "fl": d.astype(np.float32)}
    b = SegmentBuffers("fa_nan", n)
    for c in ("g", "f"):
        b.columns[c] = create_column(c, t[c], "INT")
    for c, (dt, npt) in {"d": ("DOUBLE", np.float64), "fl": ("FLOAT", np.float32)}.items():
        dictionary, ids = R.java_dictionary(t[c], npt)
        b.columns[c] = create_column_from_dict_ids(c, dictionary, ids, dt, allow_sorted=False)
    o = O.build_segment("fa_nan", {c: (t[c], "INT") for c in ("g", "f")})
    seg = ctx.pin(b)
    try:
        for hbm in (False, True):
            if hbm:
                monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
            sql = ("SELECT {k}MIN(d) FILTER(WHERE f < 5), MAX(d) FILTER(WHERE f < 5), MIN(fl) FILTER(WHERE f IN (0, 2, 3)), "
                   "MAX(fl) FILTER(WHERE f IN (0, 2, 3)), MIN(d) FILTER(WHERE f = 6), MAX(d) FILTER(WHERE f = 6) FROM t{g}")
            run(ctx, sql.format(k="g, ", g=" GROUP BY g"), [seg], [o], [t], MODE_HBM if hbm else MODE_LDS)
        run(ctx, sql.format(k="", g=""), [seg], [o], [t], MODE_AGG)
    finally:
        seg.unpin()


REFUSALS = [
    ("SELECT DISTINCTCOUNT(i) FILTER(WHERE f < 3) FROM t", "DISTINCTCOUNT with a FILTER"),
    ("SELECT DISTINCTCOUNTHLL(i) FILTER(WHERE f < 3) FROM t", "DISTINCTCOUNTHLL with a FILTER"),
    ("SELECT PERCENTILE(i, 50) FILTER(WHERE f < 3) FROM t", "PERCENTILE with a FILTER"),
    ("SELECT SUM(i * f) FILTER(WHERE f < 3) FROM t", "2-operand expression"),
    ("SET minSegmentGroupTrimSize=5; SELECT g, SUM(i) FILTER(WHERE f < 3) FROM t GROUP BY g ORDER BY g LIMIT 3",
     "segment group trim"),
    ("SET numGroupsLimit=5; SELECT g, SUM(i) FILTER(WHERE f < 3) FROM t GROUP BY g", "numGroupsLimit"),
    ("SELECT u1, u2, u3, u4, SUM(i) FILTER(WHERE f < 3) FROM t GROUP BY u1, u2, u3, u4", "beyond the dense tables"),
    ("SELECT " + ", ".join(f"SUM(i) FILTER(WHERE rng = {k})" for k in range(9)) + " FROM t", "distinct FILTER clauses"),
    ("SELECT SUM(i), SUM(l), SUM(fl), SUM(d), SUM(f) FILTER(WHERE f < 3) FROM t", "aggregated columns"),
    ("SELECT SUM(i) FILTER(WHERE f < 3 AND inv = 1) FROM t WHERE rng < 15", "several predicates"),
]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals(ctx, base, sql, word):
    with pytest.raises(UnsupportedError, match=word) as e:
        ctx.execute(parse_sql(sql), base[0])
    assert e.value.code == N.PH_ERR_UNSUPPORTED


def test_refusals_of_entry_points_and_bad_queries(ctx, base):
    segs = base[0]
    q = parse_sql("SELECT g, SUM(i) FILTER(WHERE f < 3) FROM t GROUP BY g")
    with pytest.raises(UnsupportedError, match="dense partials"):
        ctx.dense_layout(q, segs)
    with pytest.raises(BadQueryError):
        ctx.execute(parse_sql("SELECT SUM(i) FILTER(WHERE nope < 3) FROM t"), segs)
    with pytest.raises(BadQueryError):
        ctx.execute(parse_sql("SELECT SUM(i) FILTER(WHERE f < 'abc') FROM t"), segs)
    # ph_filter_execute ignores aggregation filters, as it ignores aggregations
    words, count, _ = ctx.filter(parse_sql("SELECT SUM(i) FILTER(WHERE f < 3) FROM t WHERE f < 8"), segs[1])
    assert count == int((base[2][1]["f"] < 8).sum())


def test_multi_device_context_refuses(base):
    from pinot_amd.engine import GpuContext
    c = GpuContext(devices=[0, 0])  # two logical shards of one GPU
    try:
        seg = c.pin(both("fa_multi", base[2][1])[0])
        with pytest.raises(UnsupportedError, match="multi-device"):
            c.execute(parse_sql("SELECT SUM(i) FILTER(WHERE f < 3) FROM t"), [seg])
    finally:
        c.close()
