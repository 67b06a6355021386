"""GPU: HISTOGRAM through ph_query_execute against tests/bins_ref.py; counts are compared for equality.  Docs: the
mask-word edges and 769 over two segments with different dictionaries.  Inputs: all docs in one bin (the combining adds
64 at once), or spread over every bin and both out-of-range sides.  Every query carries two HISTOGRAMs over x, one over
y (another stored type) and COUNT(*).  Group 5 holds one doc, out of range; the WHERE clause removes group 6's docs."""
from dataclasses import replace

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import decode, reduce_datatables
from pinot_amd.engine import GpuContext
from pinot_amd.native import UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_segment
from tests.bins_ref import DTYPES, KAT, counts, kat_column

pytestmark = pytest.mark.gpu

MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
ONE_DOC = 13
Y_SQL, Y_EDGES = "HISTOGRAM(y, 0, 100, 4)", ([0.0, 100.0], 4)
BINS = {  # name: (SQL arguments, edges, equal_bins); x lies in [0, 1000) except where out of range
    "b1": ("ARRAY[0, 1000]", [0.0, 1000.0], 0),
    "inf5": ('ARRAY["-Infinity", 10, 500, 990, "Infinity"]', [-np.inf, 10.0, 500.0, 990.0, np.inf], 0),
    "eq10": ("0, 1000, 10", [0.0, 1000.0], 10),
    "eq64": ("0, 1024, 64", [0.0, 1024.0], 64),
    "arr65": ("ARRAY[" + ", ".join(str(16 * k) for k in range(66)) + "]", [16.0 * k for k in range(66)], 0),
    "eq1024": ("0, 1024, 1024", [0.0, 1024.0], 1024)}


def make_table(n, spread, dtype="INT"):
    i = np.arange(n)
    x = (i * 37 % 1000) if spread else np.full(n, 321)
    x = np.where(spread & (i % 11 == 5), -7, np.where(spread & (i % 11 == 8), 4000, x))  # both out-of-range sides
    g = (i % 5).astype(np.int32)
    f = (i % 10).astype(np.int32)
    y = (i * 7 % 120 - 10) * 1.0
    if n > ONE_DOC:
        g[ONE_DOC], x[ONE_DOC], y[ONE_DOC], f[ONE_DOC] = 5, -1, -1.0, 4
    if n > 64:
        g[[30, 31]], f[[30, 31]] = 6, 9
    return {"g": (g, "INT"), "f": (f, "INT"), "x": (x.astype(DTYPES[dtype]), dtype), "y": (y, "DOUBLE"),
            "s": (np.array([f"v{k % 3}" for k in i]), "STRING")}


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def pinned(ctx, name, t, splits=()):
    n = len(t["g"][0])
    bounds = [0] + list(splits) + [n]
    return [ctx.pin(create_segment(f"bins_{name}_{k}", {c: (v[a:b], dt) for c, (v, dt) in t.items()}))
            for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]


def run(ctx, segs, sql, **options):
    for k, v in options.items():
        ctx.set_option(k, v)
    res = ctx.execute(parse_sql(sql), segs)
    for k in options:
        ctx.set_option(k, None)
    return res


def check(res, t, keep, group, specs, mode):
    # specs: (column, edges, equal_bins), or None for COUNT(*), in aggregation order
    assert res.stats.scan_kernel == N.PH_KERNEL_SCAN_BINS == 24 and res.stats.mode == mode
    assert res.stats.num_docs_scanned == int(keep.sum())
    g = t["g"][0]
    rows = sorted(set(g[keep].tolist())) if group else [None]
    assert (sorted(k[0] for k in res.keys) if group else [None]) == rows
    order = {k[0]: r for r, k in enumerate(res.keys)} if group else {None: 0}
    for key in rows:
        sel = keep & (g == key) if group else keep
        for k, spec in enumerate(specs):
            got = res.agg_columns[k][order[key]]
            if spec is None:
                assert got == int(sel.sum())
            else:
                assert got.tolist() == counts(t[spec[0]][0][sel], spec[1], spec[2]).tolist(), (key, k)


def query(bins, other, where, group):
    sql = (f"SELECT {'g, ' if group else ''}HISTOGRAM(x, {BINS[bins][0]}), HISTOGRAM(x, {BINS[other][0]}), {Y_SQL}, "
           f"COUNT(*) FROM t{' WHERE f < 9' if where else ''}{' GROUP BY g LIMIT 100' if group else ''}")
    return sql, [("x",) + BINS[bins][1:], ("x",) + BINS[other][1:], ("y",) + Y_EDGES, None]


@pytest.mark.parametrize("spread", [False, True], ids=["onebin", "spread"])
@pytest.mark.parametrize("bins", list(BINS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 769])
def test_counts_in_every_mode(ctx, n, bins, spread):
    t = make_table(n, spread)
    segs = pinned(ctx, f"{n}_{bins}_{spread}", t, (300,) if n == 769 else ())
    other = "eq10" if bins != "eq10" else "inf5"
    for where in (False, True):
        keep = t["f"][0] < 9 if where else np.ones(n, bool)
        sql, specs = query(bins, other, where, False)
        check(run(ctx, segs, sql), t, keep, False, specs, MODE_AGG)
        check(run(ctx, segs, sql, bins_table_lds_max=0), t, keep, False, specs, MODE_AGG)  # bin tables from HBM
        sql, specs = query(bins, other, where, True)
        row_cells = sum((s[2] or len(s[1]) - 1) + 1 for s in specs[:3])
        lds = len(set(t["g"][0].tolist())) * 4 * row_cells <= 64 * 1024  # choose_mode's lds_bytes
        for tab in (None, 0):  # bin tables staged in LDS, and gathered from HBM
            check(run(ctx, segs, sql, bins_table_lds_max=tab), t, keep, True, specs, MODE_LDS if lds else MODE_HBM)
            check(run(ctx, segs, sql, lds_table_max=0, bins_table_lds_max=tab), t, keep, True, specs, MODE_HBM)


def test_group_table_that_leaves_no_room_for_the_bin_tables(ctx):
    # 39 groups x 1041 cells x 4 bytes = 162 396 of a CU's 163 840 bytes of LDS: the 2 KB of bin tables no longer fit beside
    # them, so they are gathered (a launch that still staged them would be refused as exceeding the LDS)
    t = make_table(769, True)
    t["g"] = ((np.arange(769) % 39).astype(np.int32), "INT")
    sql, specs = query("eq1024", "eq10", False, True)
    res = run(ctx, pinned(ctx, "full", t, (300,)), sql, lds_table_max=160 * 1024)
    check(res, t, np.ones(769, bool), True, specs, MODE_LDS)


@pytest.mark.parametrize("dtype", ["LONG", "FLOAT", "DOUBLE"])
def test_stored_types_and_the_per_doc_decode(ctx, dtype):
    # 70 001 docs with distinct x: a 17-bit column, past the register-direct decode's 16 bits (MODE_AGG's other form)
    i = np.arange(70_001)
    t = make_table(len(i), True, dtype)
    t["x"] = ((i - 2000).astype(t["x"][0].dtype), dtype)
    segs = pinned(ctx, f"wide_{dtype}", t)
    sql = "SELECT HISTOGRAM(x, -1000.5, 60000, 64), HISTOGRAM(x, ARRAY[0, 1, 65536]), COUNT(*) FROM t WHERE f < 9"
    specs = [("x", [-1000.5, 60000.0], 64), ("x", [0.0, 1.0, 65536.0], 0), None]
    check(run(ctx, segs, sql), t, t["f"][0] < 9, False, specs, MODE_AGG)
    grouped = sql.replace("SELECT", "SELECT g,") + " GROUP BY g LIMIT 100"
    check(run(ctx, segs, grouped), t, t["f"][0] < 9, True, specs, MODE_LDS)


def test_rows_bytes_and_datatable(ctx):
    t = make_table(769, True)
    segs = pinned(ctx, "rows", t, (300,))
    sql, specs = query("inf5", "eq10", True, True)
    a, b = run(ctx, segs, sql), run(ctx, segs, sql)
    for x, y in zip(a.agg_columns, b.agg_columns):
        assert x.tobytes() == y.tobytes()
    # the one-doc group appears, all zeros where its value is out of range, COUNT(*) 1; the filtered-out group does not
    row = {k[0]: r for r, k in enumerate(a.keys)}
    assert 6 not in row and a.agg_columns[3][row[5]] == 1
    assert not a.agg_columns[1][row[5]].any() and not a.agg_columns[2][row[5]].any()
    # an aggregation-only query that matched nothing: B zeros
    none = run(ctx, segs, "SELECT HISTOGRAM(x, 0, 1000, 10), COUNT(*) FROM t WHERE f > 100")
    assert none.num_groups == 1 and none.agg_columns[0].tolist() == [[0.0] * 10] and none.agg_columns[1].tolist() == [0]
    # a DataTable round trip: each segment's response decoded and merged by the broker reduce
    q = parse_sql(sql)
    merged = reduce_datatables(q, [decode(ctx.execute_datatable(q, [s])) for s in segs])
    assert merged.columns[1] == "histogram(x)" and merged.rows == reduce_groups(q, a.keys, a.aggs).rows


def test_known_answers_of_the_reference_test(ctx):
    seg = ctx.pin(create_segment("bins_kat", {c: (kat_column(c), d["type"]) for c, d in KAT["columns"].items()}))
    for case in KAT["cases"]:
        res = ctx.execute(parse_sql(case["sql"]), [seg])
        assert res.agg_columns[0].tolist() == [case["expected"]], case["sql"]
        assert res.stats.num_docs_scanned == case["docs"] and res.stats.scan_kernel == 24


REFUSALS = [
    ("SELECT HISTOGRAM(s, 0, 10, 2) FROM t", "STRING column"),
    ("SELECT HISTOGRAM(x, 0, 10, 2), SUM(x) FROM t", "SUM beside a histogram"),
    ("SELECT HISTOGRAM(x, 0, 10, 2), VAR_POP(x) FROM t", "variance function beside a histogram"),
    ("SELECT HISTOGRAM(x, 0, 10, 2) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
    ("SELECT HISTOGRAM(x, 0, 10, 2), COUNT(*) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
    ("SET minSegmentGroupTrimSize=5; SELECT g, HISTOGRAM(x, 0, 10, 2) FROM t GROUP BY g ORDER BY g LIMIT 2",
     "segment group trim"),
    ("SET numGroupsLimit=3; SELECT g, HISTOGRAM(x, 0, 10, 2) FROM t GROUP BY g LIMIT 2", "numGroupsLimit"),
    ("SELECT HISTOGRAM(x, 0, 2000, 1025) FROM t", "more than 1024 bins"),
    ("SELECT HISTOGRAM(x, 0, 10, 1), HISTOGRAM(x, 0, 10, 2), HISTOGRAM(x, 0, 10, 3), HISTOGRAM(x, 0, 10, 4), "
     "HISTOGRAM(x, 0, 10, 5) FROM t", "more than 4 distinct"),
    ("SELECT HISTOGRAM(y, 0, 1, 3) FROM t", "out of bounds"),  # y holds the double below 1: its bin id reaches 3
    # columns a to d hold 1025 values each: 1025^4 keys are more than 2^40; 1025^2 keys of four 1024-bin histograms
    # (4 x 1025 cells and 4 x 1024 doubles a key) are 52 GB of tables, more than the 32 GB a query may allocate
    ("SELECT HISTOGRAM(x, 0, 10, 2) FROM t GROUP BY a, b, c, d LIMIT 2", "key space beyond the dense tables"),
    ("SELECT " + ", ".join(f"HISTOGRAM(x, 0, {5000 + k}, 1024)" for k in range(4)) + " FROM t GROUP BY a, b LIMIT 2",
     "key space beyond the dense tables"),
]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals(ctx, sql, word):
    t = make_table(1025, True)
    t["y"][0][3] = np.nextafter(1.0, -np.inf)
    t.update({c: (np.arange(1025, dtype=np.int32), "INT") for c in "abcd"})
    with pytest.raises(UnsupportedError, match=word):
        ctx.execute(parse_sql(sql), pinned(ctx, "refuse", t))


def test_other_entry_points_refuse(ctx):
    segs = pinned(ctx, "entry", make_table(65, True))
    q = parse_sql("SELECT HISTOGRAM(x, 0, 10, 2) FROM t")
    with pytest.raises(UnsupportedError, match="dense partials"):
        ctx.dense_layout(q, segs)
    multi = GpuContext(devices=[0, 0])
    with pytest.raises(UnsupportedError, match="multi-device"):
        multi.execute(q, [])
    multi.close()
    q.aggregations[0] = replace(q.aggregations[0], column2="y", op="+")  # (the parser yields no expression argument)
    with pytest.raises(UnsupportedError, match="2-operand expression"):
        ctx.execute(q, segs)
