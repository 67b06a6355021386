"""GPU: FIRSTWITHTIME / LASTWITHTIME through parse_sql + ph_query_execute against a numpy reference written here; values
and times are compared for equality (floats bit-equal).  Docs: the mask-word edges, 2113 (a full register-direct tile
and a partial one) and 769 over two segments with different dictionaries.  Every query carries four data columns of one
slot (every stored type; an INT column declared LONG, a FLOAT column declared DOUBLE), a second slot in the other
direction and COUNT(*).  Group 5 holds one doc; the WHERE clause removes group 6's docs."""
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

pytestmark = pytest.mark.gpu

MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
ONE_DOC = 13
# (data column, declared type) of the first slot, then of the second
AGGS = [("a", "INT"), ("d", "FLOAT"), ("e", "LONG"), ("h", "DOUBLE")], [("c", "LONG"), ("b", "DOUBLE")]


def java_long(x):
    x = np.nan_to_num(np.trunc(np.asarray(x, np.float64)), nan=0.0)
    return np.clip(x, -2.0 ** 63, 2.0 ** 63 - 1025).astype(np.int64)


def make_table(n, pattern, ttype):
    i = np.arange(n, dtype=np.int64)
    t = {"asc": i, "desc": n - i, "const": np.full(n, 7), "perm": i * 37 % 50}[pattern]
    if ttype == "LONG":
        ts, t64 = t * ((1 << 33) + 1), t * ((1 << 33) + 1)  # beyond 2^32: the key holds ranks, not values
    elif ttype == "DOUBLE":
        ts = t // 2 + np.where(i % 2 == 1, 0.9, 0.2)  # 1.2 and 1.9 tie only after the (long) cast
        t64 = java_long(ts)
    else:
        ts, t64 = t.astype(np.int32), t
    g, f = (i % 5).astype(np.int32), (i % 10).astype(np.int32)
    if n > ONE_DOC:
        g[ONE_DOC], f[ONE_DOC] = 5, 4
    if n > 64:
        g[[30, 31]], f[[30, 31]] = 6, 9
    cols = {"g": (g, "INT"), "f": (f, "INT"), "ts": (ts, ttype), "a": ((i * 3 - 1000).astype(np.int32), "INT"),
            "b": (i * 0.5 - 3, "DOUBLE"), "c": (i * (1 << 33) - 5, "LONG"), "d": ((i * 0.1).astype(np.float32), "FLOAT"),
            "e": ((7 * i).astype(np.int32), "INT"), "h": ((i * 0.3).astype(np.float32), "FLOAT"),
            "s": (np.array([f"v{k % 3}" for k in i]), "STRING")}
    return cols, t64


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def pinned(ctx, name, t, splits=()):
    n = len(t["g"][0])
    bounds = [0] + list(splits) + [n]
    return [ctx.pin(create_segment(f"wt_{name}_{k}", {c: (v[a:b], dt) for c, (v, dt) in t.items()}))
            for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]


def run(ctx, segs, sql, **options):
    for k, v in options.items():
        ctx.set_option(k, v)
    res = ctx.execute(parse_sql(sql), segs)
    for k in options:
        ctx.set_option(k, None)
    return res


def winner(t64, sel, seg_of, last):
    """The doc a row selects: the extreme time over the matched docs in call order, then the last index holding it
    within the earliest segment that has it."""
    idx = np.flatnonzero(sel)
    if not len(idx):
        return None
    hold = idx[t64[idx] == (t64[idx].max() if last else t64[idx].min())]
    return hold[seg_of[hold] == seg_of[hold].min()][-1]


def expected(t, t64, w, col, declared, last):
    if w is None:
        value = {"INT": -(1 << 31), "LONG": -(1 << 63)}.get(declared, float("nan"))
        return value, -(1 << 63) if last else (1 << 63) - 1
    v = t[col][0][w]
    return (int(v) if declared in ("INT", "LONG") else float(v)), int(t64[w])


def same(got, want):
    if isinstance(want, float):
        return np.isnan(got) if np.isnan(want) else np.float64(got).tobytes() == np.float64(want).tobytes()
    return int(got) == want


def query(last, where, group):
    dirs = ("LASTWITHTIME", "first_with_time") if last else ("FirstWithTime", "LAST_WITH_TIME")
    calls = [f"{dirs[s]}({c}, ts, '{d}')" for s in (0, 1) for c, d in AGGS[s]]
    return (f"SELECT {'g, ' if group else ''}{', '.join(calls)}, COUNT(*) FROM t{' WHERE f < 9' if where else ''}"
            f"{' GROUP BY g LIMIT 100' if group else ''}")


def check(res, t, t64, seg_of, keep, group, last, mode):
    assert res.stats.scan_kernel == N.PH_KERNEL_SCAN_WITHTIME == 25 and res.stats.mode == mode
    assert res.stats.num_docs_scanned == int(keep.sum())
    assert res.stats.num_entries_scanned_post_filter == int(keep.sum()) * (7 + group)
    g = t["g"][0]
    rows = sorted(set(g[keep].tolist())) if group else [None]
    assert (sorted(k[0] for k in res.keys) if group else [None]) == rows
    order = {k[0]: r for r, k in enumerate(res.keys)} if group else {None: 0}
    for key in rows:
        sel = keep & (g == key) if group else keep
        k = 0
        for s in (0, 1):
            w = winner(t64, sel, seg_of, last == (s == 0))
            for col, declared in AGGS[s]:
                got = res.agg_columns[k][order[key]]
                want = expected(t, t64, w, col, declared, last == (s == 0))
                assert same(got["value"], want[0]) and int(got["time"]) == want[1], (key, col, got, want)
                k += 1
        assert res.agg_columns[k][order[key]] == int(sel.sum())


@pytest.mark.parametrize("ttype", ["INT", "LONG", "DOUBLE"])
@pytest.mark.parametrize("pattern", ["asc", "desc", "const", "perm"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2113, 769])
def test_pairs_in_every_mode(ctx, n, pattern, ttype):
    t, t64 = make_table(n, pattern, ttype)
    splits = (300,) if n == 769 else ()
    segs = pinned(ctx, f"{n}_{pattern}_{ttype}", t, splits)
    seg_of = (np.arange(n) >= 300).astype(int) if splits else np.zeros(n, int)
    for last in (True, False):
        for where in (False, True):
            keep = t["f"][0] < 9 if where else np.ones(n, bool)
            sql = query(last, where, False)
            check(run(ctx, segs, sql), t, t64, seg_of, keep, False, last, MODE_AGG)  # register-direct
            check(run(ctx, segs, sql, withtime_table_lds_max=0), t, t64, seg_of, keep, False, last, MODE_AGG)
            sql = query(last, where, True)
            for tab in (None, 0):  # time-rank tables staged in LDS, and gathered from HBM
                check(run(ctx, segs, sql, withtime_table_lds_max=tab), t, t64, seg_of, keep, True, last, MODE_LDS)
                check(run(ctx, segs, sql, lds_table_max=0, withtime_table_lds_max=tab), t, t64, seg_of, keep, True, last,
                      MODE_HBM)
            check(run(ctx, segs, sql, withtime_no_combine=1), t, t64, seg_of, keep, True, last, MODE_LDS)


@pytest.mark.parametrize("pattern", ["asc", "perm"])
def test_the_per_doc_decode_of_wide_time_columns(ctx, pattern):
    # 70 001 docs: ascending times are distinct, a 17-bit column past the register-direct decode's 16 bits (MODE_AGG's
    # other form; its 280 KB of time ranks are gathered); "perm" keeps 50 times and runs the grouped modes at this size
    n = 70_001
    t, t64 = make_table(n, pattern, "LONG")
    segs = pinned(ctx, f"wide_{pattern}", t)
    seg_of, keep = np.zeros(n, int), t["f"][0] < 9
    for last in (True, False):
        check(run(ctx, segs, query(last, True, False)), t, t64, seg_of, keep, False, last, MODE_AGG)
        check(run(ctx, segs, query(last, True, True)), t, t64, seg_of, keep, True, last, MODE_LDS)


def test_defaults_rows_and_datatable(ctx):
    t, t64 = make_table(769, "perm", "INT")
    segs = pinned(ctx, "rows", t, (300,))
    # an aggregation-only query that matched nothing: the default pairs
    none = run(ctx, segs, query(True, False, False).replace("FROM t", "FROM t WHERE f > 100"))
    check(none, t, t64, np.zeros(769, int), np.zeros(769, bool), False, True, MODE_AGG)
    assert none.num_groups == 1 and np.isnan(none.agg_columns[1]["value"][0])
    # a DataTable round trip: each segment's response decoded and merged by the broker reduce, the first server kept on ties
    sql = query(True, True, True)
    q, a = parse_sql(sql), run(ctx, segs, sql)
    merged = reduce_datatables(q, [decode(ctx.execute_datatable(q, [s])) for s in segs])
    assert merged.columns[1] == "lastwithtime(a,ts,'INT')" and merged.columns[5] == "firstwithtime(c,ts,'LONG')"
    assert merged.rows == reduce_groups(q, a.keys, a.aggs).rows


REFUSALS = [
    ("SELECT LASTWITHTIME(a, ts, 'STRING') FROM t", "declared type STRING"),
    ("SELECT LASTWITHTIME(a, ts, 'BOOLEAN') FROM t", "declared type BOOLEAN"),
    ("SELECT LASTWITHTIME(c, ts, 'INT') FROM t", "declaring INT over LONG column c"),
    ("SELECT FIRSTWITHTIME(a, ts, 'FLOAT') FROM t", "declaring FLOAT over INT column a"),
    ("SELECT LASTWITHTIME(s, ts, 'INT') FROM t", "STRING column s"),
    ("SELECT LASTWITHTIME(a, s, 'INT') FROM t", "STRING column s"),
    ("SELECT LASTWITHTIME(a, ts, 'INT'), SUM(a) FROM t", "SUM beside a with-time"),
    ("SELECT LASTWITHTIME(a, ts, 'INT'), VAR_POP(a) FROM t", "variance function beside a with-time"),
    ("SELECT LASTWITHTIME(a, ts, 'INT'), HISTOGRAM(a, 0, 10, 2) FROM t", "histogram function beside a with-time"),
    ("SELECT LASTWITHTIME(a, ts, 'INT') FILTER(WHERE f < 3) FROM t", "FILTER clause"),
    ("SELECT LASTWITHTIME(a, ts, 'INT'), COUNT(*) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
    ("SET minSegmentGroupTrimSize=5; SELECT g, LASTWITHTIME(a, ts, 'INT') FROM t GROUP BY g ORDER BY g LIMIT 2",
     "segment group trim"),
    ("SET numGroupsLimit=3; SELECT g, LASTWITHTIME(a, ts, 'INT') FROM t GROUP BY g LIMIT 2", "numGroupsLimit"),
    ("SELECT " + ", ".join(f"{fn}(a, {c}, 'INT')" for c in ("ts", "f", "g") for fn in ("LASTWITHTIME", "FIRSTWITHTIME"))
     + " FROM t", "more than 4 distinct"),
    # columns w to z hold 1025 values each: 1025^4 keys are more than 2^40
    ("SELECT LASTWITHTIME(a, ts, 'INT') FROM t GROUP BY w, x, y, z LIMIT 2", "key space beyond the dense tables"),
]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[f"{k}-{w}" for k, (_, w) in enumerate(REFUSALS)])
def test_refusals(ctx, sql, word):
    t, _ = make_table(1025, "perm", "INT")
    t.update({c: (np.arange(1025, dtype=np.int32), "INT") for c in "wxyz"})
    with pytest.raises(UnsupportedError, match=word):
        ctx.execute(parse_sql(sql), pinned(ctx, "refuse", t))


def test_other_entry_points_refuse(ctx):
    segs = pinned(ctx, "entry", make_table(65, "asc", "INT")[0])
    q = parse_sql("SELECT LASTWITHTIME(a, ts, 'INT') FROM t")
    with pytest.raises(UnsupportedError, match="dense partials"):
        ctx.dense_layout(q, segs)
    multi = GpuContext(devices=[0, 0])
    with pytest.raises(UnsupportedError, match="multi-device"):
        multi.execute(q, [])
    multi.close()
    q.aggregations[0] = replace(q.aggregations[0], op="+")  # (the parser yields no expression argument)
    with pytest.raises(UnsupportedError, match="2-operand expression"):
        ctx.execute(q, segs)
