"""GPU: exact PERCENTILE through the C-ABI (ph_query_execute + ph_result_percentile_*): final values, raw histograms,
dictionary values, group keys and the statistics.  Expected answers: the reference's own known answers
(tests/golden/percentile_kat.json) and, everywhere else, a numpy sort of the values of the docs oracle.filter_docs
matches, element (int)(n * p / 100) (PercentileAggregationFunction.java:146-158)."""
import json
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.datatable import DOUBLE_LIST_OBJECT_TYPE, decode, double_list_deserialize, reduce_datatables
from pinot_amd.query import PERCENTILE, AggregationSpec, QueryContext, SelectItem, parse_sql
from pinot_amd.reduce import final_value, reduce_groups
from pinot_amd.segment import create_segment
from tests import kat_sv

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "percentile_kat.json")))
MODE_AGG, MODE_GROUP_LDS, MODE_GROUP_GLOBAL = 1, 2, 3
KERNEL_HIST_LDS, KERNEL_HIST_HBM = 18, 19  # ph_exec_stats.scan_kernel: where the scan kept the histograms


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


class Table:
    """Segments pinned once: their column dicts, oracle segments and pinned handles."""

    def __init__(self, ctx, seg_cols, **kw):
        self.cols = seg_cols
        self.ora = [O.build_segment(f"s{i}", c, inverted=kw.get("inverted", ()), range_index=kw.get("range_index", ()))
                    for i, c in enumerate(seg_cols)]
        self.gpu = [ctx.pin(create_segment(f"s{i}", c, **kw)) for i, c in enumerate(seg_cols)]


def final_of(sorted_values, p):
    """The reference's final result over the ascending values of the column's stored type, converted to double last."""
    n = len(sorted_values)
    if n == 0:
        return -math.inf
    if p == 100:
        return float(sorted_values[-1])
    return float(sorted_values[min(n - 1, int(float(n) * p / 100.0))])


def expected(t, q):
    """group key -> the matched values of every PERCENTILE column (stored type, unsorted), the matched docs, and
    the result dictionary of every PERCENTILE column: the sorted union of the segments' values."""
    groups, matched = {}, 0
    pcols = sorted({a.column for a in q.aggregations if a.function == PERCENTILE})
    for cols, oseg in zip(t.cols, t.ora):
        docs, _ = O.filter_docs(q, oseg)
        matched += int(docs.sum())
        if q.group_by:
            order = {}
            for j, key in enumerate(zip(*[cols[g][0][docs].tolist() for g in q.group_by])):
                order.setdefault(key, []).append(j)
            sel = {key: np.array(rows) for key, rows in order.items()}
        else:
            sel = {(): slice(None)} if docs.any() else {}
        for key, rows in sel.items():
            row = groups.setdefault(key, {c: [] for c in pcols})
            for c in pcols:
                row[c].append(cols[c][0][docs][rows])
    groups = {k: {c: np.concatenate(v) for c, v in row.items()} for k, row in groups.items()}
    dicts = {c: np.unique(np.concatenate([s[c][0] for s in t.cols])) for c in pcols}
    return groups, matched, dicts


def check(ctx, t, sql_or_q, mode=None, limit_rows=None, dicts=None):
    q = parse_sql(sql_or_q) if isinstance(sql_or_q, str) else sql_or_q
    r = ctx.execute(q, t.gpu)
    groups, matched, union = expected(t, q)
    dicts = dicts or union
    if not q.group_by and not groups:
        groups[()] = {a.column: np.zeros(0, dicts[a.column].dtype) for a in q.aggregations if a.function == PERCENTILE}
    if limit_rows is not None:
        groups = {k: v for k, v in groups.items() if k in limit_rows}
    assert r.num_groups == len(groups)
    got_keys = r.keys
    assert sorted(got_keys) == sorted(groups)
    for k, a in enumerate(q.aggregations):
        if a.function != PERCENTILE:
            continue
        col, d = r.agg_columns[k], dicts[a.column]
        assert col.values.dtype == d.dtype and np.array_equal(col.values, d), "result dictionary = sorted value union"
        assert col.hist.shape == (len(groups), len(d))
        for i, key in enumerate(got_keys):
            vals = np.sort(groups[key][a.column])
            hist = np.bincount(np.searchsorted(d, vals), minlength=len(d))
            assert np.array_equal(col.hist[i], hist), (key, a.column)
            exp = final_of(vals, a.percentile)
            assert col.finals[i] == exp, (key, a.column, a.percentile, col.finals[i], exp)
    assert r.stats.num_docs_scanned == matched
    ncols = len(set(q.group_by) | {c for a in q.aggregations for c in a.columns()})
    assert r.stats.num_entries_scanned_post_filter == matched * ncols  # never a metadata answer
    if mode is not None:
        assert r.stats.mode == mode
    assert r.stats.num_entries_scanned_in_filter == sum(O.filter_docs(q, o)[1] for o in t.ora if o.num_docs)
    return r


# ------------------------------------------------------------------ reference known answers
@pytest.fixture(scope="module")
def sv(ctx):
    seg = ctx.pin(create_segment("testTable_126164076_167572854", kat_sv.load_columns(), inverted=kat_sv.INVERTED))
    return [seg] * 4


@pytest.mark.parametrize("kat", KAT["kats"], ids=[f"{i}:{k['source']}" for i, k in enumerate(KAT["kats"])])
def test_reference_kat(ctx, sv, kat):
    q = parse_sql(kat["sql"].replace("{FILTER}", KAT["filter"]))
    r = ctx.execute(q, sv)
    aggs = r.aggs  # (a property: converted once)
    assert reduce_groups(q, r.keys, aggs).rows == kat["rows"], kat["source"]
    docs, in_filter, post, total = kat["stats"]
    assert r.stats.num_docs_scanned == docs and r.stats.num_total_docs == total
    assert r.stats.num_entries_scanned_post_filter == post
    if q.filter is not None:
        assert r.stats.num_entries_scanned_in_filter == in_filter
    assert r.stats.mode != -1 and (q.group_by or r.stats.mode == MODE_AGG)  # the reference scans: no metadata answer
    for k, a in enumerate(q.aggregations):  # the library's finals (rank found on the device) are the reduce's
        assert r.agg_columns[k].finals.tolist() == [final_value(a, aggs[i][k]) for i in range(r.num_groups)]


# ------------------------------------------------------------------ rank edges
@pytest.mark.parametrize("p", [0, 50, 99.9, 100])
def test_rank_edges_tiny(ctx, p):
    c = np.array([40, 10, 10, 30, 20, 7, 7, 7, 7], np.int32)
    f = np.array([1, 2, 2, 0, 2, 3, 3, 3, 3], np.int32)
    t = Table(ctx, [{"c": (c, "INT"), "f": (f, "INT")}])
    r = check(ctx, t, f"SELECT PERCENTILE(c, {p}) FROM t WHERE f = 1", MODE_AGG)  # n = 1
    assert r.agg_columns[0].finals[0] == 40.0
    r = check(ctx, t, f"SELECT PERCENTILE(c, {p}) FROM t WHERE f < 2", MODE_AGG)  # n = 2: 30, 40
    assert r.agg_columns[0].finals[0] == (30.0 if p == 0 else 40.0)
    r = check(ctx, t, f"SELECT PERCENTILE(c, {p}) FROM t WHERE f = 3", MODE_AGG)  # all docs one value
    assert r.agg_columns[0].finals[0] == 7.0 and r.agg_columns[0].hist[0].tolist() == [4, 0, 0, 0, 0]
    r = check(ctx, t, f"SELECT PERCENTILE(c, {p}) FROM t WHERE f > 5", MODE_AGG)  # empty filter
    assert r.num_groups == 1 and r.agg_columns[0].finals[0] == -math.inf and not r.agg_columns[0].hist.any()
    r = check(ctx, t, f"SELECT f, PERCENTILE(c, {p}) FROM t WHERE f > 5 GROUP BY f")
    assert r.num_groups == 0


# ------------------------------------------------------------------ dictionary sizes, both forms
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 16384, 16385])
def test_dictionary_sizes_and_forms(ctx, monkeypatch, d):
    rng = np.random.default_rng(d)
    n = max(500, min(200_000, 4 * d))
    c = rng.permutation(np.arange(n) % d).astype(np.int32) * 3 + 5
    t = Table(ctx, [{"c": (c, "INT"), "f": (rng.integers(0, 10, n).astype(np.int32), "INT")}])
    sql = "SELECT PERCENTILE(c, 0), PERCENTILE50(c), PERCENTILE(c, 99.9), PERCENTILE100(c) FROM t WHERE f < 8"
    lds = check(ctx, t, sql, MODE_AGG)
    # 4 bytes per value under the default 64 KiB bound (16 bytes go to the other tables): D = 16384 no longer fits
    assert lds.stats.scan_kernel == (KERNEL_HIST_LDS if d < 16384 else KERNEL_HIST_HBM)
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    hbm = check(ctx, t, sql, MODE_AGG)
    assert hbm.stats.scan_kernel == KERNEL_HIST_HBM
    monkeypatch.setenv("PH_LDS_TABLE_MAX", str(96 * 1024))
    big = check(ctx, t, sql, MODE_AGG)
    assert big.stats.scan_kernel == KERNEL_HIST_LDS
    for k in range(4):
        assert np.array_equal(lds.agg_columns[k].hist, hbm.agg_columns[k].hist)
        assert np.array_equal(big.agg_columns[k].hist, hbm.agg_columns[k].hist)
        assert np.array_equal(lds.agg_columns[k].finals, hbm.agg_columns[k].finals)
        assert np.array_equal(big.agg_columns[k].finals, hbm.agg_columns[k].finals)
        assert np.array_equal(lds.agg_columns[0].hist, lds.agg_columns[k].hist)  # one column, one histogram


# ------------------------------------------------------------------ no lost updates
def test_one_value_no_lost_updates(ctx, monkeypatch):
    n = 200_000
    f = (np.arange(n) % 10).astype(np.int32)
    t = Table(ctx, [{"c": (np.full(n, 42, np.int32), "INT"), "f": (f, "INT")}])
    for lds_max, kernel in ((None, KERNEL_HIST_LDS), ("0", KERNEL_HIST_HBM)):
        if lds_max:
            monkeypatch.setenv("PH_LDS_TABLE_MAX", lds_max)
        r = check(ctx, t, "SELECT PERCENTILE50(c) FROM t WHERE f < 9", MODE_AGG)
        assert r.stats.scan_kernel == kernel
        assert r.agg_columns[0].hist.tolist() == [[int((f < 9).sum())]] and r.agg_columns[0].finals[0] == 42.0


def test_skewed_column_no_lost_updates(ctx, monkeypatch):
    rng = np.random.default_rng(90)
    n, d = 200_000, 1000
    c = np.where(rng.random(n) < 0.9, 417, rng.integers(0, d, n)).astype(np.int32)
    c[:d] = np.arange(d)
    f = rng.integers(0, 100, n).astype(np.int32)
    t = Table(ctx, [{"c": (c, "INT"), "f": (f, "INT"), "g": ((np.arange(n) % 3).astype(np.int32), "INT")}])
    for lds_max, kernel in ((None, KERNEL_HIST_LDS), ("0", KERNEL_HIST_HBM)):
        if lds_max:
            monkeypatch.setenv("PH_LDS_TABLE_MAX", lds_max)
        r = check(ctx, t, "SELECT PERCENTILE(c, 3), PERCENTILE95(c) FROM t WHERE f < 95", MODE_AGG)
        assert r.stats.scan_kernel == kernel
        assert np.array_equal(r.agg_columns[0].hist[0], np.bincount(c[f < 95], minlength=d))
        g = check(ctx, t, "SELECT g, PERCENTILE(c, 3), PERCENTILE95(c) FROM t WHERE f < 95 GROUP BY g LIMIT 10")
        assert g.stats.scan_kernel == kernel and g.stats.mode == (MODE_GROUP_GLOBAL if lds_max else MODE_GROUP_LDS)


# ------------------------------------------------------------------ remap, table dictionary
@pytest.mark.parametrize("first", [(0, 300), (0, 320)], ids=["all-remapped", "identity-and-remap"])
def test_remap_across_segments(ctx, first):
    rng = np.random.default_rng(5)

    def seg(n, lo, hi):
        c = np.concatenate([np.arange(lo, hi), rng.integers(lo, hi, max(0, n - (hi - lo)))])[:n]
        return {"c": (rng.permutation(c).astype(np.int64) * 1000, "LONG"), "f": (rng.integers(0, 10, n).astype(np.int32), "INT"),
                "g": (rng.integers(0, 4, n).astype(np.int32), "INT")}
    t = Table(ctx, [seg(12345, *first), seg(65, 255, 320), seg(1, 7, 8)])
    for where in ("", " WHERE f < 7"):
        check(ctx, t, "SELECT PERCENTILE(c, 50), PERCENTILE90(c) FROM t" + where, MODE_AGG)
        check(ctx, t, "SELECT g, PERCENTILE(c, 25), COUNT(*) FROM t" + where + " GROUP BY g LIMIT 10", MODE_GROUP_LDS)


def test_table_dictionary():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    try:
        rng = np.random.default_rng(8)
        n, d = 5001, 3000
        v = (rng.integers(0, d // 2, n) * 2).astype(np.int32)
        f = (np.arange(n) % 10).astype(np.int32)
        t = Table(c, [{"c": (v, "INT"), "f": (f, "INT")}])
        full = np.arange(d, dtype=np.int32)
        c.set_table_dictionary("c", "INT", full)
        r = check(c, t, "SELECT PERCENTILE(c, 50), PERCENTILE100(c) FROM t WHERE f < 7", MODE_AGG, dicts={"c": full})
        assert r.agg_columns[0].hist.shape == (1, d) and not r.agg_columns[0].hist[0, 1::2].any()
    finally:
        c.close()


# ------------------------------------------------------------------ every eligible form over one table
@pytest.fixture(scope="module")
def forms_table(ctx):
    rng = np.random.default_rng(11)
    n = 150_001
    return Table(ctx, [{"c": (rng.integers(0, 700, n).astype(np.int32), "INT"),
                        "g": (rng.integers(0, 19, n).astype(np.int32), "INT"),
                        "f": (rng.integers(0, 50, n).astype(np.int32), "INT")}])


def test_group_forms_agree(ctx, forms_table, monkeypatch):
    t = forms_table
    agg = "SELECT PERCENTILE50(c), PERCENTILE90(c), PERCENTILE99(c) FROM t WHERE f < 33"
    grp = "SELECT g, PERCENTILE50(c), PERCENTILE90(c), PERCENTILE99(c) FROM t WHERE f < 33 GROUP BY g LIMIT 100"
    a_lds = check(ctx, t, agg, MODE_AGG)
    g_lds = check(ctx, t, grp, MODE_GROUP_LDS)  # 19 rows x 700 counters = 53 200 bytes
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    a_hbm = check(ctx, t, agg, MODE_AGG)
    g_hbm = check(ctx, t, grp, MODE_GROUP_GLOBAL)
    assert [x.stats.scan_kernel for x in (a_lds, g_lds, a_hbm, g_hbm)] == [
        KERNEL_HIST_LDS, KERNEL_HIST_LDS, KERNEL_HIST_HBM, KERNEL_HIST_HBM]
    for k in range(3):
        assert np.array_equal(a_lds.agg_columns[k].hist, a_hbm.agg_columns[k].hist)
        assert np.array_equal(g_lds.agg_columns[k].hist, g_hbm.agg_columns[k].hist) and g_lds.keys == g_hbm.keys
        assert np.array_equal(g_lds.agg_columns[k].finals, g_hbm.agg_columns[k].finals)
    # the groups' histograms add up to the aggregation-only histogram
    assert np.array_equal(g_hbm.agg_columns[0].hist.sum(axis=0), a_hbm.agg_columns[0].hist[0])


# ------------------------------------------------------------------ combinations
@pytest.fixture(scope="module")
def mixed_table(ctx):
    rng = np.random.default_rng(3)
    n = 60_007
    words = np.array(["", "a", "bb", "naïve", "zz", "日本", "q" * 17])
    cols = {"i": (rng.integers(0, 90, n).astype(np.int32) - 40, "INT"),
            # beyond 2^53: neighbouring values round to the same double, the dictionary keeps them apart
            "l": ((1 << 60) + rng.integers(0, 1500, n).astype(np.int64) * 3 - 700, "LONG"),
            "fl": (rng.integers(0, 300, n).astype(np.float32) / 4, "FLOAT"),
            "d": (np.round(rng.normal(0, 30, n), 1) + 0.0, "DOUBLE"),  # (+ 0.0: no -0.0 beside 0.0)
            "s": (words[rng.integers(0, len(words), n)], "STRING"),
            "r": (rng.integers(0, 5000, n).astype(np.int32) * 7, "INT"),
            "m": (rng.integers(0, 1 << 20, n).astype(np.int32), "INT"),
            "srt": (np.sort(rng.integers(0, 60, n)).astype(np.int32), "INT"),
            "inv": (rng.integers(0, 25, n).astype(np.int32), "INT"),
            "rng": (rng.integers(0, 400, n).astype(np.int32), "INT"),
            "g": (rng.integers(0, 12, n).astype(np.int32), "INT")}
    return Table(ctx, [cols], raw=("r",), inverted=("inv",), range_index=("rng",))


@pytest.mark.parametrize("col", ["i", "l", "fl", "d", "r"])
def test_data_types(ctx, mixed_table, col):
    r = check(ctx, mixed_table,
              f"SELECT PERCENTILE({col}, 50), PERCENTILE99({col}), PERCENTILE100({col}) FROM t WHERE m < 800000", MODE_AGG)
    check(ctx, mixed_table, f"SELECT g, PERCENTILE({col}, 12.5) FROM t WHERE m < 800000 GROUP BY g LIMIT 20")
    if col == "l":  # converted last: the double nearest the picked LONG
        v = np.sort(mixed_table.cols[0]["l"][0][mixed_table.cols[0]["m"][0] < 800000])
        assert r.agg_columns[0].finals[0] == float(int(v[len(v) // 2])) and int(v[len(v) // 2]) > (1 << 53)


def test_string_column_is_refused(ctx, mixed_table):
    _refused(lambda: ctx.execute(parse_sql("SELECT PERCENTILE50(s) FROM t WHERE m < 5000"), mixed_table.gpu),
             "PERCENTILE on STRING column s")
    check(ctx, mixed_table, "SELECT PERCENTILE50(i) FROM t WHERE m < 5000", MODE_AGG)  # still usable


def test_three_percentiles_alone_and_mixed(ctx, mixed_table):
    t = mixed_table
    alone = check(ctx, t, "SELECT PERCENTILE50(i), PERCENTILE90(i), PERCENTILE99(i) FROM t WHERE m > 1000", MODE_AGG)
    sql = ("SELECT PERCENTILE50(i), COUNT(*), SUM(m), PERCENTILE90(i), DISTINCTCOUNTHLL(fl), DISTINCTCOUNT(d), "
           "PERCENTILE99(i) FROM t WHERE m > 1000")
    mixed = check(ctx, t, sql, MODE_AGG)
    assert mixed.stats.scan_kernel == KERNEL_HIST_LDS
    e = O.execute(parse_sql("SELECT COUNT(*), SUM(m) FROM t WHERE m > 1000"), t.ora)
    assert int(mixed.agg_columns[1][0]) == e.aggs[0][0] and float(mixed.agg_columns[2][0]) == e.aggs[0][1]
    hll = ctx.execute(parse_sql("SELECT DISTINCTCOUNTHLL(fl) FROM t WHERE m > 1000"), t.gpu)
    assert np.array_equal(mixed.agg_columns[4][0], hll.agg_columns[0][0]) and hll.agg_columns[0][0].any()
    docs = t.cols[0]["m"][0] > 1000
    assert mixed.agg_columns[5].value_set(0) == frozenset(np.unique(t.cols[0]["d"][0][docs]).tolist())
    for a, b in zip((0, 1, 2), (0, 3, 6)):
        assert np.array_equal(alone.agg_columns[a].finals, mixed.agg_columns[b].finals)
        assert np.array_equal(alone.agg_columns[a].hist, mixed.agg_columns[b].hist)
    # the same mix grouped, in LDS and in HBM tables
    gsql = ("SELECT g, PERCENTILE50(i), COUNT(*), SUM(m), DISTINCTCOUNT(inv), PERCENTILE99(i), PERCENTILE(fl, 75) "
            "FROM t WHERE m > 1000 GROUP BY g LIMIT 20")
    r = check(ctx, t, gsql, MODE_GROUP_LDS)
    e = O.execute(parse_sql("SELECT g, COUNT(*), SUM(m) FROM t WHERE m > 1000 GROUP BY g LIMIT 20"), t.ora)
    exp = dict(zip(e.keys, e.aggs))
    for i, key in enumerate(r.keys):
        assert [int(r.agg_columns[1][i]), float(r.agg_columns[2][i])] == exp[key]
        sel = docs & (t.cols[0]["g"][0] == key[0])
        assert r.agg_columns[3].value_set(i) == frozenset(np.unique(t.cols[0]["inv"][0][sel]).tolist())


@pytest.mark.parametrize("where", ["m < 300000", "inv = 7", "inv IN (1, 2, 24) AND m > 5000", "srt BETWEEN 10 AND 19",
                                   "srt > 40 AND (inv = 3 OR m < 100000)", "rng BETWEEN 100 AND 250",
                                   "rng > 390 AND m > 5000"])
def test_filter_leaves(ctx, mixed_table, where):
    check(ctx, mixed_table, f"SELECT PERCENTILE(d, 50), PERCENTILE95(d) FROM t WHERE {where}", MODE_AGG)
    check(ctx, mixed_table, f"SELECT g, PERCENTILE95(d) FROM t WHERE {where} GROUP BY g LIMIT 20")


def test_num_groups_limit(ctx, mixed_table):
    # the first `limit` keys in doc order are kept (DictionaryBasedGroupKeyGenerator); every matched doc is scanned
    cols = mixed_table.cols[0]
    sql = "SET numGroupsLimit=5; SELECT g, PERCENTILE50(i) FROM t WHERE m < 900000 GROUP BY g LIMIT 20"
    docs = cols["m"][0] < 900000
    first = list(dict.fromkeys(cols["g"][0][docs].tolist()))[:5]
    r = check(ctx, mixed_table, sql, limit_rows={(k,) for k in first})
    assert r.num_groups == 5 and r.stats.num_groups_limit_reached


# ------------------------------------------------------------------ refusals
def _usable(ctx, t):
    check(ctx, t, "SELECT PERCENTILE50(c) FROM t WHERE f < 10", MODE_AGG)


def _refused(call, text):
    with pytest.raises(N.UnsupportedError) as e:
        call()
    assert e.value.code == N.PH_ERR_UNSUPPORTED and text in str(e.value), str(e.value)


def test_refusals(ctx, forms_table):
    t = forms_table
    q = parse_sql("SELECT g, PERCENTILE50(c) FROM t GROUP BY g ORDER BY g LIMIT 5")
    _refused(lambda: ctx.dense_layout(q, t.gpu), "PERCENTILE on dense partials")
    _usable(ctx, t)
    _refused(lambda: ctx.execute_dense(q, t.gpu, [0]), "PERCENTILE on dense partials")
    _usable(ctx, t)
    _refused(lambda: ctx.dense_finalize(q, t.gpu, [0], 0, 1), "PERCENTILE on dense partials")
    _usable(ctx, t)
    trim = parse_sql("SET minSegmentGroupTrimSize=5; SELECT g, PERCENTILE50(c) FROM t GROUP BY g ORDER BY g LIMIT 1")
    _refused(lambda: ctx.execute(trim, t.gpu), "PERCENTILE with segment group trim")
    _usable(ctx, t)
    from pinot_amd.distributed import DistributedQuery
    _refused(lambda: DistributedQuery(ctx).execute(q, t.gpu), "PERCENTILE on dense partials")


def test_refusal_five_columns_and_bad_percentile(ctx):
    n = 300
    cols = {f"c{i}": ((np.arange(n, dtype=np.int32) * (i + 1)) % 17, "INT") for i in range(5)}
    cols["f"] = ((np.arange(n) % 4).astype(np.int32), "INT")
    t = Table(ctx, [cols])
    five = "SELECT " + ", ".join(f"PERCENTILE50(c{i})" for i in range(5)) + " FROM t WHERE f < 3"
    _refused(lambda: ctx.execute(parse_sql(five), t.gpu), "too many PERCENTILE columns")
    check(ctx, t, "SELECT " + ", ".join(f"PERCENTILE50(c{i})" for i in range(4)) + " FROM t WHERE f < 3", MODE_AGG)
    for bad in (101.0, -0.5, math.nan):  # the parser refuses these; through the C ABI they are BAD_QUERY
        q = QueryContext(select=[SelectItem("aggregation", 0)], aggregations=[AggregationSpec(PERCENTILE, "c0", percentile=bad)])
        with pytest.raises(N.BadQueryError) as e:
            ctx.execute(q, t.gpu)
        assert e.value.code == N.PH_ERR_BAD_QUERY and "Invalid percentile" in str(e.value)
    expr = QueryContext(select=[SelectItem("aggregation", 0)],
                        aggregations=[AggregationSpec(PERCENTILE, "c0", column2="c1", op="*", percentile=50.0)])
    _refused(lambda: ctx.execute(expr, t.gpu), "PERCENTILE of an expression")


def test_refusal_multi_device(forms_table):
    from pinot_amd.engine import GpuContext
    m = GpuContext(devices=[0, 0])
    try:
        seg = m.pin(create_segment("m0", forms_table.cols[0]))
        _refused(lambda: m.execute(parse_sql("SELECT PERCENTILE50(c) FROM t WHERE f < 3"), [seg]), "multi-device")
        r = m.execute(parse_sql("SELECT COUNT(*) FROM t WHERE f < 3"), [seg])  # still usable
        assert int(r.agg_columns[0][0]) == int((forms_table.cols[0]["f"][0] < 3).sum())
    finally:
        m.close()


def test_refusal_budget_and_key_space():
    # planner arithmetic only: large table dictionaries over a small segment, nothing of that size is allocated
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    try:
        n = 1000
        cols = {"c": (np.arange(n, dtype=np.int32), "INT"), "g": (np.arange(n, dtype=np.int32) % 7, "INT"),
                "h": (np.arange(n, dtype=np.int32) % 5, "INT")}
        t = Table(c, [cols])
        full = np.arange(200_000, dtype=np.int32)
        c.set_table_dictionary("c", "INT", full)
        c.set_table_dictionary("g", "INT", np.arange(1_000_000, dtype=np.int32))
        _refused(lambda: c.execute(parse_sql("SELECT g, PERCENTILE50(c) FROM t GROUP BY g"), t.gpu), "dense table budget")
        c.set_table_dictionary("h", "INT", np.arange(1_000_000, dtype=np.int32))
        _refused(lambda: c.execute(parse_sql("SELECT g, h, PERCENTILE50(c) FROM t GROUP BY g, h"), t.gpu),
                 "beyond the dense tables")
        # the context still answers; the histogram is over the table dictionary now
        r = check(c, t, "SELECT PERCENTILE50(c) FROM t WHERE g < 3", MODE_AGG, dicts={"c": full})
        assert r.agg_columns[0].hist.shape == (1, 200_000) and r.stats.scan_kernel == KERNEL_HIST_HBM
    finally:
        c.close()


# ------------------------------------------------------------------ star-tree fallback, DataTable
def test_star_tree_segment_scans_its_docs(ctx):
    from pinot_amd.startree import attach
    from tests.test_startree_cpu import make_star, star_table
    cols = star_table(np.random.default_rng(2), 5000)
    seg, st, oseg, _ = make_star(cols, name="pctst")
    p = ctx.pin(seg)
    attach(p, st)
    served = ctx.execute(parse_sql("SELECT d1, COUNT(*) FROM t GROUP BY d1"), [p])
    assert served.stats.num_segments_star_tree == 1
    t = Table.__new__(Table)
    t.cols, t.ora, t.gpu = [cols], [oseg], [p]
    for sql in ("SELECT d1, COUNT(*), PERCENTILE50(m) FROM t GROUP BY d1", "SELECT PERCENTILE90(d3) FROM t WHERE d1 = 10"):
        r = check(ctx, t, sql)
        assert r.stats.num_segments_star_tree == 0


@pytest.mark.parametrize("sql", [
    "SELECT PERCENTILE50(i), PERCENTILE(l, 90), PERCENTILE(fl, 99.9), PERCENTILE(d, '25'), COUNT(*) FROM t WHERE m < 700000",
    "SELECT g, PERCENTILE95(d), percentile(i, 5) FROM t WHERE m < 700000 GROUP BY g ORDER BY PERCENTILE95(d) DESC, g LIMIT 20",
    "SELECT g, PERCENTILE50(i) FROM t WHERE m < 0 GROUP BY g LIMIT 20"])
def test_datatable(ctx, mixed_table, sql):
    q = parse_sql(sql)
    dt = decode(ctx.execute_datatable(q, mixed_table.gpu))
    nk = len(q.group_by)
    assert dt.column_names[nk:] == [a.result_name() for a in q.aggregations]
    assert all(tp == ("LONG" if a.function == "COUNT" else "OBJECT") for tp, a in zip(dt.column_types[nk:], q.aggregations))
    # framing as DataTableImplV4.getCustomObject reads it: each OBJECT cell is (offset, length) of the serialised
    # object, the objectType int standing before it and outside the length; the objects tile the variable section
    end = 0
    for (vo, ln), cell in zip(dt.object_spans, [v for row in dt.rows for v in row if isinstance(v, tuple)]):
        assert vo == end and vo + 4 + ln <= dt.variable_size
        end = vo + 4 + ln
        otype, payload = cell
        assert otype == DOUBLE_LIST_OBJECT_TYPE and len(payload) == ln
        assert ln == 4 + 8 * double_list_deserialize(payload).size  # 8 bytes per matched doc, as the reference's
    assert end == dt.variable_size, "the last object ends the variable-size section"
    # each row's list is the sorted matched values, as doubles
    groups, _, _ = expected(mixed_table, q)
    for row in dt.rows:
        key = tuple(row[:nk])
        for a, cell in zip(q.aggregations, row[nk:]):
            if a.function == PERCENTILE:
                got = np.frombuffer(cell[1], ">f8", offset=4)
                assert np.array_equal(got, np.sort(groups[key][a.column]).astype(np.float64)), (key, a.column)
    r = ctx.execute(q, mixed_table.gpu)
    assert reduce_datatables(q, [dt]).rows == reduce_groups(q, r.keys, r.aggs).rows


def test_broker_reduce_of_two_calls_equals_one_call(ctx):
    rng = np.random.default_rng(21)

    def seg(n, lo, hi):
        return {"c": (rng.integers(lo, hi, n).astype(np.int32) * 5, "INT"), "g": (rng.integers(0, 6, n).astype(np.int32), "INT"),
                "f": (rng.integers(0, 10, n).astype(np.int32), "INT")}
    t = Table(ctx, [seg(7000, 0, 400), seg(3001, 300, 900), seg(501, 2000, 2100)])
    for sql in ("SELECT PERCENTILE50(c), PERCENTILE(c, 99.9) FROM t WHERE f < 8",
                "SELECT g, PERCENTILE90(c), COUNT(*) FROM t WHERE f < 8 GROUP BY g ORDER BY g LIMIT 10"):
        q = parse_sql(sql)
        # two servers: their calls have different result dictionaries, the broker merges by value
        parts = [decode(ctx.execute_datatable(q, t.gpu[:1])), decode(ctx.execute_datatable(q, t.gpu[1:]))]
        whole = ctx.execute(q, t.gpu)
        rows = reduce_datatables(q, parts).rows
        assert rows == reduce_groups(q, whole.keys, whole.aggs).rows
        assert rows == reduce_datatables(q, [decode(ctx.execute_datatable(q, t.gpu))]).rows
        check(ctx, t, q)
