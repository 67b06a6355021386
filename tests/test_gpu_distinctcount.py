"""GPU: exact DISTINCTCOUNT through the C-ABI (ph_query_execute + ph_result_distinct_*): counts, raw bitset words,
dictionary values, group keys and the statistics.  Expected answers: the reference's own known answers
(tests/golden/distinctcount_kat.json) and, everywhere else, np.unique over the docs oracle.filter_docs matches."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.datatable import decode, reduce_datatables, set_deserialize
from pinot_amd.query import (DISTINCTCOUNT, AggregationSpec, QueryContext, SelectItem, parse_sql)
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_segment
from tests import kat_sv

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distinctcount_kat.json")))
MODE_AGG, MODE_GROUP_LDS, MODE_GROUP_GLOBAL = 1, 2, 3
KERNEL_DISTINCT_LDS, KERNEL_DISTINCT_HBM = 16, 17  # ph_exec_stats.scan_kernel: where the scan kept the bitsets


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
        self.ora = [O.build_segment(f"s{i}", c, inverted=kw.get("inverted", ())) for i, c in enumerate(seg_cols)]
        self.gpu = [ctx.pin(create_segment(f"s{i}", c, **kw)) for i, c in enumerate(seg_cols)]


def expected(t, q):
    """group key -> one value set per aggregation slot (None for the others), the matched docs, and the result
    dictionary of every DISTINCTCOUNT column: the sorted union of the segments' values."""
    groups, matched = {}, 0
    for cols, oseg in zip(t.cols, t.ora):
        docs, _ = O.filter_docs(q, oseg)
        matched += int(docs.sum())
        keys = list(zip(*[cols[g][0][docs].tolist() for g in q.group_by])) if q.group_by else [()] * int(docs.sum())
        rows_of = {}
        for j, key in enumerate(keys):
            rows_of.setdefault(key, []).append(j)
        for key, rows in rows_of.items():
            row = groups.setdefault(key, [set() if a.function == DISTINCTCOUNT else None for a in q.aggregations])
            for k, a in enumerate(q.aggregations):
                if a.function == DISTINCTCOUNT:
                    row[k] |= set(np.unique(cols[a.column][0][docs][rows]).tolist())
    dicts = {a.column: np.unique(np.concatenate([c[a.column][0] for c in t.cols]))
             for a in q.aggregations if a.function == DISTINCTCOUNT}
    return groups, matched, dicts


def bitset(values, dictionary):
    ids = np.searchsorted(dictionary, np.array(sorted(values), dictionary.dtype))
    w = np.zeros(max(1, (len(dictionary) + 31) // 32), np.uint32)
    np.bitwise_or.at(w, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return w


def check(ctx, t, sql_or_q, mode=None, limit_rows=None):
    q = parse_sql(sql_or_q) if isinstance(sql_or_q, str) else sql_or_q
    r = ctx.execute(q, t.gpu)
    groups, matched, dicts = expected(t, q)
    if not q.group_by and not groups:
        groups[()] = [set() if a.function == DISTINCTCOUNT else None for a in q.aggregations]
    if limit_rows is not None:
        groups = {k: v for k, v in groups.items() if k in limit_rows}
    assert r.num_groups == len(groups)
    got_keys = r.keys
    assert sorted(got_keys) == sorted(groups)
    for k, a in enumerate(q.aggregations):
        if a.function != DISTINCTCOUNT:
            continue
        col, d = r.agg_columns[k], dicts[a.column]
        vals = np.array(col.values, d.dtype) if isinstance(col.values, list) else col.values
        assert np.array_equal(vals, d), "result dictionary = sorted value union"
        assert col.bits.shape == (len(groups), max(1, (len(d) + 31) // 32))
        for i, key in enumerate(got_keys):
            exp = groups[key][k]
            assert int(col.counts[i]) == len(exp), (key, a.column)
            assert np.array_equal(col.bits[i], bitset(exp, d)), (key, a.column)
    assert r.stats.num_docs_scanned == matched
    ncols = len(set(q.group_by) | {c for a in q.aggregations for c in a.columns()})
    metadata = q.filter is None and not q.group_by and all(a.function != "SUM" for a in q.aggregations)
    assert r.stats.num_entries_scanned_post_filter == (0 if metadata else matched * ncols)
    if mode is not None:
        assert r.stats.mode == (-1 if metadata else mode)
    # the filter statistic: exactly the oracle's iterator trees' for the same filter
    assert r.stats.num_entries_scanned_in_filter == sum(O.filter_docs(q, o)[1] for o in t.ora if o.num_docs)
    return r


# ------------------------------------------------------------------ reference known answers
@pytest.fixture(scope="module")
def sv(ctx):
    seg = ctx.pin(create_segment("testTable_126164076_167572854", kat_sv.load_columns(), inverted=kat_sv.INVERTED))
    return [seg] * 4


@pytest.mark.parametrize("kat", KAT["kats"], ids=[k["source"] for k in KAT["kats"]])
def test_reference_kat(ctx, sv, kat):
    q = parse_sql(kat["sql"].replace("{FILTER}", KAT["filter"]))
    r = ctx.execute(q, sv)
    assert reduce_groups(q, r.keys, r.aggs).rows == kat["rows"], kat["source"]
    docs, in_filter, post, total = kat["stats"]
    assert r.stats.num_docs_scanned == docs and r.stats.num_total_docs == total
    assert r.stats.num_entries_scanned_post_filter == post
    if q.filter is not None:
        assert r.stats.num_entries_scanned_in_filter == in_filter
    assert (r.stats.mode == -1) == kat["metadata"]
    for k in range(len(q.aggregations)):  # the device's popcounts are the set sizes
        col = r.agg_columns[k]
        assert [int(c) for c in col.counts] == [len(col.value_set(i)) for i in range(r.num_groups)]


# ------------------------------------------------------------------ word boundaries, remap, contention
@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 65, 2049])
def test_word_boundaries(ctx, d):
    rng = np.random.default_rng(d)
    n = max(200, 3 * d)
    c = rng.permutation(np.arange(n) % d).astype(np.int32) * 3 + 5
    keep = ((c // 3) % 2 == 0) | (c == c.max())  # the last value of the dictionary stays present
    t = Table(ctx, [{"c": (c, "INT"), "k": (keep.astype(np.int32), "INT"), "g": ((np.arange(n) % 3).astype(np.int32), "INT")}])
    r = check(ctx, t, "SELECT DISTINCTCOUNT(c) FROM t WHERE k = 1", MODE_AGG)
    assert (r.agg_columns[0].bits[0, -1] >> ((d - 1) & 31)) & 1 == 1
    check(ctx, t, "SELECT g, DISTINCTCOUNT(c) FROM t WHERE k = 1 GROUP BY g LIMIT 10", MODE_GROUP_LDS)
    check(ctx, t, "SELECT DISTINCTCOUNT(c) FROM t", MODE_AGG)  # metadata: every bit below D, none past it


@pytest.mark.parametrize("first", [(0, 300), (0, 320)], ids=["all-remapped", "identity-and-remap"])
def test_remap_across_segments(ctx, first):
    rng = np.random.default_rng(5)
    def seg(n, lo, hi):
        c = np.concatenate([np.arange(lo, hi), rng.integers(lo, hi, max(0, n - (hi - lo)))])[:n]
        return {"c": (rng.permutation(c).astype(np.int64) * 1000, "LONG"), "f": (rng.integers(0, 10, n).astype(np.int32), "INT"),
                "g": (rng.integers(0, 4, n).astype(np.int32), "INT")}
    t = Table(ctx, [seg(12345, *first), seg(65, 255, 320), seg(1, 7, 8)])
    for where in ("", " WHERE f < 7"):
        check(ctx, t, "SELECT DISTINCTCOUNT(c) FROM t" + where, MODE_AGG)
        check(ctx, t, "SELECT g, DISTINCTCOUNT(c), COUNT(*) FROM t" + where + " GROUP BY g LIMIT 10", MODE_GROUP_LDS)


@pytest.mark.parametrize("d,n", [(1, 100_000), (100_000, 100_000), (2, 20_011), (256, 20_011)],
                         ids=["one-value", "all-distinct-17bit", "1bit", "8bit"])
def test_contention_and_spread(ctx, monkeypatch, d, n):
    rng = np.random.default_rng(n + d)
    c = rng.permutation(np.arange(n) % d).astype(np.int32)
    t = Table(ctx, [{"c": (c, "INT"), "f": (rng.integers(0, 100, n).astype(np.int32), "INT")}])
    for lds_max in (None, "0"):  # LDS bitset, then the HBM form
        if lds_max:
            monkeypatch.setenv("PH_LDS_TABLE_MAX", lds_max)
        r = check(ctx, t, "SELECT DISTINCTCOUNT(c) FROM t WHERE f < 90", MODE_AGG)
        assert r.stats.scan_kernel == (KERNEL_DISTINCT_HBM if lds_max else KERNEL_DISTINCT_LDS)
        assert int(r.agg_columns[0].counts[0]) == len(np.unique(c[t.cols[0]["f"][0] < 90]))


# ------------------------------------------------------------------ every eligible form over one table
@pytest.fixture(scope="module")
def forms_table(ctx):
    rng = np.random.default_rng(11)
    n = 150_001
    return Table(ctx, [{"c": (rng.integers(0, 700, n).astype(np.int32), "INT"),
                        "g": (rng.integers(0, 37, n).astype(np.int32), "INT"),
                        "f": (rng.integers(0, 50, n).astype(np.int32), "INT")}])


def test_forms_agree(ctx, forms_table, monkeypatch):
    t = forms_table
    agg, grp = "SELECT DISTINCTCOUNT(c) FROM t WHERE f < 33", "SELECT g, DISTINCTCOUNT(c) FROM t WHERE f < 33 GROUP BY g LIMIT 100"
    a_lds = check(ctx, t, agg, MODE_AGG)
    g_lds = check(ctx, t, grp, MODE_GROUP_LDS)
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    a_hbm = check(ctx, t, agg, MODE_AGG)
    g_hbm = check(ctx, t, grp, MODE_GROUP_GLOBAL)
    assert [x.stats.scan_kernel for x in (a_lds, g_lds, a_hbm, g_hbm)] == [
        KERNEL_DISTINCT_LDS, KERNEL_DISTINCT_LDS, KERNEL_DISTINCT_HBM, KERNEL_DISTINCT_HBM]
    assert np.array_equal(a_lds.agg_columns[0].bits, a_hbm.agg_columns[0].bits)
    assert np.array_equal(g_lds.agg_columns[0].bits, g_hbm.agg_columns[0].bits) and g_lds.keys == g_hbm.keys
    # the union of the groups' sets is the aggregation-only set
    assert np.array_equal(np.bitwise_or.reduce(g_hbm.agg_columns[0].bits, axis=0), a_hbm.agg_columns[0].bits[0])


# ------------------------------------------------------------------ combinations
@pytest.fixture(scope="module")
def mixed_table(ctx):
    rng = np.random.default_rng(3)
    n = 60_007
    words = np.array(["", "a", "bb", "naïve", "zz", "日本", "q" * 17])
    cols = {"i": (rng.integers(0, 90, n).astype(np.int32) - 40, "INT"),
            "l": (rng.integers(0, 1500, n).astype(np.int64) * (1 << 33), "LONG"),
            "fl": (rng.integers(0, 300, n).astype(np.float32) / 4, "FLOAT"),
            "d": (np.round(rng.normal(0, 30, n), 1) + 0.0, "DOUBLE"),  # (+ 0.0: no -0.0 beside 0.0)
            "s": (words[rng.integers(0, len(words), n)], "STRING"),
            "r": (rng.integers(0, 5000, n).astype(np.int32) * 7, "INT"),
            "m": (rng.integers(0, 1 << 20, n).astype(np.int32), "INT"),
            "srt": (np.sort(rng.integers(0, 60, n)).astype(np.int32), "INT"),
            "inv": (rng.integers(0, 25, n).astype(np.int32), "INT"),
            "g": (rng.integers(0, 12, n).astype(np.int32), "INT")}
    return Table(ctx, [cols], raw=("r",), inverted=("inv",))


@pytest.mark.parametrize("col", ["l", "fl", "d", "s", "r"])
def test_data_types(ctx, mixed_table, col):
    check(ctx, mixed_table, f"SELECT DISTINCTCOUNT({col}) FROM t WHERE m < 800000", MODE_AGG)
    check(ctx, mixed_table, f"SELECT g, DISTINCTCOUNT({col}) FROM t WHERE m < 800000 GROUP BY g LIMIT 20")


def test_two_columns_with_count_and_sum(ctx, mixed_table):
    sql = "SELECT g, DISTINCTCOUNT(i), COUNT(*), SUM(m), DISTINCTCOUNT(l) FROM t WHERE m > 1000 GROUP BY g LIMIT 20"
    q = parse_sql(sql)
    r = check(ctx, mixed_table, q)
    e = O.execute(parse_sql("SELECT g, COUNT(*), SUM(m) FROM t WHERE m > 1000 GROUP BY g LIMIT 20"), mixed_table.ora)
    exp = dict(zip(e.keys, e.aggs))
    for i, key in enumerate(r.keys):
        assert [int(r.agg_columns[1][i]), float(r.agg_columns[2][i])] == exp[key]
    check(ctx, mixed_table, "SELECT DISTINCTCOUNT(i), COUNT(*), SUM(m), DISTINCTCOUNT(s) FROM t WHERE m > 1000", MODE_AGG)


def test_lds_bound_beyond_one_cu_takes_the_hbm_form(monkeypatch):
    # lds_table_max raised to 1 MiB admits a 158.7 KiB bitset row (D = 1 300 000); with the staging areas it is past
    # one CU's 160 KiB, so the planner takes the HBM form instead of refusing the query
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    try:
        n, d = 4001, 1_300_000
        v = (np.arange(n, dtype=np.int64) * 293 % d).astype(np.int32)
        v[-1] = d - 1
        f = (np.arange(n) % 10).astype(np.int32)
        t = Table(c, [{"c": (v, "INT"), "f": (f, "INT")}])
        c.set_table_dictionary("c", "INT", np.arange(d, dtype=np.int32))
        monkeypatch.setenv("PH_LDS_TABLE_MAX", str(1 << 20))
        r = c.execute(parse_sql("SELECT DISTINCTCOUNT(c) FROM t WHERE f < 7"), t.gpu)
        assert r.stats.mode == MODE_AGG and r.stats.scan_kernel == KERNEL_DISTINCT_HBM
        exp = np.unique(v[f < 7])
        assert int(r.agg_columns[0].counts[0]) == len(exp)
        assert np.array_equal(r.agg_columns[0].bits[0], bitset(exp.tolist(), np.arange(d, dtype=np.int32)))
    finally:
        c.close()


def test_same_column_twice(ctx, mixed_table):
    spec = AggregationSpec(DISTINCTCOUNT, "i")
    q = QueryContext(select=[SelectItem("aggregation", 0), SelectItem("aggregation", 1)], aggregations=[spec, spec],
                     filter=parse_sql("SELECT COUNT(*) FROM t WHERE m < 500000").filter)
    r = check(ctx, mixed_table, q, MODE_AGG)
    assert np.array_equal(r.agg_columns[0].bits, r.agg_columns[1].bits)
    assert np.array_equal(r.agg_columns[0].counts, r.agg_columns[1].counts)


def test_empty_filter(ctx, mixed_table):
    r = check(ctx, mixed_table, "SELECT DISTINCTCOUNT(i) FROM t WHERE m < 0")
    assert r.num_groups == 1 and int(r.agg_columns[0].counts[0]) == 0 and not r.agg_columns[0].bits.any()
    r = check(ctx, mixed_table, "SELECT g, DISTINCTCOUNT(i) FROM t WHERE m < 0 GROUP BY g")
    assert r.num_groups == 0


@pytest.mark.parametrize("where", ["m < 300000", "inv = 7", "inv IN (1, 2, 24) AND m > 5000", "srt BETWEEN 10 AND 19",
                                   "srt > 40 AND (inv = 3 OR m < 100000)"])
def test_filter_leaves(ctx, mixed_table, where):
    check(ctx, mixed_table, f"SELECT DISTINCTCOUNT(l) FROM t WHERE {where}", MODE_AGG)
    check(ctx, mixed_table, f"SELECT g, DISTINCTCOUNT(l) FROM t WHERE {where} GROUP BY g LIMIT 20")


def test_num_groups_limit(ctx, mixed_table):
    # the first `limit` keys in doc order are kept (DictionaryBasedGroupKeyGenerator); every matched doc is scanned
    cols = mixed_table.cols[0]
    sql = "SET numGroupsLimit=5; SELECT g, DISTINCTCOUNT(i) FROM t WHERE m < 900000 GROUP BY g LIMIT 20"
    docs = cols["m"][0] < 900000
    first = list(dict.fromkeys(cols["g"][0][docs].tolist()))[:5]
    r = check(ctx, mixed_table, sql, limit_rows={(k,) for k in first})
    assert r.num_groups == 5 and r.stats.num_groups_limit_reached


# ------------------------------------------------------------------ refusals
def _usable(ctx, t):
    check(ctx, t, "SELECT DISTINCTCOUNT(c) FROM t WHERE f < 10", MODE_AGG)


def _refused(call, text):
    with pytest.raises(N.UnsupportedError) as e:
        call()
    assert e.value.code == N.PH_ERR_UNSUPPORTED and text in str(e.value), str(e.value)


def test_refusals(ctx, forms_table):
    t = forms_table
    q = parse_sql("SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g ORDER BY g LIMIT 5")
    _refused(lambda: ctx.dense_layout(q, t.gpu), "DISTINCTCOUNT on dense partials")
    _usable(ctx, t)
    _refused(lambda: ctx.execute_dense(q, t.gpu, [0]), "DISTINCTCOUNT on dense partials")
    _usable(ctx, t)
    _refused(lambda: ctx.dense_finalize(q, t.gpu, [0], 0, 1), "DISTINCTCOUNT on dense partials")
    _usable(ctx, t)
    trim = parse_sql("SET minSegmentGroupTrimSize=5; SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g ORDER BY g LIMIT 1")
    _refused(lambda: ctx.execute(trim, t.gpu), "segment group trim")
    _usable(ctx, t)
    from pinot_amd.distributed import DistributedQuery
    _refused(lambda: DistributedQuery(ctx).execute(q, t.gpu), "DISTINCTCOUNT on dense partials")


def test_refusal_multi_device(forms_table):
    from pinot_amd.engine import GpuContext
    m = GpuContext(devices=[0, 0])
    try:
        seg = m.pin(create_segment("m0", forms_table.cols[0]))
        _refused(lambda: m.execute(parse_sql("SELECT DISTINCTCOUNT(c) FROM t WHERE f < 3"), [seg]), "multi-device")
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
        c.set_table_dictionary("c", "INT", np.arange(4_000_000, dtype=np.int32))
        c.set_table_dictionary("g", "INT", np.arange(1_000_000, dtype=np.int32))
        _refused(lambda: c.execute(parse_sql("SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g"), t.gpu), "dense table budget")
        c.set_table_dictionary("h", "INT", np.arange(1_000_000, dtype=np.int32))
        _refused(lambda: c.execute(parse_sql("SELECT g, h, DISTINCTCOUNT(c) FROM t GROUP BY g, h"), t.gpu),
                 "beyond the dense tables")
        # the context still answers; the bitset is over the table dictionary now
        r = c.execute(parse_sql("SELECT DISTINCTCOUNT(c) FROM t WHERE g < 3"), t.gpu)
        assert int(r.agg_columns[0].counts[0]) == int((cols["g"][0] < 3).sum())
        assert len(r.agg_columns[0].values) == 4_000_000 and r.agg_columns[0].bits.shape == (1, 125_000)
    finally:
        c.close()


# ------------------------------------------------------------------ star-tree fallback, DataTable
def test_star_tree_segment_scans_its_docs(ctx):
    from pinot_amd.startree import attach
    from tests.test_startree_cpu import make_star, star_table
    cols = star_table(np.random.default_rng(2), 5000)
    seg, st, oseg, _ = make_star(cols, name="dcst")
    p = ctx.pin(seg)
    attach(p, st)
    served = ctx.execute(parse_sql("SELECT d1, COUNT(*) FROM t GROUP BY d1"), [p])
    assert served.stats.num_segments_star_tree == 1
    t = Table.__new__(Table)
    t.cols, t.ora, t.gpu = [cols], [oseg], [p]
    for sql in ("SELECT d1, COUNT(*), DISTINCTCOUNT(d2) FROM t GROUP BY d1", "SELECT DISTINCTCOUNT(d3) FROM t WHERE d1 = 10"):
        r = check(ctx, t, sql)
        assert r.stats.num_segments_star_tree == 0


@pytest.mark.parametrize("sql", [
    "SELECT DISTINCTCOUNT(i), DISTINCTCOUNT(l), DISTINCTCOUNT(fl), DISTINCTCOUNT(d), COUNT(*) FROM t WHERE m < 700000",
    "SELECT g, DISTINCTCOUNT(s), DISTINCTCOUNT(d) FROM t WHERE m < 700000 GROUP BY g ORDER BY DISTINCTCOUNT(d) DESC, g LIMIT 20",
    "SELECT g, DISTINCTCOUNT(i) FROM t WHERE m < 0 GROUP BY g LIMIT 20"])
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
        assert len(payload) == ln
        if otype in (9, 15, 16, 17, 18):  # the set decoder raises unless it consumes exactly `ln` bytes
            n_vals = len(set_deserialize(otype, payload))
            width = {9: 4, 15: 8, 16: 4, 17: 8}.get(otype)
            if width:
                assert ln == 4 + width * n_vals
    assert end == dt.variable_size, "the last object ends the variable-size section"
    r = ctx.execute(q, mixed_table.gpu)
    assert reduce_datatables(q, [dt]).rows == reduce_groups(q, r.keys, r.aggs).rows
    if all(a.function == DISTINCTCOUNT for a in q.aggregations):  # two servers' equal sets merge to the same finals
        assert reduce_datatables(q, [dt, dt]).rows == reduce_groups(q, r.keys, r.aggs).rows
