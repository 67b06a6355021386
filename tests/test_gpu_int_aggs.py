"""GPU: SUM / MIN / MAX over INT and LONG columns at the integer extremes on every kernel form, against the plain
Python-integer reference of tests/int_ref.py (not the oracle, not the library).

Contract checked (tests/int_ref.py): with A = sum|x_i| < 2^53 the SUM equals float(S) bit for bit
and sum_precision_flag is 0; elsewhere |gpu - fsum(double(x_i))| <= n * 2^-52 * fsum(|double(x_i)|), and equality
where every partial sum is an exact double (the powers-of-two groups); |SUM| >= 2^53 sets the flag.  MIN / MAX are
(double) of the exact extreme, COUNT and keys exact.  An integer SUM that could pass 2^63 over the call's docs is summed
in double by a local execute; the dense-partial paths (int64 tables that other ranks add into) may refuse it with
UnsupportedError instead -- never a wrapped number.

Every case asserts the plan it ran through stats.mode / stats.scan_kernel."""
import numpy as np
import pytest

from pinot_amd.native import UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.segment import SegmentBuffers, create_column, create_column_from_dict_ids, create_raw_column
from tests import int_ref as R

pytestmark = pytest.mark.gpu

MODE_META, MODE_AGG, MODE_GROUP_LDS, MODE_GROUP_GLOBAL, MODE_PARTITION, MODE_GROUP_HASH = -1, 1, 2, 3, 4, 5
K_SCAN, K_AGG_LEAN, K_AGG_SPARSE, K_GROUP_LDS_LEAN, K_PART_LEAN, K_PART_LEAN2, K_PART_SCAN, K_PART_REG = 1, 2, 3, 4, 5, 6, 7, 8
K_GROUP_REG, K_GROUP_SPARSE, K_AGG_CONT, K_GROUP_CONT = 11, 12, 14, 15
FILTERS = [("", None), (" WHERE f < 5", lambda t: t["f"] < 5), (" WHERE f >= 5", lambda t: t["f"] >= 5)]


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def types_of(name):
    return dict(R.VALUE_COLUMNS[name], a="LONG", p="LONG")


def build_segment(name, t, types, raw=False):
    seg = SegmentBuffers(name, len(t["g"]))
    for c in t:
        if c == "inv":
            seg.columns[c] = create_column(c, t[c], "INT", inverted=True)
        elif c in types and raw:
            seg.columns[c] = create_raw_column(c, t[c], types[c])
        elif c == "srt":
            seg.columns[c] = create_column(c, t[c], "INT")  # the sorted forward index
        else:  # bit-packed dictIds even where the docs happen to be in value order (saturate: doc 0 holds the minimum)
            dictionary, ids = np.unique(np.asarray(t[c], np.int64 if types.get(c) == "LONG" else np.int32),
                                        return_inverse=True)
            seg.columns[c] = create_column_from_dict_ids(c, dictionary, ids.reshape(-1), types.get(c, "INT"),
                                                         allow_sorted=False)
    return seg


def sql_of(cols, where="", group=(), exprs=(), tail=""):
    aggs = ["COUNT(*)"]
    for c in list(cols) + [f"{a} * {b}" for a, b in exprs]:
        aggs += [f"SUM({c})", f"MIN({c})", f"MAX({c})"]
    keys = ", ".join(group)
    return (f"SELECT {keys + ', ' if group else ''}{', '.join(aggs)} FROM t{where}"
            f"{' GROUP BY ' + keys if group else ''}{tail}")


def compare(rows, ref, flag, what):
    assert set(rows) == set(ref), (what, sorted(rows)[:20], sorted(ref)[:20])
    for key, got in rows.items():
        R.check_row(got, ref[key], (what, key))
    if flag is not None:
        R.check_flag(flag, rows, ref, what)


def run(ctx, segs, tables, cols, where="", mask=None, group=(), exprs=(), mode=None, kernels=None):
    sql = ("SET numGroupsLimit=10000000; " if group else "") + sql_of(cols, where, group, exprs)
    r = ctx.execute(parse_sql(sql), segs)
    ref = R.reference(tables, cols, mask, tuple(group) if group else False, exprs)
    compare(dict(zip(r.keys, r.aggs)), ref, r.stats.sum_precision_flag, sql)
    if mode is not None:
        assert r.stats.mode == mode, (sql, r.stats.mode, r.stats.scan_kernel)
    if kernels is not None:
        assert r.stats.scan_kernel in kernels, (sql, r.stats.mode, r.stats.scan_kernel)
    return r


def cols_of(name):
    return [c for c, _ in R.VALUE_COLUMNS[name]]


def exprs_of(name):
    return (R.WRAP_EXPR,) if name == "wrap" else ()


@pytest.fixture
def pinned(ctx):
    made = []

    def pin(name, raw=False, which=(0, 1), tables=None, types=None):
        tabs = [(tables or R.make_tables(name))[i] for i in which]
        segs = [ctx.pin(build_segment(f"ia_{name}_{k}_{i}", t, types or types_of(name), raw))
                for k, (i, t) in enumerate(zip(which, tabs))]
        made.extend(segs)
        return segs, tabs
    yield pin
    for s in made:
        s.unpin()


@pytest.mark.parametrize("raw", [False, True], ids=["dict", "raw"])
@pytest.mark.parametrize("name", R.SETS)
def test_scan_agg_and_lds_group(ctx, pinned, monkeypatch, name, raw):
    # MODE_AGG and MODE_GROUP_LDS in their default forms, then the generic forms (PH_AGG_GENERIC / PH_LDS_GENERIC) and
    # the LDS-staged lean group-by (PH_LDS_LEAN); dictionary and raw value columns.  The 64-bit-range LONG sets are not
    # frame-of-reference packed into 32 bits, so no lean kernel serves them: the cases run the generic scan and say so
    segs, tables = pinned(name, raw)
    cols, exprs = cols_of(name), exprs_of(name)
    # (int_edges: a segment whose own range needs 32 bits gets no frame-of-reference stream -- streams stop at 31 bits --
    # so its values are dictionary gathers and the generic scan runs; only two_bases reaches the lean group-by)
    lean_group = name == "two_bases" and not raw
    for env in ({}, {"PH_LDS_LEAN": "1"}, {"PH_AGG_GENERIC": "1", "PH_LDS_GENERIC": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        generic = "PH_AGG_GENERIC" in env
        for where, mask in FILTERS:
            for c in cols:
                r = run(ctx, segs, tables, [c], where, mask, mode=MODE_AGG)
                if name == "two_bases" and not raw:
                    # each segment's own frame of reference is 4 bits wide: k_agg_lean, whatever the table-wide range
                    assert r.stats.scan_kernel == (K_SCAN if generic else K_AGG_LEAN), (c, env, r.stats.scan_kernel)
                elif not raw:  # a 32-bit (int_edges) or wider stream, or a SUM planned in double: the generic scan
                    assert r.stats.scan_kernel == K_SCAN, (name, c, env, r.stats.scan_kernel)
                r = run(ctx, segs, tables, [c], where, mask, group=("g",), mode=MODE_GROUP_LDS)
                if lean_group and not generic and c != "vl2":
                    # a table-wide range of 2^32 - 1 is the last the lean group-by takes; its COUNT << 40 | SUM word
                    # would carry (2048-doc chunks x 2^32), so the unpacked k_group_lds_lean runs, never k_group_reg
                    assert r.stats.scan_kernel == K_GROUP_LDS_LEAN, (name, c, env, r.stats.scan_kernel)
                elif not raw:  # vl2: a range of exactly 2^32 leaves the lean path
                    assert r.stats.scan_kernel == K_SCAN, (name, c, env, r.stats.scan_kernel)
            run(ctx, segs, tables, cols, where, mask, exprs=exprs, mode=MODE_AGG)
            run(ctx, segs, tables, cols, where, mask, group=("g",), exprs=exprs, mode=MODE_GROUP_LDS)
            if exprs:
                run(ctx, segs, tables, [], where, mask, exprs=exprs, mode=MODE_AGG)
                run(ctx, segs, tables, [], where, mask, group=("g",), exprs=exprs, mode=MODE_GROUP_LDS)
        for k in env:
            monkeypatch.delenv(k)


def test_wrap_groups_are_not_wrapped(ctx, pinned):
    # the figures an int64 accumulator gives: 0.0, -9.2e18 and +4.6e18 for the 2^64, 2^63 and -3 * 2^62 groups
    segs, tables = pinned("wrap")
    r = ctx.execute(parse_sql("SELECT g, SUM(vl), SUM(a * p) FROM t GROUP BY g ORDER BY g LIMIT 12"), segs)
    got = {k[0]: row for k, row in zip(r.keys, r.aggs)}
    assert [got[k][0] for k in range(4)] == [2.0 ** 64, 2.0 ** 63, -3 * 2.0 ** 62, 0.0]
    assert got[4][1] >= 3 * 3.9e18 and r.stats.sum_precision_flag
    assert (r.stats.mode, r.stats.scan_kernel) == (MODE_GROUP_LDS, K_SCAN)  # both terms planned in double
    r = ctx.execute(parse_sql("SELECT SUM(vl) FROM t WHERE g = 0"), segs)
    assert r.aggs[0][0] == 2.0 ** 64 and r.stats.sum_precision_flag
    assert (r.stats.mode, r.stats.scan_kernel) == (MODE_AGG, K_SCAN)


def test_flag_at_two_to_the_53(ctx, pinned):
    # S = 2^53 - 1 (A too): exact, flag clear; S = 2^53: flag set; the negative mirror
    segs, tables = pinned("flag53")
    for g, col, want, flag in ((0, "vl", R.TWO53 - 1, False), (1, "vl", R.TWO53, True),
                               (0, "nl", 1 - R.TWO53, False), (1, "nl", -R.TWO53, True)):
        for group in ((), ("g",)):
            # a 41-bit range has no frame-of-reference stream: int64 sums of dictionary gathers in the generic scan
            r = run(ctx, segs, tables, [col], f" WHERE g = {g}", lambda t, g=g: t["g"] == g, group=group,
                    mode=MODE_GROUP_LDS if group else MODE_AGG, kernels=(K_SCAN,))
            assert r.aggs[0][1] == float(want) and bool(r.stats.sum_precision_flag) == flag, (g, col, group)
    for s, t in zip(segs, tables):  # one segment alone: the sum_bounded skip (|v| x docs < 2^52) on the small one
        r = run(ctx, [s], [t], ["vl", "nl"], group=("g",), mode=MODE_GROUP_LDS, kernels=(K_SCAN,))
        assert bool(r.stats.sum_precision_flag) == (len(t["g"]) > 8192)


@pytest.mark.parametrize("name", R.SETS)
def test_metadata_answer(ctx, pinned, name):
    # no filter, no group-by, COUNT / MIN / MAX only: the dictionary ends converted with (double)
    segs, tables = pinned(name)
    cols = cols_of(name)
    aggs = ", ".join(f"MIN({c}), MAX({c})" for c in cols)
    r = ctx.execute(parse_sql(f"SELECT COUNT(*), {aggs} FROM t"), segs)
    assert r.stats.mode == MODE_META and r.stats.num_entries_scanned_post_filter == 0
    assert not r.stats.sum_precision_flag  # no SUM in the call
    ref = R.reference(tables, cols)[()]
    assert r.aggs[0][0] == ref[0]
    for i in range(len(cols)):
        assert r.aggs[0][1 + 2 * i] == ref[1 + i].min and r.aggs[0][2 + 2 * i] == ref[1 + i].max, (name, cols[i])


@pytest.mark.parametrize("name", R.SETS)
def test_global_table_and_group_cache(ctx, pinned, monkeypatch, name):
    # MODE_GROUP_GLOBAL (no LDS table), and its per-workgroup LDS group cache (one value column, two keys)
    segs, tables = pinned(name)
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    for where, mask in FILTERS:
        run(ctx, segs, tables, cols_of(name), where, mask, group=("g",), exprs=exprs_of(name), mode=MODE_GROUP_GLOBAL)
        for c in cols_of(name):
            run(ctx, segs, tables, [c], where, mask, group=("g", "srt"), mode=MODE_GROUP_GLOBAL)


@pytest.mark.parametrize("name", R.SETS)
def test_hash_table(name):
    # MODE_GROUP_HASH, reached at this size through table dictionaries that make the key space 10^18
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    try:
        tables = R.make_tables(name)
        segs = [c.pin(build_segment(f"ih_{name}_{i}", t, types_of(name))) for i, t in enumerate(tables)]
        for k in ("g", "f", "inv"):
            c.set_table_dictionary(k, "INT", np.arange(1_000_000, dtype=np.int32))
        for where, mask in FILTERS:
            run(c, segs, tables, cols_of(name), where, mask, group=("g", "f", "inv"), exprs=exprs_of(name),
                mode=MODE_GROUP_HASH)
        for s in segs:
            s.unpin()
    finally:
        c.close()


@pytest.mark.parametrize("name", R.SETS)
def test_sparse_gathers(ctx, pinned, monkeypatch, name):
    # an inverted-index leaf: k_agg_sparse over the roaring containers and over the doc bitmap, k_group_sparse and the
    # container group form (one value column)
    segs, tables = pinned(name)
    cols = cols_of(name)
    where, mask = " WHERE inv = 1", (lambda t: t["inv"] == 1)
    run(ctx, segs, tables, cols, where, mask, mode=MODE_AGG)
    run(ctx, segs, tables, cols, where, mask, group=("g",), mode=MODE_GROUP_LDS)
    monkeypatch.setenv("PH_AGG_SPARSE", "1")
    run(ctx, segs, tables, cols, where, mask, mode=MODE_AGG, kernels=(K_AGG_CONT,))
    for e in exprs_of(name):  # the 2-operand term alone is not taken by the gather plan: the generic scan serves it
        run(ctx, segs, tables, [], where, mask, exprs=(e,), mode=MODE_AGG, kernels=(K_SCAN,))
    monkeypatch.setenv("PH_AGG_CONT", "0")
    run(ctx, segs, tables, cols, where, mask, mode=MODE_AGG, kernels=(K_AGG_SPARSE,))
    for e in exprs_of(name):
        run(ctx, segs, tables, [], where, mask, exprs=(e,), mode=MODE_AGG, kernels=(K_SCAN, K_AGG_SPARSE))
    monkeypatch.setenv("PH_GROUP_SPARSE", "1")
    for c in cols:
        run(ctx, segs, tables, [c], where, mask, group=("g",), kernels=(K_GROUP_SPARSE,))
    monkeypatch.setenv("PH_GROUP_CONT", "1")
    for c in cols:
        run(ctx, segs, tables, [c], where, mask, group=("g",), kernels=(K_GROUP_CONT,))
    monkeypatch.delenv("PH_GROUP_CONT")
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")  # the gather kernel over the group cache + HBM table
    for c in cols:
        run(ctx, segs, tables, [c], where, mask, group=("g",), mode=MODE_GROUP_GLOBAL,
            kernels=(K_GROUP_SPARSE, K_GROUP_CONT))


@pytest.mark.parametrize("name", R.SETS)
def test_sorted_leaf_conjunction_and_twice_pinned(ctx, pinned, name):
    # a sorted column's doc range, an AND of two scan leaves (FK_CONJ), and the cross-segment merge over one segment
    # pinned twice (every partial result twice: 2 x INT64_MIN, 2 x 2^62 ...)
    segs, tables = pinned(name)
    cols = cols_of(name)
    for where, mask in ((" WHERE srt = 0", lambda t: t["srt"] == 0),
                        (" WHERE f = 7 AND m > 0", lambda t: (t["f"] == 7) & (t["m"] > 0))):
        run(ctx, segs, tables, cols, where, mask, exprs=exprs_of(name), mode=MODE_AGG)
        run(ctx, segs, tables, cols, where, mask, group=("g",), exprs=exprs_of(name), mode=MODE_GROUP_LDS)
    segs, tables = pinned(name, which=(0, 0))
    for where, mask in FILTERS[:2]:
        run(ctx, segs, tables, cols, where, mask, exprs=exprs_of(name), mode=MODE_AGG)
        run(ctx, segs, tables, cols, where, mask, group=("g",), exprs=exprs_of(name), mode=MODE_GROUP_LDS)


@pytest.mark.parametrize("name", R.SETS)
def test_dense_partials(ctx, pinned, name):
    # execute_dense + dense_finalize over two key shards.  The tables are int64: a LONG SUM that could pass 2^63 over
    # 2^32 docs is refused (the call cannot see the other ranks' docs); every INT column is served
    import torch

    from pinot_amd.distributed import Layout, alloc_tables, shard_bounds
    segs, tables = pinned(name)
    ctx.set_table_dictionary("g", "INT", np.arange(R.NUM_GROUPS, dtype=np.int32))  # dense partials need it
    for c in cols_of(name):
        amax = max(abs(int(v)) for t in tables for v in (t[c].min(), t[c].max()))
        for group in ((), ("g",)):
            for where, mask in FILTERS[:2]:
                q = parse_sql(sql_of([c], where, group))
                try:
                    lay = Layout.from_native(ctx.dense_layout(q, segs))
                except UnsupportedError:
                    assert amax << 32 > 1 << 63, (name, c, "refused although it cannot wrap over 2^32 docs")
                    continue
                # safety, in exact integers: n <= 2^32 docs of |v| <= amax sum to at most amax * 2^32 in magnitude,
                # which an int64 table holds only up to 2^63 (-2^63 itself is representable, +2^63 needs v = 2^31,
                # which no INT holds)
                assert amax << 32 <= 1 << 63, (name, c, "served although the int64 tables could wrap")
                tabs = alloc_tables(lay, 2, torch.device("cuda", 0))
                ctx.execute_dense(q, segs, [t.data_ptr() for t in tabs])
                torch.cuda.synchronize()
                rows, flag = {}, False
                for rank in range(2):
                    _, g0, g1 = shard_bounds(lay.num_groups, 2, rank)
                    if g1 <= g0:
                        continue
                    shard = [t[g0 * per:g1 * per] for t, per in zip(tabs, lay.elems_per_group)]
                    res = ctx.dense_finalize(q, segs, [t.data_ptr() for t in shard], g0, g1)
                    rows.update(zip(res.keys, res.aggs))
                    flag = flag or bool(res.stats.sum_precision_flag)
                ref = R.reference(tables, [c], mask, bool(group))
                if not group and ref[()][0] == 0:
                    ref = {}  # a dense shard finalises the groups that matched docs
                compare(rows, ref, flag, (name, "dense", where, group))


@pytest.mark.parametrize("name", ["wrap", "long_edges", "flag53", "two_bases"])
def test_distributed_query_refuses_a_wrapping_sum(name):
    # DistributedQuery.execute plans the native layout first, which refuses a LONG term past 2^31: the term never reaches
    # reduce_tables, whose int64 all-reduce would wrap it (tests/test_int_aggs_cpu.py shows that it does)
    from pinot_amd.distributed import DistributedQuery
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)  # (its own context: execute puts the library on torch's stream)
    try:
        segs = [c.pin(build_segment(f"iq_{name}_{i}", t, types_of(name))) for i, t in enumerate(R.make_tables(name))]
        c.set_table_dictionary("g", "INT", np.arange(R.NUM_GROUPS, dtype=np.int32))
        dq = DistributedQuery(c)
        for group in ((), ("g",)):
            with pytest.raises(UnsupportedError):
                dq.execute(parse_sql(sql_of(cols_of(name)[:1], "", group)), segs)
            assert not dq._cache  # no table was allocated
        for s in segs:
            s.unpin()
    finally:
        c.close()


@pytest.mark.parametrize("name", R.SETS)
def test_multi_device_merge(name):
    # the in-library merge of two logical shards of one device: int64 dense tables where no shard could wrap, else the
    # value-keyed merge of the shards' doubles
    from pinot_amd.engine import GpuContext
    c = GpuContext(devices=[0, 0])
    try:
        tables = R.make_tables(name)
        segs = [c.pin(build_segment(f"im_{name}_{i}", t, types_of(name))) for i, t in enumerate(tables)]
        assert sorted(c.segment_device(s) for s in segs) == [0, 1]
        # the int64 dense tables merge a term only while max|term| x the docs of both shards stays below 9.0e18 on
        # every shard: int_edges, flag53 (2^40 x 16 578 docs: the finalised shards' flag path) and two_bases; the
        # 2^62 / INT64 sets merge by value, which records no table merge and no shard finalisation
        total = sum(len(t["g"]) for t in tables)
        amax = max(abs(int(v)) for t in tables for col in cols_of(name) for v in (t[col].min(), t[col].max()))
        dense = amax * total < 9.0e18
        assert dense == (name in ("int_edges", "flag53", "two_bases"))
        for where, mask in FILTERS[:2]:
            for group in ((), ("g",)):
                r = run(c, segs, tables, cols_of(name), where, mask, group=group, exprs=exprs_of(name),
                        mode=MODE_GROUP_LDS if group else MODE_AGG)
                assert r.stats.num_devices == 2
                assert (r.stats.finalize_ms > 0) == dense, (name, where, group, r.stats.merge_ms, r.stats.finalize_ms)
        if name == "flag53":  # the 2^53 boundary through dense_finalize's per-shard check
            for g, flag in ((0, False), (1, True)):
                r = run(c, segs, tables, ["vl", "nl"], f" WHERE g = {g}", lambda t, g=g: t["g"] == g, group=("g",),
                        mode=MODE_GROUP_LDS)
                assert r.stats.finalize_ms > 0 and bool(r.stats.sum_precision_flag) == flag, (g, flag)
        for s in segs:
            s.unpin()
    finally:
        c.close()


@pytest.mark.parametrize("name", R.SETS)
@pytest.mark.parametrize("order,desc", [("SUM", True), ("MIN", False)])
def test_segment_trim(ctx, pinned, name, order, desc):
    # each segment keeps max(5 * LIMIT, minSegmentGroupTrimSize) = 5 of its 12 groups by the ORDER BY value (ties
    # broken by g), then the kept rows merge as doubles
    segs, tables = pinned(name)
    col = cols_of(name)[0]
    sql = (f"SET minSegmentGroupTrimSize=1; SELECT g, COUNT(*), SUM({col}), MIN({col}), MAX({col}) FROM t GROUP BY g "
           f"ORDER BY {order}({col}){' DESC' if desc else ''}, g LIMIT 1")
    r = ctx.execute(parse_sql(sql), segs)
    kept = []
    for t in tables:
        ref = R.reference([t], [col], None, True)
        val = (lambda k: float(ref[k][1].S)) if order == "SUM" else (lambda k: ref[k][1].min)
        ranked = sorted(ref, key=lambda k: (-val(k) if desc else val(k), k))
        kept.append(set(ranked[:5]))
    want = {}
    for k in kept[0] | kept[1]:
        want[k] = R.reference([t for t, ks in zip(tables, kept) if k in ks], [col], lambda t, k=k: t["g"] == k[0])[()]
    compare(dict(zip(r.keys, r.aggs)), want, r.stats.sum_precision_flag, (name, sql))
    assert r.num_groups == len(want) < R.NUM_GROUPS
    # each segment is planned alone (the statistics carry the last one's plan): two_bases' segments have 4-bit ranges
    # of their own, so the packed register-direct group-by runs; every other set gathers from dictionaries
    assert r.stats.mode == MODE_GROUP_LDS
    assert r.stats.scan_kernel == (K_GROUP_REG if name == "two_bases" else K_SCAN), r.stats.scan_kernel


@pytest.mark.parametrize("name", R.SETS)
def test_datatable_round_trip_and_broker_merge(ctx, pinned, name):
    # DataTable V4 cells, and the broker's merge of two servers' tables against the reference
    from pinot_amd import datatable as DT
    segs, tables = pinned(name)
    cols = cols_of(name)
    for group in ((), ("g",)):
        for where, mask in FILTERS:
            q = parse_sql(sql_of(cols, where, group, tail=" ORDER BY g LIMIT 100" if group else ""))
            one = DT.reduce_datatables(q, [DT.decode(ctx.execute_datatable(q, segs))]).rows
            two = DT.reduce_datatables(q, [DT.decode(ctx.execute_datatable(q, [s])) for s in segs]).rows
            nk = len(group)
            ref = R.reference(tables, cols, mask, bool(group))
            # a DataTable carries no plan: the same query through execute shows the form and the flag of the call
            r = ctx.execute(q, segs)
            assert r.stats.mode == (MODE_GROUP_LDS if group else MODE_AGG), (name, where, r.stats.mode)
            if name != "two_bases":
                assert r.stats.scan_kernel == K_SCAN, (name, where, r.stats.scan_kernel)
            flag = r.stats.sum_precision_flag
            compare({tuple(r[:nk]): r[nk:] for r in one}, ref, flag, (name, "datatable", where))
            compare({tuple(r[:nk]): r[nk:] for r in two}, ref, flag, (name, "broker", where))


@pytest.mark.parametrize("w", R.SATURATE_WIDTHS)
def test_saturated_accumulators(ctx, pinned, monkeypatch, w):
    # every doc but one per segment at offset 2^w - 1 in one key: the 32-bit tile sums of k_agg_lean and the
    # COUNT << 40 | SUM(offsets) words of k_group_reg / the packed k_group_lds_lean as full as the guards let them get
    types = {"m": "INT"}
    segs, tables = pinned(f"sat{w}", tables=R.make_saturate(w), types=types)
    for where, mask in FILTERS:
        # k_agg_lean's guard: offsets below 2^26
        run(ctx, segs, tables, ["m"], where, mask, mode=MODE_AGG, kernels=(K_AGG_LEAN if w <= 26 else K_SCAN,))
        # lds_pack: wg_docs x vrange < 2^40, where a scan this small has 32-word (2048-doc) chunks, one per workgroup,
        # and wg_docs = (2 chunks - 1) / chunks x 2048 docs lies in (2048, 4096): 4096 x (2^28 - 1) < 2^40 holds for
        # w <= 28 and 2049 x (2^29 - 1) >= 2^40 fails for w = 29
        packed = w <= 28
        run(ctx, segs, tables, ["m"], where, mask, group=("k",), mode=MODE_GROUP_LDS,
            kernels=(K_GROUP_REG if packed else K_GROUP_LDS_LEAN,))
        monkeypatch.setenv("PH_LDS_LEAN", "1")
        run(ctx, segs, tables, ["m"], where, mask, group=("k",), mode=MODE_GROUP_LDS, kernels=(K_GROUP_LDS_LEAN,))
        monkeypatch.delenv("PH_LDS_LEAN")
        monkeypatch.setenv("PH_LDS_GENERIC", "1")
        run(ctx, segs, tables, ["m"], where, mask, group=("k",), mode=MODE_GROUP_LDS, kernels=(K_SCAN,))
        monkeypatch.delenv("PH_LDS_GENERIC")


def _part_record_width():
    """The widest value stream that still gets 32-bit partition records over 300 x 300 keys: klo + vbits <= 32, with
    klo = 12 lowered while the key space gives fewer than 256 partitions (the guard of the partition section)."""
    G, klo = R.PART_KEY_CARD ** 2, 12
    while klo > 8 and (G >> (klo - 1)) < 256:
        klo -= 1
    return 32 - klo


@pytest.mark.parametrize("wide", [False, True], ids=["rec32", "rec64"])
def test_saturated_partition_records(ctx, pinned, monkeypatch, wide):
    # (key << vbits) + (value - vmin) with the largest key at the largest offset, at the last width with 32-bit
    # records and the first with 64-bit ones
    w = _part_record_width() + (1 if wide else 0)
    assert w == (24 if wide else 23)
    segs, tables = pinned(f"satk{w}", tables=R.make_saturate(w, keys=True), types={"m": "INT"})
    keys = ("k1", "k2")

    def part(where, mask, kernels):
        run(ctx, segs, tables, ["m"], where, mask, group=keys, mode=MODE_PARTITION, kernels=kernels)
    for where, mask in FILTERS:
        lean = (K_PART_LEAN,) if wide else (K_PART_REG,)  # k_part_reg: 32-bit records only
        part(where, mask, lean)
        for sets in ("1", "2"):
            monkeypatch.setenv("PH_PART_SETS", sets)
            part(where, mask, lean)
            monkeypatch.setenv("PH_PART_RING_LOG2", "4")  # 16-slot rings: skewed rounds take the overflow path
            part(where, mask, lean)
            monkeypatch.delenv("PH_PART_RING_LOG2")
        monkeypatch.delenv("PH_PART_SETS")
        monkeypatch.setenv("PH_PART_LDS", "1")
        part(where, mask, (K_PART_LEAN,))
        monkeypatch.setenv("PH_PART_DEPTH", "2")
        part(where, mask, (K_PART_LEAN2,))
        monkeypatch.delenv("PH_PART_DEPTH")
        monkeypatch.delenv("PH_PART_LDS")
        monkeypatch.setenv("PH_PART_GENERIC", "1")
        part(where, mask, (K_PART_SCAN,))
        monkeypatch.delenv("PH_PART_GENERIC")
