"""GPU: SUM / MIN / MAX over DOUBLE and FLOAT columns on every kernel form, against the plain reference of
tests/float_ref.py (not the oracle, not the library).

Contract checked (the reference engine's):
* MIN / MAX are a fold of Math.min / Math.max: any scanned NaN gives NaN, -0.0 is below 0.0; compared by bit pattern
  (any NaN equals any NaN).  Without filter and group-by, and only COUNT / MIN / MAX asked, the answer comes from the
  dictionaries instead (NonScanBasedAggregationOperator.java:153-166): MIN is the first entry and MAX the last in
  Double.compare order, so MIN ignores a NaN there.
* SUM: any order of double additions of n finite terms is within (n - 1) * 2^-53 * sum|x_i| of the exact sum to first
  order.  The bar is |gpu - fsum| <= n * 2^-52 * fsum(|x_i|), a factor 2 over first order, and it is the only
  tolerance of this module.  Where every partial sum is exact in double (the zeros, lossless and cancel-integer
  columns) the bar is equality.  A NaN or both infinities among the values give NaN, one infinity that infinity.
* COUNT and keys are exact.

Value sets (tests/float_ref.make_tables): two segments of 4 099 and 193 docs whose dictionaries differ, built in
Double.compare order (-0.0 and 0.0 two entries, one canonical NaN last).  Every case asserts the plan it meant to run
through stats.mode / stats.scan_kernel."""
import math

import numpy as np
import pytest

from pinot_amd.query import parse_sql
from pinot_amd.segment import SegmentBuffers, create_column, create_column_from_dict_ids, create_raw_column
from tests import float_ref as R

pytestmark = pytest.mark.gpu

MODE_META, MODE_AGG, MODE_GROUP_LDS, MODE_GROUP_GLOBAL, MODE_GROUP_HASH = -1, 1, 2, 3, 5
K_SCAN, K_AGG_SPARSE, K_GROUP_SPARSE, K_AGG_CONT, K_GROUP_CONT = 1, 3, 12, 14, 15
TYPES = {"d": ("DOUBLE", np.float64), "d2": ("DOUBLE", np.float64), "fl": ("FLOAT", np.float32)}


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def build_segment(name, t, raw=False):
    seg = SegmentBuffers(name, len(t["g"]))
    for c in ("f", "g", "srt", "m"):
        seg.columns[c] = create_column(c, t[c], "INT")
    seg.columns["inv"] = create_column("inv", t["inv"], "INT", inverted=True)
    for c, (dt, npt) in TYPES.items():
        if c not in t:
            continue
        if raw:
            vals = t[c].copy()
            if c == "d":  # a raw column holds whatever bits were written: every second NaN has its sign bit set
                nans = np.flatnonzero(np.isnan(vals))[::2]
                vals.view(np.int64)[nans] |= np.int64(-1 << 63)
            seg.columns[c] = create_raw_column(c, vals, dt)
        else:
            dictionary, ids = R.java_dictionary(t[c], npt)
            seg.columns[c] = create_column_from_dict_ids(c, dictionary, ids, dt, allow_sorted=False)
    return seg


def sql_of(cols, where="", group=(), exprs=(), tail=""):
    aggs = ["COUNT(*)"]
    for c in list(cols) + [f"{a} + {b}" for a, b in exprs]:
        aggs += [f"SUM({c})", f"MIN({c})", f"MAX({c})"]
    keys = ", ".join(group)
    return (f"SELECT {keys + ', ' if group else ''}{', '.join(aggs)} FROM t{where}"
            f"{' GROUP BY ' + keys if group else ''}{tail}")


def compare(rows, ref, exact, what):
    """rows: {key: [count, sum, min, max, ...]}; ref: float_ref.reference's; exact: per column."""
    assert set(rows) == set(ref), (what, sorted(rows), sorted(ref))
    for key, got in rows.items():
        want = ref[key]
        assert got[0] == want[0], (what, key, "COUNT", got[0], want[0])
        for i, (wsum, bound, wmin, wmax) in enumerate(want[1:]):
            gsum, gmin, gmax = got[1 + 3 * i: 4 + 3 * i]
            print(what, key, i, "sum", gsum, wsum, "bound", bound, "min", gmin, wmin, "max", gmax, wmax)
            if not math.isfinite(wsum) or exact[i]:
                assert R.same_double(gsum, wsum), (what, key, i, "SUM", gsum, wsum)
            else:
                assert abs(gsum - wsum) <= bound, (what, key, i, "SUM", gsum, wsum, bound)
            assert R.same_double(gmin, wmin), (what, key, i, "MIN", gmin, wmin)
            assert R.same_double(gmax, wmax), (what, key, i, "MAX", gmax, wmax)


def run(ctx, segs, tables, name, where="", mask=None, group=(), cols=None, exprs=(), mode=None, kernels=None):
    spec = [(c, e) for c, e in R.VALUE_COLUMNS[name] if cols is None or c in cols]
    names = [c for c, _ in spec]
    sql = ("SET numGroupsLimit=10000000; " if group else "") + sql_of(names, where, group, exprs)
    r = ctx.execute(parse_sql(sql), segs)
    ref = R.reference(tables, names, mask, tuple(group) if group else False, exprs)
    compare(dict(zip(r.keys, r.aggs)), ref, [e for _, e in spec] + [False] * len(exprs), (name, sql))
    if mode is not None:
        assert r.stats.mode == mode, (sql, r.stats.mode, r.stats.scan_kernel)
    if kernels is not None:
        assert r.stats.scan_kernel in kernels, (sql, r.stats.mode, r.stats.scan_kernel)
    return r


FILTERS = [("", None), (" WHERE f < 5", lambda t: t["f"] < 5), (" WHERE f >= 5", lambda t: t["f"] >= 5)]


@pytest.fixture
def pinned(ctx, request):
    made = []

    def pin(name, raw=False, which=(0, 1)):
        tables = [R.make_tables(name)[i] for i in which]
        segs = [ctx.pin(build_segment(f"fa_{name}_{k}_{i}", t, raw)) for k, (i, t) in enumerate(zip(which, tables))]
        made.extend(segs)
        return segs, tables
    yield pin
    for s in made:
        s.unpin()


@pytest.mark.parametrize("raw", [False, True], ids=["dict", "raw"])
@pytest.mark.parametrize("name", R.SETS)
def test_scan_agg_and_lds_group(ctx, pinned, name, raw):
    # forms 1, 2, 7, 8: k_scan MODE_AGG, MODE_GROUP_LDS, dictionary and raw value columns, two segments whose
    # dictionaries differ; a SUM in the query makes the unfiltered case scan too
    segs, tables = pinned(name, raw)
    exprs = (("m", "d"),) if name in ("nan", "inf") else ()
    for where, mask in FILTERS:
        run(ctx, segs, tables, name, where, mask, mode=MODE_AGG)
        run(ctx, segs, tables, name, where, mask, group=("g",), mode=MODE_GROUP_LDS)
        if exprs:
            run(ctx, segs, tables, name, where, mask, cols=(), exprs=exprs, mode=MODE_AGG)
            run(ctx, segs, tables, name, where, mask, group=("g",), cols=(), exprs=exprs, mode=MODE_GROUP_LDS)


@pytest.mark.parametrize("name", R.SETS)
def test_metadata_answer_and_filtered_scan(ctx, pinned, name):
    # no filter, no group-by, COUNT / MIN / MAX only: the dictionaries answer (MIN ignores a NaN, MAX is the NaN);
    # the same query under a filter scans, and a scanned NaN gives NaN
    segs, tables = pinned(name)
    cols = [c for c, _ in R.VALUE_COLUMNS[name]]
    aggs = ", ".join(f"MIN({c}), MAX({c})" for c in cols)
    r = ctx.execute(parse_sql(f"SELECT COUNT(*), {aggs} FROM t"), segs)
    assert r.stats.mode == MODE_META and r.stats.num_entries_scanned_post_filter == 0
    assert r.aggs[0][0] == sum(len(t["g"]) for t in tables)
    for i, c in enumerate(cols):
        firsts = [R.java_dictionary(t[c], t[c].dtype)[0][0] for t in tables]
        lasts = [R.java_dictionary(t[c], t[c].dtype)[0][-1] for t in tables]
        assert R.same_double(r.aggs[0][1 + 2 * i], R.java_min(firsts)), (name, c, "MIN")
        assert R.same_double(r.aggs[0][2 + 2 * i], R.java_max(lasts)), (name, c, "MAX")
    for where, mask in FILTERS[1:]:
        r = ctx.execute(parse_sql(f"SELECT COUNT(*), {aggs} FROM t{where}"), segs)
        assert r.stats.mode == MODE_AGG and r.stats.num_entries_scanned_post_filter > 0
        ref = R.reference(tables, cols, mask)[()]
        assert r.aggs[0][0] == ref[0]
        for i, c in enumerate(cols):
            assert R.same_double(r.aggs[0][1 + 2 * i], ref[1 + i][2]), (name, c, where, "MIN")
            assert R.same_double(r.aggs[0][2 + 2 * i], ref[1 + i][3]), (name, c, where, "MAX")
    if name == "nan":
        assert not math.isnan(ctx.execute(parse_sql("SELECT MIN(d) FROM t"), segs).aggs[0][0])
        assert math.isnan(ctx.execute(parse_sql("SELECT MIN(d) FROM t WHERE f >= 5"), segs).aggs[0][0])


@pytest.mark.parametrize("name", R.SETS)
def test_global_table_and_group_cache(ctx, pinned, monkeypatch, name):
    # form 3: MODE_GROUP_GLOBAL (no LDS table), and its per-workgroup LDS group cache (one value column, two keys)
    segs, tables = pinned(name)
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    for where, mask in FILTERS:
        run(ctx, segs, tables, name, where, mask, group=("g",), mode=MODE_GROUP_GLOBAL)
        for c, _ in R.VALUE_COLUMNS[name]:
            run(ctx, segs, tables, name, where, mask, group=("g", "srt"), cols=(c,), mode=MODE_GROUP_GLOBAL)


@pytest.mark.parametrize("name", R.SETS)
def test_hash_table(name):
    # form 4: MODE_GROUP_HASH, reached at this size through table dictionaries that make the key space 10^18
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    try:
        tables = R.make_tables(name)
        segs = [c.pin(build_segment(f"fh_{name}_{i}", t)) for i, t in enumerate(tables)]
        for k in ("g", "f", "inv"):
            c.set_table_dictionary(k, "INT", np.arange(1_000_000, dtype=np.int32))
        for where, mask in FILTERS[:2]:
            run(c, segs, tables, name, where, mask, group=("g", "f", "inv"), mode=MODE_GROUP_HASH)
        for s in segs:
            s.unpin()
    finally:
        c.close()


@pytest.mark.parametrize("name", R.SETS)
def test_sparse_gathers(ctx, pinned, monkeypatch, name):
    # form 5: an inverted-index leaf; k_agg_sparse over the roaring containers and over the doc bitmap, k_group_sparse
    # (one value column)
    segs, tables = pinned(name)
    where, mask = " WHERE inv = 1", (lambda t: t["inv"] == 1)
    run(ctx, segs, tables, name, where, mask, mode=MODE_AGG)
    run(ctx, segs, tables, name, where, mask, group=("g",))
    monkeypatch.setenv("PH_AGG_SPARSE", "1")
    run(ctx, segs, tables, name, where, mask, mode=MODE_AGG, kernels=(K_AGG_CONT,))
    monkeypatch.setenv("PH_AGG_CONT", "0")
    run(ctx, segs, tables, name, where, mask, mode=MODE_AGG, kernels=(K_AGG_SPARSE,))
    monkeypatch.setenv("PH_GROUP_SPARSE", "1")
    for c, _ in R.VALUE_COLUMNS[name]:
        run(ctx, segs, tables, name, where, mask, group=("g",), cols=(c,), kernels=(K_GROUP_SPARSE, K_GROUP_CONT))
    monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")  # the gather kernel over the group cache + HBM table
    for c, _ in R.VALUE_COLUMNS[name]:
        run(ctx, segs, tables, name, where, mask, group=("g",), cols=(c,), mode=MODE_GROUP_GLOBAL,
            kernels=(K_GROUP_SPARSE, K_GROUP_CONT))


@pytest.mark.parametrize("name", R.SETS)
def test_sorted_leaf_and_conjunction(ctx, pinned, name):
    # form 6: a sorted column's doc range, and an AND of two scan leaves (FK_CONJ)
    segs, tables = pinned(name)
    for where, mask in ((" WHERE srt = 0", lambda t: t["srt"] == 0),
                        (" WHERE f = 7 AND m > 0", lambda t: (t["f"] == 7) & (t["m"] > 0))):
        run(ctx, segs, tables, name, where, mask, mode=MODE_AGG)
        run(ctx, segs, tables, name, where, mask, group=("g",), mode=MODE_GROUP_LDS)


@pytest.mark.parametrize("name", R.SETS)
def test_same_segment_pinned_twice(ctx, pinned, name):
    # form 8: the cross-segment merge of MIN / MAX keys and DOUBLE sums over equal partial results
    segs, tables = pinned(name, which=(0, 0))
    for where, mask in FILTERS[:2]:
        run(ctx, segs, tables, name, where, mask, mode=MODE_AGG)
        run(ctx, segs, tables, name, where, mask, group=("g",), mode=MODE_GROUP_LDS)


@pytest.mark.parametrize("name", R.SETS)
def test_dense_partials(ctx, pinned, name):
    # form 9: execute_dense + dense_finalize over two key shards
    import torch

    from pinot_amd.distributed import Layout, alloc_tables, shard_bounds
    segs, tables = pinned(name)
    ctx.set_table_dictionary("g", "INT", np.arange(R.NUM_GROUPS, dtype=np.int32))  # dense partials need it
    spec = R.VALUE_COLUMNS[name]
    names = [c for c, _ in spec]
    for group in ((), ("g",)):
        for where, mask in FILTERS[:2]:
            q = parse_sql(sql_of(names, where, group))
            lay = Layout.from_native(ctx.dense_layout(q, segs))
            tabs = alloc_tables(lay, 2, torch.device("cuda", 0))
            ctx.execute_dense(q, segs, [t.data_ptr() for t in tabs])
            torch.cuda.synchronize()
            rows = {}
            for rank in range(2):
                _, g0, g1 = shard_bounds(lay.num_groups, 2, rank)
                if g1 <= g0:
                    continue
                shard = [t[g0 * per:g1 * per] for t, per in zip(tabs, lay.elems_per_group)]
                res = ctx.dense_finalize(q, segs, [t.data_ptr() for t in shard], g0, g1)
                rows.update(zip(res.keys, res.aggs))
            ref = R.reference(tables, names, mask, bool(group))
            if not group and ref[()][0] == 0:
                ref = {}  # a dense shard finalises the groups that matched docs
            compare(rows, ref, [e for _, e in spec], (name, "dense", where, group))


@pytest.mark.parametrize("name", R.SETS)
def test_multi_device_merge(name):
    # form 10: the in-library merge of two logical shards of one device
    from pinot_amd.engine import GpuContext
    c = GpuContext(devices=[0, 0])
    try:
        tables = R.make_tables(name)
        segs = [c.pin(build_segment(f"fm_{name}_{i}", t)) for i, t in enumerate(tables)]
        assert sorted(c.segment_device(s) for s in segs) == [0, 1]
        for where, mask in FILTERS[:2]:
            r = run(c, segs, tables, name, where, mask)
            assert r.stats.num_devices == 2
            r = run(c, segs, tables, name, where, mask, group=("g",))
            assert r.stats.num_devices == 2
        for s in segs:
            s.unpin()
    finally:
        c.close()


def _order_key(x, desc):
    k = int(R.java_order_key(np.array([x]))[0])
    return -k if desc else k


@pytest.mark.parametrize("name,order,desc", [("nan", "MIN(d)", False), ("nan", "SUM(d)", True),
                                             ("zeros", "MIN(d)", False), ("zeros", "SUM(d)", True),
                                             # group 3 is kept by both segments, 0.0 in one and -0.0 in the other:
                                             # the combine's Math.min / Math.max of the two decides MIN and MAX
                                             ("zeros", "MIN(d)", True)])
def test_segment_trim_orders_by_double_compare(ctx, pinned, name, order, desc):
    # form 11: each segment keeps max(5 * LIMIT, minSegmentGroupTrimSize) = 5 of its 12 groups by the ORDER BY value
    # under Double.compare (NaN largest, -0.0 < 0.0; ties broken by g), then the kept rows merge
    segs, tables = pinned(name)
    sql = (f"SET minSegmentGroupTrimSize=1; SELECT g, COUNT(*), SUM(d), MIN(d), MAX(d) FROM t GROUP BY g "
           f"ORDER BY {order}{' DESC' if desc else ''}, g LIMIT 1")
    r = ctx.execute(parse_sql(sql), segs)
    kept = []
    for t in tables:
        ref = R.reference([t], ["d"], None, True)
        col = 0 if order.startswith("SUM") else 2
        ranked = sorted(ref, key=lambda k: (_order_key(ref[k][1][col], desc), k))
        kept.append(set(ranked[:5]))
    if (name, order, desc) == ("zeros", "MIN(d)", True):
        assert (3,) in kept[0] & kept[1]
    want = {}
    for k in kept[0] | kept[1]:
        want[k] = R.reference([t for t, ks in zip(tables, kept) if k in ks], ["d"], lambda t, k=k: t["g"] == k[0])[()]
    compare(dict(zip(r.keys, r.aggs)), want, [R.VALUE_COLUMNS[name][0][1]], (name, sql))
    assert r.num_groups == len(want) < R.NUM_GROUPS


@pytest.mark.parametrize("name", ["nan", "inf", "zeros"])
def test_datatable_round_trip_and_broker_merge(ctx, pinned, name):
    # form 12: DataTable V4 cells bit for bit, and the broker's merge of two servers' tables equal to one call
    from pinot_amd import datatable as DT
    segs, tables = pinned(name)
    spec = R.VALUE_COLUMNS[name]
    names = [c for c, _ in spec]
    for group in ((), ("g",)):
        for where, mask in FILTERS:
            q = parse_sql(sql_of(names, where, group, tail=" ORDER BY g LIMIT 100" if group else ""))
            one = DT.reduce_datatables(q, [DT.decode(ctx.execute_datatable(q, segs))]).rows
            two = DT.reduce_datatables(q, [DT.decode(ctx.execute_datatable(q, [s])) for s in segs]).rows
            nk = len(group)
            ref = R.reference(tables, names, mask, bool(group))
            compare({tuple(r[:nk]): r[nk:] for r in one}, ref, [e for _, e in spec], (name, "datatable", where))
            compare({tuple(r[:nk]): r[nk:] for r in two}, ref, [e for _, e in spec], (name, "broker", where))
            for a, b in zip(one, two):  # MIN / MAX / COUNT / keys of the merge: the one call's, bit for bit
                for i, (x, y) in enumerate(zip(a, b)):
                    if i < nk + 1 or (i - nk - 1) % 3 != 0:
                        assert R.same_double(x, y), (name, where, a, b)
    if name == "nan":
        assert math.isnan(DT.merge_intermediate("MIN", 1.0, math.nan)) and math.isnan(
            DT.merge_intermediate("MIN", math.nan, 1.0))
