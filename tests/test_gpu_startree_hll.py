"""GPU: DISTINCTCOUNTHLL answered from a star-tree's distinctCountHLL__<col> pair columns (the view's sketch columns:
k_scan's match list + k_hll_sketch_merge, scan_hll_sketch.hip).  The expected answer is the oracle over the RAW
documents; registers are compared raw and bit-exact, the other aggregates on the bars of test_gpu_startree.  The
per-value registers the builder merges come from the oracle itself (SELECT c, DISTINCTCOUNTHLL(c) ... GROUP BY c over
the raw segment), so nothing is hashed here.  oracle/startree.py does not know the pair, so the statistics are checked
against the GPU's own answer to the same query with SUM(m) in place of the sketches (a path test_gpu_startree checks
against the oracle)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.query import parse_sql
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_segment
from pinot_amd.startree import attach, build_star_tree
from tests.test_gpu_parity import rows_equal
from tests.test_startree_cpu import PAIRS, star_table

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SIZES = (6000, 2500, 3001)
STAR = (True, True, False)


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _table(rng, n):
    cols = star_table(rng, n)
    cols["c"] = (rng.integers(0, 300, n).astype(np.int32) * 7 - 400, "INT")
    cols["c2"] = (np.array([f"u{v:02d}" for v in rng.integers(0, 40, n)]), "STRING")
    return cols


def _doc_registers(oseg, cols, col, log2m):
    """uint8 [num_docs, 2^log2m]: each raw document's single-value registers, from the oracle's per-value sketches."""
    e = O.execute(parse_sql(f"SELECT {col}, DISTINCTCOUNTHLL({col}, {log2m}) FROM t GROUP BY {col} LIMIT 100000"), [oseg])
    values = np.asarray(cols[col][0])
    uniq, inv = np.unique(values, return_inverse=True)
    per_value = np.zeros((len(uniq), 1 << log2m), np.uint8)
    by_key = {k[0]: np.asarray(a[0], np.uint8) for k, a in zip(e.keys, e.aggs)}
    assert len(by_key) == len(uniq)
    for i, v in enumerate(uniq):
        per_value[i] = by_key[v.item() if hasattr(v, "item") else v]
    return per_value[inv]


@functools.lru_cache(maxsize=None)
def _built(log2m, max_leaf, sizes=SIZES, seed=5):
    """[(SegmentBuffers, StarTreeBuffers, oracle segment)] -- built once per shape and shared, never changed."""
    rng = np.random.default_rng(seed + 100 * log2m + max_leaf)
    out = []
    for i, n in enumerate(sizes):
        cols = _table(rng, n)
        name = f"h{log2m}_{max_leaf}_{i}"
        seg = create_segment(name, cols)
        oseg = O.build_segment(name, cols)
        vals = {c: v for c, (v, _) in cols.items()}
        for c in ("c", "c2"):
            vals[c] = _doc_registers(oseg, cols, c, log2m)
        st = build_star_tree(seg, ["d1", "d2", "d3"], PAIRS + [("distinctCountHLL", "c"), ("distinctCountHLL", "c2")],
                             max_leaf, (), values=vals)
        out.append((seg, st, oseg))
    return out


def _pin(ctx, built, star=STAR):
    gpu = []
    for (seg, st, _), has in zip(built, star):
        p = ctx.pin(seg)
        if has:
            attach(p, st)
        gpu.append(p)
    return gpu, [o for _, _, o in built]


@pytest.fixture(scope="module")
def pinned(ctx):
    cache = {}

    def get(log2m, max_leaf):
        if (log2m, max_leaf) not in cache:
            cache[(log2m, max_leaf)] = _pin(ctx, _built(log2m, max_leaf))
        return cache[(log2m, max_leaf)]
    return get


def _check(ctx, gpu, ora, sql, cmp_sql, nstar, post=True):
    """`sql` on the GPU (star-trees taken) against the raw-document oracle; statistics against `cmp_sql`, the same
    query with SUM(m) in place of the sketches."""
    q = parse_sql(sql)
    r = ctx.execute(q, gpu)
    e = O.execute(q, ora)
    rows_equal(reduce_groups(q, r.keys, r.aggs).rows, reduce_groups(q, e.keys, e.aggs).rows, RTOL)
    assert len(r.keys) == len(e.keys)
    for k, a in enumerate(q.aggregations):
        if a.function == "DISTINCTCOUNTHLL":
            gmap = {key: row[k] for key, row in zip(r.keys, r.aggs)}
            for key, row in zip(e.keys, e.aggs):
                assert np.array_equal(gmap[key], row[k]), (sql, key)
    c = ctx.execute(parse_sql(cmp_sql), gpu)
    if nstar is None:  # (a filter that matches nothing: whatever the comparator's plan takes)
        nstar = c.stats.num_segments_star_tree
    assert r.stats.num_segments_star_tree == nstar, sql
    assert c.stats.num_segments_star_tree == nstar, cmp_sql
    assert r.stats.num_docs_scanned == c.stats.num_docs_scanned, sql
    assert r.stats.num_entries_scanned_in_filter == c.stats.num_entries_scanned_in_filter, sql
    assert r.stats.num_total_docs == c.stats.num_total_docs == e.stats.num_total_docs, sql
    if post:
        assert r.stats.num_entries_scanned_post_filter == c.stats.num_entries_scanned_post_filter, sql
    return r


def _hll(col, log2m):
    return f"DISTINCTCOUNTHLL({col})" if log2m == 8 else f"DISTINCTCOUNTHLL({col}, {log2m})"


# (select list with {c} / {c2} for the sketches, the comparator's select list, the rest of the query, post-filter
# entries comparable: both project the same number of columns in the views AND in the plain segment)
SHAPES = [
    ("{c}", "SUM(m)", " WHERE d2 = 'ny' AND d1 IN (10, 30, 50)", True),                       # MODE_AGG
    ("d1, {c}", "d1, SUM(m)", " GROUP BY d1", True),                                          # LDS table
    ("d1, d3, {c}", "d1, d3, SUM(m)",
     " WHERE (d3 = 7 OR d3 = 12007 OR d3 > 30000) AND d2 <> 'tx' GROUP BY d1, d3 LIMIT 1000", True),  # remaining predicates
    ("d2, COUNT(*), SUM(m), {c}, {c2}", "d2, COUNT(*), SUM(m), MIN(m), MAX(x)", " GROUP BY d2", False),  # two sketches
    ("COUNT(*), SUM(m), {c}, {c2}", "COUNT(*), SUM(m), MIN(m), MAX(x)", " WHERE d3 < 20000", False),
    ("d1, {c}", "d1, SUM(m)", " WHERE d1 = 10 AND d1 = 20 GROUP BY d1", True),                # matches nothing
]


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("max_leaf", [3, 25])
@pytest.mark.parametrize("log2m", [4, 8, 12])
def test_sketch_queries(ctx, pinned, log2m, max_leaf, shape):
    gpu, ora = pinned(log2m, max_leaf)
    sel, cmp_sel, rest, post = SHAPES[shape]
    sql = "SELECT " + sel.format(c=_hll("c", log2m), c2=_hll("c2", log2m)) + " FROM t" + rest
    _check(ctx, gpu, ora, sql, "SELECT " + cmp_sel + " FROM t" + rest, None if "d1 = 20" in rest else 2, post)


@pytest.mark.parametrize("log2m", [4, 8, 12])
def test_sketch_group_by_in_the_hbm_table(ctx, pinned, log2m):
    gpu, ora = pinned(log2m, 25)
    sql = f"SELECT d1, {_hll('c', log2m)} FROM t GROUP BY d1"
    ctx.set_option("lds_table_max", 16)  # no group table fits: the scan aggregates in the HBM table
    try:
        _check(ctx, gpu, ora, sql, "SELECT d1, SUM(m) FROM t GROUP BY d1", 2)
    finally:
        ctx.set_option("lds_table_max", None)


@pytest.mark.parametrize("log2m", [4, 12])
def test_star_segments_only(ctx, log2m):
    built = _built(log2m, 10, sizes=(4000, 5000), seed=11)
    gpu, ora = _pin(ctx, built, star=(True, True))
    try:
        for sel, cmp_sel, rest, _ in SHAPES[:5]:
            sql = "SELECT " + sel.format(c=_hll("c", log2m), c2=_hll("c2", log2m)) + " FROM t" + rest
            # both queries project pair columns only here: in the two-sketch shapes count__* and three more each
            r = _check(ctx, gpu, ora, sql, "SELECT " + cmp_sel + " FROM t" + rest, 2, post=True)
            assert r.stats.num_segments_processed == 2
    finally:
        for p in gpu:
            p.unpin()


def test_other_log2m_is_unsupported_and_skip_star_tree(ctx, pinned):
    gpu, ora = pinned(8, 25)
    with pytest.raises(N.UnsupportedError):
        ctx.execute(parse_sql("SELECT d1, DISTINCTCOUNTHLL(c, 10) FROM t GROUP BY d1"), gpu)
    sql = "SELECT d1, COUNT(*), DISTINCTCOUNTHLL(c) FROM t WHERE d2 IN ('ca', 'wa') GROUP BY d1"
    q = parse_sql(sql)
    star = ctx.execute(q, gpu)
    qs = parse_sql("SET skipStarTree=true; " + sql)
    raw = ctx.execute(qs, gpu)
    assert star.stats.num_segments_star_tree == 2 and raw.stats.num_segments_star_tree == 0
    assert reduce_groups(q, star.keys, star.aggs).rows == reduce_groups(qs, raw.keys, raw.aggs).rows
    rmap = {key: row[1] for key, row in zip(raw.keys, raw.aggs)}
    for key, row in zip(star.keys, star.aggs):
        assert np.array_equal(rmap[key], row[1])


def test_sketch_tree_from_segment_directory(ctx, tmp_path):
    from tests import segment_dirs as SD
    seg, st, oseg = _built(8, 25)[1]
    path = str(tmp_path / "st")
    SD.write_v3(seg, path)
    SD.write_star_trees(path, [st])
    loaded = ctx.load_segment_dir(path)
    try:
        assert N.lib().ph_segment_num_star_trees(loaded.handle) == 1
        for sel, cmp_sel, rest, _ in SHAPES[:4]:
            sql = "SELECT " + sel.format(c=_hll("c", 8), c2=_hll("c2", 8)) + " FROM t" + rest
            _check(ctx, [loaded], [oseg], sql, "SELECT " + cmp_sel + " FROM t" + rest, 1, post=False)
    finally:
        loaded.unpin()


def test_segment_trim_ordered_by_the_sketch(ctx, pinned):
    # minSegmentGroupTrimSize runs one segment per call, each taking its own star-tree; the trim orders the segment's
    # groups by hll_cardinality of the merged registers.  d3's 40 groups all survive a trim size of 64, so the answer
    # is the raw documents'
    gpu, ora = pinned(8, 25)
    sql = ("SET minSegmentGroupTrimSize=64; SELECT d3, DISTINCTCOUNTHLL(c) FROM t GROUP BY d3 "
           "ORDER BY DISTINCTCOUNTHLL(c) DESC, d3 LIMIT 5")
    q = parse_sql(sql)
    r = ctx.execute(q, gpu)
    e = O.execute(q, ora)
    assert r.stats.num_segments_star_tree == 2
    assert reduce_groups(q, r.keys, r.aggs).rows == reduce_groups(q, e.keys, e.aggs).rows


def test_sketch_queries_on_two_logical_devices():
    from pinot_amd.engine import GpuContext
    m = GpuContext(devices=[0, 0])
    try:
        gpu, ora = _pin(m, _built(8, 25))
        for i in (1, 3):
            sel, cmp_sel, rest, _ = SHAPES[i]
            sql = "SELECT " + sel.format(c=_hll("c", 8), c2=_hll("c2", 8)) + " FROM t" + rest
            _check(m, gpu, ora, sql, "SELECT " + cmp_sel + " FROM t" + rest, 2, post=False)
    finally:
        m.close()
