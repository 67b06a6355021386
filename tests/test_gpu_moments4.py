"""GPU: SKEWNESS / KURTOSIS through ph_query_execute against tests/moments4_ref.py (exact Fractions), layout x mode.

Shapes: 1, 63, 64, 65 docs (the mask-word edges) and 4 * 64 * 3 + 1 = 769 docs split over two segments with different
dictionaries, so the shift K is the call's.  Group 5 holds exactly one doc, group 6 four docs of one value.  Every
query carries both functions over the layout's column, one over a second (narrow, M4_L8) column and COUNT(*), so a call
mixes layouts and shares a slot.

Tolerances.  Integer layouts: n exact, m1 within 2^-52 relative of the exact mean and m_k within (k + 1) 2^-52 relative
of the exact m_k (the finish's k + 1 roundings, doubled), exactly 0.0 where the exact value is 0, and two calls give
the same bits.  Real layout: the finish evaluates, with a = S1 / n and S_k the accumulated sum(d^k) of d = x - K,
  m1 = K + a,  m2 = S2 - a S1,  m3 = S3 - 3 a S2 + 2 a^2 S1,  m4 = S4 - 4 a S3 + 6 a^2 S2 - 3 a^3 S1,
so under the DOUBLE SUM rule (1e-9 relative to the sum of the magnitudes of the terms, T_k = sum|d|^k) the bounds are
1e-9 times  |K| + T1 / n,  T2 + |a| T1,  T3 + 3 |a| T2 + 2 a^2 T1  and  T4 + 4 |a| T3 + 6 a^2 T2 + 3 |a|^3 T1.
The real inputs are spread evenly about K, so the bounds of m2 and m4 stay within 4x and 8x the exact moments."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import decode, fourthmoment_deserialize, reduce_datatables
from pinot_amd.native import UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.reduce import fourthmoment_serialize, reduce_groups
from pinot_amd.segment import create_segment
from tests.moments4_ref import exact_groups

pytestmark = pytest.mark.gpu

K_MOMENTS4 = 23
MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
ONE_DOC, EQUAL_DOCS = 13, (22, 43, 302, 604)  # docs of groups 5 and 6 (all pass the range filter on f)
ULP = Fraction(1, 2 ** 52)


def column(layout, n):
    i = np.arange(n, dtype=np.int64)
    if layout == "l8":  # one cell per power, on an offset where a double sum(x^4) would be useless
        return (1_700_000_000 + i * 37 % 250).astype(np.int32), "INT", True
    if layout == "l16":  # a range near 2^16
        return (1000 + i * 7919 % 65500).astype(np.int32), "INT", True
    if layout == "l32_carry":  # d ~ 2^32: every limb sum is large, so reassembly carries through every word
        return np.where(i % 7 == 3, i, np.where(i % 2 == 0, INT_MIN, INT_MAX)).astype(np.int32), "INT", True
    if layout == "long_k62":  # the integer path with a K that does not fit a double
        return ((1 << 62) + 12345 + i * 2654435761 % (1 << 31)).astype(np.int64), "LONG", True
    if layout == "long_real":  # a range of 2^41: the real layout reached from integers
        return ((i * 2654435761 % (1 << 9) - (1 << 8)) << 32).astype(np.int64), "LONG", False
    if layout == "real_double":
        return 1000.5 + (i % 101 - 50) * 0.375, "DOUBLE", False
    return (-3.25 + (i * 5 % 64) * 0.125 + 4.0).astype(np.float32), "FLOAT", False  # real_float


LAYOUTS = ["l8", "l16", "l32_carry", "long_k62", "long_real", "real_double", "real_float"]


def make_table(layout, n):
    i = np.arange(n)
    x, dtype, _ = column(layout, n)
    g = (i % 5).astype(np.int32)
    if n > ONE_DOC:
        g[ONE_DOC] = 5
    if n > max(EQUAL_DOCS):
        g[list(EQUAL_DOCS)] = 6
        x[list(EQUAL_DOCS)] = x[EQUAL_DOCS[0]]
    return {"g": (g, "INT"), "f": ((i % 10).astype(np.int32), "INT"), "x": (x, dtype),
            "y": ((i * 11 % 200 - 90).astype(np.int32), "INT"), "s": (np.array([f"v{k % 3}" for k in i]), "STRING")}


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def pinned(ctx, name, t, splits):
    n = len(next(iter(t.values()))[0])
    bounds = [0] + list(splits) + [n]
    return [ctx.pin(create_segment(f"m4_{name}_{n}_{k}", {c: (v[a:b], dt) for c, (v, dt) in t.items()}))
            for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]


def check_integer(got, exact, what):
    assert got[0] == exact[0], what
    for k in range(1, 5):
        bound = (1 if k == 1 else k + 1) * ULP * abs(exact[k])  # m1: 2^-52; m_k: (k + 1) 2^-52
        assert abs(Fraction(got[k]) - exact[k]) <= bound, (what, k, got[k], float(exact[k]))
        if exact[k] == 0:
            assert got[k] == 0.0, (what, k)


def check_real(got, exact, values, kx, spread, what):
    d = [Fraction(v) - kx for v in values.tolist()]
    n, a = len(d), abs(sum(d)) / len(d)
    t1, t2, t3, t4 = (sum(abs(x) ** k for x in d) for k in (1, 2, 3, 4))
    bounds = [abs(kx) + t1 / n, t2 + a * t1, t3 + 3 * a * t2 + 2 * a * a * t1,
              t4 + 4 * a * t3 + 6 * a * a * t2 + 3 * a ** 3 * t1]
    if spread:
        assert bounds[1] <= 4 * exact[2] and bounds[3] <= 8 * exact[4], "the inputs are not spread about K"
    assert got[0] == exact[0], what
    for k in range(1, 5):
        assert abs(Fraction(got[k]) - exact[k]) <= Fraction(1, 10 ** 9) * bounds[k - 1], (what, k, got[k], float(exact[k]))


WHERE = {"none": ("", lambda t: np.ones(len(t["f"][0]), bool)),
         "range": (" WHERE f BETWEEN 2 AND 7", lambda t: (t["f"][0] >= 2) & (t["f"][0] <= 7)),
         "nothing": (" WHERE f > 100", lambda t: np.zeros(len(t["f"][0]), bool))}


def run(ctx, t, segs, layout, where, mode):
    clause, mask_of = WHERE[where]
    grouped = mode != MODE_AGG
    sql = (f"SELECT {'g, ' if grouped else ''}SKEWNESS(x), KURTOSIS(x), SKEWNESS(y), COUNT(*) FROM t{clause}"
           f"{' GROUP BY g ORDER BY g LIMIT 100' if grouped else ''}")
    q = parse_sql(sql)
    r = ctx.execute(q, segs)
    assert r.stats.scan_kernel == K_MOMENTS4 and r.stats.mode == mode, (sql, r.stats.scan_kernel, r.stats.mode)
    mask = mask_of(t)
    keys = t["g"][0] if grouped else None
    integer = column(layout, 1)[2]
    ex, ey = exact_groups(keys, t["x"][0], mask), exact_groups(keys, t["y"][0], mask)
    xs_all = t["x"][0].tolist()
    kx = Fraction(0.5 * float(min(xs_all)) + 0.5 * float(max(xs_all)))  # the call's K of a real layout

    def check_rows(rows):  # {key: [tuple of x, tuple of x, tuple of y, count]}
        if not grouped and not mask.any():  # the empty tuple
            (row,) = rows.values()
            assert row[3] == 0 and all(c[0] == 0 and all(math.isnan(m) for m in c[1:]) for c in row[:3]), row
            return
        assert sorted(rows) == sorted(ex), sql
        for key, row in rows.items():
            sel = mask & (keys == key[0]) if grouped else mask
            assert fourthmoment_serialize(row[0]) == fourthmoment_serialize(row[1]) and row[3] == ex[key][0], (sql, key)
            print(sql, key, "x", row[0], "exact", [float(c) for c in ex[key]], "y", row[2])
            if integer:
                check_integer(row[0], ex[key], (sql, key))
            else:
                check_real(row[0], ex[key], t["x"][0][sel], kx, not grouped and where == "none", (sql, key))
            check_integer(row[2], ey[key], (sql, key, "y"))

    rows = dict(zip(r.keys, r.aggs))
    check_rows(rows)
    assert r.stats.num_docs_scanned == int(mask.sum())
    assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * (2 + grouped)
    # (a scan leaf examines every doc; on the 1-doc segment the dictionary already shows the filter empty)
    assert r.stats.num_entries_scanned_in_filter == (len(mask) if where == "range" and mask.any() else 0)
    # SQL -> ph_query_execute -> DataTable -> broker reduce -> the final doubles: a second call, which meets the same
    # bounds and, on an integer layout, gives the same bits
    dt = decode(ctx.execute_datatable(q, segs))
    assert dt.column_names == grouped * ["g"] + ["skewness(x)", "kurtosis(x)", "skewness(y)", "count(*)"]
    nk = int(grouped)
    again = {tuple(row[:nk]): [fourthmoment_deserialize(c[1]) if isinstance(c, tuple) and c[0] == 34 else c
                               for c in row[nk:]] for row in dt.rows}
    check_rows(again)
    table = reduce_datatables(q, [dt])
    if integer:
        assert {k: [fourthmoment_serialize(c) for c in v[:3]] for k, v in again.items()} == \
               {k: [fourthmoment_serialize(c) for c in v[:3]] for k, v in rows.items()}, sql
        want = reduce_groups(q, r.keys, r.aggs)
        assert table.columns == want.columns
        np.testing.assert_equal(table.rows, want.rows)  # (NaN equals NaN here)
    if grouped and where != "nothing" and len(mask) > max(EQUAL_DOCS):
        by_key = {row[0]: row for row in table.rows}
        assert math.isnan(by_key[5][1]) and math.isnan(by_key[5][2]) and by_key[5][4] == 1
        assert by_key[6][1] == 0.0 and by_key[6][2] == 0.0 and by_key[6][4] == 4


@pytest.mark.parametrize("mode", [MODE_AGG, MODE_LDS, MODE_HBM], ids=["agg", "lds", "hbm"])
@pytest.mark.parametrize("where", sorted(WHERE))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_segments(ctx, monkeypatch, layout, where, mode):
    if mode == MODE_HBM:
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    t = make_table(layout, 4 * 64 * 3 + 1)
    segs = pinned(ctx, layout, t, [500])
    try:
        run(ctx, t, segs, layout, where, mode)
    finally:
        for s in segs:
            s.unpin()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_word_edges(ctx, layout, n):
    t = make_table(layout, n)
    segs = pinned(ctx, layout, t, [])
    try:
        for where in ("none", "range"):
            run(ctx, t, segs, layout, where, MODE_AGG)
            run(ctx, t, segs, layout, where, MODE_LDS)
    finally:
        segs[0].unpin()


def test_kat(ctx):
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fourthmoment_kat.json")))
    cols = list(zip(*kat["inputs"]))
    t = {"groupingCol": (np.array(cols[0]), "STRING"), "val": (np.array(cols[2], dtype=np.int32), "INT")}
    segs = pinned(ctx, "kat", t, [])
    try:
        for sql, want in [
                ("SELECT groupingCol, SKEWNESS(val), KURTOSIS(val) FROM t GROUP BY groupingCol ORDER BY groupingCol LIMIT 10",
                 kat["grouped_outputs"]),
                ("SELECT SKEWNESS(val), KURTOSIS(val) FROM t WHERE groupingCol = 'a'", kat["filtered_outputs"])]:
            q = parse_sql(sql)
            r = ctx.execute(q, segs)
            assert r.stats.scan_kernel == K_MOMENTS4
            got = reduce_groups(q, r.keys, r.aggs).rows
            print(sql, got)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g[:-2] == w[:-2] and g[-2:] == pytest.approx(w[-2:], rel=1e-12, abs=0), (sql, g, w)
    finally:
        segs[0].unpin()


REFUSALS = [("SELECT SKEWNESS(s) FROM t", "STRING column"),
            ("SELECT SUM(x), SKEWNESS(x) FROM t", "SUM beside a fourth-moment function"),
            ("SELECT VAR_POP(x), KURTOSIS(x) FROM t", "variance function beside a fourth-moment function"),
            ("SELECT SKEWNESS(x) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
            ("SET numGroupsLimit=5; SELECT g, SKEWNESS(x) FROM t GROUP BY g",
             "fourth-moment functions where a segment could reach numGroupsLimit"),
            ("SET minSegmentGroupTrimSize=1; SELECT g, SKEWNESS(x) FROM t GROUP BY g ORDER BY g LIMIT 5",
             "fourth-moment functions with segment group trim"),
            ("dense", "dense partials")]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals(ctx, sql, word):
    segs = pinned(ctx, "l8", make_table("l8", 65), [])
    try:
        with pytest.raises(UnsupportedError, match=word) as e:
            if sql == "dense":
                ctx.dense_layout(parse_sql("SELECT g, SKEWNESS(x) FROM t GROUP BY g"), segs)
            else:
                ctx.execute(parse_sql(sql), segs)
        assert e.value.code == N.PH_ERR_UNSUPPORTED
    finally:
        segs[0].unpin()
