"""GPU: VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP through ph_query_execute against tests/moments_ref.py (exact
Fractions), form x mode.

Shapes: 1, 63, 64, 65 docs (the mask-word edges) and 4 * 64 * 3 + 1 = 769 docs split over two segments with different
dictionaries, so the shift K is the call's.  Group 5 holds exactly one doc, group 6 four docs of one value.  Every
query carries two functions over the form's column, one over a second (narrow) column and COUNT(*), so a call mixes
forms.  Tolerances: integer forms -- count exact, sum the correctly rounded exact sum, m2 within 2^-51 relative (the
finish's two roundings, doubled) and exactly 0.0 where the exact m2 is 0; real form -- the DOUBLE SUM rule, 1e-9
relative, on the two accumulated sums: |sum - exact| <= 1e-9 sum|x|, |m2 - exact| <= 1e-9 sum((x - K)^2)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import decode, reduce_datatables, variance_deserialize
from pinot_amd.native import UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_segment
from tests.moments_ref import exact_groups

pytestmark = pytest.mark.gpu

K_MOMENTS = 21
MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
ONE_DOC, EQUAL_DOCS = 13, (22, 43, 302, 604)  # docs of groups 5 and 6 (all pass the range filter on f)


def column(form, n):
    i = np.arange(n, dtype=np.int64)
    if form == "narrow":  # a large offset: SUM(x * x) in double would cancel
        return (1_700_000_000 + i * 37 % 1000).astype(np.int32), "INT", True
    if form == "wide_carry":  # d^2 ~ 2^62: the sum crosses 2^64 from 8 docs on
        return np.where(i % 7 == 3, i, np.where(i % 2 == 0, INT_MIN, INT_MAX)).astype(np.int32), "INT", True
    if form == "wide_product":  # |d| up to 2^40: d^2 > 2^64
        return (i * 2654435761 % (1 << 41) - (1 << 40)).astype(np.int64), "LONG", True
    if form == "real_double":  # spread evenly about the midpoint of the range
        return 1000.5 + (i % 101 - 50) * 0.37, "DOUBLE", False
    return (-3.25 + (i * 5 % 64) * 0.125 + 4.0).astype(np.float32), "FLOAT", False  # real_float


FORMS = ["narrow", "wide_carry", "wide_product", "real_double", "real_float"]


def make_table(form, n):
    i = np.arange(n)
    x, dtype, _ = column(form, n)
    g = (i % 5).astype(np.int32)
    if n > ONE_DOC:
        g[ONE_DOC] = 5
    if n > max(EQUAL_DOCS):
        g[list(EQUAL_DOCS)] = 6
        x[list(EQUAL_DOCS)] = x[EQUAL_DOCS[0]]
    return {"g": (g, "INT"), "f": ((i % 10).astype(np.int32), "INT"), "x": (x, dtype),
            "y": ((i * 11 % 257 - 90).astype(np.int32), "INT"), "s": (np.array([f"v{k % 3}" for k in i]), "STRING")}


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def pinned(ctx, form, n, splits):
    t = make_table(form, n)
    bounds = [0] + list(splits) + [n]
    return t, [ctx.pin(create_segment(f"mo_{form}_{n}_{k}", {c: (v[a:b], dt) for c, (v, dt) in t.items()}))
               for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]


def check_tuple(got, exact, values, integer, what):
    n, s, m2 = exact
    assert got[0] == n, what
    if integer:
        assert got[1] == float(s), what
        assert abs(Fraction(got[2]) - m2) <= Fraction(1, 2 ** 51) * m2, (what, got[2], float(m2))
        if m2 == 0:
            assert got[2] == 0.0, what
    else:  # (m2 is checked by the caller, which knows the call's K)
        assert abs(Fraction(got[1]) - s) <= Fraction(1, 10 ** 9) * sum(abs(Fraction(v)) for v in values.tolist()), what


WHERE = {"none": ("", lambda t: np.ones(len(t["f"][0]), bool)),
         "range": (" WHERE f BETWEEN 2 AND 7", lambda t: (t["f"][0] >= 2) & (t["f"][0] <= 7)),
         "nothing": (" WHERE f > 100", lambda t: np.zeros(len(t["f"][0]), bool))}


def run(ctx, t, segs, form, where, mode):
    clause, mask_of = WHERE[where]
    grouped = mode != MODE_AGG
    sql = (f"SELECT {'g, ' if grouped else ''}VAR_POP(x), STDDEV_SAMP(x), VAR_SAMP(y), COUNT(*) FROM t{clause}"
           f"{' GROUP BY g ORDER BY g LIMIT 100' if grouped else ''}")
    q = parse_sql(sql)
    r = ctx.execute(q, segs)
    assert r.stats.scan_kernel == K_MOMENTS and r.stats.mode == mode, (sql, r.stats.scan_kernel, r.stats.mode)
    mask = mask_of(t)
    keys = t["g"][0] if grouped else None
    integer = column(form, 1)[2]
    ex, ey = exact_groups(keys, t["x"][0], mask), exact_groups(keys, t["y"][0], mask)
    xs_all = [Fraction(v) for v in t["x"][0].tolist()]
    kx = Fraction(float(min(xs_all))) / 2 + Fraction(float(max(xs_all))) / 2  # the call's K of a real column

    def check_rows(rows):  # {key: [tuple of x, tuple of x, tuple of y, count]}
        if not grouped and not mask.any():
            assert rows == {(): [(0, 0.0, 0.0), (0, 0.0, 0.0), (0, 0.0, 0.0), 0]}
        assert sorted(rows) == sorted(ex), sql
        for key, row in rows.items():
            sel = mask & (keys == key[0]) if grouped else mask
            assert row[0] == row[1] and row[3] == ex[key][0], (sql, key)
            print(sql, key, "x", row[0], "exact", ex[key][0], float(ex[key][1]), float(ex[key][2]), "y", row[2])
            check_tuple(row[0], ex[key], t["x"][0][sel], integer, (sql, key))
            if not integer:
                s2 = sum((Fraction(v) - kx) ** 2 for v in t["x"][0][sel].tolist())
                if not grouped and where == "none":
                    assert s2 <= 4 * ex[key][2], "the inputs are not spread about K"  # so the bound is <= 4e-9 of m2
                assert abs(Fraction(row[0][2]) - ex[key][2]) <= Fraction(1, 10 ** 9) * s2, (sql, key, row[0][2])
            check_tuple(row[2], ey[key], t["y"][0][sel], True, (sql, key, "y"))

    check_rows(dict(zip(r.keys, r.aggs)))
    assert r.stats.num_docs_scanned == int(mask.sum())
    assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * (2 + grouped)
    # (a scan leaf examines every doc; on the 1-doc segment the dictionary already shows the filter empty)
    assert r.stats.num_entries_scanned_in_filter == (len(mask) if where == "range" and mask.any() else 0)
    # SQL -> ph_query_execute -> DataTable -> broker reduce -> the final doubles.  A second call: its tuples meet the
    # same bounds (a real form's sums depend on the order of the atomics, an integer form's are the same bits)
    dt = decode(ctx.execute_datatable(q, segs))
    assert dt.column_names == grouped * ["g"] + ["varpop(x)", "stddevsamp(x)", "varsamp(y)", "count(*)"]
    nk = int(grouped)
    check_rows({tuple(row[:nk]): [variance_deserialize(c[1]) if isinstance(c, tuple) and c[0] == 33 else c
                                  for c in row[nk:]] for row in dt.rows})
    table = reduce_datatables(q, [dt])
    if integer:
        want = reduce_groups(q, r.keys, r.aggs)
        assert table.columns == want.columns and table.rows == want.rows, sql
    if grouped and where != "nothing" and len(mask) > ONE_DOC:
        one = [row for row in table.rows if row[0] == 5][0]
        assert one[1] == 0.0 and one[2] == -math.inf and one[3] == -math.inf and one[4] == 1  # pop 0, sample -Infinity
    return r


@pytest.mark.parametrize("mode", [MODE_AGG, MODE_LDS, MODE_HBM], ids=["agg", "lds", "hbm"])
@pytest.mark.parametrize("where", sorted(WHERE))
@pytest.mark.parametrize("form", FORMS)
def test_two_segments(ctx, monkeypatch, form, where, mode):
    if mode == MODE_HBM:
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    t, segs = pinned(ctx, form, 4 * 64 * 3 + 1, [500])
    try:
        run(ctx, t, segs, form, where, mode)
    finally:
        for s in segs:
            s.unpin()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("form", FORMS)
def test_mask_word_edges(ctx, form, n):
    t, segs = pinned(ctx, form, n, [])
    try:
        for where in ("none", "range"):
            run(ctx, t, segs, form, where, MODE_AGG)
            run(ctx, t, segs, form, where, MODE_LDS)
    finally:
        segs[0].unpin()


REFUSALS = [("SELECT VAR_POP(s) FROM t", "STRING column"),
            ("SELECT SUM(x), VAR_POP(x) FROM t", "SUM beside a variance function"),
            ("SELECT VAR_POP(x) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
            ("SET numGroupsLimit=5; SELECT g, VAR_POP(x) FROM t GROUP BY g",
             "variance functions where a segment could reach numGroupsLimit"),
            ("SET minSegmentGroupTrimSize=1; SELECT g, VAR_POP(x) FROM t GROUP BY g ORDER BY g LIMIT 5",
             "variance functions with segment group trim"),
            ("dense", "dense partials")]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals(ctx, sql, word):
    t, segs = pinned(ctx, "narrow", 65, [])
    try:
        with pytest.raises(UnsupportedError, match=word) as e:
            if sql == "dense":
                ctx.dense_layout(parse_sql("SELECT g, VAR_POP(x) FROM t GROUP BY g"), segs)
            else:
                ctx.execute(parse_sql(sql), segs)
        assert e.value.code == N.PH_ERR_UNSUPPORTED
    finally:
        segs[0].unpin()
