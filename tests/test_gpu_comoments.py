"""GPU: COVAR_POP / COVAR_SAMP through ph_query_execute against tests/comoments_ref.py (exact Fractions), form x mode.

Shapes: 1, 31, 32, 33, 63, 64, 65 docs (a lane's 32-doc run and the mask-word edges), 2048 + 33 docs (a full tile and a
ragged second one) and 2 * 2048 + 1 docs split over two segments with different dictionaries of every column, so Kx, Ky
are the call's and the group-by remap is in play.  Group 5 holds exactly one doc (13); group 6 is the run of equal keys
30..35, which crosses a lane boundary.  Every query carries COVAR_POP(x, y), COVAR_SAMP(x, y), COVAR_POP(y, x) and
COUNT(*).  Integer forms: count exact and each sum equal to float(exact Fraction), the correctly rounded value, bit for
bit.  Real forms: the DOUBLE SUM rule, |got - exact| <= 1e-9 sum|term| per component.

The `widths` form holds a 1-bit stream beside a 17-bit one.  A 32-bit stream cannot be pinned: the segment format's
width is getNumBitsPerValue(cardinality - 1), at most 31 bits, and 18 bits and more need 2^17 distinct values and
docs.  17 bits selects the kernels' 8-register decode, whose one compile-time switch covers the widths 17..32."""
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import covariance_deserialize, decode, reduce_datatables
from pinot_amd.native import UnsupportedError
from pinot_amd.query import parse_sql
from pinot_amd.reduce import covariance_final
from pinot_amd.segment import create_segment
from tests.comoments_ref import exact_groups

pytestmark = pytest.mark.gpu

K_COMOMENTS = 22
MODE_AGG, MODE_LDS, MODE_HBM = 1, 2, 3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
ONE_DOC, RUN = 13, slice(30, 36)
TWO_SEGMENTS = 2 * 2048 + 1


def columns(form, n):
    """x, y and whether the form is an integer one"""
    i = np.arange(n, dtype=np.int64)
    small = (i * 11 % 257 - 90).astype(np.int32)
    if form == "narrow":  # a large offset: SUM(x * y) in double would round
        return ((1_700_000_000 + i * 37 % 1000).astype(np.int32), "INT"), (small, "INT"), True
    if form == "wide_carry":  # dx dy is 0 or (2^32 - 1)^2: the low cell carries within a few docs
        return ((np.where(i % 2 == 0, INT_MIN, INT_MAX).astype(np.int32), "INT"),
                (np.where(i % 3 == 0, INT_MIN, INT_MAX).astype(np.int32), "INT"), True)
    if form == "wide_product":  # ranges of 2^41: one product passes 2^64
        return (((i * 2654435761 % (1 << 41) - (1 << 40)).astype(np.int64), "LONG"),
                (((i + 1) * 40503 * 7919 % (1 << 41) - (1 << 40)).astype(np.int64), "LONG"), True)
    if form == "real_double":
        return (1000.5 + (i % 101 - 50) * 0.37, "DOUBLE"), (-3.25 + (i * 7 % 64) * 0.125, "DOUBLE"), False
    if form == "real_mixed":
        return ((-3.25 + (i * 5 % 64) * 0.125).astype(np.float32), "FLOAT"), (small, "INT"), False
    return ((i % 2).astype(np.int32), "INT"), ((i * 3 - 70_000).astype(np.int32), "INT"), True  # widths: 1 and 17 bits


FORMS = ["narrow", "wide_carry", "wide_product", "real_double", "real_mixed"]


def make_table(form, n, split):
    i = np.arange(n)
    (x, xt), (y, yt), _ = columns(form, n)
    g = (i % 5).astype(np.int32)
    if split:  # other dictionaries in the second segment: groups 1..4 and 7, and (integer columns) other values
        g[split:] = 1 + i[split:] % 4
        g[split + 3] = 7
        if form in ("narrow", "wide_product"):
            x[split:] += 5000
            y[split:] -= 300
    if n > ONE_DOC:
        g[ONE_DOC] = 5
    if n > RUN.stop:
        g[RUN] = 6
    return {"g": (g, "INT"), "f": ((i % 10).astype(np.int32), "INT"), "x": (x, xt), "y": (y, yt),
            "s": (np.array([f"v{k % 3}" for k in i]), "STRING")}


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd.engine import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def pinned(ctx, form, n, split=0):
    t = make_table(form, n, split)
    bounds = [0, split, n] if split else [0, n]
    return t, [ctx.pin(create_segment(f"co_{form}_{n}_{k}", {c: (v[a:b], dt) for c, (v, dt) in t.items()}))
               for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]


WHERE = {"none": ("", lambda f: np.ones(len(f), bool)),
         "range": (" WHERE f BETWEEN 2 AND 7", lambda f: (f >= 2) & (f <= 7)),
         "nothing": (" WHERE f > 100", lambda f: np.zeros(len(f), bool))}


def run(ctx, t, segs, form, where, mode):
    clause, mask_of = WHERE[where]
    grouped = mode != MODE_AGG
    sql = (f"SELECT {'g, ' if grouped else ''}COVAR_POP(x, y), COVAR_SAMP(x, y), COVAR_POP(y, x), COUNT(*) FROM t{clause}"
           f"{' GROUP BY g ORDER BY g LIMIT 100' if grouped else ''}")
    q = parse_sql(sql)
    r = ctx.execute(q, segs)
    assert r.stats.scan_kernel == K_COMOMENTS and r.stats.mode == mode, (sql, r.stats.scan_kernel, r.stats.mode)
    mask = mask_of(t["f"][0])
    keys, x, y = (t["g"][0] if grouped else None), t["x"][0], t["y"][0]
    integer = columns(form, 1)[2]
    exact = exact_groups(keys, x, y, mask)

    def check_rows(rows):  # {key: [tuple of (x, y), the same, tuple of (y, x), count]}
        if not grouped and not mask.any():
            assert rows == {(): [(0.0, 0.0, 0.0, 0)] * 3 + [0]}
        assert sorted(rows) == sorted(exact), sql
        for key, (pop, samp, swapped, count) in rows.items():
            n, sx, sy, sxy = exact[key]
            print(sql, key, "got", pop, "exact", n, float(sx), float(sy), float(sxy))
            assert pop[3] == samp[3] == swapped[3] == count == n, (sql, key)
            if integer:
                assert tuple(pop) == tuple(samp) == (float(sx), float(sy), float(sxy), n), (sql, key, pop)
                assert tuple(swapped) == (pop[1], pop[0], pop[2], n), (sql, key, swapped)
                continue
            sel = mask & (keys == key[0]) if grouped else mask
            ax = sum(abs(Fraction(v)) for v in x[sel].tolist())
            ay = sum(abs(Fraction(v)) for v in y[sel].tolist())
            axy = sum(abs(Fraction(a) * Fraction(b)) for a, b in zip(x[sel].tolist(), y[sel].tolist()))
            for got in (pop, samp, (swapped[1], swapped[0], swapped[2])):
                for value, want, terms in zip(got, (sx, sy, sxy), (ax, ay, axy)):
                    assert abs(Fraction(value) - want) <= Fraction(1, 10 ** 9) * terms, (sql, key, value, float(want))

    check_rows(dict(zip(r.keys, r.aggs)))
    assert r.stats.num_docs_scanned == int(mask.sum())
    assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * (2 + grouped)
    # SQL -> ph_query_execute -> DataTable -> broker reduce -> the final doubles (a second call: a real form's sums
    # depend on the order of the atomics, an integer form's are the same bits)
    dt = decode(ctx.execute_datatable(q, segs))
    assert dt.column_names == grouped * ["g"] + ["covarpop(x,y)", "covarsamp(x,y)", "covarpop(y,x)", "count(*)"]
    nk = int(grouped)
    rows = {tuple(row[:nk]): [covariance_deserialize(c[1]) if isinstance(c, tuple) and c[0] == 32 else c
                              for c in row[nk:]] for row in dt.rows}
    check_rows(rows)
    table = reduce_datatables(q, [dt])
    if grouped or mask.any():
        want = [list(k) + [covariance_final(v[0], "COVARPOP"), covariance_final(v[1], "COVARSAMP"),
                           covariance_final(v[2], "COVARPOP"), v[3]] for k, v in sorted(rows.items())]
        assert table.rows == want, sql
    else:
        assert table.rows == [[-np.inf, -np.inf, -np.inf, 0]]


@pytest.mark.parametrize("mode", [MODE_AGG, MODE_LDS, MODE_HBM], ids=["agg", "lds", "hbm"])
@pytest.mark.parametrize("form", FORMS)
def test_two_segments(ctx, monkeypatch, form, mode):
    if mode == MODE_HBM:
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    t, segs = pinned(ctx, form, TWO_SEGMENTS, 2048)
    try:
        for where in sorted(WHERE):
            run(ctx, t, segs, form, where, mode)
    finally:
        for s in segs:
            s.unpin()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2048 + 33])
@pytest.mark.parametrize("form", ["narrow", "wide_carry", "real_mixed"])
def test_run_and_tile_edges(ctx, form, n):
    t, segs = pinned(ctx, form, n)
    try:
        for where in ("none", "range"):
            run(ctx, t, segs, form, where, MODE_AGG)
            run(ctx, t, segs, form, where, MODE_LDS)
    finally:
        segs[0].unpin()


@pytest.mark.parametrize("mode", [MODE_AGG, MODE_LDS, MODE_HBM], ids=["agg", "lds", "hbm"])
def test_stream_widths(ctx, monkeypatch, mode):
    if mode == MODE_HBM:
        monkeypatch.setenv("PH_LDS_TABLE_MAX", "0")
    t, segs = pinned(ctx, "widths", (1 << 16) + 77)
    try:
        run(ctx, t, segs, "widths", "range", mode)
    finally:
        segs[0].unpin()


REFUSALS = [("SELECT COVAR_POP(s, x) FROM t", "STRING column"),
            ("SELECT SUM(x), COVAR_POP(x, y) FROM t", "SUM beside a covariance function"),
            ("SELECT VAR_POP(x), COVAR_POP(x, y) FROM t", "variance function beside a covariance function"),
            ("SELECT COVAR_POP(x, y) FILTER(WHERE f < 3) FROM t", "FILTER clause"),
            ("SET numGroupsLimit=5; SELECT g, COVAR_POP(x, y) FROM t GROUP BY g",
             "covariance functions where a segment could reach numGroupsLimit"),
            ("SET minSegmentGroupTrimSize=1; SELECT g, COVAR_POP(x, y) FROM t GROUP BY g ORDER BY g LIMIT 5",
             "covariance functions with segment group trim"),
            ("dense", "dense partials")]


@pytest.mark.parametrize("sql,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals(ctx, sql, word):
    t, segs = pinned(ctx, "narrow", 65)
    try:
        with pytest.raises(UnsupportedError, match=word) as e:
            if sql == "dense":
                ctx.dense_layout(parse_sql("SELECT g, COVAR_POP(x, y) FROM t GROUP BY g"), segs)
            else:
                ctx.execute(parse_sql(sql), segs)
        assert e.value.code == N.PH_ERR_UNSUPPORTED
    finally:
        segs[0].unpin()
