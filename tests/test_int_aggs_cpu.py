"""CPU: the integer aggregation reference (tests/int_ref.py) on hand-written cases, its value sets against their own
conditions (A < 2^53 exactly where equality is claimed, the powers-of-two groups exact under sequential double sums in
both directions), the oracle's SUM / MIN / MAX against the contract on every set, and the host merges of per-segment
integer SUM / MIN / MAX at the extremes."""
import math
import os
import socket

import numpy as np
import pytest

from tests import float_ref as F
from tests import int_ref as R

MASKS = (None, lambda t: t["f"] < 5, lambda t: t["f"] >= 5)


def test_exact_sum_min_max_hand_cases():
    assert R.exact_int_sum([]) == 0 and R.exact_int_sum(np.array([1, -2, 3], np.int64)) == 2
    assert R.exact_int_sum([1 << 62] * 4) == 1 << 64  # the int64 sum is 0
    assert int(np.array([1 << 62] * 4, np.int64).sum()) == 0
    assert R.exact_int_sum([1 << 62] * 2) == 1 << 63 and float(R.exact_int_sum([1 << 62] * 2)) == 9.223372036854775808e18
    assert R.exact_int_sum([-(1 << 62)] * 3) == -3 * (1 << 62)
    assert R.exact_int_sum(np.array([R.INT64_MIN, R.INT64_MAX], np.int64)) == -1
    assert float(R.INT64_MIN) == -9.223372036854775808e18 == R.java_long_min([R.INT64_MIN, 0])
    assert R.java_long_max([R.INT64_MAX]) == 9.223372036854775808e18  # rounds up to 2^63
    assert R.java_long_max([R.TWO53 + 1]) == float(R.TWO53)  # nearest-even
    assert R.java_long_max([R.TWO53 + 3]) == float(R.TWO53 + 4)
    assert R.java_long_min([]) == math.inf and R.java_long_max([]) == -math.inf
    a = R.aggregate([1 << 62] * 4)
    assert a.S == 1 << 64 and a.A == 1 << 64 and a.n == 4 and a.fsum == 1.8446744073709552e19 and a.exact
    assert R.aggregate([R.TWO53 - 1]).exact and R.aggregate([R.TWO53 - 1, 1]).exact is False
    assert R.aggregate([1 << 40] * 8192).exact and not R.aggregate([R.TWO53 + 1]).exact
    assert not R.aggregate([R.INT64_MAX]).exact  # double(INT64_MAX) is not INT64_MAX
    assert R.aggregate([R.INT64_MIN, R.INT64_MIN]).exact


def _all_tables():
    for name in R.SETS:
        yield name, R.make_tables(name), [c for c, _ in R.VALUE_COLUMNS[name]]
    for w in R.SATURATE_WIDTHS:
        yield f"saturate_{w}", R.make_saturate(w), ["m"]
    yield "saturate_keys", R.make_saturate(23, keys=True), ["m"]


def test_value_sets_hold_what_they_claim():
    ref = R.reference(R.make_tables("int_edges"), ["vi"], group=True)
    assert ref[(0,)][1].min == ref[(0,)][1].max == float(R.INT32_MIN) and ref[(1,)][1].min == float(R.INT32_MAX)
    ref = R.reference(R.make_tables("long_edges"), ["vl"], group=True)
    assert ref[(0,)][1].S == -(ref[(0,)][0] // 2) and ref[(0,)][1].fsum == 0.0
    assert ref[(1,)][1].S == 3 * R.INT64_MAX and ref[(2,)][1].S == ref[(2,)][0] * R.INT64_MIN
    assert ref[(3,)][1].S == 7 * 2 and ref[(3,)][1].A > R.TWO53
    ref = R.reference(R.make_tables("wrap"), ["vl"], group=True, exprs=(R.WRAP_EXPR,))
    assert [ref[(k,)][1].S for k in range(4)] == [1 << 64, 1 << 63, -3 * (1 << 62), 0]
    assert all(ref[(k,)][1].exact for k in range(4))
    # what an int64 accumulator would return for them: the failures the wrap set is built to show
    assert [float(np.array([ref[(k,)][1].S % (1 << 64)], np.uint64).view(np.int64)[0]) for k in range(3)] == \
        [0.0, -9.223372036854775808e18, 4.611686018427387904e18]
    assert ref[(4,)][2].S >= 3 * 39 * 10 ** 17 > 1 << 63 and ref[(4,)][2].max == 3.9e18 < 4.0e18
    for t in R.make_tables("wrap"):  # every filter of the tests takes the huge docs or leaves them, together
        huge = (np.abs(t["vl"]) == 1 << 62) | (t["a"] > 10 ** 9)
        assert huge.sum() in (9, 5)
        assert (t["f"][huge] == 7).all() and (t["inv"][huge] == 1).all() and (t["srt"][huge] == 0).all()
    ref = R.reference(R.make_tables("flag53"), ["vl", "nl"], group=True)
    assert ref[(0,)][1].S == R.TWO53 - 1 == ref[(0,)][1].A and ref[(0,)][0] == 8192
    assert ref[(1,)][1].S == R.TWO53 and ref[(1,)][1].exact
    assert ref[(0,)][2].S == 1 - R.TWO53 and ref[(1,)][2].S == -R.TWO53
    tb = R.make_tables("two_bases")
    assert max(int(t["vl"].max()) for t in tb) - min(int(t["vl"].min()) for t in tb) == (1 << 32) - 1
    assert max(int(t["vl2"].max()) for t in tb) - min(int(t["vl2"].min()) for t in tb) == 1 << 32
    for w in R.SATURATE_WIDTHS:
        for si, t in enumerate(R.make_saturate(w)):
            off = t["m"].astype(np.int64) - int(t["m"].min())
            assert int(t["m"].min()) < 0 and off[si] == 0 and (np.delete(off, si) == (1 << w) - 1).all()
            assert (np.delete(t["g"], si) == 2).all() and t["g"][si] == 0
    for t in R.make_saturate(24, keys=True):
        off = t["m"].astype(np.int64) - int(t["m"].min())
        assert off.min() == 0 and off.max() == (1 << 24) - 1
        assert (off[(t["k1"] == 299) & (t["k2"] == 299)] == (1 << 24) - 1).all()
        assert ((t["k1"] == 299) & (t["k2"] == 299)).any()


def test_reference_stays_inside_its_own_conditions():
    # per row of every set, filter and grouping: exact is claimed only where sequential double sums in both directions
    # give float(S); elsewhere the sequential sum stays inside the bar
    checked = exact = 0
    for name, tables, cols in _all_tables():
        for mask in MASKS:
            for group in (False, True):
                for key, row in R.reference(tables, cols, mask, group).items():
                    assert row[0] == row[1].n
                for c in cols:
                    for key in R.reference(tables, [c], mask, group):
                        vals = np.concatenate([
                            t[c][(np.ones(len(t["g"]), bool) if mask is None else mask(t)) &
                                 ((t["g"] == key[0]) if group else True)] for t in tables])
                        a = R.aggregate(vals)
                        dbl = np.array([float(int(v)) for v in vals], np.float64)
                        fwd, rev = F.sequential_sum(dbl), F.sequential_sum(dbl[::-1])
                        if a.A < R.TWO53:
                            assert a.exact
                        if a.exact:
                            assert fwd == rev == float(a.S) == a.fsum, (name, c, key)
                            exact += 1
                        else:
                            assert abs(fwd - a.fsum) <= a.bound and abs(rev - a.fsum) <= a.bound, (name, c, key)
                        checked += 1
    assert checked > 300 and exact > 100


def _oracle_segments(name, tables, types):
    from oracle import oracle as O
    return [O.build_segment(f"io_{name}_{i}", {c: (t[c], types.get(c, "INT")) for c in t}) for i, t in enumerate(tables)]


@pytest.mark.parametrize("name", R.SETS)
def test_oracle_meets_the_contract(name):
    from oracle import oracle as O
    from pinot_amd.query import parse_sql
    tables = R.make_tables(name)
    types = dict(R.VALUE_COLUMNS[name], a="LONG", p="LONG")
    segs = _oracle_segments(name, tables, types)
    cols = [c for c, _ in R.VALUE_COLUMNS[name]]
    exprs = (R.WRAP_EXPR,) if name == "wrap" else ()
    aggs = ", ".join(f"SUM({c}), MIN({c}), MAX({c})" for c in cols + [f"{a} * {b}" for a, b in exprs])
    for where, mask in zip(("", " WHERE f < 5", " WHERE f >= 5"), MASKS):
        e = O.execute(parse_sql(f"SELECT COUNT(*), {aggs} FROM t{where}"), segs)
        R.check_row(e.aggs[0], R.reference(tables, cols, mask, False, exprs)[()], (name, where))
        e = O.execute(parse_sql(f"SELECT g, COUNT(*), {aggs} FROM t{where} GROUP BY g LIMIT 100"), segs)
        ref = R.reference(tables, cols, mask, True, exprs)
        assert sorted(e.keys) == sorted(ref)
        for k, row in zip(e.keys, e.aggs):
            R.check_row(row, ref[tuple(k)], (name, where, k))


def test_host_merges_do_not_wrap():
    # per-segment (per-shard) intermediate results are doubles: the merge of 3 x 2^62 and 2^62 is 2^64, not 0
    from pinot_amd import datatable as DT
    from pinot_amd.query import parse_sql
    from pinot_amd.reduce import merge_intermediate, reduce_groups
    tables = R.make_tables("wrap")
    per_seg = [R.reference([t], ["vl"], None, True) for t in tables]
    both = R.reference(tables, ["vl"], None, True)
    for merge in (merge_intermediate, DT.merge_intermediate):
        for k in both:
            a, b = per_seg[0][k][1], per_seg[1][k][1]
            # the partials as doubles and, where a segment's own sum fits int64, as integer-typed values (numpy int64
            # addition of the two wraps: 2^62 + 2^62 -> -2^63)
            forms = [(float(a.S), float(b.S)), (np.float64(a.S), np.float64(b.S)), (int(a.S), int(b.S))]
            if max(abs(a.S), abs(b.S)) < 1 << 63:
                forms.append((np.int64(a.S), np.int64(b.S)))
            for x, y in forms:
                s = merge("SUM", x, y)
                assert isinstance(s, float) and s == float(both[k][1].S), (k, type(x), s)
            assert merge("MIN", a.min, b.min) == both[k][1].min and merge("MAX", a.max, b.max) == both[k][1].max
        assert merge("SUM", np.int64(1 << 62), np.int64(1 << 62)) == 9.223372036854775808e18
        assert merge("SUM", np.int64(-(1 << 62)), np.int64(-(1 << 63))) == -1.3835058055282164e19
        assert float(merge("MIN", np.int64(R.INT64_MIN), np.int64(R.INT64_MAX))) == -9.223372036854775808e18
        assert float(merge("MAX", np.int64(R.INT64_MIN), np.int64(R.INT64_MAX))) == 9.223372036854775808e18
        assert merge("COUNT", np.int64(1 << 40), 5) == (1 << 40) + 5
        assert merge("SUM", float(3 << 62), float(1 << 62)) == 1.8446744073709552e19
        assert merge("SUM", float(1 << 62), float(1 << 62)) == 9.223372036854775808e18
        assert merge("MIN", float(R.INT64_MIN), float(R.INT64_MAX)) == -9.223372036854775808e18
        assert merge("MAX", float(R.INT64_MIN), float(R.INT64_MAX)) == 9.223372036854775808e18
    q = parse_sql("SELECT g, SUM(vl), MIN(vl), MAX(vl) FROM t GROUP BY g ORDER BY SUM(vl) DESC LIMIT 12")
    keys = sorted(both)
    rows = reduce_groups(q, keys, [[float(both[k][1].S), both[k][1].min, both[k][1].max] for k in keys]).rows
    assert rows[0] == [0, 1.8446744073709552e19, 0.0, float(1 << 62)] and rows[1][0] == 1
    assert rows[-1][0] == 2 and rows[-1][1] == -3.0 * 2.0 ** 62


# ---------------------------------------------------------------- pinot_amd.distributed.reduce_tables, two gloo ranks
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED_SUM, RED_MIN, RED_MAX = 0, 2, 3  # PH_REDUCE_SUM_I64 / MIN_I64 / MAX_I64


def _rank_tables(rank):
    """One rank's dense int64 tables over 12 keys (count, SUM, MIN, MAX of one value column) from its segment of a set,
    the way the library fills them: int64 sums, identities where a key matched no doc."""
    out = {}
    for name, col in (("int_edges", "vi"), ("long_edges", "vl")):
        ref = R.reference([R.make_tables(name)[rank]], [col], None, True)
        cnt = np.zeros(R.NUM_GROUPS, np.int64)
        sm = np.zeros(R.NUM_GROUPS, np.int64)
        mn = np.full(R.NUM_GROUPS, R.INT64_MAX, np.int64)
        mx = np.full(R.NUM_GROUPS, R.INT64_MIN, np.int64)
        for (g,), (n, a) in ref.items():
            cnt[g], mn[g], mx[g] = n, int(a.min) if name == "int_edges" else min_max_int(name, col, rank, g)[0], \
                int(a.max) if name == "int_edges" else min_max_int(name, col, rank, g)[1]
            sm[g] = a.S if name == "int_edges" else 0  # (the LONG sums never reach the tables: see the guard test)
        out[name] = [cnt, sm, mn, mx]
    return out


def min_max_int(name, col, rank, g):
    t = R.make_tables(name)[rank]
    v = [int(x) for x in t[col][t["g"] == g]]
    return min(v), max(v)


def _reduce_worker(rank, world, port):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    from pinot_amd.distributed import Layout, reduce_tables
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        layout = Layout(R.NUM_GROUPS, [1, 1, 1, 1], [RED_SUM, RED_SUM, RED_MIN, RED_MAX])
        for name, col in (("int_edges", "vi"), ("long_edges", "vl")):
            tabs = [torch.from_numpy(a.copy()) for a in _rank_tables(rank)[name]]
            shards, g0, g1 = reduce_tables(tabs, layout)
            if rank != 0:
                assert g1 == g0  # a small key space is all-reduced and owned by rank 0
                continue
            assert (g0, g1) == (0, R.NUM_GROUPS)
            cnt, sm, mn, mx = [s.numpy() for s in shards]
            ref = R.reference(R.make_tables(name), [col], None, True)
            for (g,), (n, a) in ref.items():
                lo = min(min_max_int(name, col, r, g)[0] for r in range(world))
                hi = max(min_max_int(name, col, r, g)[1] for r in range(world))
                assert int(cnt[g]) == n and int(mn[g]) == lo and int(mx[g]) == hi, (name, g)
                assert float(int(mn[g])) == a.min and float(int(mx[g])) == a.max, (name, g)
                if name == "int_edges":  # INT sums merge exactly: |v| <= 2^31 cannot wrap below 2^32 docs
                    assert int(sm[g]) == a.S, (name, g, int(sm[g]), a.S)
            if name == "long_edges":
                assert int(mn[2]) == R.INT64_MIN and int(mx[1]) == R.INT64_MAX and (int(mn[0]), int(mx[0])) == (
                    R.INT64_MIN, R.INT64_MAX)
        # why a LONG term past 2^31 must never reach reduce_tables: its all-reduce adds int64 and wraps.  The native
        # layout refuses such a term (tests/test_gpu_int_aggs.py::test_distributed_query_refuses_a_wrapping_sum), so
        # DistributedQuery.execute raises before any table is allocated
        lay1 = Layout(1, [1], [RED_SUM])
        part = torch.tensor([1 << 62], dtype=torch.int64)
        shards, g0, g1 = reduce_tables([part], lay1)
        if rank == 0:
            assert int(shards[0][0]) == -(1 << 63) != R.exact_int_sum([1 << 62, 1 << 62])
    finally:
        dist.destroy_process_group()


def test_reduce_tables_gloo_world2_at_the_extremes():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_reduce_worker, args=(2, port), nprocs=2, join=True)
