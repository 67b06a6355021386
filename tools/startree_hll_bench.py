"""device_ms of `SELECT d1, DISTINCTCOUNTHLL(c) FROM t GROUP BY d1` served from star-tree sketch columns, beside the
same query with skipStarTree (the raw path: the per-dictId table lookup over every document) on the same build.

Two data sets: the 3-segment 6000 / 2500 / 3001 test data (third segment without a tree), and one large segment
(--docs, default 2M; d3 with --d3 distinct values so the tree holds tens of thousands of records).  The two plans
alternate inside one timed loop after a warm-up; the figures are medians of the calls' device_ms (device events
around the scan and the sketch merge) and of the host wall time around the synchronous call.  One JSON line each.

    python tools/startree_hll_bench.py [--docs 2000000] [--d3 1000] [--steps 40] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle as O  # noqa: E402
from pinot_amd.engine import GpuContext  # noqa: E402
from pinot_amd.query import parse_sql  # noqa: E402
from pinot_amd.segment import create_segment  # noqa: E402
from pinot_amd.startree import attach, build_star_tree  # noqa: E402

LOG2M = 8
SQL = "SELECT d1, DISTINCTCOUNTHLL(c) FROM t GROUP BY d1"


def table(rng, n, d3):
    return {
        "d1": (rng.integers(0, 6, n).astype(np.int32) * 10, "INT"),
        "d2": (rng.choice(np.array(["ca", "ny", "tx", "wa", "or", "fl", "il", "ga"]), n), "STRING"),
        "d3": (rng.integers(0, d3, n).astype(np.int64) * 1000 + 7, "LONG"),
        "c": (rng.integers(0, 300, n).astype(np.int32) * 7 - 400, "INT"),
    }


def build(name, cols, max_leaf):
    seg = create_segment(name, cols)
    oseg = O.build_segment(name, cols)
    e = O.execute(parse_sql(f"SELECT c, DISTINCTCOUNTHLL(c, {LOG2M}) FROM t GROUP BY c LIMIT 100000"), [oseg])
    uniq, inv = np.unique(cols["c"][0], return_inverse=True)
    by_key = {k[0]: np.asarray(a[0], np.uint8) for k, a in zip(e.keys, e.aggs)}
    regs = np.stack([by_key[int(v)] for v in uniq])[inv]
    st = build_star_tree(seg, ["d1", "d2", "d3"], [("count", "*"), ("distinctCountHLL", "c")], max_leaf, (),
                         values={"c": regs})
    return seg, st, oseg


def measure(ctx, label, gpu, ora, steps, warmup, docs, records):
    q_star, q_raw = parse_sql(SQL), parse_sql("SET skipStarTree=true; " + SQL)
    e = O.execute(q_star, ora)
    exp = {k: np.asarray(a[0]) for k, a in zip(e.keys, e.aggs)}
    out = {}
    for name, q in (("star", q_star), ("raw", q_raw)):
        r = ctx.execute(q, gpu)
        assert len(r.keys) == len(exp) and all(np.array_equal(exp[k], a[0]) for k, a in zip(r.keys, r.aggs)), name
        out[name] = {"device_ms": [], "wall_ms": [], "star_segments": int(r.stats.num_segments_star_tree)}
    for i in range(warmup + steps):
        for name, q in (("star", q_star), ("raw", q_raw)):
            t0 = time.perf_counter()
            r = ctx.execute(q, gpu)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                out[name]["device_ms"].append(r.stats.device_ms)
                out[name]["wall_ms"].append(wall)
    res = {"data": label, "docs": docs, "star_records": records, "steps": steps, "sql": SQL}
    for name in ("star", "raw"):
        d = np.array(out[name]["device_ms"])
        res[name] = {"device_ms_median": round(float(np.median(d)), 4), "device_ms_min": round(float(d.min()), 4),
                     "device_ms_p90": round(float(np.percentile(d, 90)), 4),
                     "wall_ms_median": round(float(np.median(out[name]["wall_ms"])), 4),
                     "star_segments": out[name]["star_segments"]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=2_000_000)
    ap.add_argument("--d3", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(17)
    small = [build(f"s{i}", table(rng, n, 40), 25) for i, n in enumerate((6000, 2500, 3001))]
    big = build("big", table(rng, a.docs, a.d3), 1000) if a.docs > 0 else None
    ctx = GpuContext(0)
    try:
        gpu = []
        for i, (seg, st, _) in enumerate(small):
            p = ctx.pin(seg)
            if i < 2:
                attach(p, st)
            gpu.append(p)
        measure(ctx, "3 segments 6000/2500/3001", gpu, [o for _, _, o in small], a.steps, a.warmup, 11501,
                small[0][1].num_docs + small[1][1].num_docs)
        if big:
            p = ctx.pin(big[0])
            attach(p, big[1])
            measure(ctx, "1 segment", [p], [big[2]], a.steps, a.warmup, a.docs, big[1].num_docs)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
