"""Plain Python / numpy reference of floating-point SUM / MIN / MAX as the reference engine computes them, and the
Java-order dictionary the segment creator writes.  It is neither the oracle nor the library: the tests of both compare
against it.

* ``java_min`` / ``java_max``: a fold of Math.min / Math.max from +Infinity / -Infinity (MinAggregationFunction.java:
  89-118, MaxAggregationFunction.java:90-119): any NaN gives NaN, -0.0 is below 0.0, no values give the start value.
* ``exact_sum``: math.fsum over the values as doubles (the correctly rounded sum); NaN when the values hold a NaN or
  both infinities, the infinity when they hold one.
* ``sum_bound``: any order of double additions of n finite terms is within (n - 1) * 2^-53 * sum|x_i| of the exact
  sum to first order; the bar is n * 2^-52 * fsum(|x_i|), a factor 2 over that.
* ``java_dictionary``: the distinct values in Double.compare order (-0.0 before 0.0, one canonical NaN last) and each
  value's dictId.
"""
import math

import numpy as np

CANONICAL_NAN = np.array([0x7FF8000000000000], np.int64).view(np.float64)[0]


def bits(x) -> int:
    """The value's float64 bit pattern; every NaN maps to the canonical one (Math.min returns the argument's NaN,
    so which NaN comes out is not specified)."""
    x = float(x)
    if x != x:
        return 0x7FF8000000000000
    return int(np.array([x], np.float64).view(np.int64)[0])


def same_double(a, b) -> bool:
    return bits(a) == bits(b)


def _math_min(a: float, b: float) -> float:
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return a if math.copysign(1.0, a) < 0 else b
    return a if a <= b else b


def _math_max(a: float, b: float) -> float:
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return a if math.copysign(1.0, a) > 0 else b
    return a if a >= b else b


def java_min(values) -> float:
    acc = math.inf
    for v in np.asarray(values, np.float64).tolist():
        acc = _math_min(acc, v)
    return acc


def java_max(values) -> float:
    acc = -math.inf
    for v in np.asarray(values, np.float64).tolist():
        acc = _math_max(acc, v)
    return acc


def exact_sum(values) -> float:
    v = np.asarray(values).astype(np.float64)  # FLOAT widens, LONG converts as (double)
    if np.isnan(v).any():
        return math.nan
    pos, neg = bool(np.isposinf(v).any()), bool(np.isneginf(v).any())
    if pos and neg:
        return math.nan
    if pos or neg:
        return math.inf if pos else -math.inf
    try:
        return math.fsum(v.tolist())
    except OverflowError:  # the exact sum is beyond the doubles: every order of additions overflows the same way
        return math.inf if math.fsum((v / 4).tolist()) > 0 else -math.inf


def sum_bound(values) -> float:
    """n * 2^-52 * fsum(|x_i|) over the finite values."""
    v = np.abs(np.asarray(values).astype(np.float64))
    try:
        return len(v) * 2.0 ** -52 * math.fsum(v.tolist())
    except OverflowError:  # sum|x_i| itself is beyond the doubles (only where the exact sum is): scaled by 2^-52 first
        return len(v) * math.fsum((v * 2.0 ** -52).tolist())


def sequential_sum(values) -> float:
    """The reference's order: one float64 accumulator over the docs in order."""
    acc = np.float64(0.0)
    with np.errstate(all="ignore"):
        for x in np.asarray(values).astype(np.float64):
            acc = acc + x
    return float(acc)


def java_order_key(values: np.ndarray) -> np.ndarray:
    """An int64 key whose order is Double.compare's: the sign-folded bit pattern, every NaN the largest."""
    v = np.asarray(values).astype(np.float64)
    b = v.view(np.int64).copy()
    b[np.isnan(v)] = 0x7FF8000000000000
    return np.where(b >= 0, b, b ^ np.int64(0x7FFFFFFFFFFFFFFF))


def java_dictionary(values, dtype=np.float64):
    """-> (dictionary in Double.compare / Float.compare order, dictIds).  -0.0 and 0.0 are two entries, all NaNs one
    canonical entry, last."""
    v = np.asarray(values, dtype=dtype)
    keys = java_order_key(v)
    uk, first, ids = np.unique(keys, return_index=True, return_inverse=True)
    dictionary = v[first].copy()
    dictionary[np.isnan(dictionary)] = np.nan  # the canonical NaN of the type
    return dictionary, ids.reshape(-1).astype(np.int32)


# --------------------------------------------------------------------------- the value sets of the aggregation tests
SEGMENT_DOCS = (4099, 64 * 3 + 1)  # both off every tile multiple
NUM_GROUPS = 12
SETS = ("zeros", "nan", "inf", "extremes", "cancel", "lossless")
DMAX4 = float(np.finfo(np.float64).max) / 4
# per set: the aggregated columns and whether their sums are exact under every order of additions
VALUE_COLUMNS = {"zeros": (("d", True), ("fl", True)), "nan": (("d", False), ("fl", False)),
                 "inf": (("d", False), ("fl", False)), "extremes": (("d", False), ("fl", False)),
                 "cancel": (("d", True), ("d2", False)), "lossless": (("d", True), ("fl", True))}


def make_tables(name: str):
    """The set's two segments: name -> numpy array per column.  d DOUBLE, fl FLOAT (cancel: d2 DOUBLE too), f INT 0..9
    (filter), g INT 0..11 (groups), inv INT 0..3 (inverted index), srt INT sorted, m INT (second operand)."""
    out = []
    for si, n in enumerate(SEGMENT_DOCS):
        rng = np.random.default_rng(1000 * (SETS.index(name) + 1) + si)
        doc = np.arange(n)
        g = (doc % NUM_GROUPS).astype(np.int32)
        f = rng.integers(0, 10, n).astype(np.int32)
        inv = rng.integers(0, 4, n).astype(np.int32)
        srt = (doc * 5 // n).astype(np.int32)
        m = rng.integers(-1000, 1000, n).astype(np.int32)
        d = np.round(rng.normal(0, 100, n), 2)
        fl = np.round(rng.normal(0, 100, n), 2).astype(np.float32)
        t = {"f": f, "g": g, "inv": inv, "srt": srt, "m": m}
        if name == "zeros":
            pool = np.array([-0.0, 0.0, 1.5, -1.5])
            d = pool[rng.integers(0, 4, n)]
            fl = pool[rng.integers(0, 4, n)].astype(np.float32)
            for col in (d, fl):
                col[g < 2] = -0.0  # only -0.0: SUM +0.0 (the accumulator starts at +0.0), MIN = MAX = -0.0
                both = np.flatnonzero(g == 2)  # both zeros in one segment -- segment 0: 0.0 first; 1: -0.0 first
                col[both] = np.where(np.arange(len(both)) % 2 == si, 0.0, -0.0)
                col[g == 3] = 0.0 if si == 0 else -0.0  # one zero per segment: the segments' merge decides
        elif name == "nan":
            hit = (rng.random(n) < 0.01) & (g >= 4)
            hit[:NUM_GROUPS * 3] |= g[:NUM_GROUPS * 3] == 5  # every segment has some
            hit |= g == 11                                   # one group is all NaN
            f[hit] = 5 + (doc[hit] % 5)                      # f < 5 excludes every NaN doc, f >= 5 includes them
            d[hit] = np.nan
            fl[hit] = np.nan
        elif name == "inf":
            some = doc % 7 == 0
            d[some & (g < 3)] = np.inf
            d[some & (g >= 3) & (g < 6)] = -np.inf
            d[some & (g == 6)] = np.where(doc[some & (g == 6)] // NUM_GROUPS % 2 == 0, np.inf, -np.inf)
            fl = d.astype(np.float32)
        elif name == "extremes":
            d = np.array([5e-324, 2.2e-308, 1.0, -1.0, -5e-324])[rng.integers(0, 5, n)]
            fl = np.array([np.finfo(np.float32).max, 1e-45, 0.1, -0.1], np.float32)[rng.integers(0, 4, n)]
            if si == 0:
                # the huge values sit in docs every filter of the tests takes or leaves together (f = 7, inv = 1,
                # srt = 0, m = 500), so that no partial selection makes the sum depend on the order of additions: group 5 holds
                # 8 x MAX/4 (overflows to +Infinity), groups 1 / 2 and 3 / 4 one +-MAX/4 each
                big = np.concatenate([5 + NUM_GROUPS * np.arange(8), [1, 2, 3, 4]])
                d[big] = [DMAX4] * 8 + [DMAX4, DMAX4, -DMAX4, -DMAX4]
                f[big], inv[big], m[big] = 7, 1, 500
        elif name == "cancel":
            k = np.arange((n - 1) // 2, dtype=np.float64)
            d = np.concatenate([2.0 ** 40 + k, -(2.0 ** 40 + k), [7.0] * (n - 2 * len(k))])
            rng.shuffle(d)
            t["d2"] = np.round(rng.normal(0, 1e6, n), 3)
            fl = rng.integers(-1000, 1000, n).astype(np.float32)
        elif name == "lossless":
            d = rng.integers(-(1 << 22) + 1, 1 << 22, n) * 0.25
            fl = (rng.integers(-(1 << 22) + 1, 1 << 22, n) * 0.25).astype(np.float32)
        t["d"], t["fl"] = np.asarray(d, np.float64), np.asarray(fl, np.float32)
        out.append(t)
    return out


def reference(tables, columns, mask=None, group=False, exprs=()):
    """-> {key tuple: [count, (sum, bound, min, max) per column / expression]} over the docs of every table that
    `mask(table)` keeps; `group`: True (by g) or the key columns.  `exprs`: (a, b) pairs evaluated per doc as double(a) + double(b)."""
    cols = {c: [] for c in list(columns) + list(exprs)}
    keys = []
    for t in tables:
        keep = np.ones(len(t["g"]), bool) if mask is None else mask(t)
        keys.append(np.stack([t[c][keep] for c in (("g",) if group in (True, False) else group)], axis=1))
        for c in columns:
            cols[c].append(t[c][keep].astype(np.float64))
        for a, b in exprs:
            cols[(a, b)].append(t[a][keep].astype(np.float64) + t[b][keep].astype(np.float64))
    keys = np.concatenate(keys)
    cols = {c: np.concatenate(v) for c, v in cols.items()}
    out = {}
    for key in (sorted(set(map(tuple, keys.tolist()))) if group else [None]):
        sel = np.ones(len(keys), bool) if key is None else (keys == np.array(key)).all(axis=1)
        row = [int(sel.sum())]  # (an aggregation without groups has its one row even over no docs)
        for c in cols:
            v = cols[c][sel]
            row.append((exact_sum(v), sum_bound(v[np.isfinite(v)]), java_min(v), java_max(v)))
        out[() if key is None else key] = row
    return out
