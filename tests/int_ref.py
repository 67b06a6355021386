"""Plain Python reference of SUM / MIN / MAX over INT and LONG columns as the reference engine computes them, with
Python integers as the high-precision arithmetic.  It is neither the oracle nor the library: the tests of both compare
against it.

* ``exact_int_sum``: the sum as a Python int, unbounded.
* ``java_long_min`` / ``java_long_max``: float(min(values)) / float(max(values)) -- (double) of a long rounds to
  nearest-even, as float(int) does; no docs give +Infinity / -Infinity (Min/MaxAggregationFunction's defaults).

SUM contract.  Let x_i be the n matched values, S their exact sum and A = sum|x_i| (Python ints), and
A_d = fsum(|double(x_i)|).  The reference engine adds double(x_i) into one double accumulator.
* A < 2^53: every partial sum of every order is an exact double.  The result must equal float(S) bit for bit and
  sum_precision_flag must be 0.
* Otherwise the answer is some order of double additions of double(x_i), and the bar is the floating-point one
  (float_ref.sum_bound): |got - fsum(double(x_i))| <= n * 2^-52 * A_d.  No other tolerance exists.
* Where every x_i is a multiple of one power of two P, every double(x_i) == x_i and A / P < 2^53, every partial sum of
  every order is again an exact double (a multiple of P below 2^53 P): the bar is equality with float(S).  The
  powers-of-two sets (wrap, flag53) hold such groups; ``Agg.exact`` says so per row.
* Whenever |got| >= 2^53 the flag must be 1.
A sum wrapped through int64 is far outside the bar (2^64 -> 0).
"""
import math
from collections import namedtuple

import numpy as np

from tests import float_ref as F

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TWO53 = 1 << 53
NUM_GROUPS = 12
SEGMENT_DOCS = (4099, 64 * 3 + 1)
SATURATE_DOCS = (8193, 4097)
FLAG53_DOCS = (16385, 193)
SATURATE_WIDTHS = (26, 27, 28, 29)
PART_KEY_CARD = 300  # saturate_keys: 300 x 300 keys
SETS = ("int_edges", "long_edges", "wrap", "flag53", "two_bases")
# per set: the aggregated columns and their types
VALUE_COLUMNS = {"int_edges": (("vi", "INT"),), "long_edges": (("vl", "LONG"),), "wrap": (("vl", "LONG"),),
                 "flag53": (("vl", "LONG"), ("nl", "LONG")), "two_bases": (("vl", "LONG"), ("vl2", "LONG")),
                 "saturate": (("m", "INT"),), "saturate_keys": (("m", "INT"),)}
WRAP_EXPR = ("a", "p")  # wrap: SUM(a * p), 3.9e18 per huge doc

# (S, A, n, min, max) as the contract names them; fsum = fsum(double(x_i)), bound = n 2^-52 A_d, exact: equality holds
Agg = namedtuple("Agg", "S A n min max fsum bound exact")


def exact_int_sum(values) -> int:
    return sum(int(v) for v in values)


def java_long_min(values) -> float:
    vals = [int(v) for v in values]
    return float(min(vals)) if vals else math.inf


def java_long_max(values) -> float:
    vals = [int(v) for v in values]
    return float(max(vals)) if vals else -math.inf


def sum_is_exact(values) -> bool:
    """Every partial sum of every order of double additions is exact: the values are doubles, multiples of one power of
    two P, and sum|x_i| / P < 2^53 (P = 1 is the plain A < 2^53 case)."""
    vals = [int(v) for v in values]
    a = sum(abs(v) for v in vals)
    if a == 0:
        return True
    if any(int(float(v)) != v for v in vals):
        return False
    low = 0
    for v in vals:
        low |= v
    p = low & -low  # the largest power of two that divides every value
    return a // p < TWO53


def aggregate(values) -> Agg:
    vals = [int(v) for v in values]
    dbl = [float(v) for v in vals]
    return Agg(sum(vals), sum(abs(v) for v in vals), len(vals), java_long_min(vals), java_long_max(vals),
               math.fsum(dbl), F.sum_bound(np.array(dbl, np.float64)), sum_is_exact(vals))


def _common(n, seed):
    rng = np.random.default_rng(seed)
    doc = np.arange(n)
    t = {"f": rng.integers(0, 10, n).astype(np.int32), "g": (doc % NUM_GROUPS).astype(np.int32),
         "inv": rng.integers(0, 4, n).astype(np.int32), "srt": (doc * 5 // n).astype(np.int32),
         "m": rng.integers(-1000, 1000, n).astype(np.int32)}
    return rng, doc, t


def make_tables(name: str):
    """The set's two segments: name -> numpy array per column.  f INT 0..9 (filter), g INT (groups: doc % 12 but in
    flag53 and the saturate sets), inv INT 0..3 (inverted index), srt INT sorted, m INT, and the set's value columns
    (VALUE_COLUMNS)."""
    out = []
    for si, n in enumerate(FLAG53_DOCS if name == "flag53" else SEGMENT_DOCS):
        rng, doc, t = _common(n, 7000 * (SETS.index(name) + 1) + si)
        g = t["g"]
        if name == "int_edges":
            v = np.array([INT32_MIN, INT32_MAX, -1, 0, 1], np.int64)[rng.integers(0, 5, n)]
            v[g == 0] = INT32_MIN
            v[g == 1] = INT32_MAX
            t["vi"] = v.astype(np.int32)
        elif name == "long_edges":
            pool = np.array([INT64_MIN, INT64_MAX, -1, 0, 1, TWO53 + 1, -(TWO53 + 1)], np.int64)
            v = pool[rng.integers(0, 7, n)]
            g0 = np.flatnonzero(g == 0)  # INT64_MIN and INT64_MAX in equal numbers (an odd doc left over holds 0)
            v[g0] = np.where(np.arange(len(g0)) % 2 == 0, INT64_MIN, INT64_MAX)
            if len(g0) % 2:
                v[g0[-1]] = 0
            v[g == 1] = 0
            if si == 0:
                v[np.flatnonzero(g == 1)[:3]] = INT64_MAX  # three INT64_MAX
            v[g == 2] = INT64_MIN
            g3 = np.flatnonzero(g == 3)  # +-(2^53 + 1) in cancelling pairs and a 7
            v[g3] = np.where(np.arange(len(g3)) % 2 == 0, TWO53 + 1, -(TWO53 + 1))
            v[g3[-1]] = 7
            if len(g3) % 2 == 0:
                v[g3[-2]] = 0
            t["vl"] = v
        elif name == "wrap":
            v = rng.integers(-1000, 1000, n).astype(np.int64)
            a = rng.integers(0, 1000, n).astype(np.int64)
            p = rng.integers(0, 10, n).astype(np.int64)
            v[g < 4] = 0
            # the huge docs, split over the segments so that only the merge passes 2^63: group 0 four 2^62 (S = 2^64),
            # group 1 two (S = 2^63), group 2 three -2^62, group 3 one of each sign (S = 0); group 4 three docs of
            # a * p = 3.9e18.  They share f = 7, inv = 1, srt = 0, m = 500: every filter of the tests takes or leaves
            # them together
            huge = {0: ([0, 12, 24], [0]), 1: ([1], [1]), 2: ([2, 14], [2]), 3: ([3], [3]), 4: ([4, 16], [4])}
            for k, docs in huge.items():
                d = np.array(docs[si])
                if k == 4:
                    a[d], p[d] = 1_950_000_000, 2_000_000_000
                else:
                    v[d] = -(1 << 62) if k == 2 or (k == 3 and si == 1) else (1 << 62)
                for c, x in (("f", 7), ("inv", 1), ("m", 500)):
                    t[c][d] = x
                assert (t["srt"][d] == 0).all()
            t["vl"], t["a"], t["p"] = v, a, p
        elif name == "flag53":
            # group 0: 8191 docs of 2^40 and one of 2^40 - 1 (S = 2^53 - 1); group 1: 8192 docs of 2^40 (S = 2^53);
            # nl = -vl is the negative mirror.  Two groups of 8192 docs fill segment 0; the rest holds small values
            v = (doc % 10 + 2).astype(np.int64)
            if si == 0:
                g[:] = np.where(doc < 8192, 0, np.where(doc < 16384, 1, 4))
                v[:16384] = 1 << 40
                v[100] = (1 << 40) - 1
            else:
                g[:] = 2 + doc % 10
            t["vl"], t["nl"] = v, -v
        elif name == "two_bases":
            lo = rng.integers(0, 11, n).astype(np.int64)
            lo[:2] = [0, 10]
            # vl: vmax - vmin = 2^32 - 1, the last range the lean group-by accepts, and offset 0xffffffff present;
            # vl2: a range of exactly 2^32
            t["vl"] = lo if si == 0 else (1 << 32) - 11 + lo
            t["vl2"] = lo if si == 0 else (1 << 32) - 10 + lo
        out.append(t)
    return out


def make_saturate(w: int, keys: bool = False):
    """m = base + off, off in [0, 2^w - 1], base negative.  One doc per segment carries offset 0 (segment 0 doc 0,
    segment 1 doc 1) in a key of their own (g = 0: both segments then hold the same key dictionary, which the lean
    group-by needs); every other doc sits at 2^w - 1 in one single key (g = 2).  keys=True
    (saturate_keys): k1, k2 in [0, 300), random offsets, offset 0 on key (0, 0) and the largest offset on the largest
    key (299, 299) in every segment."""
    base = -1_000_000
    out = []
    for si, n in enumerate(SATURATE_DOCS):
        rng, doc, t = _common(n, 9000 + 10 * w + si + (5 if keys else 0))
        top = (1 << w) - 1
        if keys:
            off = rng.integers(0, top + 1, n, dtype=np.int64)
            k1 = rng.integers(0, PART_KEY_CARD, n).astype(np.int32)
            k2 = rng.integers(0, PART_KEY_CARD, n).astype(np.int32)
            k1[:PART_KEY_CARD] = k2[:PART_KEY_CARD] = np.arange(PART_KEY_CARD)  # complete dictionaries
            off[0] = 0
            last = np.flatnonzero((k1 == PART_KEY_CARD - 1) & (k2 == PART_KEY_CARD - 1))
            off[last] = top
            off[5::7][:200] = top  # and on other keys
            t["k1"], t["k2"] = k1, k2
        else:
            off = np.full(n, top, np.int64)
            off[si] = 0
            t["g"] = np.full(n, 2, np.int32)
            t["g"][si] = 0
            t["k"] = t["g"].copy()  # the same keys under a name no test gives a table dictionary
        t["m"] = (base + off).astype(np.int32)
        del t["inv"], t["srt"]
        out.append(t)
    return out


def reference(tables, columns, mask=None, group=False, exprs=()):
    """-> {key tuple: [count, Agg per column / expression]} over the docs of every table that `mask(table)` keeps;
    `group`: True (by g) or the key columns.  `exprs`: (a, b) pairs evaluated per doc as the exact product a * b (each
    product of the sets is an exact double, so double(a) * double(b) is the same number)."""
    names = list(columns) + list(exprs)
    gcols = ("g",) if group in (True, False) else tuple(group)
    rows = {}
    for t in tables:
        keep = np.flatnonzero(np.ones(len(t["g"]), bool) if mask is None else mask(t))
        keys = list(zip(*[t[c][keep].tolist() for c in gcols])) if group else [()] * len(keep)
        vals = []
        for c in names:
            if isinstance(c, tuple):
                vals.append([x * y for x, y in zip(t[c[0]][keep].tolist(), t[c[1]][keep].tolist())])
            else:
                vals.append(t[c][keep].tolist())
        for i, k in enumerate(keys):
            row = rows.setdefault(k, [[] for _ in names])
            for j in range(len(names)):
                row[j].append(vals[j][i])
    if not group:
        rows.setdefault((), [[] for _ in names])  # an aggregation without groups has its one row even over no docs
    return {k: [len(v[0]) if names else 0] + [aggregate(x) for x in v] for k, v in sorted(rows.items())}


def check_row(got, want, what):
    """got: [count, sum, min, max, ...] of one result row; want: [count, Agg, ...] -- the SUM contract above, MIN / MAX
    as (double) of the exact extreme, COUNT exact.  Prints each figure before it asserts."""
    assert got[0] == want[0], (what, "COUNT", got[0], want[0])
    for i, a in enumerate(want[1:]):
        gsum, gmin, gmax = got[1 + 3 * i: 4 + 3 * i]
        print(what, i, "sum", gsum, "S", a.S, "fsum", a.fsum, "bound", a.bound, "exact", a.exact, "min", gmin, a.min,
              "max", gmax, a.max)
        if a.exact:
            assert gsum == float(a.S), (what, i, "SUM", gsum, a.S)
        else:
            assert abs(gsum - a.fsum) <= a.bound, (what, i, "SUM", gsum, a.fsum, a.bound)
        assert gmin == a.min and gmax == a.max, (what, i, "MIN/MAX", gmin, a.min, gmax, a.max)


def check_flag(flag, rows, ref, what):
    """sum_precision_flag of one call: 0 when every row's A < 2^53, 1 whenever a returned |SUM| >= 2^53."""
    if all(a.A < TWO53 for want in ref.values() for a in want[1:]):
        assert not flag, (what, "flag set although every sum|x_i| < 2^53")
    if any(abs(got[1 + 3 * i]) >= float(TWO53) for got in rows.values() for i in range((len(got) - 1) // 3)):
        assert flag, (what, "flag clear although a SUM reached 2^53")
