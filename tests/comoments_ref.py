"""The exact reference of COVAR_POP / COVAR_SAMP: count, sum(x), sum(y) and sum(x y) of a set of docs in
``fractions.Fraction`` over the values as the stored type holds them, with no rounding."""
from fractions import Fraction

import numpy as np


def exact_tuple(x, y):
    xs = [Fraction(v) for v in np.asarray(x).tolist()]  # (an int, a float32 or a float64 converts exactly)
    ys = [Fraction(v) for v in np.asarray(y).tolist()]
    return len(xs), sum(xs, Fraction(0)), sum(ys, Fraction(0)), sum((a * b for a, b in zip(xs, ys)), Fraction(0))


def exact_groups(keys, x, y, mask):
    """{key: (n, sum x, sum y, sum x y) of the masked docs of that key}; ``keys`` None: the one group ()."""
    if keys is None:
        return {(): exact_tuple(x[mask], y[mask])}
    return {(int(k),): exact_tuple(x[mask & (keys == k)], y[mask & (keys == k)]) for k in np.unique(keys[mask])}
