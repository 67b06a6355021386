"""The exact reference of the variance family: the VarianceTuple (count, sum, m2) of a set of values in
``fractions.Fraction`` -- count, sum(x) and m2 = sum(x^2) - sum(x)^2 / n = sum((x - mean)^2), with no rounding."""
from fractions import Fraction

import numpy as np


def exact_tuple(values):
    xs = [Fraction(v) for v in np.asarray(values).tolist()]  # (a float32 / float64 converts exactly)
    n = len(xs)
    if n == 0:
        return 0, Fraction(0), Fraction(0)
    s = sum(xs)
    return n, s, sum(x * x for x in xs) - s * s / n


def exact_groups(keys, values, mask):
    """{key: exact_tuple of the masked values of that key}; ``keys`` None: the one group ()."""
    if keys is None:
        return {(): exact_tuple(values[mask])}
    return {(int(k),): exact_tuple(values[mask & (keys == k)]) for k in np.unique(keys[mask])}
