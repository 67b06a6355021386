"""The exact reference of SKEWNESS / KURTOSIS: the PinotFourthMoment (n, mean, m2, m3, m4) of a set of values in
``fractions.Fraction`` -- m_k = sum((x - mean)^k), with no rounding."""
from fractions import Fraction

import numpy as np


def exact_tuple(values):
    xs = [Fraction(v) for v in np.asarray(values).tolist()]  # (a float32 / float64 converts exactly)
    n = len(xs)
    if n == 0:
        return 0, None, None, None, None
    mean = sum(xs) / n
    return (n, mean) + tuple(sum((x - mean) ** k for x in xs) for k in (2, 3, 4))


def exact_groups(keys, values, mask):
    """{key: exact_tuple of the masked values of that key}; ``keys`` None: the one group ()."""
    if keys is None:
        return {(): exact_tuple(values[mask])}
    return {(int(k),): exact_tuple(values[mask & (keys == k)]) for k in np.unique(keys[mask])}
