"""Plain numpy float64 restatement of HistogramAggregationFunction.getBinId (HistogramAggregationFunction.java:117-141):
the reference of the HISTOGRAM tests.  -1 is a value outside every bin, OUT_OF_BOUNDS one Java would index its list
out of bounds with (the GPU path refuses those).  Also the known answers of HistogramQueriesTest and their columns."""
import json
import os

import numpy as np

OUT_OF_BOUNDS = -2
DTYPES = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "histogram_kat.json")))


def kat_column(name):
    col = KAT["columns"][name]
    return (np.arange(KAT["num_docs"]) * col["scale"] + col["offset"]).astype(DTYPES[col["type"]])


def bin_ids(values, edges, equal_bins=0):
    """values: the stored values (any numeric dtype; converted to double first, as getDoubleValuesSV does)."""
    val = np.asarray(values).astype(np.float64)
    edges = np.asarray(edges, np.float64)
    lower, upper = edges[0], edges[-1]
    nbins = equal_bins or len(edges) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        if equal_bins:
            f = np.floor((val - lower) / ((upper - lower) / equal_bins))
            ids = np.where(np.isnan(f), 0.0, np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)  # Java's (int)
        else:  # the binary search returns the last edge that is not above val (every edge for a NaN: the last one)
            ids = np.where(np.isnan(val), len(edges) - 1, np.searchsorted(edges, val, side="right") - 1)
        ids = np.where((ids < 0) | (ids >= nbins), OUT_OF_BOUNDS, ids)
        ids = np.where(val == upper, nbins - 1, ids)
        return np.where((val > upper) | (val < lower), -1, ids)


def counts(values, edges, equal_bins=0):
    """The B bin counts of `values` as the reference's DoubleArrayList holds them."""
    ids = bin_ids(values, edges, equal_bins)
    assert not (ids == OUT_OF_BOUNDS).any()
    return np.bincount(ids[ids >= 0], minlength=equal_bins or len(edges) - 1).astype(np.float64)
