"""bench.py --dump-outputs: the writer of the result columns (dump_outputs) on hand-made results, without a GPU."""
import os
import types

import numpy as np

import bench


def _result(n, seed):
    rng = np.random.default_rng(seed)
    return types.SimpleNamespace(
        key_columns=[rng.integers(0, 1 << 31, n).astype(np.int32), [("k%d" % (i % 7)) * (i % 3) for i in range(n)]],
        agg_columns=[rng.integers(0, 1 << 52, n).astype(np.int64), rng.normal(0, 1e9, n),
                     rng.integers(0, 64, (n, 16)).astype(np.uint8)])


def test_dump_is_lossless_float_and_repeatable(tmp_path):
    r = _result(1001, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("", r), ("q01_", _result(1, 4))])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"{p}{c}.npy" for p in ("", "q01_") for c in ("key0", "key1", "agg0", "agg1", "agg2"))
    got = {f: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert got[f].dtype in (np.float32, np.float64)
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))
    assert np.array_equal(got["key0.npy"].astype(np.int32), r.key_columns[0])
    assert np.array_equal(got["agg0.npy"].astype(np.int64), r.agg_columns[0])
    assert np.array_equal(got["agg1.npy"], r.agg_columns[1])
    assert np.array_equal(got["agg2.npy"].astype(np.uint8), r.agg_columns[2])
    text = [bytes(row.astype(np.uint8)).rstrip(b"\0").decode() for row in got["key1.npy"]]
    assert text == r.key_columns[1]


def test_dump_samples_large_outputs_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    r = _result(5000, 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("", r)])
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(a.nbytes for a in got.values()) <= 20_000
    rows = {len(a) for a in got.values()}
    assert len(rows) == 1 and 0 < rows.pop() < 5000
    for f, a in got.items():  # the same seeded sample every time, the same rows in every column
        assert np.array_equal(a, np.load(tmp_path / "b" / f))
    keep = np.flatnonzero(np.isin(r.key_columns[0], got["key0.npy"].astype(np.int32)))
    assert np.array_equal(got["agg1.npy"], r.agg_columns[1][keep])
