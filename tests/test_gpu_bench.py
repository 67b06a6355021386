"""GPU: bench.py as a command at a small size -- a plain run times --steps steps and does nothing after them but
print its line and, with --dump-outputs, write the last step's result columns (checked against the oracle here);
--full adds the CPU baseline and the parity check.

bench.py runs in a child process (the test process itself has initialised the GPU and must not exec)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import oracle as O
from pinot_amd.query import parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZE = ["--rows", "300000", "--segment-rows", "100000"]  # 3 segments of the headline workload


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *SIZE, *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    line = _bench("--dump-outputs", str(out))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["value"] == pytest.approx(300000 / (line["ms_per_step"] / 1000.0))
    assert "cpu_baseline" not in line and "parity_sample" not in line
    query, cols, _ = bench.WORKLOADS["config3"]
    q = parse_sql(query)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["agg0", "agg1", "agg2", "agg3", "key0", "key1"]
    assert all(a.dtype == np.float64 and a.shape == (line["groups"],) for a in got.values())
    # the same seeded table through the oracle: keys, SUM, COUNT, MIN, MAX bit-exact
    bufs = [bench.make_segment_buffers(i, 100000, seed=1000, cols=cols) for i in range(3)]
    keys, aggs = O.execute_timed(q, bench.oracle_segments(bufs), 1)[1:]
    order = np.argsort(keys)
    k_gpu = got["key0"].astype(np.uint64) + got["key1"].astype(np.uint64) * np.uint64(cols["g1"][0])
    og = np.argsort(k_gpu)
    assert np.array_equal(k_gpu[og], keys[order])
    assert np.array_equal(np.stack([got[f"agg{k}"] for k in range(4)], axis=1)[og], aggs[order])


def test_full_run_adds_cpu_baseline_and_parity():
    line = _bench("--full", "--cpu-seconds", "0.2")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "rows/s"
    assert line["parity_sample"]["bit_exact"] is True and line["parity_sample"]["segments"] >= 1
