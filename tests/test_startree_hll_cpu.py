"""CPU: the star-tree distinctCountHLL pair column (DistinctCountHLLValueAggregator: BYTES, one serialized HyperLogLog
per star-tree record, a var-byte chunk forward index).  The builder (pinot_amd.startree) merges the raw documents'
registers by elementwise max and writes the pair with hll_serialize + write_var_byte_raw_forward_index; the library's
host parse (ph_star_tree_hll_pair_check, the validation ph_segment_add_star_tree runs at pin) reads it back, and every
malformed buffer is PH_ERR_INVALID_ARGUMENT.  The same parser runs under AddressSanitizer + UBSan in a stand-alone
program (tests/sanitize/asan_hll_pair.cpp) over its own corpus and over the buffers mutated here."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from pinot_amd import native as N
from pinot_amd.datatable import hll_deserialize
from pinot_amd.reduce import hll_serialize
from pinot_amd.segment import create_segment, write_var_byte_raw_forward_index
from pinot_amd.startree import FUNCTIONS, build_star_tree
from tests.test_startree_cpu import PAIRS, star_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(buf, num_docs):
    b = np.ascontiguousarray(buf, np.uint8)
    lm = ctypes.c_int32(-1)
    code = N.lib().ph_star_tree_hll_pair_check(b.ctypes.data, b.nbytes, num_docs, ctypes.byref(lm))
    return code, lm.value


def _values(buf, num_docs, docs_per_chunk=1000):
    """The writer's own reader: the values of a version-2 PASS_THROUGH var-byte index."""
    raw = bytes(np.asarray(buf, np.uint8))
    head = np.frombuffer(raw[:28], ">i4")
    assert (head[0], head[2], head[4], head[5], head[6]) == (2, docs_per_chunk, num_docs, 0, 28)
    offs = list(np.frombuffer(raw[28:28 + 4 * head[1]], ">i4")) + [len(raw)]
    out = []
    for c in range(head[1]):
        chunk = raw[offs[c]:offs[c + 1]]
        starts = np.frombuffer(chunk[:4 * docs_per_chunk], ">i4")
        for r in range(min(docs_per_chunk, num_docs - c * docs_per_chunk)):
            end = len(chunk) if r + 1 == docs_per_chunk or starts[r + 1] == 0 else starts[r + 1]
            out.append(chunk[starts[r]:end])
    return out


def _doc_registers(rng, n, log2m, distinct=37):
    """Single-value sketches: one register set per raw document (a document's value sets one register)."""
    m = 1 << log2m
    per_value = np.zeros((distinct, m), np.uint8)
    per_value[np.arange(distinct), rng.integers(0, m, distinct)] = rng.integers(1, 20, distinct)
    return per_value[rng.integers(0, distinct, n)]


def _star(log2m, n=2600, seed=3):
    rng = np.random.default_rng(seed + log2m)
    cols = star_table(rng, n)
    regs = _doc_registers(rng, n, log2m)
    seg = create_segment("h", cols)
    vals = {c: v for c, (v, _) in cols.items()}
    vals["c"] = regs
    st = build_star_tree(seg, ["d1", "d2", "d3"], PAIRS + [("distinctCountHLL", "c")], 10, (), values=vals)
    return cols, regs, seg, st


@pytest.mark.parametrize("log2m", [4, 8, 12])
def test_builder_pair_round_trip(log2m):
    assert "distinctCountHLL" in FUNCTIONS
    cols, regs, seg, st = _star(log2m)
    name = "distinctCountHLL__c"
    assert name in st.pairs and st.num_docs > 1000  # more than one chunk, the last one partial
    buf = st.metric_fwd[name]
    assert _check(buf, st.num_docs) == (N.PH_OK, log2m)
    vals = _values(buf, st.num_docs)
    assert len(vals) == st.num_docs and {len(v) for v in vals} == {8 + 4 * ((1 << log2m) // 6 + 1)}
    got = np.array([hll_deserialize(v)[1] for v in vals])
    assert all(hll_deserialize(v)[0] == log2m for v in vals[:5])
    assert np.array_equal(got, st.metrics[name])
    # the records are the elementwise max of their raw documents' registers: the root's aggregated document holds all
    tree = np.frombuffer(st.tree.tobytes()[-28 * _num_nodes(st):], "<i4").reshape(-1, 7)
    assert np.array_equal(st.metrics[name][tree[0, 4]], regs.max(axis=0))
    # and of the documents of their own dimension tuple (the first records are the sorted, merged raw documents)
    ids = {d: np.searchsorted(np.unique(cols[d][0]), cols[d][0]) for d in ("d1", "d2", "d3")}
    key = tuple(st.dim_ids[0])
    mask = (ids["d1"] == key[0]) & (ids["d2"] == key[1]) & (ids["d3"] == key[2])
    assert mask.any() and np.array_equal(st.metrics[name][0], regs[mask].max(axis=0))


def _num_nodes(st):
    nn = ctypes.c_int32()
    N.check(N.lib().ph_star_tree_check(st.tree.ctypes.data, st.tree.nbytes, ctypes.byref(nn), None))
    return nn.value


def test_existing_pairs_unchanged_beside_the_hll_pair():
    # the four existing functions' columns are byte-identical with and without the new pair
    cols, regs, seg, st = _star(8)
    plain = build_star_tree(seg, ["d1", "d2", "d3"], PAIRS, 10, (), values={c: v for c, (v, _) in cols.items()})
    assert plain.num_docs == st.num_docs and np.array_equal(plain.tree, st.tree)
    for p in plain.pairs:
        assert np.array_equal(plain.metric_fwd[p], st.metric_fwd[p]), p
    for d in plain.dimensions:
        assert np.array_equal(plain.dim_fwd[d], st.dim_fwd[d]), d


def _records(n, log2m, rng):
    return [hll_serialize(rng.integers(0, 25, 1 << log2m).astype(np.uint8), log2m) for _ in range(n)]


def _malformed(rng):
    """(name, buffer, num_docs) of every malformed case; 25 records of log2m 8 in chunks of 10 (the last partial)."""
    n, per = 25, 10
    recs = _records(n, 8, rng)
    good = write_var_byte_raw_forward_index(recs, per)
    assert _check(good, n) == (N.PH_OK, 8)
    first_chunk = 28 + 4 * 3
    out = []
    for cut in (0, 11, 27, 30, first_chunk + 6, first_chunk + 4 * per + 3, len(good) - 180 * 7, len(good) - 1):
        out.append((f"cut{cut}", good[:cut], n))  # header, chunk offsets, value offsets, mid-value, the last byte
    short = list(recs)
    short[7] = short[7][:-4]
    out.append(("short_word", write_var_byte_raw_forward_index(short, per), n))
    mixed = list(recs)
    mixed[n - 1] = _records(1, 7, rng)[0]
    out.append(("mixed_log2m", write_var_byte_raw_forward_index(mixed, per), n))
    past = good.copy()
    past[28 + 4:28 + 8] = np.frombuffer(np.array([len(good) + 100], ">i4").tobytes(), np.uint8)
    out.append(("chunk_offset_past_buffer", past, n))
    inner = good.copy()
    inner[first_chunk + 4:first_chunk + 8] = np.frombuffer(np.array([1 << 30], ">i4").tobytes(), np.uint8)
    out.append(("value_offset_past_chunk", inner, n))
    out.append(("more_docs_than_file", good, n + 1))
    size_field = list(recs)
    size_field[0] = size_field[0][:4] + np.array([4], ">i4").tobytes() + size_field[0][8:]
    out.append(("size_field", write_var_byte_raw_forward_index(size_field, per), n))
    big = list(recs)
    big[0] = np.array([17, 4 * 43], ">i4").tobytes() + big[0][8:]
    out.append(("log2m_17", write_var_byte_raw_forward_index(big, per), n))
    return good, out


def test_malformed_pair_columns_are_invalid_argument():
    good, cases = _malformed(np.random.default_rng(8))
    for name, buf, n in cases:
        code, _ = _check(buf, n)
        assert code == N.PH_ERR_INVALID_ARGUMENT, (name, code)
    assert N.lib().ph_star_tree_hll_pair_check(None, 0, 1, None) == N.PH_ERR_INVALID_ARGUMENT
    # the message names the pair (at pin: its column name)
    _check(cases[0][1], cases[0][2])
    assert b"distinctCountHLL" in N.lib().ph_last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_pair_parser_under_asan_ubsan(tmp_path):
    exe = os.path.join(ROOT, "build", "sanitize", "asan_hll_pair")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "pinot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-I" + src, "-o", exe,
                    os.path.join(ROOT, "tests", "sanitize", "asan_hll_pair.cpp"), os.path.join(src, "rawfwd.cpp"),
                    "-ldl", "-lpthread"], check=True, timeout=600)
    good, cases = _malformed(np.random.default_rng(8))
    args = []
    for name, buf, n in [("good", good, 25)] + cases:
        p = str(tmp_path / f"{name}.bin")
        np.asarray(buf, np.uint8).tofile(p)
        args += [p, str(n)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "no sanitizer report" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    codes = dict(line.rsplit(" ", 1) for line in r.stdout.splitlines() if ".bin " in line)
    assert codes[str(tmp_path / "good.bin")] == "0"
    for name, _, _ in cases:
        assert codes[str(tmp_path / f"{name}.bin")] == str(N.PH_ERR_INVALID_ARGUMENT), name
