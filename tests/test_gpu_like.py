"""GPU: the LIKE predicate (k_like_dict over the pinned STRING dictionary, then a scan leaf over the matching dictIds)
against the reference's semantics restated in tests/like_ref.py.  Every LIKE query must return the rows the oracle
returns for `s IN (<the values like_ref selects>)`, with the doc set and statistics of that IN query on a column without
an index, and a scan leaf's num_entries_scanned_in_filter whatever the index (the sorted copy, a table in another doc
order, is held to the same rows pinned without the sorted index)."""
import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.query import parse_sql
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_column_from_dict_ids, create_segment
from tests.like_ref import like_matches, like_select
from tests.test_gpu_parity import rows_equal

pytestmark = pytest.mark.gpu

# the widest is 17 bytes: one value of exactly the entry width, one a byte short, 2- / 3- / 4-byte code points beside
# `_`, line terminators inside and at the end, prefixes of one another, and what the patterns' escapes name
VALUES = ["", "a", "ab", "abc", "abcd", "aXbYc", "a%", "a%z", "a\\", "a\\b", "a\\%", "ba", "b", "cba", "xa\n", "a\nb",
          "ab\n", "a\r\n", "é", "éa", "éé", "é€", "é😀", "xé€", "a😀", "€", "😀", "0123456789abcdefg",
          "0123456789abcdef", "zz", "a_c", "%"]
SEG_VALUES = [VALUES[:23], VALUES[9:]]  # two dictionaries
PATTERNS = ["%", "", "a%", "%a", "%a%", "a%b%c", "_", "__%", "%_", "a\\%%", "%é_", "%%", "zz%q", "a\\%", "%é_%",
            "_________________", "%a\\%z"]


def _columns(values, n, seed):
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.arange(len(values)), rng.integers(0, len(values), n - len(values))])
    rng.shuffle(ids)
    return {"s": (np.array(values, dtype=object)[ids], "STRING"), "g": (rng.integers(0, 5, n).astype(np.int32), "INT"),
            "m": (rng.integers(-1000, 1000, n).astype(np.int32), "INT"), "f": (rng.integers(0, 100, n).astype(np.int32), "INT")}


@pytest.fixture(scope="module")
def tables():
    from pinot_amd.engine import GpuContext
    ctx = GpuContext(0)
    cols = [_columns(SEG_VALUES[0], 2048, 1), _columns(SEG_VALUES[1], 33, 2)]
    orders = [np.argsort(np.array([v.encode() for v in c["s"][0]], dtype=object), kind="stable") for c in cols]
    by_s = [{k: (v[o], t) for k, (v, t) in c.items()} for c, o in zip(cols, orders)]
    t ={"ctx": ctx, "oracle": [O.build_segment(f"o{i}", c) for i, c in enumerate(cols)]}
    t["plain"] = [ctx.pin(create_segment(f"p{i}", c)) for i, c in enumerate(cols)]
    t["inverted"] = [ctx.pin(create_segment(f"i{i}", c, inverted=("s",))) for i, c in enumerate(cols)]
    t["sorted"] = [ctx.pin(create_segment(f"s{i}", c)) for i, c in enumerate(by_s)]
    t["sorted_flat"] = []
    for i, c in enumerate(by_s):  # the sorted table's rows with `s` as a plain forward index
        b = create_segment(f"u{i}", c)
        assert b.columns["s"].is_sorted
        d, ids = np.unique(np.asarray(c["s"][0]).astype(str), return_inverse=True)
        b.columns["s"] = create_column_from_dict_ids("s", d, ids.reshape(-1), "STRING", allow_sorted=False)
        t["sorted_flat"].append(ctx.pin(b))
    yield t
    ctx.close()


def _in_list(pattern):
    keep = like_select(pattern, VALUES) or ["no such value"]
    return "s IN (" + ", ".join("'" + v.replace("'", "''") + "'" for v in keep) + ")"


FORMS = [("s LIKE '{p}'", "{i}"), ("s NOT LIKE '{p}'", "NOT ({i})"), ("s LIKE '{p}' AND f BETWEEN 20 AND 70", "{i} AND f BETWEEN 20 AND 70")]
SELECTS = ["SELECT COUNT(*), SUM(m) FROM t WHERE {w}", "SELECT g, COUNT(*), SUM(m) FROM t WHERE {w} GROUP BY g ORDER BY g LIMIT 10"]
STATS = ("num_docs_scanned", "num_entries_scanned_in_filter", "num_entries_scanned_post_filter", "num_total_docs")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_like_rows_and_statistics(tables, pattern):
    ctx = tables["ctx"]
    for like_form, in_form in FORMS:
        w_like, w_in = like_form.format(p=pattern), in_form.format(i=_in_list(pattern))
        for select in SELECTS:
            q, q_in = parse_sql(select.format(w=w_like)), parse_sql(select.format(w=w_in))
            e = O.execute(q_in, tables["oracle"])
            r = {k: ctx.execute(q, tables[k]) for k in ("plain", "inverted", "sorted", "sorted_flat")}
            for x in r.values():
                rows_equal(reduce_groups(q, x.keys, x.aggs).rows, reduce_groups(q_in, e.keys, e.aggs).rows)
            r_in = ctx.execute(q_in, tables["plain"])
            for s in STATS:
                assert getattr(r["plain"].stats, s) == getattr(r_in.stats, s), (w_like, s)
            assert r["inverted"].stats.num_entries_scanned_in_filter == r["plain"].stats.num_entries_scanned_in_filter
            assert r["sorted"].stats.num_entries_scanned_in_filter == r["sorted_flat"].stats.num_entries_scanned_in_filter
        for seg in tables["plain"]:  # the doc set, per segment
            words, cnt, _ = ctx.filter("SELECT COUNT(*) FROM t WHERE " + w_like, seg)
            words_in, cnt_in, _ = ctx.filter("SELECT COUNT(*) FROM t WHERE " + w_in, seg)
            assert cnt == cnt_in and np.array_equal(words, words_in), w_like


def _dictionary(card, width, seed):
    """`card` distinct values of at most `width` bytes, some of exactly `width` and of `width - 1`."""
    if width == 1:
        return [chr(c) for c in dict.fromkeys(list(b"ab\n%_c\r") + list(range(33, 127)))][:card]
    rng = np.random.default_rng(seed)
    atoms, out = ["a", "b", "c", "\n", "%", "é", "€", "😀"], {"", "a" * width, "b" * (width - 1), "a" * (width - 2) + "é"}
    while len(out) < card:
        v = ""
        for a in rng.choice(atoms, int(rng.integers(1, width + 1))):
            if len((v + a).encode()) <= width:
                v += a
        out.add(v)
    return sorted(out)


@pytest.mark.parametrize("card,width", [(1, 1), (63, 1), (64, 3), (65, 4), (257, 17), (65, 200), (257, 200)])
def test_filter_execute_bitmap_and_count(tables, card, width):
    # ballot-word and tile edges (cardinality), LDS stride, byte / dword row writes and the shrunk tile (width)
    ctx = tables["ctx"]
    values = _dictionary(card, width, card * 1000 + width)
    assert len(values) == card and max(len(v.encode()) for v in values) == width
    n = 2 * card + 61
    col = np.array(values, dtype=object)[np.arange(n) % card]
    seg = ctx.pin(create_segment("d", {"s": (col, "STRING")}))
    for pattern in ("%a_", "a%") if width > 1 else ("_", "a"):
        words, cnt, st = ctx.filter(f"SELECT COUNT(*) FROM t WHERE s LIKE '{pattern}'", seg)
        mask = np.array([like_matches(pattern, v) for v in col])
        assert cnt == int(mask.sum()) and np.array_equal(words, O.doc_words(mask)), (pattern, card, width)
        assert st.num_entries_scanned_in_filter in (n, 0)  # a scan leaf, or folded to all / none
    seg.unpin()


@pytest.mark.parametrize("where,column,message", [
    ("f LIKE '1%'", ("x", "STRING"), "non-STRING"),
    ("s LIKE '" + "a" * 200 + "'", ("x", "STRING"), "LIKE pattern"),
    ("s LIKE 'a%'", ("y" * 600, "STRING"), "wider than"),
])
def test_refusals(tables, where, column, message):
    cols = {"s": (np.array(["a", column[0]], dtype=object), column[1]), "f": (np.array([1, 2], np.int32), "INT")}
    seg = tables["ctx"].pin(create_segment("r", cols))
    with pytest.raises(N.UnsupportedError, match=message):
        tables["ctx"].execute(parse_sql("SELECT COUNT(*) FROM t WHERE " + where), [seg])
    seg.unpin()
