"""GPU: the REGEXP_LIKE predicate (a host-compiled byte-level DFA, k_regex_dict over the pinned STRING dictionary, then a
scan leaf over the matching dictIds) against java.util.regex's find() under CASE_INSENSITIVE | UNICODE_CASE as
tests/regex_ref.py restates it.  Every query must return the rows the oracle returns for `s IN (<the values regex_ref
selects>)`, with the doc set and statistics of that IN query on a column without an index, and a scan leaf's
num_entries_scanned_in_filter whatever the index, as tests/test_gpu_like.py holds LIKE to."""
import numpy as np
import pytest

from oracle import oracle as O
from pinot_amd import native as N
from pinot_amd.query import parse_sql
from pinot_amd.reduce import reduce_groups
from pinot_amd.segment import create_column_from_dict_ids, create_segment
from tests.regex_ref import regex_matches, regex_select
from tests.test_gpu_like import SELECTS, STATS, VALUES as LIKE_VALUES, _columns, _dictionary
from tests.test_gpu_parity import rows_equal

pytestmark = pytest.mark.gpu

# the LIKE test's values (the widest, 17 bytes, is the entry width) and: upper-case twins, the four code points that
# fold to an ASCII letter beside those letters, one and two final line terminators, a line terminator between letters
VALUES = LIKE_VALUES + ["AB", "Abc", "K", "\u212a", "s", "\u017f", "I", "\u0130", "\u0131", "a\n", "a\n\n", "a\nc",
                        "aaa", "ABABC", "x7"]
SEG_VALUES = [VALUES[:30], VALUES[12:]]  # two dictionaries
PATTERNS = ["AB", "k", "s", "i", "[a-z]", "[^a]", "\\w+", "\\d", "a|b", "(ab)+c", "a.c", "a.*c", "^a", "a$", "a$\\n",
            "^$", "a{2,3}", "x*", "zzq", "^.{17}$", "\\S\\s$"]


@pytest.fixture(scope="module")
def tables():
    from pinot_amd.engine import GpuContext
    ctx = GpuContext(0)
    cols = [_columns(SEG_VALUES[0], 2048, 1), _columns(SEG_VALUES[1], 64, 2)]
    orders = [np.argsort(np.array([v.encode() for v in c["s"][0]], dtype=object), kind="stable") for c in cols]
    by_s = [{k: (v[o], t) for k, (v, t) in c.items()} for c, o in zip(cols, orders)]
    t = {"ctx": ctx, "oracle": [O.build_segment(f"o{i}", c) for i, c in enumerate(cols)]}
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
    keep = regex_select(pattern, VALUES) or ["no such value"]
    return "s IN (" + ", ".join("'" + v.replace("'", "''") + "'" for v in keep) + ")"


FORMS = [("REGEXP_LIKE(s, '%s')", "%s"), ("NOT REGEXP_LIKE(s, '%s')", "NOT (%s)"),
         ("REGEXP_LIKE(s, '%s') AND f BETWEEN 20 AND 70", "%s AND f BETWEEN 20 AND 70")]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regexp_like_rows_and_statistics(tables, pattern):
    ctx = tables["ctx"]
    for regex_form, in_form in FORMS:
        w_regex, w_in = regex_form % pattern, in_form % _in_list(pattern)
        for select in SELECTS:
            q, q_in = parse_sql(select.format(w=w_regex)), parse_sql(select.format(w=w_in))
            e = O.execute(q_in, tables["oracle"])
            r = {k: ctx.execute(q, tables[k]) for k in ("plain", "inverted", "sorted", "sorted_flat")}
            for x in r.values():
                rows_equal(reduce_groups(q, x.keys, x.aggs).rows, reduce_groups(q_in, e.keys, e.aggs).rows)
            r_in = ctx.execute(q_in, tables["plain"])
            for s in STATS:
                assert getattr(r["plain"].stats, s) == getattr(r_in.stats, s), (w_regex, s)
            assert r["inverted"].stats.num_entries_scanned_in_filter == r["plain"].stats.num_entries_scanned_in_filter
            assert r["sorted"].stats.num_entries_scanned_in_filter == r["sorted_flat"].stats.num_entries_scanned_in_filter
        for seg in tables["plain"]:  # the doc set, per segment
            words, cnt, _ = ctx.filter("SELECT COUNT(*) FROM t WHERE " + w_regex, seg)
            words_in, cnt_in, _ = ctx.filter("SELECT COUNT(*) FROM t WHERE " + w_in, seg)
            assert cnt == cnt_in and np.array_equal(words, words_in), w_regex


def test_like_and_regexp_like_of_one_text_are_kept_apart(tables):
    # the column keeps the last answer: `LIKE 'ab'` (`^ab$`, case-sensitive) must not serve REGEXP_LIKE(s, 'ab')
    ctx, seg = tables["ctx"], tables["plain"][0]
    counts = [ctx.filter("SELECT COUNT(*) FROM t WHERE " + w, seg)[1]
              for w in ("s LIKE 'ab'", "REGEXP_LIKE(s, 'ab')", "s LIKE 'ab'")]
    in_counts = [ctx.filter("SELECT COUNT(*) FROM t WHERE " + w, seg)[1] for w in ("s IN ('ab', 'ab\n')", _in_list("ab"))]
    assert counts == [in_counts[0], in_counts[1], in_counts[0]] and in_counts[0] < in_counts[1]


def test_filtered_aggregation_rows_and_column_name(tables):
    from pinot_amd.datatable import decode
    ctx, sql = tables["ctx"], "SELECT COUNT(*) FILTER(WHERE %s), SUM(m) FILTER(WHERE NOT %s AND f < 50), COUNT(*) FROM t"
    regex, in_list = "REGEXP_LIKE(s, 'a.c|^K')", _in_list("a.c|^K")
    q, q_in = parse_sql(sql % (regex, regex)), parse_sql(sql % (in_list, "(" + in_list + ")"))
    assert decode(ctx.execute_datatable(q, tables["plain"][:1])).column_names[0] == \
        "count(*) FILTER(WHERE regexp_like(s,'a.c|^K'))"
    r, r_in = ctx.execute(q, tables["plain"]), ctx.execute(q_in, tables["plain"])
    rows_equal(reduce_groups(q, r.keys, r.aggs).rows, reduce_groups(q_in, r_in.keys, r_in.aggs).rows)


@pytest.mark.parametrize("card,width", [(1, 1), (63, 1), (64, 3), (65, 4), (65, 5), (257, 17), (65, 200), (257, 200)])
def test_filter_execute_bitmap_and_count(tables, card, width):
    # ballot-word and tile edges (cardinality); byte / dword rows, the last dword's padding (widths 1, 3, 5, 17), entries
    # with no zero terminator and the shrunk tile (width)
    ctx = tables["ctx"]
    values = _dictionary(card, width, card * 1000 + width)
    assert len(values) == card and max(len(v.encode()) for v in values) == width
    n = 2 * card + 61
    col = np.array(values, dtype=object)[np.arange(n) % card]
    seg = ctx.pin(create_segment("d", {"s": (col, "STRING")}))
    for pattern in ("(A|\\W).?b$", "^[^b]*c") if width > 1 else ("[a-c]", "^\\W$"):
        words, cnt, st = ctx.filter(f"SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(s, '{pattern}')", seg)
        mask = np.array([regex_matches(pattern, v) for v in col])
        assert cnt == int(mask.sum()) and np.array_equal(words, O.doc_words(mask)), (pattern, card, width)
        assert st.num_entries_scanned_in_filter in (n, 0)  # a scan leaf, or folded to all / none
    seg.unpin()


@pytest.mark.parametrize("where,column,message", [
    ("REGEXP_LIKE(f, '1')", ("x", "STRING"), "non-STRING"),
    ("REGEXP_LIKE(s, '(a)\\1')", ("x", "STRING"), "backreference"),
    ("REGEXP_LIKE(s, '\u00e9')", ("x", "STRING"), "non-ASCII"),
    ("REGEXP_LIKE(s, 'a{200}{200}')", ("x", "STRING"), "counted repetition"),
    ("REGEXP_LIKE(s, '(a{200}){200}')", ("x", "STRING"), "more than 1024 NFA nodes"),
    ("REGEXP_LIKE(s, '[ab]*a[ab]{9}')", ("x", "STRING"), "more than 255 DFA states"),
    ("REGEXP_LIKE(s, 'a')", ("y" * 600, "STRING"), "wider than"),
])
def test_refusals(tables, where, column, message):
    cols = {"s": (np.array(["a", column[0]], dtype=object), column[1]), "f": (np.array([1, 2], np.int32), "INT")}
    seg = tables["ctx"].pin(create_segment("r", cols))
    with pytest.raises(N.UnsupportedError, match=message):
        tables["ctx"].execute(parse_sql("SELECT COUNT(*) FROM t WHERE " + where), [seg])
    seg.unpin()
