"""CPU: the LIKE predicate's parser forms, and the reference restatement the GPU tests compare against
(tests/like_ref.py) on cases that can be read off RegexpPatternConverterUtils.likeToRegexpLike and java.util.regex."""
import pytest

from pinot_amd.query import LikePredicate, SqlParseError, like_to_regexp_like, parse_sql
from tests.like_ref import like_matches, like_to_regexp


def test_like_parses_to_the_new_predicate():
    f = parse_sql("SELECT COUNT(*) FROM t WHERE s LIKE 'UNITED KI%'").filter
    assert f.type == "PREDICATE" and f.predicate == LikePredicate("s", "UNITED KI%")
    assert f.predicate.TYPE == "LIKE" and f.to_string() == "regexp_like(s,'^UNITED KI')"
    n = parse_sql("SELECT COUNT(*) FROM t WHERE s NOT LIKE 'it''s_' AND f > 3").filter
    assert n.type == "AND" and n.children[0].type == "NOT"
    assert n.children[0].children[0].predicate == LikePredicate("s", "it's_")


@pytest.mark.parametrize("where", ["s LIKE 5", "s LIKE other", "s LIKE", "s NOT 'a%'"])
def test_like_needs_a_string_literal(where):
    with pytest.raises(SqlParseError):
        parse_sql("SELECT COUNT(*) FROM t WHERE " + where)


CONVERSIONS = [("", "^$"), ("%", ""), ("%%", ""), ("a%", "^a"), ("%a", "a$"), ("%a%", "a"), ("a_c", "^a.c$"),
               ("a\\%b", "^a\\%b$"), ("a.b", "^a\\.b$"), ("a\\", "^a\\\\$"), ("a\\b", "^a\\\\b$"),
               ("a%b%c", "^a.*b.*c$"), ("a\\%%", "^a\\\\")]


@pytest.mark.parametrize("like,regex", CONVERSIONS)
def test_conversion_cases(like, regex):
    assert like_to_regexp(like) == regex
    assert like_to_regexp_like(like) == regex  # the package's own restatement (LikePredicate.to_string)


MATCHES = [("", "", True), ("", "\n", True), ("", "a", False), ("%", "x\ny", True), ("a%", "ab", True),
           ("a%", "ba", False), ("%a", "ba", True), ("%a", "a\n", True), ("%a", "a\r\n", True), ("%a", "a\n\n", False),
           ("a_c", "abc", True), ("a_c", "aéc", True), ("a_c", "a\U0001f600c", True), ("a_c", "a\nc", False),
           ("a_c", "abbc", False), ("a%c", "a\nc", False), ("%b%c", "a\nbxc", True), ("a\\%b", "a%b", True),
           ("a\\%b", "axb", False), ("a.b", "a.b", True), ("a.b", "axb", False), ("a\\", "a\\", True),
           ("_", "\u2028", False), ("_", "€", True), ("__%", "a", False), ("%_", "a\n", True)]


@pytest.mark.parametrize("like,value,verdict", MATCHES)
def test_match_cases(like, value, verdict):
    assert like_matches(like, value) is verdict
