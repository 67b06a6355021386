"""The reference's LIKE as plain Python: RegexpPatternConverterUtils.likeToRegexpLike (:43-131) restated, and the regex it
emits evaluated with Matcher.find()'s semantics (no flags) through ``re.search``.  Python's ``.`` and ``$`` know ``\\n``
only, so the two are spelled out as java.util.regex defines them: ``.`` is any code point but the line terminators
\\n, \\r, U+0085, U+2028, U+2029; ``$`` is the end of input or the place before one final line terminator (\\r\\n is one,
and there is no match between its two characters)."""
import re

META = "^$.{}[]()*+?|<>-&/"  # REGEXP_METACHARACTERS
_DOT = "[^\n\r\u0085\u2028\u2029]"
_DOLLAR = "(?:(?=\r\n\\Z)|(?=[\r\u0085\u2028\u2029]\\Z)|(?<!\r)(?=\n\\Z)|\\Z)"


def like_to_regexp(like: str) -> str:
    start, end, prefix, suffix = 0, len(like), "^", "$"
    if len(like) == 0:
        return "^$"
    if len(like) == 1:
        if like == "%":
            return ""
    else:
        if like[0] == "%":
            start = next((i for i, c in enumerate(like) if c != "%"), -1)
            if start == -1:
                return ""
            prefix = ""
        if like[-1] == "%":
            end = max(i for i, c in enumerate(like) if c != "%") + 1
            suffix = ""
    out, prev_backslash = prefix, False
    for c in like[start:end]:
        if c == "_":
            out += c if prev_backslash else "."
        elif c == "%":
            out += c if prev_backslash else ".*"
        else:
            if c in META or prev_backslash:
                out += "\\"
            out += c
        prev_backslash = c == "\\"
    if prev_backslash:
        out += "\\"
    return out + suffix


def _python_form(java_regex: str) -> str:
    out, i, n = "", 0, len(java_regex)
    while i < n:
        c = java_regex[i]
        if c == "\\":
            out += re.escape(java_regex[i + 1])
            i += 2
            continue
        if c == "^" and i == 0:
            out += "\\A"
        elif c == "$" and i == n - 1:
            out += _DOLLAR
        elif c == ".":
            out += _DOT
        else:
            out += c  # `*` after a dot
        i += 1
    return out


def like_matches(like: str, value: str) -> bool:
    return re.search(_python_form(like_to_regexp(like)), value) is not None


def like_select(like: str, values) -> list:
    return sorted({v for v in values if like_matches(like, v)})  # the distinct values `col LIKE like` keeps
