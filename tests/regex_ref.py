"""The reference's REGEXP_LIKE as plain Python: a java.util.regex pattern from the subset the GPU path accepts, evaluated
with Matcher.find()'s semantics under CASE_INSENSITIVE | UNICODE_CASE (RegexpLikePredicate.java:49) through
``re.search(..., re.IGNORECASE)``.  As in tests/like_ref.py, ``.``, ``$`` and ``^`` are spelled out as java.util.regex
defines them.  Python's IGNORECASE over ``str`` adds to ASCII letters and lower-case ranges exactly the four code points
Java adds (U+0130, U+0131, U+017F, U+212A); the predefined classes are ASCII-defined and do not fold in Java, so they
are spelled out with the flag switched off.  Not faithful, and not used: a range of upper-case letters only (Java keeps
U+0130 and U+212A out of ``[A-Z]``, Python lets them in) and ``\\w`` / a negated predefined class inside brackets."""
import re

from tests.like_ref import _DOLLAR, _DOT

_CLASSES = {"d": "0-9", "w": "a-zA-Z0-9_", "s": " \t\n\x0b\f\r"}


def _python_form(java_regex: str) -> str:
    out, i, n, in_class = "", 0, len(java_regex), False
    while i < n:
        c = java_regex[i]
        i += 1
        if c == "\\":
            e = java_regex[i]
            i += 1
            if e.lower() in _CLASSES:
                members = _CLASSES[e.lower()]
                if in_class:
                    if e in "wDWS":
                        raise NotImplementedError(java_regex)
                    out += members
                else:
                    out += "(?-i:[" + ("^" if e.isupper() else "") + members + "])"
            else:
                out += "\\" + e if in_class or e.isalnum() else re.escape(e)
        elif in_class:
            in_class = c != "]"
            out += c
        elif c == "[":
            in_class = True
            out += c
        else:
            out += {"^": "\\A", "$": _DOLLAR, ".": _DOT}.get(c, c)
    return out


def regex_matches(java_regex: str, value: str) -> bool:
    return re.search(_python_form(java_regex), value, re.IGNORECASE) is not None


def regex_select(java_regex: str, values) -> list:
    return sorted({v for v in values if regex_matches(java_regex, v)})  # the distinct values REGEXP_LIKE keeps
