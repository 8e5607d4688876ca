"""The three grammars of the query box, restated from the header comments of host/boolean.hpp, grouped.hpp and quorum.hpp.

A query is cut into items with regular expressions: a group `[+-]( body )` with its optional `~digits`, or a piece of
non-space bytes.  The tokens of a body or piece are the search tokenizer's (nsbind.base_terms).  parse(text, dialect) gives the
terms in nsbind's format for that dialect and the set of things the text made the grammar do (`seen`), from which the tests
compute reach.
"""
import re

import nsbind

SHOULD, MUST, NOT = nsbind.NS_ROLE_SHOULD, nsbind.NS_ROLE_MUST, nsbind.NS_ROLE_NOT
NEED_CAP = 1000000
BOOLEAN, GROUPED, QUORUM = 0, 1, 2

_SPACE = " \t\n\r\f\v"
_PIECE = re.compile("[^" + _SPACE + "]+")
_GROUP = re.compile(r"([+-]?)\(([^)]*)(\))?")
_NEED = re.compile(r"~([0-9]+)")
_ROLE = {"+": MUST, "-": NOT, "": SHOULD}


def _items(text, dialect):
    """('group', role, body, need or None, closed) and ('piece', role, rest) and ('min', m), in query order"""
    at = 0
    while True:
        while at < len(text) and text[at] in _SPACE:
            at += 1
        if at == len(text):
            return
        g = _GROUP.match(text, at) if dialect != BOOLEAN else None
        if g:
            at = g.end()
            need = None
            tilde = False
            if dialect == QUORUM and g.group(3):
                tilde = text.startswith("~", at)
                m = _NEED.match(text, at)
                if m:
                    need, at = min(int(m.group(1)), NEED_CAP), m.end()
            yield ("group", _ROLE[g.group(1)], g.group(2), need, bool(g.group(3)), tilde)
            continue
        piece = _PIECE.match(text, at).group(0)
        at += len(piece)
        if dialect == QUORUM and _NEED.fullmatch(piece):
            yield ("min", min(int(piece[1:]), NEED_CAP))
        elif piece[0] in "+-":
            yield ("piece", _ROLE[piece[0]], piece[1:])
        else:
            yield ("piece", SHOULD, piece)


def parse(text, dialect):
    """-> (terms [(word, role, clause, need, promoted)], min_should, seen)"""
    terms, seen = [], set()
    n_clauses = min_should = 0
    for item in _items(text, dialect):
        if item[0] == "min":
            min_should = item[1]
            continue
        if item[0] == "piece":
            for w in nsbind.base_terms(item[2]):
                terms.append((w, item[1], n_clauses if item[1] == MUST else 0, 1 if item[1] == MUST else 0, False))
                n_clauses += item[1] == MUST
            continue
        _, role, body, need, closed, tilde = item
        words = nsbind.base_terms(body)
        if not closed:
            seen.add("unclosed group")
        if tilde and need is None:
            seen.add(")~ with no digit")
        if role == NOT and need is not None:
            seen.add("-( )~m")
        if not words:
            seen.add("empty body")
        if need and role == SHOULD:
            role = MUST   # `(a b c)~2` is `+(a b c)~2`
        need = max(need or 0, 1) if role == MUST else 0
        if words and need >= 2:
            seen.add("group with need >= 2")
        if words:
            seen.add("group")
        terms += [(w, role, n_clauses if role == MUST else 0, need, False) for w in words]
        n_clauses += bool(words) and role == MUST
    if min_should:
        if not any(r == SHOULD for _, r, _, _, _ in terms):
            seen.add("~m with nothing to promote")
        elif "group" in seen:
            seen.add("promoted term next to a group")
        terms = [(w, MUST, n_clauses, min_should, True) if r == SHOULD else (w, r, c, n, p) for w, r, c, n, p in terms]
    if len({c for _, r, c, _, _ in terms if r == MUST}) >= 2:
        seen.add("two or more clauses")
    return terms, min_should, seen


def parse_boolean(text):
    return [(w, r) for w, r, _, _, _ in parse(text, BOOLEAN)[0]]


def parse_grouped(text):
    return [(w, r, c) for w, r, c, _, _ in parse(text, GROUPED)[0]]


def parse_quorum(text):
    terms, m, _ = parse(text, QUORUM)
    return terms, m
