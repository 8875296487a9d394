"""femto_amd_bquery_compile on the host (no GPU): the boolean layer of the query language -- tree shape, distances, what is no
operator, syntax and type errors, the leaves' own pipeline, the echo.  The reference's flex/bison front end cannot be generated
for these tests and oracle/ref_tool.c `ast` reads regular expressions only, so the answers are derived by hand from
src/main/posix.bison.y:122-135, src/main/posix.flex.l:270-287 and src/main/ast.c (AST_NODE_BOOL), as
femto_amd/csrc/query_parser.hpp's known answers are."""
import numpy as np
import pytest

import bquery_util as bu
import femto_amd
from femto_amd import (BQUERY_AND, BQUERY_DOCUMENTS, BQUERY_LEAF, BQUERY_NOT, BQUERY_OR, BQUERY_PAIRS, BQUERY_THEN, BQUERY_WITHIN,
                       BooleanQuery, FemtoAmdError)

INT_MAX = 2 ** 31 - 1


def _shape(q, i=None):
    """the tree as nested tuples: a leaf is its literal as bytes, an operator (op, distance, left, right)"""
    i = len(q.nodes) - 1 if i is None else i
    n = q.nodes[i]
    if n["op"] == BQUERY_LEAF:
        assert n["left"] == n["right"] == -1
        return (n["literal"] - 5).astype(np.uint8).tobytes() if n["literal"] is not None else n["echo"]
    assert 0 <= n["left"] < i and 0 <= n["right"] < i          # postfix: both children stand before their parent
    return (n["op"], n["distance"], _shape(q, n["left"]), _shape(q, n["right"]))


def test_tree_shape():
    A, O, N = BQUERY_AND, BQUERY_OR, BQUERY_NOT
    assert _shape(BooleanQuery(b"a AND b OR c NOT d")) == (N, 0, (O, 0, (A, 0, b"a", b"b"), b"c"), b"d")      # left-associative, no precedence
    assert _shape(BooleanQuery(b"a AND (b OR c)")) == (A, 0, b"a", (O, 0, b"b", b"c"))
    assert _shape(BooleanQuery(b"((a AND b) OR c)")) == (O, 0, (A, 0, b"a", b"b"), b"c")
    assert _shape(BooleanQuery(b"a and b or c not d")) == _shape(BooleanQuery(b"a AND b OR c NOT d"))
    q = BooleanQuery(b"a AND b OR c NOT d")
    assert len(q.nodes) == 7 and q.num_leaves == 4 and [n["op"] for n in q.nodes] == [0, 0, A, 0, O, 0, N]
    # the plain-Python parser the GPU tests generate their cases with reads the same trees
    for text in ("a AND b OR c NOT d", "a AND (b OR c)", "((a AND b) OR c)", "a then 20 b", "(a THEN b) AND c", "a WITHIN 5 (b within 2 c)"):
        def conv(t):
            return t[1].encode() if t[0] == "leaf" else (t[0], t[1], conv(t[2]), conv(t[3]))
        assert _shape(BooleanQuery(text.encode())) == conv(bu.parse(text)), text


def test_distances():
    assert _shape(BooleanQuery(b"a THEN b")) == (BQUERY_THEN, INT_MAX, b"a", b"b")
    assert _shape(BooleanQuery(b"a then 20 b")) == (BQUERY_THEN, 20, b"a", b"b")           # the digits belong to the operator, not to the leaf
    assert _shape(BooleanQuery(b"a then 200 b")) == (BQUERY_THEN, 200, b"a", b"b")
    assert _shape(BooleanQuery(b"a then  b")) == (BQUERY_THEN, INT_MAX, b"a", b"b")
    assert _shape(BooleanQuery(b"a then 20b")) == (BQUERY_THEN, INT_MAX, b"a", b"20b")     # no whitespace behind the digits: they are a term
    assert _shape(BooleanQuery(b"a THEN 010 b")) == (BQUERY_THEN, 8, b"a", b"b")           # read_int_part: sscanf %i
    assert _shape(BooleanQuery(b"a WITHIN 5 b")) == (BQUERY_WITHIN, 5, b"a", b"b")
    assert _shape(BooleanQuery(b"a WITHIN b")) == b"aWITHINb"                              # WITHIN without a number is no keyword
    with pytest.raises(FemtoAmdError, match="distance too large"):
        BooleanQuery(b"a THEN 99999999999 b")


def test_what_is_no_operator():
    for text, lit in ((b"blackANDsheep", b"blackANDsheep"), (b"'AND' x", b"ANDx"), (b'a "OR " b', b"aOR b"), (b"a [AND] b", None)):
        q = BooleanQuery(text)
        assert len(q.nodes) == 1 and q.num_leaves == 1 and q.result_type == BQUERY_DOCUMENTS, text
        if lit is not None:
            assert _shape(q) == lit, text


@pytest.mark.parametrize("text", [b"(a AND b)+", b"x(a AND b)", b"a AND", b"AND a", b"(a AND b", b"(a AND b) c", b"a AND (b", b"a AND b)", b"(AND a)",
                                  b"a AND OR b", b"((a AND b))", b"(a AND b){2}"])
def test_syntax_errors(text):
    with pytest.raises(FemtoAmdError) as e:
        BooleanQuery(text)
    assert e.value.args and "type error" not in str(e.value) and ("syntax" in str(e.value) or "missing )" in str(e.value) or "expected" in str(e.value))


def test_type_checks():
    for text, op, at in ((b"(a THEN b) OR c", "OR", 11), (b"(a AND b) THEN c", "THEN", 10), (b"a WITHIN 3 (b OR c)", "WITHIN", 2),
                         (b"c OR (a THEN b)", "OR", 2)):
        with pytest.raises(FemtoAmdError, match=r"type error: %s at byte %d\b" % (op, at)) as e:
            BooleanQuery(text)
        assert e.value.code == 3      # FEMTO_AMD_ERR_PARAM
        with pytest.raises(bu.TypeError_):
            bu.type_of(bu.parse(text.decode()))
    for text, want in ((b"(a THEN b) OR (c WITHIN 3 d)", BQUERY_PAIRS), (b"(a THEN b) AND c", BQUERY_DOCUMENTS), (b"a THEN b", BQUERY_PAIRS),
                       (b"a OR b", BQUERY_DOCUMENTS), (b"(a WITHIN 2 b) NOT (c THEN d)", BQUERY_DOCUMENTS), (b"a", BQUERY_DOCUMENTS),
                       (b"(a THEN b) THEN 3 c", BQUERY_PAIRS)):
        assert BooleanQuery(text).result_type == want == bu.type_of(bu.parse(text.decode())), text


def test_leaves_and_echo():
    q = BooleanQuery(b"APPROX 1 black AND sheep")
    assert q.nodes[0]["settings"] == (2, 1, 1, 1) and q.nodes[0]["literal"] is None         # cost_bound = max_cost + 1; not a plain string
    assert q.nodes[1]["settings"] == (1, 1, 1, 1) and _shape(q, 1) == b"sheep"
    assert q.echo == b'"black" AND "sheep"'
    q = BooleanQuery(b"sheep AND APPROX 2:1:2:3 black")                                      # APPROX may lead every leaf
    assert q.nodes[1]["settings"] == (3, 1, 2, 3)
    q = BooleanQuery(b"Black AND shEEp", icase=True)                                         # icase reaches every leaf
    assert [n["echo"] for n in q.nodes[:2]] == [b"[Bb][Ll][Aa][Cc][Kk]", b"[Ss][Hh][Ee][Ee][Pp]"] and q.echo == b"[Bb][Ll][Aa][Cc][Kk] AND [Ss][Hh][Ee][Ee][Pp]"
    # ast_to_string, AST_NODE_BOOL: left, " OP " (THEN / WITHIN with %i of the distance), right -- no parentheses
    assert BooleanQuery(b"a AND (b OR c)").echo == b'"a" AND "b" OR "c"'
    assert BooleanQuery(b"black then 20 sheep").echo == b'"black" THEN 20 "sheep"'
    assert BooleanQuery(b"black THEN sheep").echo == b'"black" THEN 2147483647 "sheep"'
    assert BooleanQuery(b"(a within 3 b) NOT th[ae]").echo == b'"a" WITHIN 3 "b" NOT th[ae]'
    # every leaf is streamlined and simplified as a query of its own (query_planning.c:33, ast.c:1244)
    q = BooleanQuery(b"x*abc+ OR (a|b)c")
    assert _shape(q, 0) == b"abc" and q.nodes[1]["literal"] is None and q.echo == b'"abc" OR (a|b)c'
    assert BooleanQuery(b"x*abc+ OR (a|b)c", streamline=False).nodes[0]["literal"] is None
    # a word before the ')' of a boolean group leaves its last letter behind as it does before any punctuation
    # (posix.flex.l:307); simplify_query joins the two again
    assert _shape(BooleanQuery(b"(a AND bcde)")) == (BQUERY_AND, 0, b"a", b"bcde")
    assert BooleanQuery(b"(a AND [xy]bcde)").echo == b'"a" AND [xy] "bcd"e' and BooleanQuery(b"a AND [xy]bcde").echo == b'"a" AND [xy] "bcde"'
    leaf = femto_amd.Nfa.from_query(b"th[ae]+x")
    q = BooleanQuery(b"foo AND th[ae]+x")
    assert q.nodes[1]["echo"] == leaf[2] and q.nodes[1]["literal"] is None


def test_plain_compile_still_refuses_the_operators():
    with pytest.raises(FemtoAmdError, match="boolean"):
        femto_amd.Nfa.from_query(b"black AND sheep")
