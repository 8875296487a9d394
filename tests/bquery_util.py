"""Boolean queries in plain Python -- the specification tests/test_gpu_bquery.py holds femto_amd_bquery_run_batch to
(include/femto_amd.h "boolean queries"): a small recursive-descent parser of the boolean layer (posix.bison.y:122-135:
left-associative, no precedence, a group that holds an operator), the typing rules (setup_generic_boolean_query, server.c:5369;
results.c:513-545, 763-773) and a tree evaluator over brute-force leaf lists -- docpos_util.loop (the reference's two-pointer
loops) for THEN / WITHIN / OR of pairs, set operations for AND / OR / NOT of documents.

A leaf here is one blank-free word without parentheses (the tests' vocabulary); what it means -- a string, a regular
expression, an APPROX term -- is the caller's business: evaluate() asks `pairs_of(leaf)` for its (document, offset) rows."""
import re

import numpy as np

import docpos_util as dp

LEAF, AND, OR, NOT, THEN, WITHIN = 0, 1, 2, 3, 4, 5
DOCUMENTS, PAIRS = 0, 1
INT_MAX = 2 ** 31 - 1
_OPS = {"AND": AND, "OR": OR, "NOT": NOT, "THEN": THEN, "WITHIN": WITHIN}
NAMES = {v: k for k, v in _OPS.items()}


class TypeError_(ValueError):
    pass


def tokens(text):
    """('(' | ')' | ('op', op, distance) | ('leaf', word)) -- keywords need whitespace behind them, THEN takes a number only
    when whitespace follows it, WITHIN always has one"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c.isspace():
            i += 1
        elif c in "()":
            out.append(c)
            i += 1
        else:
            m = re.compile(r"[^\s()]+").match(text, i)
            w = m.group(0)
            i = m.end()
            if w.upper() in _OPS and w in (w.upper(), w.lower()) and i < n and text[i].isspace():
                op, d = _OPS[w.upper()], 0
                if op in (THEN, WITHIN):
                    d = INT_MAX
                    m = re.compile(r"\s+([0-9]+)(?=\s)").match(text, i)
                    if m:
                        d = int(m.group(1), 8 if m.group(1).startswith("0") and len(m.group(1)) > 1 else 10)
                        i = m.end()
                    elif op == WITHIN:          # "a WITHIN b" is the string aWITHINb
                        out.append(("leaf", w))
                        continue
                out.append(("op", op, d))
            else:
                out.append(("leaf", w))
    return out


def parse(text):
    """the tree as nested tuples: ('leaf', word) | (op, distance, left, right); raises ValueError on a syntax error"""
    toks = tokens(text)
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else None

    def rest():
        t = peek()
        if t == "(":
            pos[0] += 1
            node = exp()
            if node[0] == "leaf" or peek() != ")":
                raise ValueError("syntax error")
            pos[0] += 1
            return node
        if isinstance(t, tuple) and t[0] == "leaf":
            pos[0] += 1
            return t
        raise ValueError("syntax error")

    def exp():
        left = rest()
        while isinstance(peek(), tuple) and peek()[0] == "op":
            _, op, d = peek()
            pos[0] += 1
            left = (op, d, left, rest())
        return left

    tree = exp()
    if pos[0] != len(toks):
        raise ValueError("syntax error")
    return tree


def type_of(tree, wanted=DOCUMENTS):
    """the result type; raises TypeError_ where the reference would fail with ERR_PARAM"""
    if tree[0] == "leaf":
        return wanted
    op, _, left, right = tree
    ask = PAIRS if op in (THEN, WITHIN) else DOCUMENTS
    lt, rt = type_of(left, ask), type_of(right, ask)
    if op in (AND, NOT):
        return DOCUMENTS
    if op == OR:
        if lt != rt:
            raise TypeError_("OR of different kinds")
        return lt
    if lt != PAIRS or rt != PAIRS:
        raise TypeError_(NAMES[op] + " needs pairs")
    return PAIRS


def to_text(tree, rng=None, leaf_text=lambda w: w):
    """the tree written back: a right operand that is an operator needs its parentheses, a left one may have them;
    leaf_text(word) = how the vocabulary's word is written in the query language"""
    if tree[0] == "leaf":
        return leaf_text(tree[1])
    op, d, left, right = tree
    lt, rt = to_text(left, rng, leaf_text), to_text(right, rng, leaf_text)
    if left[0] != "leaf" and rng is not None and rng.integers(0, 2):
        lt = "(" + lt + ")"
    if right[0] != "leaf":
        rt = "(" + rt + ")"
    word = NAMES[op] if rng is None or rng.integers(0, 2) else NAMES[op].lower()
    num = "" if op not in (THEN, WITHIN) or (op == THEN and d == INT_MAX) else " %d" % d
    return "%s %s%s %s" % (lt, word, num, rt)


def height(tree):
    return 0 if tree[0] == "leaf" else 1 + max(height(tree[2]), height(tree[3]))


def levels(tree, out=None):
    """{height: set of families ('docset' / 'docpos')} of the operator nodes"""
    out = {} if out is None else out
    if tree[0] != "leaf":
        fam = "docpos" if tree[0] in (THEN, WITHIN) or (tree[0] == OR and type_of(tree, DOCUMENTS) == PAIRS) else "docset"
        out.setdefault(height(tree), set()).add(fam)
        levels(tree[2], out)
        levels(tree[3], out)
    return out


def evaluate(tree, pairs_of, wanted=DOCUMENTS):
    """(type, result): documents as an ascending int64 array, pairs as an (n, 2) array; pairs_of(word) = the leaf's rows as an
    (n, 2) array of (document, offset), ascending, each once"""
    if tree[0] == "leaf":
        p = dp.pairs(pairs_of(tree[1]))
        return (PAIRS, p) if wanted == PAIRS else (DOCUMENTS, np.unique(p[:, 0]))
    op, d, left, right = tree
    ask = PAIRS if op in (THEN, WITHIN) else DOCUMENTS
    (lt, lv), (rt, rv) = evaluate(left, pairs_of, ask), evaluate(right, pairs_of, ask)
    if op in (AND, NOT):
        a = lv if lt == DOCUMENTS else np.unique(lv[:, 0])         # a pair-typed operand gives each of its documents once
        b = rv if rt == DOCUMENTS else np.unique(rv[:, 0])
        return DOCUMENTS, (np.intersect1d(a, b) if op == AND else np.setdiff1d(a, b)).astype(np.int64)
    if op == OR:
        if lt != rt:
            raise TypeError_("OR of different kinds")
        if lt == DOCUMENTS:
            return DOCUMENTS, np.union1d(lv, rv).astype(np.int64)
        return PAIRS, dp.loop(lv, rv, dp.OR, 0)
    if lt != PAIRS or rt != PAIRS:
        raise TypeError_(NAMES[op] + " needs pairs")
    return PAIRS, dp.loop(lv, rv, dp.THEN if op == THEN else dp.WITHIN, d)


def packed(results):
    """(res_starts, res_type, res_doc, res_off) of a list of evaluate() results, as femto_amd_bquery_run_batch packs them"""
    starts, types, docs, offs = [0], [], [], []
    for t, v in results:
        types.append(t)
        if t == PAIRS:
            docs.append(v[:, 0])
            offs.append(v[:, 1])
        else:
            docs.append(v)
            offs.append(np.zeros(len(v), dtype=np.int64))
        starts.append(starts[-1] + len(v))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, dtype=np.int64)
    return np.array(starts, dtype=np.int64), np.array(types, dtype=np.int32), cat(docs), cat(offs)


def random_tree(rng, nleaves, vocab, distances=(1, 3, 10, 40, INT_MAX)):
    """a random tree of nleaves leaves that types (drawn again until it does)"""
    def build(n):
        if n == 1:
            return ("leaf", vocab[int(rng.integers(0, len(vocab)))])
        k = int(rng.integers(1, n))
        op = int(rng.integers(AND, WITHIN + 1))
        d = 0
        if op in (THEN, WITHIN):
            d = int(distances[int(rng.integers(0, len(distances) - (1 if op == WITHIN else 0)))])      # (WITHIN always has a number)
        return (op, d, build(k), build(n - k))

    while True:
        t = build(nleaves)
        try:
            type_of(t)
            return t
        except TypeError_:
            continue
