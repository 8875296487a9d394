"""No GPU: the yardstick of search within edit distance (tests/edit_util.py) on hand-written cases, against a plain dynamic programme
over every distinct substring of two tiny texts, and against the CPU oracle's count on every fixture and the whole pattern set --
every string occurs exactly as often as the yardstick's windows say and (first, length) ascends strictly within a pattern --; then
the library's exports and its argument checks before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import edit_util as eu
import femto_amd
import mismatch_util as mu
from edit_util import expected, pattern_set, plain_variants, tiny_patterns, variants
from mismatch_util import OFFSET, SEOF, prepared
from oracle import pyoracle

FIXTURES = ["acgt48k", "b1000", "bytes256", "eng2doc", "chunks2doc", "runs3doc", "counter400_small", "construct_kat"]


def _codes(s):
    return np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + OFFSET


def _str(v):
    """the string with $ for SEOF"""
    return bytes(36 if c == SEOF else int(c) - OFFSET for c in v.symbols)


def _list(text, pattern, k):
    return [(_str(v), v.rows, v.cost) for v in variants(text, pattern, 2) if v.cost <= k]


def test_hand_written_cases():
    t = prepared([b"abcabd", b"xbc"])
    # deletions at both ends, an insertion behind the pattern, substitutions at both ends; "ab" holds "abc" and "abca": nested
    assert _list(t, _codes(b"abc"), 1) == [(b"ab", 2, 1), (b"abc", 1, 0), (b"abca", 1, 1), (b"abd", 1, 1), (b"bc", 2, 1), (b"xbc", 1, 1)]
    assert _list(t, _codes(b"abc"), 0) == [(b"abc", 1, 0)]
    # the pattern itself, reached by an insertion and a deletion too, is one result of cost 0; "abd" at cost 1 and (delete c, insert
    # d) at cost 2 is one result of cost 1
    assert _list(t, _codes(b"abc"), 2) == [
        (b"a", 2, 2), (b"ab", 2, 1), (b"abc", 1, 0), (b"abca", 1, 1), (b"abcab", 1, 2), (b"abd", 1, 1), (b"b", 3, 2), (b"bc", 2, 1),
        (b"bca", 1, 2), (b"bd", 1, 2), (b"c", 2, 2), (b"cab", 1, 2), (b"cabd", 1, 2), (b"xb", 1, 2), (b"xbc", 1, 1)]
    # the empty string for a pattern of length <= k: every row
    assert _list(t, _codes(b"a"), 1) == [(b"", 11, 1), (b"a", 2, 0), (b"ab", 2, 1), (b"b", 3, 1), (b"c", 2, 1), (b"ca", 1, 1), (b"d", 1, 1),
                                         (b"x", 1, 1)]
    assert _list(t, _codes(b"ab"), 1)[0] == (b"a", 2, 1) and _list(t, _codes(b"ab"), 2)[0] == (b"", 11, 2)
    assert _list(t, [], 0) == [(b"", 11, 0)] and _list(t, [], 1) == [(b"", 11, 0), (b"a", 2, 1), (b"b", 3, 1), (b"c", 2, 1), (b"d", 1, 1), (b"x", 1, 1)]
    # a character the text lacks is deleted, or substituted, like any other
    assert _list(t, _codes(b"abNc"), 1) == [(b"abc", 1, 1)]
    assert _list(t, _codes(b"aNc"), 1) == [(b"abc", 1, 1)] and _list(t, _codes(b"NabcN"), 1) == []
    assert (b"abc", 1, 2) in _list(t, _codes(b"NabcN"), 2)
    # SEOF is matched exactly, never deleted, and takes no insertion behind it: "bd$x" is in the text, one substitution and one
    # insertion away, and is not listed; no byte string is listed either, for SEOF would have to go
    end = np.concatenate([_codes(b"bc"), [SEOF]])
    assert _list(t, end, 2) == [(b"$", 2, 2), (b"abd$", 1, 2), (b"bc$", 1, 0), (b"bd$", 1, 1), (b"c$", 1, 1), (b"d$", 1, 2), (b"xbc$", 1, 1)]
    assert b"bd$x" in bytes(36 if c == SEOF else int(c) - OFFSET for c in t)
    # ... and in front of it one goes in: "bd$" from "b$"; a window never runs over a document's end otherwise
    assert _list(t, np.concatenate([_codes(b"b"), [SEOF]]), 1) == [(b"$", 2, 1), (b"bc$", 1, 1), (b"bd$", 1, 1), (b"c$", 1, 1), (b"d$", 1, 1)]
    assert _list(t, _codes(b"dx"), 1) == [(b"d", 1, 1), (b"x", 1, 1)]          # ("d$x" would need SEOF inserted)
    # an insertion in front of the pattern
    assert (b"xabc", 1, 1) in _list(prepared([b"xabcd"]), _codes(b"abc"), 1)
    assert _list(prepared([b"xabcd"]), _codes(b"abc"), 1) == [(b"ab", 1, 1), (b"abc", 1, 0), (b"abcd", 1, 1), (b"bc", 1, 1), (b"xabc", 1, 1)]
    # a run: every deletion gives the same string, every insertion too
    r = prepared([b"aaaa"])
    assert _list(r, _codes(b"aa"), 2) == [(b"", 5, 2), (b"a", 4, 1), (b"aa", 3, 0), (b"aaa", 2, 1), (b"aaaa", 1, 2)]
    assert _list(r, _codes(b"aaaaa"), 1) == [(b"aaaa", 1, 1)] and _list(r, _codes(b"ba"), 1) == [(b"a", 4, 1), (b"aa", 3, 1)]
    start, flat, cost, length = expected([variants(t, _codes(b"abc"), 2), variants(r, _codes(b"aa"), 2)], 1)
    assert start.tolist() == [0, 6, 9] and cost.tolist() == [1, 0, 1, 1, 1, 1, 1, 0, 1] and length.tolist() == [2, 3, 4, 3, 2, 3, 1, 2, 3]


@pytest.mark.parametrize("name", ["one", "two"])
def test_yardstick_against_a_plain_dynamic_programme(name):
    text = prepared(mu.as_arrays(mu.TINY_TEXTS[name]))
    pats = tiny_patterns()
    assert len(pats) == 2 * (3 + 9 + 27 + 81) + 1
    seen = {0: 0, 1: 0, 2: 0}
    for p in pats:
        vs = variants(text, p, 2)
        for k in (0, 1, 2):
            got = [(tuple(v.symbols.tolist()), v.rows, v.cost) for v in vs if v.cost <= k]
            assert got == plain_variants(text, p, k), (name, p.tolist(), k)
        for v in vs:
            seen[v.cost] += 1
        flat = lambda some: [(tuple(v.symbols.tolist()), v.rows, v.cost) for v in some]          # the narrower band finds the same
        assert flat(variants(text, p, 1)) == flat([v for v in vs if v.cost <= 1])
    # on "one" the patterns that occur are a, aa, aaa, aaaa, the four with SEOF behind them and the empty one
    assert seen[0] >= 9 and seen[1] > 50 and seen[2] > 50, seen


def _nested_pairs(first, last, start):
    n = 0
    for q in range(len(start) - 1):
        f, l = first[start[q]:start[q + 1]], last[start[q]:start[q + 1]]
        n += int(((f[1:] >= f[:-1]) & (l[1:] <= l[:-1])).sum())
    return n


@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_against_the_oracle(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    assert np.array_equal(text, fx.prepared_text())
    ps = pattern_set(fx.docs, name)
    again = pattern_set(fx.docs, name)
    assert len(ps) == 120 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))
    tags = {t for t, _ in ps}
    assert {"empty", "len1", "len2", "len20", "len64", "len65", "seof_end", "random", "twice", "run", "cut_del", "cut_ins", "cut_del_ins",
            "cut_del_del", "cut_ins_ins_gap", "edit_first_del", "edit_last_ins"} <= tags
    assert ("straddle" in tags) == (len(fx.docs) > 1) and ("lacks_two" in tags) == (name != "bytes256")
    per = [variants(text, p, 2) for _, p in ps]
    for (tag, p), vs in zip(ps, per):          # the planted edits are found: the cut they were made from occurs
        if tag.startswith(("cut_", "edit_", "run")):
            assert vs and min(v.cost for v in vs) <= 2, tag
    start, flat, cost, length = expected(per, 2)
    assert all((cost == c).sum() > 0 for c in (0, 1, 2))
    m = np.repeat(np.array([len(p) for _, p in ps]), np.diff(start))
    assert set((length - m).tolist()) == {-2, -1, 0, 1, 2}
    o = pyoracle.Oracle(fx.index)
    try:
        first, last = o.count([v.symbols for v in flat])
    finally:
        o.close()
    rows = np.array([v.rows for v in flat], dtype=np.int64)
    assert np.array_equal(last - first + 1, rows), np.nonzero(last - first + 1 != rows)[0][:8]
    for q, (tag, p) in enumerate(ps):          # (first, length) ascends strictly: distinct strings, in the order the call owes
        f, n = first[start[q]:start[q + 1]], length[start[q]:start[q + 1]]
        assert ((np.diff(f) > 0) | ((np.diff(f) == 0) & (np.diff(n) > 0))).all(), tag
    assert _nested_pairs(first, last, start) >= 1


def test_library_exports_the_calls():
    for sym in ("femto_amd_edit_device", "femto_amd_edit", "femto_amd_edit_free"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("edit", "edit_device"):
        assert callable(getattr(femto_amd.Index, m))


def test_arguments_are_checked_before_the_device(fixtures):
    lib = femto_amd.lib()
    one = np.zeros(8, dtype=np.int64)
    p = C.c_void_p(one.ctypes.data)
    r = femto_amd.EditResult()
    assert lib.femto_amd_edit_device(None, 1, 1, p, p, 1, 0, p, None, None, None, None, p, None) == 3
    assert lib.femto_amd_edit(None, 0, None, None, 1, C.byref(r)) == 3
    assert lib.femto_amd_edit(None, 0, None, None, 1, None) == 3
    lib.femto_amd_edit_free(C.byref(r))
    lib.femto_amd_edit_free(None)
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)          # parsed, no device
    try:
        h = ix.handle
        dev = lambda npat, nsyms, syms, starts, k, cap, rs, a, tot: lib.femto_amd_edit_device(h, npat, nsyms, syms, starts, k, cap, rs, a, a, a, a, tot, None)
        assert dev(1, 1, p, p, 3, 0, p, None, p) == 3 and dev(1, 1, p, p, -1, 0, p, None, p) == 3          # k
        assert dev(1, 1, None, p, 1, 0, p, None, p) == 3 and dev(1, 1, p, None, 1, 0, p, None, p) == 3      # NULL inputs
        assert dev(1, 1, p, p, 1, 0, p, None, None) == 3 and dev(1, 1, p, p, 1, 4, None, p, p) == 3         # NULL total; result_start with a capacity
        assert dev(1, 1, p, p, 1, 4, p, None, p) == 3 and dev(1, 1, p, p, 1, -1, p, None, p) == 3           # capacity without arrays, negative
        assert dev(0, 1, p, p, 1, 0, p, None, p) == 3 and dev(-1, 0, p, p, 1, 0, p, None, p) == 3           # symbols without patterns
        assert dev(1, 1 << 31, p, p, 1, 0, p, None, p) == 3 and dev(1, 1, p, p, 1, 1 << 31, p, p, p) == 3   # the bounds the header states
        assert dev(1, 1, p, p, 1, 0, p, None, p) == 6          # the arguments are good: the handle has no device
        for k in (3, -1):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                ix.edit([np.array([70, 71], dtype=np.uint16)], k)
            assert e.value.code == 3 and "0, 1 or 2" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.edit([np.full(32769, 70, dtype=np.uint16)], 1)
        assert e.value.code == 3 and "32768" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.edit([np.array([70, 261], dtype=np.uint16)], 1)
        assert e.value.code == 3 and "ALPHA_SIZE" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.edit([np.array([70, 71], dtype=np.uint16)], 1)
        assert e.value.code == 6 and "without a device" in str(e.value)
    finally:
        ix.close()


# ---- the preconditions of tests/test_gpu_edit_edges.py and of the full-size case ---------------------------------------------------

def _windows(text, p):
    """the windows of `text` that hold `p`"""
    p = np.asarray(p, dtype=np.uint16)
    cand = np.arange(len(text) - len(p) + 1)
    for j, c in enumerate(p):
        cand = cand[text[cand + j] == c]
    return len(cand)


def test_passage_patterns_keep_a_wide_range_to_the_end():
    """from the text alone: every pattern of the groups a, b, c and e lies within two operations of a string that stands in at
    least as many windows as its passage has documents, so the wide range survives to the walk's end; a pattern of group d (six
    symbols of one document, which two operations cannot take away, then the passage's head) stands in one window while its head
    stands in that many, so the range falls from hundreds of rows to one inside the walk -- and its lists differ between k = 1
    and k = 2; P3 and P5 end the documents that are nothing else"""
    import corpus_util as cu
    lib = cu.library_docs()
    text = prepared(mu.as_arrays(lib.docs))
    ps = eu.passage_patterns(lib)
    again = eu.passage_patterns(lib)
    assert len(ps) > 150 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))
    assert {t[3] for t, _ in ps} == set("abcdef") and sum("_e_shortened" in t for t, _ in ps) >= 4 and all(len(p) <= 60 for _, p in ps)
    wide2 = 0
    for tag, p in ps:
        ndocs = cu.PASSAGE_DOCS[int(tag[1]) - 1]
        assert ndocs >= 64
        vs = variants(text, p, 2)
        if tag[3] in "abce":
            assert max(v.rows for v in vs) >= ndocs, tag
            wide2 += sum(v.cost == 2 and v.rows >= 64 for v in vs)
        elif tag[3] == "d":
            bare = next(q for t, q in ps if t == tag[:5] + "bare")
            assert _windows(text, bare) == 1 and _windows(text, bare[eu.NOISE:]) >= ndocs and _windows(text, bare[eu.NOISE - 1:]) < ndocs, tag
            assert sum(v.cost <= 1 for v in vs) != len(vs) and len(vs) >= 1 and max(v.rows for v in vs) < ndocs, tag
        else:
            assert [v.rows for v in vs if v.cost == 0] == [cu.PURE.count(int(tag[1]) - 1)] and (p[-1] == SEOF) and not (p[:-1] == SEOF).any(), tag
    assert wide2 > 100
    for name, docs in (("edges", cu.edges_docs()), ("library", lib.docs)):
        cs = eu.corpus_pattern_set(docs, name)
        assert all(not (p[:-1] == SEOF).any() for _, p in cs)          # SEOF at a pattern's end alone
        assert sum(len(p) > 0 and p[-1] == SEOF for _, p in cs) >= 1 + 20 + 120 + 3 and [t for t, _ in cs[:120]] == [t for t, _ in pattern_set(mu.as_arrays(docs), name)]


def test_batches_and_cap_patterns(fixtures):
    order = eu.repeated(120, 70001, 70001)
    assert len(order) == 70001 and np.array_equal(np.sort(order[:120]), np.arange(120)) and np.bincount(order).min() >= 583
    assert len({int(order[i]) for i in range(255, 70001, 256)}) > 100          # the workgroups' ends land on many base patterns
    fx = fixtures("acgt48k")
    planted, cut, less = (p for _, p in eu.cap_patterns(fx.docs[0]))
    assert len(planted) == len(cut) == 32768 and len(less) == 32767
    assert np.array_equal(np.delete(planted, 24000)[:8000], cut[:8000]) and np.array_equal(np.delete(planted, 24000)[8000:], cut[8001:])
    assert _windows(prepared(fx.docs), cut) == 1 and _windows(prepared(fx.docs), planted) == 0


def test_fullsize_front_has_no_results(fixtures):
    """the front of test_edit_second_launch_at_the_shipped_chunk: where its sites end, that no suffix of three symbols of any of
    its patterns occurs in bytes256 (so the ranges of all sites but a pattern's last three are empty), and that the yardstick
    lists nothing for a sample of them"""
    fx = fixtures("bytes256")
    text = prepared(fx.docs)
    front = eu.fullsize_front()
    assert len(np.unique(np.concatenate(fx.docs))) == 256 and eu.EDIT_LANES == 2 * 256 + 1
    assert sum(len(p) for p in front) + len(front) == eu.FRONT_SITES == 4186111 and (eu.FRONT_BEHIND, eu.FRONT_EDIT) == (16, 497)
    assert (eu.FRONT_SITES + eu.FRONT_BEHIND) * eu.EDIT_LANES + eu.FRONT_EDIT == 1 << 31
    three = {(int(a), int(b), int(c)) for a, b, c in zip(text[:-2], text[1:-1], text[2:])}
    assert all(tuple(int(c) for c in p[-3:]) not in three for p in front)
    assert all(variants(text, p, 2) == [] for p in front[::16])
