"""No GPU: the yardstick of search with character classes (tests/classes_util.py) against the committed reference results
(tests/golden/<fixture>_regexp.npz: the reference's own result lists for ten regular expressions that are class patterns) and
against the CPU oracle's count of its strings; femto_amd_class_pattern_compile / femto_amd.class_patterns; femto_amd.iupac_patterns;
the library's exports and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
from classes_util import (CLASS, GOLDEN, OFFSET, SEOF, Table, allowed, automaton_may_differ, class_words, expected, golden_case, icase_symbols, members_of, pattern_set,
                          regex_of, strings)
from mismatch_util import prepared
from oracle import pyoracle

FIXTURES = ["acgt48k", "eng2doc", "bytes256", "runs3doc", "chunks2doc"]


def _codes(s):
    return np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + OFFSET


def _bytes(f):
    return bytes((f.symbols - OFFSET).astype(np.uint8))


def _cls(*members):
    return np.stack([class_words(m) for m in members]) if members else np.zeros((0, 4), dtype=np.uint64)


def test_hand_written_cases():
    t = prepared([b"abcabd", b"xbc", b"Abc"])
    ab, any_byte = _cls(b"ab", range(256))
    cls = np.stack([ab, any_byte, class_words(b"")])
    A, P, E = CLASS | 0, CLASS | 1, CLASS | 2
    c = lambda s: list(_codes(s))
    got = strings(t, c(b"ab") + [P], cls)
    assert [(_bytes(f), f.rows) for f in got] == [(b"abc", 1), (b"abd", 1)]
    assert [(_bytes(f), f.rows) for f in strings(t, [P] + c(b"bc"), cls)] == [(b"Abc", 1), (b"abc", 1), (b"xbc", 1)]
    assert [(_bytes(f), f.rows) for f in strings(t, [A, A], cls)] == [(b"ab", 2)]
    assert [(_bytes(f), f.rows) for f in strings(t, [A], cls)] == [(b"a", 2), (b"b", 4)]
    # a class holds bytes alone: no window runs over a document's end, unless the pattern holds SEOF there
    assert strings(t, c(b"d") + [P], cls) == [] and strings(t, [P, P, P, P, P, P, P], cls) == []
    assert [f.symbols.tolist() for f in strings(t, [P, SEOF], cls)] == [[ord("c") + 5, SEOF], [ord("d") + 5, SEOF]]
    assert [f.rows for f in strings(t, [P, SEOF], cls)] == [2, 1]
    # the empty pattern, the empty class, a class the table lacks, a symbol that is no alpha code
    e = strings(t, [], cls)
    assert len(e) == 1 and e[0].rows == len(t) and len(e[0].symbols) == 0
    assert strings(t, c(b"a") + [E], cls) == [] and strings(t, c(b"a") + [CLASS | 3], cls) == [] and strings(t, c(b"a") + [261], cls) == []
    assert allowed([CLASS | 3], cls) is None and allowed([261], cls) is None and allowed([A], cls).sum() == 2
    start, flat = expected([got, [], e])
    assert start.tolist() == [0, 2, 2, 3] and len(flat) == 3
    assert members_of(class_words([0, 63, 64, 255])) == [0, 63, 64, 255]
    assert regex_of(c(b"a") + [A, P, SEOF], cls) == b"\\x61[\\x61\\x62].\\x-03" and regex_of([E], cls) is None


@pytest.mark.parametrize("name,regex,count", GOLDEN)
def test_yardstick_reproduces_the_reference_results(fixtures, name, regex, count):
    """the strings, the rows per string and the order: lexicographic order is the reference's order by first"""
    first, last, mlen = golden_case(name, regex)
    assert len(first) == count
    pats, cls = femto_amd.class_patterns([regex])
    found = strings(prepared(fixtures(name).docs), pats[0], cls)
    assert len(found) == count
    assert np.array_equal(np.array([f.rows for f in found], dtype=np.int64), last - first + 1)
    assert (np.diff(first) > 0).all() and (mlen == len(pats[0])).all()


def test_pattern_set_holds_the_listed_cases(fixtures):
    for name in FIXTURES:
        docs = fixtures(name).docs
        ps, cls = pattern_set(docs, name)
        tags = [t for t, _ in ps]
        assert len(ps) == 200 and len(cls) <= 4096 and cls.dtype == np.uint64 and cls.shape[1] == 4, name
        assert {"empty", "literal1", "literal20", "class_first", "class_mid", "class_last", "class_all_three", "every1", "every2", "every20", "deep",
                "period1", "period2", "icase", "nobody_mid", "empty_class", "lacks", "absent", "seof_end", "seof_end_class", "shared"} <= set(tags)
        deep = ps[tags.index("deep")][1]
        assert len(deep) == 300 and (deep & CLASS).all() and all(len(members_of(cls[int(s) & ~CLASS])) == 2 for s in deep)
        assert members_of(cls[int(ps[tags.index("period1")][1][0]) & ~CLASS]) == list(range(256))
        tw = [p for t, p in ps if t == "twice"]
        assert len(tw) == 2 and np.array_equal(tw[0], tw[1]) and int(((tw[0] & CLASS) != 0).sum()) == 3
        sh = [p for t, p in ps if t == "shared"]
        assert len(sh) == 3 and len({int(p[len(p) // 2]) for p in sh[:2]} | {int(s) for s in sh[2]}) == 1 and tags.count("wide") == 30
        assert all(allowed(p, cls) is not None for _, p in ps)
        for t, p in ps:          # SEOF stands at a pattern's end and nowhere else
            assert not (p[:-1] == SEOF).any(), t
        assert len(ps) > 256 or sum(len(p) for _, p in ps) > 512          # the stack crosses what a workgroup's lanes cover
        again, cls2 = pattern_set(docs, name)
        assert np.array_equal(cls, cls2) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))


@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_against_the_oracle(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    ps, cls = pattern_set(fx.docs, name)
    per = [strings(text, p, cls) for _, p in ps]
    tags = [t for t, _ in ps]
    assert len(per[tags.index("deep")]) >= 1 and len(per[tags.index("period2")]) > len(per[tags.index("period1")]) > 1
    assert all(per[i] == [] for i, t in enumerate(tags) if t.startswith(("nobody", "empty_class", "lacks", "absent")))
    assert per[tags.index("seof_alone")][0].rows == len(fx.docs) and sum(len(fs) > 1 for fs in per) > 15
    start, flat = expected(per)
    sample = flat[::max(1, len(flat) // 600)]
    o = pyoracle.Oracle(fx.index)
    try:
        first, last = o.count([f.symbols for f in sample])
        f0, l0 = o.count([p for t, p in ps if t.startswith("literal")])
    finally:
        o.close()
    rows = np.array([f.rows for f in sample], dtype=np.int64)
    assert np.array_equal(last - first + 1, rows), np.nonzero(last - first + 1 != rows)[0][:8]
    lit = [fs for t, fs in zip(tags, per) if t.startswith("literal")]
    assert np.array_equal(l0 - f0 + 1, np.array([fs[0].rows if fs else 0 for fs in lit], dtype=np.int64))
    # distinct, and the lexicographic order is the order of first: on the whole lists of the widest patterns
    for i in sorted(range(len(per)), key=lambda i: -len(per[i]))[:3]:
        fs = per[i][:2000]
        o = pyoracle.Oracle(fx.index)
        try:
            f, _ = o.count([x.symbols for x in fs])
        finally:
            o.close()
        assert (np.diff(f) > 0).all(), tags[i]


@pytest.mark.parametrize("name", ["eng2doc", "runs3doc", "bytes256"])
def test_where_the_automaton_route_may_list_less(fixtures, name):
    """do_regexp_query (the CPU oracle's restatement) gives the yardstick's list wherever classes_util.automaton_may_differ says
    that it must, and a sub-list elsewhere; on eng2doc `..` is such a case: every ' is followed by s"""
    fx = fixtures(name)
    tagged, cls = pattern_set(fx.docs, name)
    some = [(t, p) for t, p in tagged if 0 < len(p) <= 40 and (p & CLASS).any() and (p >= OFFSET).all() and regex_of(p, cls) is not None][:64]
    text = prepared(fx.docs)
    o = pyoracle.Oracle(fx.index)
    try:
        less = []
        for tag, p in some:
            code, first, last, mlen, cost = o.nfa_search(femto_amd.Nfa.from_regex(regex_of(p, cls)))
            want = strings(text, p, cls)
            assert code == 0 and len(first) <= len(want), tag
            if not automaton_may_differ(text, p, cls):
                assert [int(r) for r in last - first + 1] == [f.rows for f in want] and (mlen == len(p)).all(), tag
            elif len(first) < len(want):
                less.append((tag, len(first), len(want)))
        assert less == ([("period2", 1980, 1999)] if name == "eng2doc" else []), less
    finally:
        o.close()


# ---- femto_amd_class_pattern_compile / class_patterns ------------------------------------------------------------------------------

def _one(query, icase=False):
    pats, cls = femto_amd.class_patterns([query], icase=icase)
    return pats[0].tolist(), [bytes(members_of(w)) for w in cls]


def test_compile_the_golden_regexes():
    A, Cc, G, T = (ord(x) + OFFSET for x in "ACGT")
    not_a = bytes(b for b in range(256) if b != ord("A"))
    every = bytes(range(256))
    assert _one(b"G[AC]T[^A]GG") == ([G, CLASS, T, CLASS | 1, G, G], [b"AC", not_a])
    assert _one(b"TTT.TTT") == ([T, T, T, CLASS, T, T, T], [every])
    assert _one(b"[AC][AC][GT][GT]ACG") == ([CLASS, CLASS, CLASS | 1, CLASS | 1, A, Cc, G], [b"AC", b"GT"])          # equal sets are shared
    assert _one(b"q.") == ([ord("q") + OFFSET, CLASS], [every])
    assert _one(b"\\n.") == ([10 + OFFSET, CLASS], [every])
    assert _one(b"[^a-z ]") == ([CLASS], [bytes(b for b in range(256) if not (97 <= b <= 122 or b == 32))])
    assert _one(b"\\x00.") == ([OFFSET, CLASS], [every])
    assert _one(b"[\\x80-\\xff][\\x00-\\x10]") == ([CLASS, CLASS | 1], [bytes(range(128, 256)), bytes(range(17))])
    assert _one(b"[\\x00-\\xff]\\x7f") == ([CLASS, 127 + OFFSET], [every])          # a set of all bytes and a period are one class
    assert _one(b"[\\x00-\\xff].")[0] == [CLASS, CLASS]
    assert _one(b"b.b") == ([ord("b") + OFFSET, CLASS, ord("b") + OFFSET], [every])


def test_compile_escapes_quotes_and_one_member_sets():
    c = lambda s: [b + OFFSET for b in s]
    assert _one(b"abc") == (c(b"abc"), []) and _one(b"a b  c") == (c(b"abc"), [])          # unescaped whitespace separates terms
    assert _one(b"a\\ b\\.\\[") == (c(b"a b.["), []) and _one(b"\\t\\x41\\\\") == (c(b"\tA\\"), [])
    assert _one(b"'a.b [c]'") == (c(b"a.b [c]"), []) and _one(b'"a\\x20\\"b"') == (c(b'a "b'), [])
    assert _one(b"{x 41 42}[x]") == (c(b"ABx"), [])          # a set with one member is a literal
    assert _one(b"[x-x]y[\\.]") == (c(b"xy."), [])
    assert _one(b"ab\\x-03") == (c(b"ab") + [SEOF], [])          # a code below the bytes is a literal
    assert _one(b"[z-a]b") == ([CLASS, ord("b") + OFFSET], [b""])          # a reversed range is the empty class
    assert _one(b"[ab]# the rest is a comment") == ([CLASS], [b"ab"])
    assert _one(b"[ab] x [ba][a-b]") == ([CLASS, ord("x") + OFFSET, CLASS, CLASS], [b"ab"])


def test_compile_icase():
    assert _one(b"aB1", True) == ([CLASS, CLASS | 1, ord("1") + OFFSET], [b"Aa", b"Bb"])          # a digit has one case: a literal
    assert _one(b"'it is'", True) == ([CLASS, CLASS | 1, 32 + OFFSET, CLASS, CLASS | 2], [b"Ii", b"Tt", b"Ss"])
    assert _one(b"[a-c]", True) == ([CLASS], [b"ABCabc"]) and _one(b"[a0]x", True) == ([CLASS, CLASS | 1], [b"0Aa", b"Xx"])
    assert _one(b"[a]", True) == ([CLASS], [b"Aa"]) and _one(b"[1].", True)[0] == [ord("1") + OFFSET, CLASS]
    assert _one(b"aA", True) == ([CLASS, CLASS], [b"Aa"])
    # the numpy restatement the GPU tests' pattern set uses says the same
    T = Table()
    text = b"Hello, World 42 times"
    assert icase_symbols(_codes(text), T).tolist() == _one(b"'" + text + b"'", True)[0] and len(T.words) == 11
    both = femto_amd.class_patterns([b"[ab]c", b"x[ba]", b"[cd][ab]"])          # the tables of a batch are merged
    assert [p.tolist() for p in both[0]] == [[CLASS, ord("c") + OFFSET], [ord("x") + OFFSET, CLASS], [CLASS | 1, CLASS]] and len(both[1]) == 2
    assert femto_amd.class_patterns([])[0] == [] and femto_amd.class_patterns([])[1].shape == (0, 4)


@pytest.mark.parametrize("query", [b"a+b", b"(ab|c)d", b"a?", b"APPROX 1 abc", b"a AND b", b"ab|cd", b"a{2}", b"(ab)", b"x*", b"a OR b", b"a THEN b"])
def test_compile_refuses_what_is_no_class_pattern(query):
    for icase in (False, True):
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            femto_amd.class_patterns([query], icase=icase)
        assert e.value.code == femto_amd.ERR_INVALID and "not a class pattern" in str(e.value), query


def test_compile_buffers_and_arguments():
    lib = femto_amd.lib()
    q = np.frombuffer(b"[ab]cd[ef]\0", dtype=np.uint8)
    syms, cls = np.full(8, 7, dtype=np.uint16), np.full((8, 4), 7, dtype=np.uint64)
    ns, nc = C.c_int64(-1), C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda scap, ccap: lib.femto_amd_class_pattern_compile(p(q), 10, 0, p(syms), scap, C.byref(ns), p(cls), ccap, C.byref(nc))
    for scap, ccap in ((3, 8), (8, 1), (0, 0)):          # too small: the sizes are reported and nothing is written
        assert call(scap, ccap) == femto_amd.ERR_FULL and (ns.value, nc.value) == (4, 2)
        assert (syms == 7).all() and (cls == 7).all()
    assert lib.femto_amd_class_pattern_compile(p(q), 10, 0, None, 0, C.byref(ns), None, 0, C.byref(nc)) == femto_amd.ERR_FULL and ns.value == 4
    assert call(4, 2) == 0 and (ns.value, nc.value) == (4, 2)
    assert syms[:4].tolist() == [CLASS, ord("c") + OFFSET, ord("d") + OFFSET, CLASS | 1] and (syms[4:] == 7).all() and (cls[2:] == 7).all()
    assert lib.femto_amd_class_pattern_compile(p(q), 10, 0, p(syms), 8, None, p(cls), 8, C.byref(nc)) == femto_amd.ERR_PARAM
    assert lib.femto_amd_class_pattern_compile(None, 10, 0, p(syms), 8, C.byref(ns), p(cls), 8, C.byref(nc)) == femto_amd.ERR_PARAM
    assert lib.femto_amd_class_pattern_compile(p(q), -1, 0, p(syms), 8, C.byref(ns), p(cls), 8, C.byref(nc)) == femto_amd.ERR_PARAM
    assert lib.femto_amd_class_pattern_compile(p(q), 10, 0, None, 8, C.byref(ns), p(cls), 8, C.byref(nc)) == femto_amd.ERR_PARAM
    assert lib.femto_amd_class_pattern_compile(None, 0, 0, p(syms), 8, C.byref(ns), p(cls), 8, C.byref(nc)) == femto_amd.ERR_PARAM          # the grammar has no empty query
    for bad in (b"[ab", b"a)", b"'ab"):
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            femto_amd.class_patterns([bad])
        assert e.value.code == femto_amd.ERR_PARAM


def test_iupac_patterns():
    pats, cls = femto_amd.iupac_patterns(["ACGT", b"ANNT", "RYSWKMBDHVN", ""])
    assert cls.shape == (11, 4) and cls.dtype == np.uint64
    assert [p.tolist() for p in pats[:2]] == [[ord(x) + OFFSET for x in "ACGT"], [ord("A") + OFFSET, CLASS | 10, CLASS | 10, ord("T") + OFFSET]]
    assert pats[2].tolist() == [CLASS | i for i in range(11)] and len(pats[3]) == 0 and all(p.dtype == np.uint16 for p in pats)
    want = {"R": b"AG", "Y": b"CT", "S": b"CG", "W": b"AT", "K": b"GT", "M": b"AC", "B": b"CGT", "D": b"AGT", "H": b"ACT", "V": b"ACG", "N": b"ACGT"}
    for sym, code in zip(pats[2], "RYSWKMBDHVN"):
        assert bytes(members_of(cls[int(sym) & ~CLASS])) == want[code], code
    for bad in ("ACGU", "acgt", "AC GT"):
        with pytest.raises(ValueError):
            femto_amd.iupac_patterns([bad])
    # a read with N is the period pattern restricted to the four bases
    text = prepared([b"ACGTTACGAAC"])
    p, c = femto_amd.iupac_patterns(["ACGN", "NACR"])
    assert [_bytes(f) for f in strings(text, p[0], c)] == [b"ACGA", b"ACGT"] and [_bytes(f) for f in strings(text, p[1], c)] == [b"TACG"]


# ---- the library before it needs a device -------------------------------------------------------------------------------------------

def test_library_exports_the_calls():
    for sym in ("femto_amd_classes_device", "femto_amd_classes", "femto_amd_classes_free", "femto_amd_class_pattern_compile"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("classes", "classes_device"):
        assert callable(getattr(femto_amd.Index, m))
    assert femto_amd.CLASS_SYMBOL == CLASS == 0x8000 and femto_amd.MAX_CLASSES == 4096


def test_arguments_are_checked_before_the_device(fixtures):
    lib = femto_amd.lib()
    one = np.zeros(8, dtype=np.int64)
    p = C.c_void_p(one.ctypes.data)
    r = femto_amd.ClassesResult()
    assert lib.femto_amd_classes_device(None, 1, 1, p, p, 0, None, 0, p, None, None, p, None) == 3
    assert lib.femto_amd_classes(None, 0, None, None, 0, None, C.byref(r)) == 3
    lib.femto_amd_classes_free(C.byref(r))
    lib.femto_amd_classes_free(None)
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)
    try:
        h = ix.handle
        dev = lambda npat, nsyms, syms, starts, ncl, cl, cap, rs, a, tot: lib.femto_amd_classes_device(h, npat, nsyms, syms, starts, ncl, cl, cap, rs, a, a, tot, None)
        assert dev(1, 1, None, p, 0, None, 0, p, None, p) == 3 and dev(1, 1, p, None, 0, None, 0, p, None, p) == 3      # NULL inputs
        assert dev(1, 1, p, p, 0, None, 0, None, None, p) == 3 and dev(1, 1, p, p, 0, None, 0, p, None, None) == 3      # NULL result_start / total
        assert dev(1, 1, p, p, 0, None, 4, p, None, p) == 3 and dev(1, 1, p, p, 0, None, -1, p, None, p) == 3           # capacity without arrays, negative
        assert dev(0, 1, p, p, 0, None, 0, p, None, p) == 3 and dev(-1, 0, p, p, 0, None, 0, p, None, p) == 3           # symbols without patterns
        assert dev(1, 1 << 31, p, p, 0, None, 0, p, None, p) == 3 and dev(1 << 31, 1, p, p, 0, None, 0, p, None, p) == 3 and dev(1, 1, p, p, 0, None, 1 << 31, p, p, p) == 3
        assert dev(1, 1, p, p, 4097, p, 0, p, None, p) == 3 and dev(1, 1, p, p, -1, p, 0, p, None, p) == 3              # nclasses
        assert dev(1, 1, p, p, 2, None, 0, p, None, p) == 3                                                             # a NULL table with classes
        assert "class table" in lib.femto_amd_last_error().decode()
        assert dev(1, 1, p, p, 4096, p, 0, p, None, p) == 6 and dev(1, 1, p, p, 0, None, 0, p, None, p) == 6          # the arguments are good: the handle has no device
        cls = _cls(b"ab")
        for pat, table, word in (([70, CLASS | 1], cls, "class"), ([70, CLASS], np.zeros((0, 4), dtype=np.uint64), "class"), ([70, 261], cls, "ALPHA_SIZE"),
                                 ([70, 0x7fff], cls, "ALPHA_SIZE")):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                ix.classes([np.array(pat, dtype=np.uint16)], table)
            assert e.value.code == 3 and word in str(e.value), pat
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.classes([np.full(32769, 70, dtype=np.uint16)], cls)
        assert e.value.code == 3 and "32768" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.classes([np.array([70], dtype=np.uint16)], np.zeros((4097, 4), dtype=np.uint64))
        assert e.value.code == 3 and "4096" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.classes([np.array([70, CLASS], dtype=np.uint16)], cls)
        assert e.value.code == 6 and "without a device" in str(e.value)
    finally:
        ix.close()


# ---- the inputs of tests/test_gpu_classes_edges.py ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["one", "two"])
def test_yardstick_against_a_plain_triple_loop(name):
    import classes_util as xu
    import mismatch_util as mu
    docs = mu.TINY_TEXTS[name]
    text = prepared(mu.as_arrays(docs))
    pats, cls = xu.tiny_patterns()
    assert len(pats) == 2 * (9 + 81 + 729) + 1 and len(cls) == 6 and [len(members_of(w)) for w in cls] == [2, 3, 2, 1, 256, 0]
    some = 0
    for p in pats:
        got = [(tuple(f.symbols.tolist()), f.rows) for f in strings(text, p, cls)]
        assert got == xu.plain_strings(docs, p, cls), (name, p.tolist())
        some += len(got) > 0
    assert some == (169 if name == "one" else 408)


def test_corpus_pattern_sets_end_in_seof_alone():
    import classes_util as xu
    import corpus_util as cu
    for name, docs in (("edges", cu.edges_docs()), ("library", cu.library_docs().docs)):
        ps, cls = xu.corpus_pattern_set(docs, name)
        base, base_cls = pattern_set([np.frombuffer(bytes(d), dtype=np.uint8) if isinstance(d, bytes) else d for d in docs], name)
        assert np.array_equal(cls[:len(base_cls)], base_cls) and len(cls) <= 4096 and len({w.tobytes() for w in cls}) == len(cls)
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, base)) and len(ps) > 512
        assert all(allowed(p, cls) is not None and not (p[:-1] == SEOF).any() for _, p in ps)
        tags = [t for t, _ in ps]
        assert sum("_classed1" in t for t in tags) > 100 and sum("_classed2" in t for t in tags) > 80
        for t, p in ps:
            if "_classed" in t:
                assert int(((p & CLASS) != 0).sum()) == int(t[-1]) and p[-1] == SEOF, t
        assert [t for t in tags[-3:]] == ["seof_after_period", "seof_after_period2", "seof_after_abn"]


def test_long_class_patterns_and_the_table_of_4096(fixtures):
    """every pattern of classes_util.long_patterns has a string; the cut with a class at every one of its 32768 positions has
    exactly the strings that a check of every window against the two bytes each position takes finds (one: a random text fixes a
    string after a dozen symbols); the 4096 classes are distinct and every pattern of theirs has a string"""
    import classes_util as xu
    fx = fixtures("acgt48k")
    doc = fx.docs[0]
    text = prepared(fx.docs)
    tagged, cls = xu.long_patterns(doc)
    assert [len(p) for _, p in tagged] == [32768] * 5 + [32767] * 5 + [32768, 32767, 4097] and len(cls) <= 6
    assert [int(((p & CLASS) != 0).sum()) for _, p in tagged] == [1, 1, 2, 2, 2] * 2 + [32768, 32767, 4097]
    assert (tagged[3][1][32766:] & CLASS).all() and (tagged[2][1][[0, 32767]] & CLASS).all()
    per = [strings(text, p, cls) for _, p in tagged]
    assert all(len(fs) >= 1 for fs in per)
    deep = tagged[10][1]
    takes = np.array([[b + OFFSET for b in members_of(cls[int(s) & ~CLASS])] for s in deep], dtype=np.uint16)          # two bytes per position
    cand = np.arange(len(text) - len(deep) + 1)
    for lo in range(0, len(deep), 64):          # every window, 64 positions at a time
        w = text[cand[:, None] + np.arange(lo, min(lo + 64, len(deep)))]
        t = takes[lo:lo + 64]
        cand = cand[((w == t[:, 0]) | (w == t[:, 1])).all(axis=1)]
    assert [f.symbols.tolist() for f in per[10]] == [text[c:c + len(deep)].tolist() for c in cand] and 1 <= len(cand) <= 4
    o = pyoracle.Oracle(fx.index)
    try:
        first, last = o.count([f.symbols for f in per[10]])
    finally:
        o.close()
    assert (last - first + 1).tolist() == [f.rows for f in per[10]]
    t4, c4 = xu.table_4096(doc)
    assert c4.shape == (4096, 4) and len({w.tobytes() for w in c4}) == 4096 and all(len(set(members_of(w)) & set(b"ACGT")) >= 2 for w in c4[::97])
    assert all(int(p[i % 12]) == CLASS | i and int((p & CLASS != 0).sum()) == 1 for i, (_, p) in enumerate(t4))
    n = np.array([len(strings(text, p, c4)) for _, p in t4])
    assert (n >= 1).all() and (n > 1).sum() >= 10
