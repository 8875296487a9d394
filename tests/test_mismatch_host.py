"""No GPU: the yardstick of search with substitutions (tests/mismatch_util.py) against the CPU oracle's count on every fixture and
the whole pattern set -- every variant occurs exactly as often as the yardstick's windows say, and no two variants of a pattern
share a first row --, hand-written cases, the library's exports and argument checks before it needs a device, and what the pattern
sets of tests/test_gpu_mismatch_edges.py and of the full-size case must hold for those cases to mean anything."""
import ctypes as C

import numpy as np
import pytest

import corpus_util as cu
import femto_amd
import mismatch_util as mu
from mismatch_util import OFFSET, SEOF, expected, pattern_set, prepared, variants
from oracle import pyoracle

FIXTURES = ["acgt48k", "b1000", "bytes256", "eng2doc", "chunks2doc", "runs3doc", "counter400_small", "construct_kat"]


def _codes(s):
    return np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + OFFSET


def _str(v):
    return bytes((v.symbols - OFFSET).astype(np.uint8))


def test_hand_written_cases():
    t = prepared([b"abcabd", b"xbc"])
    got = variants(t, _codes(b"abc"), 1)
    assert [(_str(v), v.rows, v.subs) for v in got] == [(b"abc", 1, ()), (b"abd", 1, ((2, ord("d") + 5),)), (b"xbc", 1, ((0, ord("x") + 5),))]
    assert [_str(v) for v in variants(t, _codes(b"abc"), 0)] == [b"abc"]
    two = variants(t, _codes(b"abc"), 2)          # "bca", "cab" differ everywhere; "dSx" would need SEOF as a substitute
    assert [_str(v) for v in two] == [b"abc", b"abd", b"xbc"]
    # a character the text lacks is substituted like any other; two of them need k = 2
    assert [(_str(v), v.subs) for v in variants(t, _codes(b"aNc"), 1)] == [(b"abc", ((1, ord("b") + 5),))]
    assert variants(t, _codes(b"NNc"), 1) == [] and [_str(v) for v in variants(t, _codes(b"NNc"), 2)] == [b"abc", b"xbc"]
    # the last character is substituted too, and a window never runs over a document's end ...
    assert [_str(v) for v in variants(t, _codes(b"abx"), 1)] == [b"abc", b"abd"]
    assert variants(t, _codes(b"dxq"), 2) == []          # ("dSx" and "Sxb" would need SEOF as a substitute)
    # ... unless the pattern holds SEOF there, which is matched exactly
    p = np.concatenate([_codes(b"bd"), [SEOF], _codes(b"x")])
    assert [v.subs for v in variants(t, p, 0)] == [()] and variants(t, np.concatenate([_codes(b"bc"), [SEOF], _codes(b"y")]), 1) == []
    assert [v.subs for v in variants(t, np.concatenate([_codes(b"bc"), [SEOF], _codes(b"x")]), 2)] == [((1, ord("d") + 5),)]
    assert [v.subs for v in variants(t, np.concatenate([_codes(b"bd"), [SEOF], _codes(b"y")]), 1)] == [((3, ord("x") + 5),)]
    assert [(v.symbols[:2].tolist(), v.subs) for v in variants(t, np.concatenate([_codes(b"ab"), [SEOF]]), 2)] == [
        ([ord("b") + 5, ord("c") + 5], ((0, ord("b") + 5), (1, ord("c") + 5))), ([ord("b") + 5, ord("d") + 5], ((0, ord("b") + 5), (1, ord("d") + 5)))]
    # the empty pattern, a pattern longer than the text, the same string twice in the text
    e = variants(t, [], 2)
    assert len(e) == 1 and e[0].rows == len(t) and e[0].subs == () and len(e[0].symbols) == 0
    assert variants(t, _codes(b"abcabdxbcabc"), 2) == []
    assert [(_str(v), v.rows) for v in variants(prepared([b"abab"]), _codes(b"ab"), 0)] == [(b"ab", 2)]
    start, flat, cost, pos, sym = expected([got, two], 1)
    assert start.tolist() == [0, 3, 6] and cost.tolist() == [0, 1, 1, 0, 1, 1]
    assert pos.tolist()[:3] == [[-1, -1], [2, -1], [0, -1]] and sym.tolist()[:3] == [[0, 0], [ord("d") + 5, 0], [ord("x") + 5, 0]]
    assert expected([got], 0)[0].tolist() == [0, 1]


def test_pattern_set_holds_the_listed_cases(fixtures):
    for name in FIXTURES:
        docs = fixtures(name).docs
        ps = pattern_set(docs, name)
        tags = [t for t, _ in ps]
        lens = {len(p) for _, p in ps}
        assert len(ps) == 300 and {0, 1, 2, 20, 64, 65} <= lens, name
        assert {"empty", "cut", "planted_first", "planted_mid", "planted_last", "planted_first_last", "seof_end", "random"} <= set(tags)
        assert ("straddle" in tags) == (len(docs) > 1) and ("lacks_two" in tags) == (name != "bytes256")
        if name != "acgt48k":
            assert len(ps[tags.index("long")][1]) == min(len(d) for d in docs) + 1
        tw = [p for t, p in ps if t == "twice"]
        assert len(tw) == 2 and np.array_equal(tw[0], tw[1])
        assert sum(len(p) for _, p in ps) > 512          # positions and patterns cross 256-lane blocks
        again = pattern_set(docs, name)
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(ps, again))


@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_against_the_oracle(fixtures, name, tmp_path):
    fx = fixtures(name)
    text = prepared(fx.docs)
    assert np.array_equal(text, fx.prepared_text())
    ps = pattern_set(fx.docs, name)
    per = [variants(text, p, 2) for _, p in ps]
    flat = [v for vs in per for v in vs]
    assert sum(len(v.subs) == 2 for v in flat) > 0 and sum(len(v.subs) == 1 for v in flat) > 0 and sum(len(v.subs) == 0 for v in flat) > 3
    o = pyoracle.Oracle(fx.index)
    try:
        first, last = o.count([v.symbols for v in flat])
    finally:
        o.close()
    rows = np.array([v.rows for v in flat], dtype=np.int64)
    assert np.array_equal(last - first + 1, rows), np.nonzero(last - first + 1 != rows)[0][:8]
    at = 0
    for (tag, p), vs in zip(ps, per):
        f = first[at:at + len(vs)]
        assert (np.diff(f) > 0).all(), (tag, f[:8])          # distinct, and the lexicographic order is the order of first
        at += len(vs)
    exact = np.array([any(not v.subs for v in vs) for vs in per])
    o = pyoracle.Oracle(fx.index)
    try:
        f, l = o.count([p for _, p in ps])
    finally:
        o.close()
    assert np.array_equal(f <= l, exact), [ps[i][0] for i in np.nonzero((f <= l) != exact)[0]]
    # what the yardstick does NOT list does not occur: every pattern's one-substitution neighbours at its first and last position
    tried, absent = set(), []
    have = np.unique(np.concatenate(fx.docs)).astype(np.uint16) + OFFSET
    for (tag, p), vs in list(zip(ps, per))[:60]:
        listed = {v.symbols.tobytes() for v in vs}
        for i in ({0, len(p) - 1} if len(p) else ()):
            if p[i] < OFFSET:
                continue
            for c in have[:6]:
                q = p.copy()
                q[i] = c
                if q.tobytes() not in listed and q.tobytes() not in tried:
                    tried.add(q.tobytes())
                    absent.append(q)
    if absent:
        o = pyoracle.Oracle(fx.index)
        try:
            f, l = o.count(absent)
        finally:
            o.close()
        assert (f > l).all()
    if pyoracle.have_ref():          # the genuine parallel_count on a sample
        sample = flat[::max(1, len(flat) // 200)]
        f, l = pyoracle.ref_count(fx.index, [v.symbols for v in sample], str(tmp_path))
        assert np.array_equal(l - f + 1, np.array([v.rows for v in sample], dtype=np.int64))


# ---- what tests/test_gpu_mismatch_edges.py and the full-size case of tests/test_gpu_fullsize.py rely on, from numpy alone --------

def _corpus(name):
    return mu.as_arrays(cu.edges_docs() if name == "edges" else cu.library_docs().docs)


@pytest.mark.parametrize("name,ndocs,nempty,nchars", [("edges", 816, 17, 31), ("library", 507, 0, 21)])
def test_corpus_pattern_sets_reach_what_the_gpu_tests_assert(name, ndocs, nempty, nchars):
    docs = _corpus(name)
    assert len(docs) == ndocs and sum(len(d) == 0 for d in docs) == nempty and len(np.unique(np.concatenate(docs))) + 1 == nchars
    ps = mu.corpus_pattern_set(docs, name)
    again = mu.corpus_pattern_set(docs, name)
    assert len(ps) == len(again) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))
    tags = [t for t, _ in ps]
    # the SEOF family: alone, behind every byte character of the text and one it lacks, behind 120 tails, behind three documents
    assert tags.count("seof_alone") == 1 and sum(t.startswith("seof_after_") for t in tags) == nchars
    assert sum(t.startswith("seof_tail") for t in tags) == 120 and tags.count("seof_whole") == 3
    for n in (1, 2, 5, 12):
        for nsub in (0, 1, 2):
            assert tags.count("seof_tail%d_%d" % (n, nsub)) == 10
    for t, p in ps:          # SEOF stands at a pattern's end and nowhere else, but for pattern_set's one "seof_inside"
        assert t == "seof_inside" or not (p[:-1] == SEOF).any(), t
        assert not t.startswith("seof_") or t == "seof_inside" or p[-1] == SEOF
    text = prepared(docs)
    per = [variants(text, p, 2) for _, p in ps]
    flat = [v for vs in per for v in vs]
    assert all(sum(len(v.subs) == c for v in flat) > 100 for c in (0, 1, 2))
    alone = per[tags.index("seof_alone")]
    assert len(alone) == 1 and alone[0].rows == ndocs          # one row per document, the empty ones included
    behind = [v for t, vs in zip(tags, per) if t.startswith("seof_") and t != "seof_inside" for v in vs]
    assert max(v.rows for v in behind) > 256 and sum(len(v.subs) == 2 for v in behind) > 100          # wide SEOF ranges under a substitution lane
    # variants substituted at the byte in front of the final SEOF: their lanes step from the SEOF range itself (ndocs rows)
    through = [v for (t, p), vs in zip(ps, per) if len(p) > 1 and p[-1] == SEOF for v in vs if any(i == len(p) - 2 for i, _ in v.subs)]
    assert ndocs > 256 and len(through) > 100 and sum(len(v.subs) == 2 for v in through) > 50 and max(v.rows for v in through) > 16
    assert max(v.rows for vs, (t, p) in zip(per, ps) if len(p) for v in vs) > 256
    assert max(len(vs) for vs in per) > 1000
    lacking = [vs for t, vs in zip(tags, per) if t.startswith("seof_after_")][-1]
    assert lacking and all(len(v.subs) == 1 and v.subs[0][0] == 0 for v in lacking)          # found through a substitution alone


def test_tiny_alphabets_are_exhaustive():
    pats = mu.tiny_patterns()
    assert len(pats) == 2 * 363 + 1 and len({p.tobytes() for p in pats}) == len(pats)
    assert sorted({len(p) for p in pats}) == list(range(0, mu.TINY_MAX + 2))
    a, b = ord("a") + OFFSET, ord("b") + OFFSET
    for name, nsub in (("one", 1), ("two", 2)):
        docs = mu.as_arrays(mu.TINY_TEXTS[name])
        assert len(np.unique(np.concatenate(docs))) == nsub and (name == "two") == any(len(d) == 0 for d in docs)
        text = prepared(docs)
        per = [variants(text, p, 2) for p in pats]
        flat = [v for vs in per for v in vs]
        assert all(sum(len(v.subs) == c for v in flat) > 10 for c in (0, 1, 2)), name
        assert all(s in ((a,) if name == "one" else (a, b)) for v in flat for _, s in v.subs)
        if name == "one":          # the one character is never substituted: a pattern of a alone has its exact result and no other
            for p, vs in zip(pats, per):
                if len(p) and (p == a).all():
                    assert [v.subs for v in vs] == ([()] if len(p) <= 7 else [])
            assert max(len(vs) for vs in per) == 1


def test_long_patterns_have_exactly_the_planted_variant(fixtures):
    doc = fixtures("acgt48k").docs[0]
    text = prepared([doc])
    longs = mu.long_patterns(doc)
    assert [len(p) for _, p, _ in longs].count(32768) == 6 and [len(p) for _, p, _ in longs].count(32767) == 5 and len(longs) == 15
    for tag, p, at in longs:
        vs = variants(text, p, 2)
        assert len(vs) == 1 and vs[0].rows == 1 and tuple(i for i, _ in vs[0].subs) == at, tag
        assert all(int(s) != int(p[i]) and OFFSET <= s for i, s in vs[0].subs)
    ats = [at for _, _, at in longs]
    assert (32767,) in ats and (0, 32767) in ats and (32766, 32767) in ats and (16383, 16384) in ats and (32766,) in ats and ats[-1] == ()


def test_full_size_front_is_two_to_the_31_lanes_less_768(fixtures):
    docs = fixtures("bytes256").docs
    nsub = len(np.unique(np.concatenate(docs)))
    front = mu.fullsize_front()
    assert nsub == 256 and len(front) == 256 and sum(len(p) for p in front) == mu.FRONT_SYMS
    assert [len(p) for p in front] == [32768] * 255 + [32765] and mu.FRONT_SYMS * nsub == (1 << 31) - 768
    tail = [p for _, p in pattern_set(docs, "bytes256")][:40]
    assert [len(p) for p in tail[:4]] == [0, 1, 2, 20]
    # lane 2^31 is the first lane of the tail's fourth symbol: the first symbol of its fourth pattern
    assert (1 << 31) % nsub == 0 and (1 << 31) // nsub - mu.FRONT_SYMS == 3 == sum(len(p) for p in tail[:3])
    assert (sum(len(p) for p in tail) + mu.FRONT_SYMS) * nsub > (1 << 31) + 256 * nsub
    text = prepared(docs)
    assert all(variants(text, p, 2) == [] for p in front)
    # ... and no lane of the front goes far: no suffix of three symbols and more of a front pattern occurs in the text
    have = {text[i:i + 3].tobytes() for i in range(len(text) - 2)}
    assert not any(p[-3:].tobytes() in have for p in front)


def test_library_exports_the_calls():
    for sym in ("femto_amd_mismatch_device", "femto_amd_mismatch", "femto_amd_mismatch_free"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("mismatch", "mismatch_device"):
        assert callable(getattr(femto_amd.Index, m))


def test_arguments_are_checked_before_the_device(fixtures):
    lib = femto_amd.lib()
    one = np.zeros(8, dtype=np.int64)
    p = C.c_void_p(one.ctypes.data)
    r = femto_amd.MismatchResult()
    assert lib.femto_amd_mismatch_device(None, 1, 1, p, p, 1, 0, p, None, None, None, None, None, p, None) == 3
    assert lib.femto_amd_mismatch(None, 0, None, None, 1, C.byref(r)) == 3
    lib.femto_amd_mismatch_free(C.byref(r))
    lib.femto_amd_mismatch_free(None)
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)
    try:
        h = ix.handle
        dev = lambda npat, nsyms, syms, starts, k, cap, rs, a, tot: lib.femto_amd_mismatch_device(h, npat, nsyms, syms, starts, k, cap, rs, a, a, a, a, a, tot, None)
        assert dev(1, 1, p, p, 3, 0, p, None, p) == 3 and dev(1, 1, p, p, -1, 0, p, None, p) == 3          # k
        assert dev(1, 1, None, p, 1, 0, p, None, p) == 3 and dev(1, 1, p, None, 1, 0, p, None, p) == 3      # NULL inputs
        assert dev(1, 1, p, p, 1, 0, None, None, p) == 3 and dev(1, 1, p, p, 1, 0, p, None, None) == 3      # NULL result_start / total
        assert dev(1, 1, p, p, 1, 4, p, None, p) == 3 and dev(1, 1, p, p, 1, -1, p, None, p) == 3           # capacity without arrays, negative
        assert dev(0, 1, p, p, 1, 0, p, None, p) == 3 and dev(-1, 0, p, p, 1, 0, p, None, p) == 3           # symbols without patterns
        assert dev(1, 1, p, p, 1, 0, p, None, p) == 6          # the arguments are good: the handle has no device
        for k in (3, -1):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                ix.mismatch([np.array([70, 71], dtype=np.uint16)], k)
            assert e.value.code == 3 and "0, 1 or 2" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.mismatch([np.full(32769, 70, dtype=np.uint16)], 1)
        assert e.value.code == 3 and "32768" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.mismatch([np.array([70, 261], dtype=np.uint16)], 1)
        assert e.value.code == 3 and "ALPHA_SIZE" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.mismatch([np.array([70, 71], dtype=np.uint16)], 1)
        assert e.value.code == 6 and "without a device" in str(e.value)
    finally:
        ix.close()
