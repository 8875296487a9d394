"""No GPU: the yardstick of search with substitutions (tests/mismatch_util.py) against the CPU oracle's count on every fixture and
the whole pattern set -- every variant occurs exactly as often as the yardstick's windows say, and no two variants of a pattern
share a first row --, hand-written cases, and the library's exports and argument checks before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
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
