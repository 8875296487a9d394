"""No GPU: the yardstick of occurrences within k substitutions (tests/hamming_util.py) against a plain double loop, against the
yardstick of search with substitutions (tests/mismatch_util.py) for k <= 2, and against the CPU oracle's locate; the piece rule
and the ownership rule that the GPU route relies on, replayed in numpy; what the pattern sets must hold; the library's exports."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
import hamming_util as hu
import mismatch_util as mu
from hamming_util import OFFSET, SEOF, occurrences, pattern_set, pieces, prepared
from oracle import pyoracle

FIXTURES = ["acgt48k", "b1000", "bytes256", "eng2doc", "chunks2doc", "runs3doc", "counter400_small", "construct_kat"]


def _codes(s):
    return np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + OFFSET


def _double_loop(text, p, k):
    out = []
    for at in range(len(text) - len(p) + 1):
        cost, ok = 0, True
        for j in range(len(p)):
            if text[at + j] != p[j]:
                cost += 1
                ok = ok and text[at + j] >= OFFSET
        if ok and cost <= k:
            out.append((at, cost))
    return out


def test_yardstick_against_a_double_loop():
    rng = np.random.default_rng(7)
    docs = [rng.integers(97, 100, size=n).astype(np.uint8) for n in (40, 1, 0, 23)]
    text = prepared(docs)
    assert len(text) == 68 and int((text == SEOF).sum()) == 4
    seen = 0
    for k in (0, 1, 2, 3, 5):
        for m in range(k + 1, 12):
            for _ in range(6):
                p = rng.integers(97, 101, size=m).astype(np.uint16) + OFFSET          # (100 is a character the text lacks)
                o, c = occurrences(text, p, k)
                assert list(zip(o.tolist(), c.tolist())) == _double_loop(text, p, k)
                assert o.dtype == np.int64 and c.dtype == np.int32
                seen += len(o)
    assert seen > 500
    t = prepared([b"abcabd", b"xbc"])
    assert [x.tolist() for x in occurrences(t, _codes(b"abc"), 1)] == [[0, 3, 7], [0, 1, 1]]
    assert [x.tolist() for x in occurrences(t, _codes(b"aNc"), 1)] == [[0], [1]]          # a lacking character costs one
    assert len(occurrences(t, _codes(b"dxq"), 2)[0]) == 0         # "dSx" would need SEOF as a substitute
    assert len(occurrences(t, _codes(b"abcabdxbcabc"), 2)[0]) == 0          # longer than the text
    assert pieces(10, 2) == [(0, 3), (3, 6), (6, 10)] and pieces(3, 2) == [(0, 1), (1, 2), (2, 3)] and pieces(5, 0) == [(0, 5)]
    start, off, cost = hu.expected(t, [_codes(b"abc"), _codes(b"zz"), _codes(b"bc")], 1)
    assert start.tolist() == [0, 3, 3, 6] and off.tolist() == [0, 3, 7, 1, 4, 8] and cost.tolist() == [0, 1, 1, 0, 1, 0]


def route(text, p, k):
    """the GPU route in numpy: every piece's exact windows moved back by the piece's start, the window kept inside the text, at
    most k differing positions, each under a byte character, and no EARLIER piece unchanged.  -> (candidates, [(offset, cost)])"""
    m, n = len(p), len(text)
    found, ncand = [], 0
    bounds = pieces(m, k)
    for j, (b0, b1) in enumerate(bounds):
        at, _ = occurrences(text, p[b0:b1], 0)
        ncand += len(at)
        for a in at:
            w = int(a) - b0
            if w < 0 or w > n - m:
                continue
            win = text[w:w + m]
            neq = win != p
            if neq.sum() > k or (win[neq] < OFFSET).any():
                continue
            if any(not neq[c0:c1].any() for c0, c1 in bounds[:j]):
                continue
            found.append((w, int(neq.sum())))
    return ncand, found


@pytest.mark.parametrize("name", FIXTURES)
def test_every_occurrence_has_one_owner_among_the_pieces(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    assert np.array_equal(text, fx.prepared_text())
    owned = shared = 0
    for k in (0, 2, 5):
        for tag, p in pattern_set(fx.docs, name, k)[::5]:
            if name == "runs3doc" and len(p) < 24:          # (hundreds of thousands of candidates: the GPU test has them)
                continue
            o, c = occurrences(text, p, k)
            ncand, found = route(text, p, k)
            assert sorted(found) == list(zip(o.tolist(), c.tolist())), (name, k, tag)          # each once: no duplicate, none missing
            assert ncand >= len(o)
            owned += len(o)
            for w in o[:50]:          # ... and the pigeonhole itself
                exact = [not (text[w + b0:w + b1] != p[b0:b1]).any() for b0, b1 in pieces(len(p), k)]
                assert any(exact)
                shared += sum(exact) > 1
    assert owned > 10 and (shared > 0 or name == "bytes256")          # occurrences that several pieces point at: the ownership rule is needed


@pytest.mark.parametrize("name", FIXTURES)
def test_windows_are_the_variants_of_search_with_substitutions(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    n = 0
    for k in (0, 1, 2):
        for tag, p in pattern_set(fx.docs, name, k)[::3]:
            o, c = occurrences(text, p, k)
            vs = mu.variants(text, p, k)
            mine = {}
            for w, cost in zip(o, c):
                key = text[w:w + len(p)].tobytes()
                mine.setdefault(key, [0, int(cost)])[0] += 1
                assert mine[key][1] == int(cost)
            assert mine == {v.symbols.tobytes(): [v.rows, len(v.subs)] for v in vs}, (name, k, tag)
            n += len(vs)
    assert n > 30


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_offsets_are_what_the_oracle_locates(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    o = pyoracle.Oracle(fx.index)
    try:
        seen = 0
        for k in (1, 3, 8):
            for tag, p in pattern_set(fx.docs, name, k)[::4]:
                if len(p) < 24 and k == 8:          # (every other window of the text: covered on the GPU)
                    continue
                offs, _ = occurrences(text, p, k)
                windows = {}
                for w in offs.tolist():
                    windows.setdefault(text[w:w + len(p)].tobytes(), []).append(w)
                keys = sorted(windows)[:40]
                if not keys:
                    continue
                noccs, located = o.locate([np.frombuffer(b, dtype=np.uint16) for b in keys], 1 << 30)
                at = 0
                for b, cnt in zip(keys, noccs):
                    assert sorted(located[at:at + cnt].tolist()) == windows[b], (name, k, tag)
                    at += cnt
                seen += len(keys)
        assert seen > 50
    finally:
        o.close()


def test_pattern_sets_hold_the_listed_cases(fixtures):
    for name in FIXTURES:
        docs = fixtures(name).docs
        text = prepared(docs)
        for k in hu.KS:
            ps = pattern_set(docs, name, k)
            tags = [t for t, _ in ps]
            lens = {len(p) for _, p in ps}
            assert (90 if name != "construct_kat" else 25) <= len(ps) <= 140, (name, k, len(ps))          # (construct_kat: 24 symbols of text)
            assert min(lens) == k + 1 and all(k < len(p) <= mu.MAX_PATTERN for _, p in ps)
            assert all(((p >= OFFSET) & (p < hu.ALPHA)).all() for _, p in ps)
            assert {"from_offset_0", "to_last_byte", "random"} <= set(tags)
            assert ("straddle" in tags) == (len(docs) > 1 and min(len(docs[0]), len(docs[1])) >= 12)
            assert ("longer_than_the_text" in tags) == (len(text) + 1 <= mu.MAX_PATTERN)
            assert k == 0 or any(len(p) % (k + 1) for _, p in ps)
            longest = max(len(d) for d in docs)
            assert {m for m in hu.LENGTHS if k < m <= longest} <= lens
            again = pattern_set(docs, name, k)
            assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))
            by = dict(reversed(ps))          # (the first pattern of a tag: to_last_byte of document 0)
            assert occurrences(text, by["from_offset_0"], k)[0][0] == 0
            end0 = len(docs[0]) - len(by["to_last_byte"])
            assert end0 in occurrences(text, by["to_last_byte"], k)[0].tolist()
            if "straddle" in by:          # no result where the two documents meet
                assert len(docs[0]) - 12 not in occurrences(text, by["straddle"], k)[0].tolist()
            if "lacks_too_many" in by:
                assert len(occurrences(text, by["lacks_too_many"], k)[0]) == 0
    # runs3doc: patterns of which EVERY piece occurs thousands of times
    docs = fixtures("runs3doc").docs
    text = prepared(docs)
    heavy = 0
    for tag, p in pattern_set(docs, "runs3doc", 2):
        if len(p) >= 24:
            heavy += min(len(occurrences(text, p[b0:b1], 0)[0]) for b0, b1 in pieces(len(p), 2)) >= 1000
    assert heavy >= 10


def test_library_exports_the_calls():
    for sym in ("femto_amd_hamming_device", "femto_amd_hamming", "femto_amd_hamming_free"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("hamming", "hamming_device"):
        assert callable(getattr(femto_amd.Index, m)) and callable(getattr(femto_amd.Extractor, m))


def test_arguments_are_checked_before_the_device():
    lib = femto_amd.lib()
    one = np.zeros(8, dtype=np.int64)
    p = C.c_void_p(one.ctypes.data)
    r = femto_amd.HammingResult()
    assert lib.femto_amd_hamming_device(None, 1, 1, p, p, 1, 0, 0, p, None, None, p, None) == 3
    assert lib.femto_amd_hamming(None, 0, None, None, 1, C.byref(r)) == 3
    assert lib.femto_amd_hamming(None, 0, None, None, 1, None) == 3
    lib.femto_amd_hamming_free(C.byref(r))
    lib.femto_amd_hamming_free(None)
    assert not one.any()
