"""No GPU: the yardstick of occurrences within k edits (tests/leven_util.py) against a plain double loop over the definition, against
the yardstick of occurrences within k substitutions (tests/hamming_util.py) for containment, against the strings of search within
edit distance (tests/edit_util.py) for k <= 2, and against plain search for k = 0; the route of femto_amd/leven/leven.hip -- pieces,
every seed, the right extension's cr and tr, the left extension's cl(t), the least (cost, length) per offset -- replayed in Python
statement for statement and held against the yardstick; what the pattern sets must hold; the library's exports."""
import ctypes as C

import numpy as np
import pytest

import edit_util as eu
import femto_amd
import hamming_util as hu
import leven_util as lu
from leven_util import MAX_PATTERN, OFFSET, SEOF, codes, expected, occurrences, pattern_set, pieces, prepared, route, route_answer

FIXTURES = ["acgt48k", "b1000", "bytes256", "eng2doc", "chunks2doc", "runs3doc", "counter400_small", "construct_kat"]


def _distance(a, b):
    """Levenshtein distance, the full table"""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[len(a)][len(b)]


def _double_loop(text, p, k):
    """the definition: every start, every end, a full table each"""
    t, p = [int(v) for v in text], [int(v) for v in p]
    out = []
    for s in range(len(t)):
        best = None
        for e in range(s + 1, min(len(t), s + len(p) + k) + 1):
            if t[e - 1] < OFFSET:
                break
            d = _distance(p, t[s:e])
            if d <= k and (best is None or d < best[0]):
                best = (d, e - s)
        if best:
            out.append((s,) + best)
    return out


def _triples(r):
    return list(zip(*(x.tolist() for x in r)))


def _small_corpora():
    """(text, k, pattern): alphabets of 2, 4 and 20 letters, several documents, empty ones among them, k = 0 .. 4; cuts with edits
    planted and random strings (with a letter the text lacks)"""
    rng = np.random.default_rng(11)
    for sigma in (2, 4, 20):
        for _ in range(24):
            docs = [rng.integers(97, 97 + sigma, size=int(rng.integers(0, 26))).astype(np.uint8) for _ in range(int(rng.integers(1, 5)))]
            text = prepared(docs)
            have = np.arange(97, 97 + sigma)
            for k in range(5):
                m = int(rng.integers(k + 1, 13))
                if rng.random() < 0.6 and len(text) > m + 2:
                    at = int(rng.integers(0, len(text) - m))
                    p = text[at:at + m].copy()
                    p[p < OFFSET] = 97 + OFFSET
                    p = lu.plant(rng, p, int(rng.integers(0, k + 1)), "mix", have, k)
                else:
                    p = (rng.integers(97, 97 + sigma + 1, size=m) + OFFSET).astype(np.uint16)
                yield text, k, p


def test_yardstick_against_a_double_loop():
    seen = 0
    for text, k, p in _small_corpora():
        got = occurrences(text, p, k)
        assert _triples(got) == _double_loop(text, p, k), (text.tolist(), p.tolist(), k)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
        seen += len(got[0])
    assert seen > 1000
    t = prepared([b"abcabd", b"xbc"])
    assert _triples(occurrences(t, codes(b"abc"), 0)) == [(0, 0, 3)]
    # every offset is listed: the clean hit at 0 brings offset 1 (a deleted) with it; "abd" is one substitution, "bd" two edits away
    assert _triples(occurrences(t, codes(b"abc"), 1)) == [(0, 0, 3), (1, 1, 2), (3, 1, 2), (7, 1, 3), (8, 1, 2)]
    assert _triples(occurrences(t, codes(b"aNc"), 1)) == [(0, 1, 3)]          # a lacking character costs one, substituted ...
    assert _triples(occurrences(t, codes(b"abNc"), 1)) == [(0, 1, 3)]          # ... or deleted
    for p, k in ((b"bdx", 0), (b"bdxb", 1), (b"dxbc", 2)):          # SEOF is never consumed: no result runs from "abd" into "xbc"
        o, c, length = occurrences(t, codes(p), k)
        assert _triples((o, c, length)) == _double_loop(t, codes(p), k) and not ((o < 6) & (o + length > 6)).any()
    start, off, cost, length = expected(t, [codes(b"abc"), codes(b"zz"), codes(b"xbc")], 0)
    assert start.tolist() == [0, 1, 1, 2] and off.tolist() == [0, 7] and cost.tolist() == [0, 0] and length.tolist() == [3, 3]


def test_the_route_of_the_kernel_equals_the_yardstick():
    """pieces, every seed, two extensions, the least (cost, length) per offset: the contract of the raw records"""
    raws = results = 0
    for text, k, p in _small_corpora():
        want = occurrences(text, p, k)
        got = route_answer(text, p, k)
        assert _triples(got) == _triples(want), (text.tolist(), p.tolist(), k)
        raw, cands = route(text, p, k)
        assert cands == sum(len(hu.occurrences(text, p[b0:b1], 0)[0]) for b0, b1 in pieces(len(p), k))
        raws += len(raw)
        results += len(want[0])
    assert raws > results > 1000          # several records reach one offset: the de-duplication is needed


@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc", "construct_kat", "bytes256"])
def test_the_route_on_fixtures(fixtures, name):
    fx = fixtures(name)
    text = prepared(fx.docs)
    assert np.array_equal(text, fx.prepared_text())
    seen = 0
    for k in (1, 3):
        for tag, p in pattern_set(fx.docs, name, k)[::3]:
            if len(p) < 24 and name != "construct_kat" or len(p) > 100:          # (short pieces: thousands of seeds, each a Python loop)
                continue
            want = occurrences(text, p, k)
            assert _triples(route_answer(text, p, k)) == _triples(want), (name, k, tag)
            seen += len(want[0])
    assert seen > 10


@pytest.mark.parametrize("name", FIXTURES)
def test_every_occurrence_within_k_substitutions_is_a_result(fixtures, name):
    text = prepared(fixtures(name).docs)
    seen = 0
    for k in (1, 3):
        for tag, p in hu.pattern_set(fixtures(name).docs, name, k)[::6]:
            ho, hc = hu.occurrences(text, p, k)
            o, c, length = occurrences(text, p, k)
            mine = dict(zip(o.tolist(), c.tolist()))
            assert all(w in mine and mine[w] <= cost for w, cost in zip(ho.tolist(), hc.tolist())), (name, k, tag)
            seen += len(ho)
    assert seen > 10


@pytest.mark.parametrize("name", ["chunks2doc", "eng2doc", "construct_kat"])
def test_results_are_the_strings_of_search_within_edit_distance(fixtures, name):
    """k <= 2: the string of every result is one of edit_util's strings, with its cost; every window of such a string is a result
    of no higher cost"""
    text = prepared(fixtures(name).docs)
    seen = 0
    for k in (1, 2):
        for tag, p in pattern_set(fixtures(name).docs, name, k)[::7]:
            if len(p) > 100:
                continue
            vs = {v.symbols.tobytes(): v.cost for v in eu.variants(text, p, k) if v.cost <= k}
            o, c, length = occurrences(text, p, k)
            mine = dict(zip(o.tolist(), c.tolist()))
            for w, cost, ln in zip(o.tolist(), c.tolist(), length.tolist()):
                assert vs.get(text[w:w + ln].tobytes()) == cost, (name, k, tag, w)
            for s, cost in vs.items():
                v = np.frombuffer(s, dtype=np.uint16)
                for w in hu.occurrences(text, v, 0)[0].tolist():
                    assert mine[w] <= cost, (name, k, tag, w)
            seen += len(o)
    assert seen > 10


@pytest.mark.parametrize("name", FIXTURES)
def test_k_0_is_plain_search(fixtures, name):
    text = prepared(fixtures(name).docs)
    seen = 0
    for tag, p in pattern_set(fixtures(name).docs, name, 0)[::2]:
        o, c, length = occurrences(text, p, 0)
        assert np.array_equal(o, hu.occurrences(text, p, 0)[0]) and not c.any() and (length == len(p)).all()
        seen += len(o)
    assert seen > 10


def test_pattern_sets_hold_the_listed_cases(fixtures):
    for name in FIXTURES:
        docs = fixtures(name).docs
        text = prepared(docs)
        longest = max(len(d) for d in docs)
        for k in lu.KS:
            ps = pattern_set(docs, name, k)
            tags = [t for t, _ in ps]
            assert all(k < len(p) <= MAX_PATTERN and ((p >= OFFSET) & (p < lu.ALPHA)).all() for _, p in ps)
            assert {"from_offset_0", "to_last_byte", "random"} <= set(tags)
            assert ("straddle" in tags) == (len(docs) > 1 and min(len(docs[0]), len(docs[1])) >= 12)
            assert ("longer_than_the_text" in tags) == (len(text) + 1 <= MAX_PATTERN)
            assert k == 0 or any(len(p) % (k + 1) for _, p in ps)
            for m, count in set(lu.CUTS) | {(k + 1, 8)}:
                if k < m <= longest:
                    assert sum(t.startswith("cut%d_" % m) for t in tags) >= count
            assert k < 2 or {t.rsplit("_", 1)[1] for t in tags if t.startswith("cut")} == set(lu.KINDS)
            again = pattern_set(docs, name, k)
            assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ps, again))
    # what the named cases must hold, where the yardstick is quick
    for name in ("eng2doc", "chunks2doc", "bytes256"):
        docs = fixtures(name).docs
        text = prepared(docs)
        for k in (0, 2):
            by = dict(reversed(pattern_set(docs, name, k)))          # (the first pattern of a tag: to_last_byte of document 0)
            assert occurrences(text, by["from_offset_0"], k)[0][0] == 0
            o, c, length = occurrences(text, by["to_last_byte"], k)
            at = o.tolist().index(len(docs[0]) - len(by["to_last_byte"]))
            assert c[at] == 0 and length[at] == len(by["to_last_byte"])
            if "straddle" in by:          # no result where the two documents meet: the pattern would have to consume SEOF
                o, c, length = occurrences(text, by["straddle"], k)
                assert not ((o < len(docs[0])) & (o + length > len(docs[0]))).any()
                assert len(docs[0]) - 12 not in o.tolist()
            if "lacks_too_many" in by:
                assert len(occurrences(text, by["lacks_too_many"], k)[0]) == 0
            if "longer_than_the_text" in by:
                assert len(occurrences(text, by["longer_than_the_text"], k)[0]) == 0
            for tag, p in pattern_set(docs, name, k):          # every planted cut occurs
                if tag.startswith("cut") and len(p) <= 64:
                    assert len(occurrences(text, p, k)[0]) >= 1, (name, k, tag)


# ---- what the builders of tests/test_gpu_leven_edges.py must hold, from the builders and the yardstick alone --------------------

def test_the_banded_yardstick_of_long_patterns_is_the_yardstick():
    """leven_util.around: the rows of a pattern nearly as long as its slice, over a band of columns alone"""
    rng = np.random.default_rng(5)
    docs = [rng.integers(97, 101, size=n).astype(np.uint8) for n in (700, 40, 300)]
    text = prepared(docs)
    seen = 0
    for k in (0, 1, 3, 6):
        for at, m in ((0, 50), (100, 200), (500, 180), (640, 61), (741, 40), (750, 290)):
            p = lu.plant(rng, np.where(text[at:at + m] < OFFSET, 97 + OFFSET, text[at:at + m]).astype(np.uint16), k, "mix", np.arange(97, 101), k)
            lo, hi = max(0, at - 2 * k - 8), min(len(text), at + len(p) + 2 * k + 8)
            o, c, length = occurrences(text[lo:hi], p, k)
            assert _triples(lu.around(text, p, k, at)) == _triples((o + lo, c, length)), (k, at, m)
            seen += len(o)
    assert seen >= 16          # (the four cuts that lie inside one document occur, under every k)


def test_edge_builders_hold_what_their_names_say():
    docs = hu.acgt_docs()
    text = prepared(docs)
    for k in lu.GEOMETRY_KS:
        batch = lu.geometry_batch(docs, k)
        lens = {len(p) for tag, p in batch if "_exact_" in tag}
        assert lens == {m for m in set(lu.GEOMETRY_MS) | {k + 1} if m > k} and all(len(p) > k for _, p in batch)
        tags = {tag.rsplit("_", 2)[0].split("_", 1)[1] for tag, _ in batch if not tag.startswith("filler")}
        assert {"exact", "ins_at0", "del_at7", "sub_at8", "seam1_left", "seam%d_right" % k, "owner%d" % k, "every_piece"} <= tags
        for tag, p in batch[::9]:          # at most k edits in a cut: it occurs
            assert "every_piece" in tag or len(occurrences(text, p, k)[0]) >= 1, (k, tag)
    for k in (1, 3):
        for tag, p, at, most in lu.bounds_patterns(docs, k):
            o, c, _ = occurrences(text, p, k)
            assert (at in o.tolist()) == (most is not None) and (most is None or c[o.tolist().index(at)] <= most), (k, tag)
    for k in lu.LARGE_KS:
        want = expected(text, [p for _, p in lu.large_k_batch(docs, k)], k)
        assert (want[2] == 0).any() and (want[2] == k).any() and (np.diff(want[0]) == 0).any()
    for ncodes in (256, 255):
        ad = hu.alphabet_docs(ncodes)
        batch = lu.lacking_opposite(ad, 1)
        assert len(batch) == ncodes          # every distinct byte of the text (SEOF is the other code), and the pattern that lacks twice
        want = expected(prepared(ad), [p for _, p in batch], 1)
        n = np.diff(want[0])
        assert (n[:-1] >= 1).all() and n[-1] == 0 and want[2].min() == 1


def test_exports_and_null_arguments():
    lib = femto_amd.lib()
    for sym in ("femto_amd_leven_device", "femto_amd_leven", "femto_amd_leven_free"):
        assert hasattr(lib, sym)
    for m in ("leven", "leven_device"):
        assert hasattr(femto_amd.Index, m) and hasattr(femto_amd.Extractor, m)
    p = C.c_void_p(8)
    r = femto_amd.LevenResult()
    assert lib.femto_amd_leven_device(None, 1, 1, p, p, 1, 0, 0, p, None, None, None, p, None) == 3
    assert lib.femto_amd_leven(None, 0, None, None, 1, C.byref(r)) == 3
    assert lib.femto_amd_leven(None, 0, None, None, 1, None) == 3
    lib.femto_amd_leven_free(C.byref(r))
    lib.femto_amd_leven_free(None)
    assert SEOF == 2
