"""No GPU: the yardstick of occurrences within k substitutions (tests/hamming_util.py) against a plain double loop, against the
yardstick of search with substitutions (tests/mismatch_util.py) for k <= 2, and against the CPU oracle's locate; the piece rule
and the ownership rule that the GPU route relies on, replayed in numpy; what the pattern sets must hold; what the builders of
tests/test_gpu_hamming_edges.py must hold for its cases to reach what they are named for; the library's exports."""
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


# ---- what the builders of tests/test_gpu_hamming_edges.py must hold, from the builders and the yardstick alone --------------------

def _results(text, ps, k):
    """[(tag, pattern, offsets, costs)] of a builder's batch"""
    return [(c[0], c[1]) + occurrences(text, c[1], k) for c in ps]


def test_alphabet_corpora_meet_every_character_with_the_lacking_byte():
    for ncodes in (256, 255):
        docs = hu.alphabet_docs(ncodes)
        text = prepared(docs)
        assert len(docs) == 3 and 4000 <= len(text) <= 4200 and len(np.unique(text)) == ncodes
        have = np.unique(np.concatenate(docs))
        lacks = np.setdiff1d(np.arange(256), have)
        assert len(have) == ncodes - 1 and len(lacks) == 257 - ncodes
        for k in (1, 3):
            res = _results(text, hu.alphabet_patterns(docs, k), k)
            tags = [r[0] for r in res]
            met = set()
            for tag, p, o, c in res:
                if tag.startswith("opposite_"):
                    at = np.nonzero(p == int(lacks[0]) + OFFSET)[0]
                    assert len(p) == 24 and len(at) == 1 and str(at[0]) == tag.split("_")[2]
                    if k == 1:          # the one difference lies opposite the character, and the window is a result of cost 1
                        assert len(o) == 1 and c[0] == 1 and (text[o[0]:o[0] + 24] != p).sum() == 1
                    assert int(text[o[0] + at[0]]) - OFFSET == int(tag.split("_")[1])
                    met.add(int(text[o[0] + at[0]]) - OFFSET)
            assert met == set(have.tolist())
            by = {r[0]: r for r in res}
            assert len(by["two_lacking"][2]) == (0 if k == 1 else 1) and len(by["lack_owner%d" % (k + 1)][2]) == 0
            assert len(by["lack_opposite_seof"][2]) == 0 and len(by["lack_over_the_end"][2]) == 0
            for j in range(k + 1):          # the lacking byte in piece j: the window's owner is piece 0, or piece 1 where j = 0
                _, p, o, c = by["lack_in_piece%d" % j]
                assert c.tolist() == [1] and hu.owners(text, p, k, o).tolist() == [1 if j == 0 else 0]
            for j in range(1, k + 1):
                _, p, o, c = by["lack_owner%d" % j]
                assert c.tolist() == [j] and hu.owners(text, p, k, o).tolist() == [j]
                assert len(by["lack_seam%d" % j][2]) == (1 if k >= 2 else 0)
            assert any(len(p) % (k + 1) for _, p, _, _ in res) and sum(t.startswith("plain") for t in tags) == 8


def test_geometry_battery_reaches_every_alignment_length_and_owner():
    docs = hu.acgt_docs()
    text = prepared(docs)
    assert len(docs) == 2 and 4000 <= len(text) <= 4200 and len(np.unique(text)) == 5
    for k in hu.GEOMETRY_KS:
        ps = hu.geometry_batch(docs, k)
        starts = np.concatenate([[0], np.cumsum([len(p) for _, p in ps])])
        pairs, owner, ms, tags = set(), set(), set(), set()
        ends_on_a_word = several_in_a_word = none = 0
        for q, (tag, p, o, c) in enumerate(_results(text, ps, k)):
            assert k < len(p) and (not tag.startswith("filler") or k < len(p) <= k + 8)
            if not len(o):
                none += 1
                continue
            pairs |= {(int(x) & 7, int(starts[q]) & 7) for x in o}
            owner |= set(hu.owners(text, p, k, o).tolist())
            if not tag.startswith("filler"):
                ms.add(len(p))
                tags.add(tag.split("_r")[0].split("_", 1)[1])
            ends = [b1 for _, b1 in pieces(len(p), k)]
            ends_on_a_word += any(b1 % 8 == 0 for b1 in ends[:-1])
            several_in_a_word += any((ends[i] - 1) // 8 == (ends[i + 1] - 1) // 8 for i in range(k))
        assert len(pairs) == 64 and owner == set(range(k + 1)), (k, len(pairs), owner)
        assert ms == {k + 1} | {m for m in hu.GEOMETRY_MS if m > k} and ends_on_a_word > 0 and several_in_a_word > 0 and none > 0
        want = {"exact", "at0", "at7", "at8"} | {"owner%d" % j for j in range(1, k + 1)} | ({"seam%d" % j for j in range(1, k + 1)} if k > 1 else set())
        assert want <= tags, (k, want - tags)
    for k in hu.RUN_KS:
        for name, docs in hu.RUN_TEXTS.items():
            text = prepared(docs)
            res = _results(text, hu.run_patterns(k), k)
            assert sum(len(o) for _, _, o, _ in res) > 100 and len(np.unique(text)) == (2 if name == "one" else 3)
            assert name == "one" or {j for _, p, o, _ in res if len(o) for j in hu.owners(text, p, k, o).tolist()} >= set(range(min(k, 1) + 1))


def test_large_k_batches_hold_cost_0_cost_k_and_nothing():
    docs = hu.acgt_docs()
    text = prepared(docs)
    for k in hu.LARGE_KS:
        res = _results(text, hu.large_k_batch(docs, k), k)
        assert {len(p) for _, p, _, _ in res} >= {k + 1, k + 2, 2 * k + 1, 300} and 10 <= len(res) <= 40
        costs = np.concatenate([c for _, _, _, c in res])
        assert (costs == 0).any() and (costs == k).any() and any(len(o) == 0 for _, _, o, _ in res)
        by = {r[0]: r for r in res}
        for m in (k + 1, 2 * k + 1):          # the cut itself, with one and with k letters changed, is found where it was cut
            assert {0} <= set(by["cut%d_0" % m][3].tolist()) and {1} <= set(by["cut%d_1" % m][3].tolist()) and {k} <= set(by["cut%d_%d" % (m, k)][3].tolist())
        assert len(by["lacking"][2]) == 0 and (k < 31 or len(by["cut%d_%d" % (2 * k + 1, k + 1)][2]) == 0)


def test_bounds_patterns_have_the_pieces_they_were_built_for():
    docs = hu.acgt_docs()
    text = prepared(docs)
    n = len(text)
    for k in (1, 3):
        cases = hu.bounds_patterns(docs, k)
        assert {c[0] for c in cases} >= {"piece1_at_the_start", "piece%d_at_the_start" % k, "piece0_at_the_end", "one_symbol_too_far", "window_0", "window_last"}
        for tag, p, piece, at in cases:
            m = len(p)
            o, c = occurrences(text, p, k)
            if piece is None:
                assert at in (0, n - m - 1) and at in o.tolist()
                continue
            b0, b1 = pieces(m, k)[piece]
            assert at in occurrences(text, p[b0:b1], 0)[0].tolist()          # the candidate is there ...
            w = at - b0
            assert w < 0 or w > n - m, tag          # ... and its window leaves the text
            assert w not in o.tolist()
        by = {c[0]: c for c in cases}
        assert by["one_symbol_too_far"][3] == n - hu.BOUNDS_M + 1 and by["piece0_at_the_end"][3] > n - hu.BOUNDS_M + 1
        assert hu.owners(text, by["window_0_owner1"][1], k, [0]).tolist() == [1]
        assert hu.owners(text, by["window_last_owner%d" % k][1], k, [n - hu.BOUNDS_M - 1]).tolist() == [k]



def test_many_document_batches_straddle_at_every_split():
    import corpus_util as cu
    for name, docs in (("edges", cu.edges_docs()), ("library", cu.library_docs().docs)):
        text = prepared(hu._as_arrays(docs))
        for k in hu.MANY_KS:
            ps = hu.many_docs_patterns(docs, name, k)
            tags = {t for t, _ in ps}
            assert {"straddle%d_%d_%d" % (m, i, e) for m in hu.STRADDLE_MS for i in range(1, m) for e in {0, k - 1}} <= tags
            assert {"to_last_byte", "from_first_byte", "longer_than_its_document", "frequent0"} <= tags
            assert ("across_an_empty_document" in tags) == (name == "edges") and len(ps) <= 130
            if k != 2:
                continue
            res = _results(text, ps, k)
            assert sum(len(o) for _, _, o, _ in res) > 100
            for tag, p, o, c in res:
                if tag.startswith("straddle"):          # the window it was cut from: SEOF under position i, at most k differences in all
                    i = int(tag.split("_")[1])
                    at = [w for w in np.nonzero(text == SEOF)[0] - i if w >= 0 and w + len(p) <= len(text) and (text[w:w + len(p)] != p).sum() <= k]
                    assert at and not set(at) & set(o.tolist()), tag


def test_yardstick_on_the_builders_against_the_double_loop():
    import corpus_util as cu
    docs = hu.acgt_docs()
    text = prepared(docs)
    batches = [(text, hu.geometry_batch(docs, 3)[::97], 3), (text, hu.large_k_batch(docs, 16)[::5], 16), (text, hu.bounds_patterns(docs, 3)[::2], 3)]
    adocs = hu.alphabet_docs(256)
    batches.append((prepared(adocs), hu.alphabet_patterns(adocs, 3)[::40], 3))
    edges = cu.edges_docs()
    batches.append((prepared(hu._as_arrays(edges))[:9000], hu.many_docs_patterns(edges, "edges", 2)[::30], 2))
    seen = 0
    for t, ps, k in batches:
        for c in ps:
            o, cost = occurrences(t, c[1], k)
            assert list(zip(o.tolist(), cost.tolist())) == _double_loop(t, c[1], k), c[0]
            seen += len(o)
    assert seen > 1000


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
