"""No GPU: the restatement of the common-sequence rule (tests/similar_util.py) on hand-written cases and against the oracle's
count (the string of len[j] occurs, the string one byte longer does not); the library exports the calls and refuses bad
arguments before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import corpus_util as cu
import femto_amd
from oracle import pyoracle
from similar_util import Text, document_scores, groups_of, index_numerator, match_lengths, ranked, select


def test_abcabc():
    t = Text([b"xabcx", b"ybcay"])
    q = b"abcabc"
    lens = match_lengths(t, q)
    assert lens.tolist() == [1, 2, 3, 3, 2, 3]        # "abc", then "bca" (not "abca"), "ab" (neither "bcab" nor "cab"), "abc"
    assert select(lens, 2) == [2, 3, 5]               # the tie len[3] == len[2] keeps j = 2; j = 4 is inside the match ending at 5
    assert select(lens, 3) == [2, 3, 5] and select(lens, 4) == [] and select(lens, 0) == []      # (0: the default 8)
    seqs, groups, group_of = groups_of(q, lens, 2)
    assert seqs == [(0, 3), (1, 3), (3, 3)]
    assert [(g.bytes, g.here, g.min_start) for g in groups] == [(b"abc", 2, 0), (b"bca", 1, 1)] and group_of == [0, 1, 0]
    assert index_numerator(t, groups) == 3 * 1 + 3 * 1          # "abc" twice here, once there
    score, nseq = document_scores(2, groups, lambda g: t.hits(g.bytes))
    assert score.tolist() == [3, 3] and nseq.tolist() == [1, 1]
    assert ranked(t, len(q), score, nseq) == [(0, 3, 1, 3 / 5), (1, 3, 1, 3 / 5)]      # min(6, 5 document bytes)
    assert index_numerator(t, groups, kept=[0, 1]) == 3


def test_caps_and_boundaries():
    t = Text([b"abcdefgh", b"efghijkl"])
    assert match_lengths(t, b"abcdefgh", 3).tolist() == [1, 2, 3, 3, 3, 3, 3, 3]      # max_len
    assert match_lengths(t, b"abcdefgh").tolist() == [1, 2, 3, 4, 5, 6, 7, 8]          # runs into the start of the query
    assert match_lengths(t, b"ghef").tolist() == [1, 2, 1, 2]                          # "ghe" would cross the documents' boundary
    assert match_lengths(t, b"zaz").tolist() == [0, 1, 0] and match_lengths(t, b"").tolist() == []
    lens = match_lengths(t, b"abcdefghijkl")
    assert lens.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 5, 6, 7, 8] and select(lens) == [7, 11]
    assert select(lens, 9) == [] and select(np.array([8, 9, 9, 8], dtype=np.int32)) == [1, 2, 3]


def test_repeats_group_by_bytes():
    t = Text([b"0123456789" * 3])
    q = b"0123456789x0123456789"
    lens = match_lengths(t, q)
    seqs, groups, group_of = groups_of(q, lens)
    assert seqs == [(0, 10), (11, 10)] and len(groups) == 1 and groups[0].here == 2 and groups[0].min_start == 0 and group_of == [0, 0]
    assert len(t.occurrences(groups[0].bytes)) == 3 and index_numerator(t, groups) == 20
    assert groups[0].pattern.tolist() == [ord(c) + 5 for c in "0123456789"]


@pytest.mark.parametrize("name", ["eng2doc", "runs3doc"])
def test_lengths_against_the_oracle(fixtures, name):
    fx = fixtures(name)
    t = Text(fx.docs)
    allb = np.concatenate(fx.docs)
    q = allb[len(allb) // 3:len(allb) // 3 + 300].copy()
    q[::37] ^= 0x55
    for max_len in (0, 7):
        lens = match_lengths(t, q, max_len)
        cap = 32768 if max_len == 0 else max_len
        assert lens.max() > 4 and (lens < np.minimum(np.arange(300) + 1, cap)).any()
        sym = q.astype(np.uint16) + 5
        found = [sym[j - lens[j] + 1:j + 1] for j in range(300)]
        longer = [sym[j - lens[j]:j + 1] for j in range(300) if j - lens[j] >= 0 and lens[j] < cap]
        o = pyoracle.Oracle(fx.index)
        try:
            first, last = o.count(found)
            assert (first <= last).all()
            assert first[lens == 0].tolist() == [0] * int((lens == 0).sum()) and (last[lens == 0] == t.total_length - 1).all()
            first, last = o.count(longer)
            assert len(longer) >= 8 and (first > last).all()      # (at least the 8 substituted bytes end a match)
        finally:
            o.close()


def test_library_exports_the_calls():
    for sym in ("femto_amd_match_stats_device", "femto_amd_match_stats_steps_device", "femto_amd_common_sequences_device",
                "femto_amd_common_groups_device", "femto_amd_similar_documents_device", "femto_amd_similar", "femto_amd_similar_free"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("match_stats", "similar", "match_stats_device", "common_sequences_device", "common_groups_device", "similar_documents_device"):
        assert callable(getattr(femto_amd.Index, m))


def test_arguments_are_checked_before_the_device(fixtures):
    lib = femto_amd.lib()
    one = np.zeros(4, dtype=np.int64)
    p = C.c_void_p(one.ctypes.data)
    r = femto_amd.SimilarResult()
    assert lib.femto_amd_match_stats_device(None, 1, p, 0, p, None, None, None) == 3
    assert lib.femto_amd_common_sequences_device(None, 1, p, p, p, 0, p, p, p, p, 1, p, None) == 3
    assert lib.femto_amd_common_groups_device(None, 1, p, p, p, p, p, p, p, p, p, p, p, p, None) == 3
    assert lib.femto_amd_similar_documents_device(None, 1, p, p, p, p, p, None, 0, p, 1, p, p, p, None) == 3
    assert lib.femto_amd_similar(None, p, 1, 0, 0, 0, 0, None, C.byref(r)) == 3
    lib.femto_amd_similar_free(C.byref(r))
    lib.femto_amd_similar_free(None)
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)
    try:
        h = ix.handle
        assert lib.femto_amd_match_stats_device(h, -1, p, 0, p, None, None, None) == 3
        assert lib.femto_amd_match_stats_device(h, 1, p, 0, p, p, None, None) == 3          # d_first without d_last
        assert lib.femto_amd_match_stats_device(h, 1, None, 0, p, None, None, None) == 3
        assert lib.femto_amd_common_sequences_device(h, 1, p, p, p, 0, p, p, p, p, -1, p, None) == 3
        assert lib.femto_amd_common_sequences_device(h, 1, p, p, p, 0, p, p, p, p, 1, None, None) == 3
        assert lib.femto_amd_common_groups_device(h, 1 << 31, p, p, p, p, p, p, p, p, p, p, p, p, None) == 3
        assert lib.femto_amd_common_groups_device(h, 1, p, p, p, p, p, p, p, p, p, p, p, None, None) == 3
        assert lib.femto_amd_similar_documents_device(h, 1, p, p, p, p, p, None, 0, None, 1, p, p, p, None) == 3
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.similar(b"abcdefgh", max_len=65536)
        assert e.value.code == 3 and "65535" in str(e.value)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.similar(b"abcdefgh")
        assert e.value.code == 6 and "without a device" in str(e.value)
        assert lib.femto_amd_match_stats_device(h, 1, p, 0, p, None, None, None) == 6
    finally:
        ix.close()


# ---- the built corpus "library" (tests/corpus_util.py): what tests/test_gpu_edges.py relies on, from the restatement alone -------

def test_library_corpus_is_what_the_issue_lists():
    lib = cu.library_docs()
    t = Text(lib.docs)
    lens = [len(d) for d in lib.docs]
    assert len(lib.docs) >= 500 and 40000 <= sum(lens) <= 60000 and min(lens) >= 12 and max(lens) <= 200
    assert set(b"".join(lib.docs)) <= set(bytes(cu.ALPHABET20))
    assert [len(p) for p in lib.passages] == list(cu.PASSAGE_LENS)
    assert [len(t.hits(p)) for p in lib.passages] == list(cu.PASSAGE_DOCS)          # exactly 1, 2, 64, 65, 150 and 300 documents
    for k, held in enumerate(lib.twice):
        assert len(held) == (5 if cu.PASSAGE_DOCS[k] >= 64 else 0) and all(t.hits(lib.passages[k])[d] == 2 for d in held)
    assert sorted(lib.docs[d] for d in lib.pure) == sorted(lib.passages[k] for k in cu.PURE)
    a, b = lib.twins
    assert a != b and lib.docs[a] == lib.docs[b] and sum(d == lib.docs[a] for d in lib.docs) == 2
    assert cu.library_docs().docs == lib.docs and cu.library_query(lib) == cu.library_query(cu.library_docs())       # seeded


def test_library_query_reaches_every_case():
    lib = cu.library_docs()
    t = Text(lib.docs)
    q = cu.library_query(lib)
    n = len(q)
    assert 2000 <= n <= 3000
    lens = match_lengths(t, q)
    seqs, groups, group_of = groups_of(q, lens)
    assert len(groups) >= 6 and max(g.here for g in groups) > 1
    assert {g.bytes for g in groups} >= set(lib.passages)
    there = [len(t.occurrences(g.bytes)) for g in groups]
    assert max(there) < 1000          # max_occs = 1000: no range reaches the clamp, Text.hits decides every expectation
    assert max(there) > 101           # ... and the default clamp would cut
    assert max(len(t.hits(g.bytes)) for g in groups) >= 150
    assert any(max(t.hits(g.bytes).values()) > 1 for g in groups)          # a document that holds a sequence twice
    score, nseq = document_scores(len(t.docs), groups, lambda g: t.hits(g.bytes))
    rows = ranked(t, n, score, nseq)
    assert len(rows) >= 300 and nseq.max() >= 3
    assert sum(a[3] == b[3] for a, b in zip(rows, rows[1:])) >= 2          # ties in score: ordered by document
    a, b = lib.twins
    assert score[a] == score[b] > 0
    assert all(len(t.docs[r[0]]) < n for r in rows) and all(score[d] > 0 for d in lib.pure)      # the divisor is the document's length
    assert any(r[3] != r[1] / n for r in rows)
