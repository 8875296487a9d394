"""Extraction without a GPU: the two restatements of include/femto_amd.h "extraction" agree on every fixture, the library
exports the new entry points, and a parse-only handle refuses an extractor cleanly; the inputs of
tests/test_gpu_extract_edges.py -- the two corpora of tests/corpus_util.py and the request batches of tests/extract_util.py -- hold
the cases that file is there for (nothing here reads a result of the library's)."""
import os

import numpy as np
import pytest

import corpus_util as cu
import femto_amd
from extract_util import (FIXTURES, SEOF, Restated, TextRestated, all_empty_requests, crowded_requests, long_requests, packed_starts,
                          random_requests)

TILE_SYMS = 2048          # extract.hip kTileSyms: the output symbols one workgroup of xcopy_kernel covers per turn
PAIRS = ((0, 1), (1, 0), (7, 7), (64, 64), (3, 200), (2047, 2047))
CORPORA = {"edges": cu.edges_docs, "dna": cu.dna_docs}
# the most SEOFs inside one block of 2^shift positions
MOST_EOFS = {"edges": {0: 1, 1: 2, 3: 4, 6: 11, 16: 816}, "dna": {0: 1, 1: 2, 3: 4, 6: 11, 16: 803}}

NEW_SYMBOLS = ["femto_amd_extractor_open", "femto_amd_extractor_free", "femto_amd_extractor_info", "femto_amd_extractor_eof_rows",
               "femto_amd_extract_device", "femto_amd_context_device", "femto_amd_extract", "femto_amd_context",
               "femto_amd_extract_document"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatements_agree(fixtures, name):
    fx = fixtures(name)
    R = Restated(fx)
    assert R.N == len(R.L)
    # the suffix array from the text and the reference's own BWT: L[row] = T[SA[row] - 1]
    assert np.array_equal(R.L, R.T[(R.sa - 1) % R.N].astype(np.int64))
    rng = np.random.default_rng(7)
    rows = np.arange(R.N) if R.N <= 2000 else np.concatenate([np.arange(64), rng.integers(0, R.N, 600)])
    for before, after in ((0, 1), (1, 0), (7, 7), (64, 64), (3, 200)):
        win = R.context_window(R.sa[rows], before, after)
        for k, r in enumerate(rows):
            a = R.context_rows(int(r), before, after)
            assert np.array_equal(a, R.context_text(int(R.sa[r]), before, after)), (r, before, after)
            assert np.array_equal(a, win[k]), (r, before, after)
    # a document is the context of its EOF row with before = doc_len - 1, after = 1 (server.c:6405-6430)
    assert np.array_equal(R.eof_rows_gold, R.isa[R.doc_ends - 1])
    for d in range(len(fx.docs)):
        doc = R.document(d)
        assert np.array_equal(R.context_rows(int(R.eof_rows_gold[d]), len(doc) - 1, 1), doc)


def test_resolve_golden_lengths(fixtures):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resolve_golden.npz"))
    for name in FIXTURES:
        R = Restated(fixtures(name))
        assert np.array_equal(np.array([len(R.document(d)) for d in range(len(R.doc_ends))]), g[name + "_len"]), name


def test_library_exports_the_extraction_symbols():
    lib = femto_amd.lib()
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert femto_amd.Extractor.PATH_TEXT == 0 and femto_amd.Extractor.PATH_SAMPLES == 1


def test_parse_only_handle_refuses_an_extractor(fixtures):
    ix = femto_amd.Index(fixtures("acgt48k").index, device=-1)
    with pytest.raises(femto_amd.FemtoAmdError) as e:
        ix.extractor()
    assert e.value.code == 6                        # FEMTO_AMD_ERR_INVALID
    with pytest.raises(femto_amd.FemtoAmdError) as e:
        ix.extract_document(0)
    assert e.value.code == 6
    ix.close()


# ---- the inputs of tests/test_gpu_extract_edges.py ------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=sorted(CORPORA))
def corpus(request):
    R = TextRestated(CORPORA[request.param]())
    R.name = request.param
    return R


def _anchors(R):
    """every SEOF, every document's first position, positions 0 and N - 1, 1 500 seeded anchors: (all of them, the seeded ones)"""
    seeded = np.random.default_rng(20250715).integers(0, R.N, 1500).astype(np.int64)
    starts = np.concatenate([[0], R.doc_ends[:-1]])
    return np.unique(np.concatenate([R.doc_ends - 1, starts, [0, R.N - 1], seeded])), seeded


def test_window_equals_stepping_on_the_corpora(corpus):
    R = corpus
    a, _ = _anchors(R)
    for before, after in PAIRS:
        win = R.context_window(a, before, after)
        for k, p in enumerate(a):
            want = R.context_text(int(p), before, after)
            assert np.array_equal(win[k], want), (R.name, before, after, int(p), np.nonzero(win[k] != want)[0][:8])


def test_the_corpora_hold_the_cases(corpus):
    R = corpus
    docs = CORPORA[R.name]()
    lens = np.array([len(d) for d in docs])
    assert R.N == lens.sum() + len(docs) < 65536 and len(R.doc_ends) == len(docs) >= 300
    symbols = len(np.unique(R.T))          # SEOF among them
    if R.name == "dna":
        assert symbols <= 8 and lens[0] > 0 and lens[-1] == 0 and (lens >= 3000).sum() == 2
    else:
        assert 9 <= symbols <= 256 and lens[0] == 0 and lens[-1] > 0
    assert (lens == 0).sum() >= 10 and (lens == 1).sum() >= 10
    eof = R.doc_ends - 1
    assert (R.T[eof] == SEOF).all() and (R.T == SEOF).sum() == len(docs)
    for shift, most in MOST_EOFS[R.name].items():
        assert np.bincount(eof >> shift).max() == most, (R.name, shift)
    assert (np.bincount(eof >> 6) >= 2).sum() >= 100
    assert (np.diff(eof) == 1).sum() >= 10          # two SEOFs side by side
    assert np.array_equal(R.eof_rows, R.isa[eof]) and len(np.unique(R.eof_rows)) == len(docs)


def test_the_request_batches_hold_the_cases(corpus):
    N = corpus.N
    nextra = len(random_requests(N, 1, n=0)[0])
    # crowded
    pos, lens = crowded_requests(N, 1)
    assert len(lens) >= 12000 and set(lens[:12000].tolist()) == {0, 1, 2} and lens[0] == 0 and lens[-1] == 0
    z = np.concatenate([[0], (lens == 0).astype(np.int64), [0]])
    runs = np.diff(np.nonzero(np.diff(z))[0])[::2]          # the lengths of the runs of empty requests
    first_run, last_run = int(np.argmax(lens != 0)), int(np.argmax(lens[::-1] != 0))
    assert first_run >= 300 and last_run >= 300 and (runs >= 300).sum() >= 4
    cum = packed_starts(lens)
    nonempty = np.nonzero(lens > 0)[0]
    per_tile = np.bincount(cum[nonempty] // TILE_SYMS)          # the requests that BEGIN in each tile
    assert per_tile.max() > 1000 and len(per_tile) >= 3
    # all_empty
    pos, lens = all_empty_requests(N, 2)
    assert len(lens) == 500 + nextra and not lens.any() and (pos < 0).any() and (pos >= N).any()
    # long
    pos, lens = long_requests(N, 3)
    assert len(lens) == 200 + nextra
    for want in ((0, N), (-5, N + 10), (N - 3000, 6000)):
        assert want in list(zip(pos[1:199].tolist(), lens[1:199].tolist()))
    cum = packed_starts(lens)
    tiles = (cum[1:] - 1) // TILE_SYMS - cum[:-1] // TILE_SYMS + 1
    assert (tiles[lens > 0] >= 3).sum() >= 3 and (lens[:200] <= 40).sum() == 197
    # every batch ends with the out-of-range extras (crowded: in front of its last run)
    for p in (random_requests(N, 4)[0], long_requests(N, 3)[0], all_empty_requests(N, 2)[0], crowded_requests(N, 1)[0][:-300]):
        assert (p[-nextra:] == random_requests(N, 1, n=0)[0]).all()


def test_the_stop_rule_matters_on_the_corpora(corpus):
    """without the stop rule a context is the plain T[p - 64 : p + 64]: the expectation must differ from it often, on both sides"""
    R = corpus
    _, seeded = _anchors(R)
    win = R.context_window(seeded, 64, 64)
    q = seeded[:, None] - 64 + np.arange(128)[None, :]
    plain = np.where((q >= 0) & (q < R.N), R.T[np.clip(q, 0, R.N - 1)], 0).astype(np.uint16)
    differs = (win != plain).any(axis=1)
    assert differs.sum() * 4 >= len(seeded), (R.name, int(differs.sum()))
    both = (win[:, :64] == 0).any(axis=1) & (win[:, 64:] == 0).any(axis=1)
    assert both.sum() >= 50, (R.name, int(both.sum()))
