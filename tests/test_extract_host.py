"""Extraction without a GPU: the two restatements of include/femto_amd.h "extraction" agree on every fixture, the library
exports the new entry points, and a parse-only handle refuses an extractor cleanly."""
import os

import numpy as np
import pytest

import femto_amd
from extract_util import FIXTURES, Restated

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
