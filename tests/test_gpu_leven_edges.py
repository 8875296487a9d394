"""`-m gpu`: occurrences within k edits by exact seeds (femto_amd/leven/leven.hip) at the smallest shapes at which the extension can
go wrong, on the small corpora of tests/hamming_util.py: every pattern length around the words' ends at every pair of alignments
with an insertion, a deletion or a substitution at every place a piece ends, in pieces 0 .. j - 1 for every j and in every piece;
windows that hang off either end of the text; hundreds of documents with a pattern symbol opposite SEOF, empty documents, documents
shorter than the pattern and of one byte; texts of one and of two characters; k = 15 .. 31; the longest pattern; alphabets of 256
and 255 codes; two calls on one extractor from two streams; the sample path with one window per chunk and with refused patterns.
Every expectation is the yardstick of tests/leven_util.py, bit for
bit, and the candidates are the sum of ix.count over the pieces."""
import numpy as np
import pytest

import corpus_util as cu
import femto_amd
import hamming_util as hu
import leven_util as lu
from leven_util import expected, prepared
from regexp_util import open_kind
from test_gpu_leven import DEV, FIELDS, _device_run, _got, _handed, _patterns, _piece_candidates, _same

pytestmark = pytest.mark.gpu

TEXT, SAMPLES = femto_amd.Extractor.PATH_TEXT, femto_amd.Extractor.PATH_SAMPLES


class Built:
    """an index built here: docs (uint8 arrays), index (its path), text (prepared), want(tag, pats, k): the yardstick's answer, kept"""

    def __init__(self, tmp_path_factory, name, docs):
        self.name, self.docs = name, hu._as_arrays(docs)
        self.index = str(tmp_path_factory.mktemp(name) / "index")
        femto_amd.build_index(self.index, self.docs, params=None, infos=["%s%d" % (name, i) for i in range(len(self.docs))], device=0)
        self.text = prepared(self.docs)
        self._want = {}

    def want(self, tag, pats, k):
        if (tag, k) not in self._want:
            self._want[tag, k] = expected(self.text, pats, k)
        return self._want[tag, k]

    def open(self, kind=None):
        ix = open_kind(self.index, kind) if kind else femto_amd.Index(self.index, device=0)
        assert ix.info.number_of_documents == len(self.docs) and ix.info.total_length == len(self.text)
        return ix


def _check(ix, want, pats, k, what, **kw):
    """the host form against the yardstick's answer `want`, and the candidates against the pieces' counts"""
    start, off, cost, length, cands, raw = ix.leven(pats, k, **kw)
    _same((start, off, cost, length), want, what)
    assert cands == _piece_candidates(ix, pats, k) and raw >= len(off), what
    return cands, raw


@pytest.fixture(scope="module")
def acgt(tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, "acgt", hu.acgt_docs())


# ---- 1. the extension's geometry on a text of four letters ------------------------------------------------------------------------

@pytest.mark.parametrize("k", lu.GEOMETRY_KS)
def test_extension_geometry(acgt, k):
    """m = 7 .. 65 and k + 1, text and pattern at all 64 pairs of alignments, one insertion, deletion or substitution at 0, 7, 8 and
    m - 1 and on either side of every piece's end, one edit in each of pieces 0 .. j - 1 for every j, one in every piece"""
    batch = lu.geometry_batch(acgt.docs, k)
    pats = [p for _, p in batch]
    ix = acgt.open()
    try:
        assert ix.extractor().info()["path"] == TEXT
        want = acgt.want("geometry", pats, k)
        cands, raw = _check(ix, want, pats, k, ("geometry", k))
        n = np.diff(want[0])
        for q, (tag, _) in enumerate(batch):          # at most k edits in a cut: it occurs
            assert n[q] >= 1 or tag.endswith("every_piece") or "_every_piece_" in tag, tag
        assert cands > len(pats) and raw > len(want[1])
        if k == 2:
            _check(ix, want, pats, k, ("geometry", k, "samples"), force_samples=True)
    finally:
        ix.close()


# ---- 2. the bounds of the window ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
def test_windows_that_hang_off_the_text(acgt, k):
    """the pattern's front hangs off the text's start, its back over the last document's end: offset 0 (the cut's start) is a result
    when what hangs off can be deleted within k, and is none with k + 1 symbols hanging, although a piece is found there"""
    cases = lu.bounds_patterns(acgt.docs, k)
    pats = [c[1] for c in cases]
    ix = acgt.open()
    try:
        want = acgt.want("bounds", pats, k)
        for kw in ({}, dict(force_samples=True)):
            _check(ix, want, pats, k, ("bounds", k, kw), **kw)
        for q, (tag, p, at, most) in enumerate(cases):
            assert _piece_candidates(ix, [p], k) > 0, tag
            offs, costs = want[1][want[0][q]:want[0][q + 1]].tolist(), want[2][want[0][q]:want[0][q + 1]].tolist()
            assert (at in offs) == (most is not None), tag
            assert most is None or costs[offs.index(at)] <= most, tag
    finally:
        ix.close()


# ---- 3. document ends ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, "edges", cu.edges_docs())


@pytest.mark.parametrize("kind", ["ind", "wave"])
def test_many_documents(corpus, kind):
    """816 documents, empty ones and documents of one byte among them: a pattern laid over two neighbours with one symbol opposite
    SEOF is never a result through that window (the insertion step must not swallow SEOF); documents shorter than m - k"""
    B = corpus
    lens = np.array([len(d) for d in B.docs])
    assert (lens == 0).any() and (lens == 1).any()
    ends = np.cumsum(lens + 1) - 1          # the offsets of the SEOFs
    ix = B.open(kind)
    try:
        for k in (1, 2, 5):
            pats = [p for _, p in hu.many_docs_patterns(B.docs, B.name, k)]
            want = B.want("many", pats, k)
            _check(ix, want, pats, k, (B.name, kind, k))
            assert len(want[1]) > 100
            nxt = ends[np.searchsorted(ends, want[1])]          # no result runs over its document's end
            assert (want[1] + want[3] <= nxt).all()
            if kind == "ind" and k == 2:
                _check(ix, want, pats, k, (B.name, kind, k, "samples"), force_samples=True)
    finally:
        ix.close()


# ---- 4. runs ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["one", "two"])
def runs(request, tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, "runs_" + request.param, hu.RUN_TEXTS[request.param])


def test_texts_of_one_and_two_characters(runs):
    """patterns of one character on runs of it: every piece occurs at every place, many candidates reach every offset with several
    records each: the de-duplication at its heaviest"""
    ix = runs.open()
    try:
        for k in hu.RUN_KS:
            pats = [p for _, p in hu.run_patterns(k)]
            want = runs.want("runs", pats, k)
            cands, raw = _check(ix, want, pats, k, (runs.name, k))
            assert len(want[1]) > 100 and cands >= (k + 1) * 100 and (k == 0 or raw > 3 * len(want[1]))
    finally:
        ix.close()


# ---- 5. large k ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", lu.LARGE_KS)
def test_large_k(acgt, k):
    """m = k + 1, k + 2, 2 k + 1 and 300 with 0, 1, k and k + 1 edits planted: pieces of one symbol, rows of up to 65 entries"""
    pats = [p for _, p in lu.large_k_batch(acgt.docs, k)]
    ix = acgt.open()
    try:
        want = acgt.want("large", pats, k)
        cands, _ = _check(ix, want, pats, k, ("large k", k))
        assert (want[2] == 0).any() and (want[2] == k).any() and (np.diff(want[0]) == 0).any() and cands > 1000 * k
        if k == 16:
            import torch
            total = len(want[1])
            raw = ix.leven(pats, k)[5]
            r = _device_run(ix, pats, k, cands, raw + 3, torch.cuda.Stream(device=DEV))
            assert r["total"].tolist() == [total, 0, raw, cands, 0]
            _same(_got(r, total), want, ("large k, device form", k))
    finally:
        ix.close()


def test_the_longest_pattern_under_k_31(fixtures, gpu_ok):
    """32768 symbols in 32 pieces of 1024: found with none and with 31 letters changed, and with one symbol removed beside 30
    changed; not with 32 changed.  The yardstick slides over the 33 k symbols around the cut alone"""
    fx = fixtures("acgt48k")
    text = prepared(fx.docs)
    batch = lu.long_batch(fx.docs[0])
    per = [lu.around(text, p, 31, 200) for _, p in batch]
    want = (np.concatenate([[0], np.cumsum([len(r[0]) for r in per])]).astype(np.int64),) + tuple(np.concatenate([r[i] for r in per]) for i in range(3))
    n = np.diff(want[0]).tolist()
    assert n[0] == 63 and n[1] >= 1 and n[2] == 0 and n[3] >= 1 and 200 in per[1][0].tolist() and 200 in per[3][0].tolist()
    ix = femto_amd.Index(fx.index, device=0)
    try:
        cands, _ = _check(ix, want, [p for _, p in batch], 31, ("longest",))
        assert cands >= 32 + 1
    finally:
        ix.close()


# ---- 6. alphabets of 256 and of 255 codes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncodes", [256, 255])
def test_alphabets_of_256_and_255_codes(tmp_path_factory, gpu_ok, ncodes):
    """the lacking byte opposite every distinct byte of the text in turn, and twice: it costs one wherever it stands"""
    B = Built(tmp_path_factory, "alphabet%d" % ncodes, hu.alphabet_docs(ncodes))
    assert len(np.unique(B.text)) == ncodes
    ix = B.open("ind")
    try:
        assert ix.extractor().info()["path"] == TEXT
        for k in (1, 2):
            batch = lu.lacking_opposite(B.docs, k)
            pats = [p for _, p in batch]
            want = B.want("alphabet", pats, k)
            _check(ix, want, pats, k, (B.name, k))
            if k == 1:
                _check(ix, want, pats, k, (B.name, k, "samples"), force_samples=True)
            n = np.diff(want[0])
            for q, (tag, _) in enumerate(batch):
                own = want[2][want[0][q]:want[0][q + 1]]
                assert (n[q] >= 1 and own.min() == 1) if tag.startswith("opposite_") else (n[q] >= 1) == (k >= 2), tag
    finally:
        ix.close()


# ---- 7. two calls on one extractor from two streams ---------------------------------------------------------------------------------

def test_two_streams_on_one_extractor(acgt):
    """calls in turn on two streams, nothing waited for on the host in between: each has the answer it has alone"""
    import torch
    ix = acgt.open()
    try:
        streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
        calls = []
        for k, count in [(2, 40), (5, 12), (1, 150), (3, 60)]:
            pats = hu.pool(acgt.docs, k, count)
            want = acgt.want("pool%d" % count, pats, k)
            calls.append((pats, k, want, _piece_candidates(ix, pats, k), ix.leven(pats, k)[5]))
        torch.cuda.synchronize()
        queued = [_device_run(ix, pats, k, cands, raw + 5, streams[n % 2], wait=False) for n, (pats, k, want, cands, raw) in enumerate(calls)]
        for s in streams:
            s.synchronize()
        for n, ((pats, k, want, cands, raw), (o, _)) in enumerate(zip(calls, queued)):
            r = {key: v.cpu().numpy() for key, v in o.items()}
            total = len(want[1])
            assert r["total"].tolist() == [total, 0, raw, cands, 0], n
            _same(_got(r, total), want, ("two streams", n))
            for f in FIELDS[1:]:
                assert (r[f][total:] == -3).all()
    finally:
        ix.close()


# ---- 8. the sample path ---------------------------------------------------------------------------------------------------------------

def test_one_window_per_chunk(acgt, monkeypatch):
    """FEMTO_AMD_LEVEN_CHUNK=1: fewer symbols than one window takes, so every chunk is one candidate's window -- of cuts from inside
    the text and of patterns whose windows are clipped at either end of it; with k + 1 symbols hanging off, a pattern stays empty
    although a piece of it is found"""
    k = 2
    cases = lu.bounds_patterns(acgt.docs, k)
    pats = [p for p in hu.pool(acgt.docs, k) if len(p) >= 24][:12] + [c[1] for c in cases]
    assert len(pats) == 20 and [c[0] for c in cases][4:6] == ["front_hangs_3", "back_hangs_3"]
    want = acgt.want("one window", pats, k)
    assert np.diff(want[0]).tolist() == [5, 5, 1, 5, 5, 1, 5, 3, 5, 1, 5, 4] + [2, 3, 1, 1, 0, 0, 3, 5]
    monkeypatch.setenv("FEMTO_AMD_LEVEN_CHUNK", "1")
    ix = acgt.open()
    try:
        assert all(_piece_candidates(ix, [p], k) > 0 for p in pats[16:18])
        text_path = ix.leven(pats, k)
        _same(text_path[:4], want, ("text path",))
        assert text_path[4] == _piece_candidates(ix, pats, k) and text_path[5] >= len(want[1])
        samples = ix.leven(pats, k, force_samples=True)
        _same(samples[:4], text_path[:4], ("one window per chunk",))
        assert samples[4:] == text_path[4:]
    finally:
        ix.close()


def test_sample_path_refuses_patterns_and_keeps_their_neighbours(fixtures, gpu_ok):
    """what test_gpu_leven hands the device form on the text path, with force_samples: the refused patterns have neither candidates
    nor results and their neighbours keep theirs; the windows' stride follows the longest SERVED pattern plus 2 k, so two refused
    ones are longer than every served one (2000 symbols with a code that is no byte character, and 32769 symbols)"""
    import torch
    name, k = "acgt48k", 2
    fx = fixtures(name)
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    base = [p for p in _patterns(fixtures, name, k) if 9 <= len(p) <= 100][:24]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        assert ix.extractor(-1, True).info()["path"] == SAMPLES
        st = torch.cuda.Stream(device=DEV)

        def entry(at, value):
            def edit(starts, flat, nsyms):
                starts[at] = value
                return starts, flat, nsyms
            return edit

        def code(at, value):
            def edit(starts, flat, nsyms):
                flat[starts[at] + 1] = value
                return starts, flat, nsyms
            return edit

        def handed(pats, refused, edit, what):
            _handed(fixtures, ix, st, pats, k, refused, edit, what, force_samples=True)

        handed(base, {4, 5}, entry(5, -4), "negative start")
        handed(base, {6, 7}, entry(7, sum(len(p) for p in base) + 10), "start behind the symbols")
        for at, value in ((3, 2), (3, 4), (8, 261), (9, 0xffff)):
            handed(base, {at}, code(at, value), "code %d" % value)
        short = [doc[10:10 + k].astype(np.uint16) + lu.OFFSET, doc[30:31].astype(np.uint16) + lu.OFFSET]          # m = k and m = 1
        handed(base[:7] + short + base[7:], {7, 8}, None, "m <= k")
        long_bad = doc[500:2500].astype(np.uint16) + lu.OFFSET          # occurs, but for the code planted in it
        long_bad[1000] = 4
        too_long = doc[100:100 + 32769].astype(np.uint16) + lu.OFFSET
        handed(base[:7] + [long_bad] + base[7:] + [too_long], {7, len(base) + 1}, None, "a bad code in 2000 symbols, m = 32769")
    finally:
        ix.close()
