"""`-m gpu`: occurrences within k substitutions by exact seeds (femto_amd/hamming/hamming.hip) where the golden fixtures do not
reach: texts of exactly 256 and 255 codes (the symbol-by-symbol route of patterns that hold a character the text lacks, and the
fast route beside it), the word compare at every pair of alignments with a difference at every place a piece or a word ends and
every owner, texts of one and of two characters, k = 15 .. 255 and the longest pattern, windows that start in front of the text
or end behind it, hundreds of documents with SEOF under a difference at every place of the pattern, the work area under batches
of changing size and k, on two streams and from two threads, candidate capacity 0, and the sample path with refused patterns and
with one window per chunk.  Every expectation is the yardstick of tests/hamming_util.py (occurrences / expected), bit for bit,
and the candidates are the sum of ix.count over the pieces; the builders are hamming_util's, and what they must hold is asserted
without a GPU in tests/test_hamming_host.py."""
import threading

import numpy as np
import pytest

import corpus_util as cu
import femto_amd
import hamming_util as hu
from hamming_util import OFFSET, codes, expected, occurrences, prepared
from regexp_util import KINDS, open_kind
from test_gpu_hamming import _device_run, _patterns, _picked, _piece_candidates, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
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
    start, off, cost, cands = ix.hamming(pats, k, **kw)
    _same((start, off, cost), want, what)
    assert cands == _piece_candidates(ix, pats, k), what
    return cands


def _check_device(ix, want, pats, k, st, what, cands=None, **kw):
    cands = _piece_candidates(ix, pats, k) if cands is None else cands
    total = len(want[1])
    r = _device_run(ix, pats, k, cands, total + 3, st, **kw)
    assert r["total"].tolist() == [total, 0, cands, 0], what
    _same((r["start"], r["offset"][:total], r["cost"][:total]), want, what)
    assert (r["offset"][total:] == -3).all() and (r["cost"][total:] == -3).all(), what


@pytest.fixture(scope="module")
def acgt(tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, "acgt", hu.acgt_docs())


# ---- 1. alphabets of 256 and of 255 codes ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[256, 255])
def alphabet(request, tmp_path_factory, gpu_ok):
    B = Built(tmp_path_factory, "alphabet%d" % request.param, hu.alphabet_docs(request.param))
    B.ncodes = request.param
    return B


@pytest.mark.parametrize("kind", [kind for kind, v in KINDS.items() if v.applies(256) and v.applies(255)])
def test_alphabets_of_256_and_255_codes(alphabet, kind):
    """256 codes: the text holds dense code 255, so 0xff cannot mark a pattern's lacking character -- such patterns are compared
    symbol by symbol (kSlow), the others by words, in one batch.  255 codes: the marker is free and every pattern goes by words.
    The lacking byte stands opposite every distinct character of the text in turn; under k = 1 that window's cost is 1"""
    import torch
    B = alphabet
    assert len(np.unique(B.text)) == B.ncodes
    ix = B.open(kind)
    try:
        assert ix.extractor().info()["path"] == TEXT, (B.name, kind)
        assert ix.extractor(-1, True).info()["path"] == SAMPLES
        for k in (1, 3):
            ps = hu.alphabet_patterns(B.docs, k)
            pats = [p for _, p in ps]
            want = B.want("alphabet", pats, k)
            cands = _check(ix, want, pats, k, (B.name, kind, k))
            assert _check(ix, want, pats, k, (B.name, kind, k, "samples"), force_samples=True) == cands
            n = np.diff(want[0])
            for q, (tag, _) in enumerate(ps):
                if tag.startswith("opposite_") and k == 1:
                    assert n[q] == 1 and want[2][want[0][q]] == 1, tag
                if tag in ("lack_opposite_seof", "lack_owner%d" % (k + 1)) or (tag == "two_lacking" and k == 1):
                    assert n[q] == 0, tag
            if kind == "ind" and k == 3:
                _check_device(ix, want, pats, k, torch.cuda.Stream(device=DEV), (B.name, "device form"), cands)
    finally:
        ix.close()


# ---- 2. the word compare's geometry and the owner rule --------------------------------------------------------------------------

@pytest.mark.parametrize("k", hu.GEOMETRY_KS)
def test_word_compare_geometry(acgt, k):
    """every m of 7 .. 65 around the words' ends, text and pattern at all 64 pairs of alignments, a difference at byte 0, 7, 8,
    m - 1, on both sides of every piece's end, in pieces 0 .. j - 1 for every owner j, in every piece, and k + 1 of them"""
    pats = [p for _, p in hu.geometry_batch(acgt.docs, k)]
    ix = acgt.open()
    try:
        assert ix.extractor().info()["path"] == TEXT
        cands = _check(ix, acgt.want("geometry", pats, k), pats, k, ("geometry", k))
        assert cands > len(pats)
    finally:
        ix.close()


def test_word_compare_geometry_on_one_workgroup(acgt, monkeypatch):
    """FEMTO_AMD_HAMMING_GRID=1: every lane of one workgroup takes thousands of candidates in turn"""
    k = 3
    pats = [p for _, p in hu.geometry_batch(acgt.docs, k)]
    monkeypatch.setenv("FEMTO_AMD_HAMMING_GRID", "1")
    ix = acgt.open()
    try:
        assert _check(ix, acgt.want("geometry", pats, k), pats, k, ("geometry, one workgroup", k)) > 256 * 1000
    finally:
        ix.close()


@pytest.fixture(scope="module", params=["one", "two"])
def runs(request, tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, "runs_" + request.param, hu.RUN_TEXTS[request.param])


def test_texts_of_one_and_two_characters(runs):
    """patterns of one character on runs of it: every piece occurs at every place, k + 1 candidates point at each window, and
    each window comes out once (from piece 0, or from the first piece behind the other character)"""
    ix = runs.open()
    try:
        assert ix.extractor().info()["path"] == TEXT
        for k in hu.RUN_KS:
            pats = [p for _, p in hu.run_patterns(k)]
            want = runs.want("runs", pats, k)
            cands = _check(ix, want, pats, k, (runs.name, k))
            assert len(want[1]) > 100 and cands >= (k + 1) * 100
    finally:
        ix.close()


# ---- 3. large k -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", hu.LARGE_KS)
def test_large_k(acgt, k):
    """more than 16 pieces per pattern (the second trip of the piece table's lanes), thousands of pieces of one symbol to search
    the candidate's piece among, and up to eight pieces that end in one word of the compare"""
    pats = [p for _, p in hu.large_k_batch(acgt.docs, k)]
    ix = acgt.open()
    try:
        want = acgt.want("large", pats, k)
        cands = _check(ix, want, pats, k, ("large k", k))
        assert (want[2] == 0).any() and (want[2] == k).any() and (np.diff(want[0]) == 0).any() and cands > 1000 * k
    finally:
        ix.close()


def test_large_k_through_the_device_form_and_the_samples(acgt):
    import torch
    ix = acgt.open()
    try:
        k = 16
        pats = [p for _, p in hu.large_k_batch(acgt.docs, k)]
        _check_device(ix, acgt.want("large", pats, k), pats, k, torch.cuda.Stream(device=DEV), ("large k, device form", k))
        k = 17          # (the stride is the longest pattern: a handful, none longer than 2k + 1)
        pats = [p for _, p in hu.large_k_batch(acgt.docs, k) if len(p) <= 2 * k + 1][::2]
        assert 4 <= len(pats) <= 8
        want = expected(acgt.text, pats, k)
        assert len(want[1]) > 1000
        _check(ix, want, pats, k, ("large k, samples", k), force_samples=True)
    finally:
        ix.close()


def test_the_longest_pattern_under_k_255(fixtures, gpu_ok):
    """32768 symbols in 256 pieces of 128: found with none and with 255 letters changed, not with 256"""
    fx = fixtures("acgt48k")
    pats = [p for _, p in hu.long_batch(fx.docs[0])]
    want = expected(prepared(fx.docs), pats, 255)
    assert want[0].tolist() == [0, 1, 2, 2] and want[1].tolist() == [200, 200] and want[2].tolist() == [0, 255]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        assert _check(ix, want, pats, 255, ("longest",)) >= 256 + 1
    finally:
        ix.close()


# ---- 4. the bounds of the window ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
def test_windows_that_leave_the_text(acgt, k):
    """a later piece found at offset 0 (the window would start in front of the text), piece 0 found at the text's last letters
    and one symbol too far right (the window would end behind it): dropped, although the candidate is there; the first window and
    the last that can be a result are results, from piece 0 and from a later piece"""
    cases = hu.bounds_patterns(acgt.docs, k)
    pats = [c[1] for c in cases]
    ix = acgt.open()
    try:
        want = acgt.want("bounds", pats, k)
        _check(ix, want, pats, k, ("bounds", k))
        n = len(acgt.text)
        for q, (tag, p, piece, at) in enumerate(cases):
            assert _piece_candidates(ix, [p], k) > 0, tag
            offs = want[1][want[0][q]:want[0][q + 1]]
            assert (at in offs.tolist()) == (piece is None), tag
            assert ((offs >= 0) & (offs <= n - len(p) - 1)).all()
    finally:
        ix.close()


# ---- 5. many documents ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["edges", "library"])
def corpus(request, tmp_path_factory, gpu_ok):
    name = request.param
    return Built(tmp_path_factory, name, cu.edges_docs() if name == "edges" else cu.library_docs().docs)


@pytest.mark.parametrize("kind", ["ind", "pack2", "wave"])
def test_many_documents(corpus, kind):
    """816 documents (17 of them empty) and 507: SEOF under a difference at every place of a pattern of 9 and of 24 symbols, with
    nothing else wrong and with k - 1 further differences; cuts to a document's last and from its first byte; patterns longer
    than their document; the bytes around an empty document; strings that hundreds of documents hold"""
    B = corpus
    ix = B.open(kind)
    try:
        for k in hu.MANY_KS:
            pats = [p for _, p in hu.many_docs_patterns(B.docs, B.name, k)]
            want = B.want("many", pats, k)
            _check(ix, want, pats, k, (B.name, kind, k))
            assert len(want[1]) > 100
            if kind == "ind" and k == 2:
                _check(ix, want, pats, k, (B.name, kind, k, "samples"), force_samples=True)
    finally:
        ix.close()


# ---- 6. the work area -------------------------------------------------------------------------------------------------------------

class _Batches:
    """batches picked from hamming_util.pool: (pats, k, want, cands) by name, every answer the yardstick's own"""

    def __init__(self, B, ix):
        self.B, self.ix, self.per, self.made = B, ix, {}, {}

    def get(self, k, n, seed=0):
        if (k, n, seed) not in self.made:
            if k not in self.per:
                pool = hu.pool(self.B.docs, k)
                self.per[k] = pool, [occurrences(self.B.text, p, k) for p in pool]
            pool, per = self.per[k]
            pick = np.random.default_rng(1000 * k + n + seed).integers(0, len(pool), size=n)
            pats = [pool[i] for i in pick]
            self.made[k, n, seed] = (pats, k, _picked(per, pick), _piece_candidates(self.ix, pats, k))
        return self.made[k, n, seed]


def _whole(r, want, cands, what):
    total = len(want[1])
    assert r["total"].tolist() == [total, 0, cands, 0], what
    _same((r["start"], r["offset"][:total], r["cost"][:total]), want, what)
    assert (r["offset"][total:] == -3).all() and (r["cost"][total:] == -3).all(), what


def test_work_area_under_batches_of_changing_size_and_k(acgt):
    """2000 patterns at k = 5, 3 at k = 1, 300 at k = 8, the first again, a batch without a candidate, the first again: what a
    larger batch left in the piece table, the flags, the dense codes, the candidates' starts and the counters is not read"""
    import torch
    ix = acgt.open()
    try:
        st = torch.cuda.Stream(device=DEV)
        S = _Batches(acgt, ix)
        for n, (k, npat) in enumerate([(5, 2000), (1, 3), (8, 300), (5, 2000)]):
            pats, k, want, cands = S.get(k, npat)
            assert len(want[1]) > 0 and cands > len(want[1])
            _whole(_device_run(ix, pats, k, cands, len(want[1]) + 5, st), want, cands, ("sequence", n, k, npat))
        absent = [codes(b"n" * (6 + i % 20)) for i in range(100)]          # a letter the text lacks: no piece occurs
        assert _piece_candidates(ix, absent, 5) == 0
        for cand_capacity in (64, 0):
            r = _device_run(ix, absent, 5, cand_capacity, 5, st)
            assert r["total"].tolist() == [0, 0, 0, 0] and not r["start"].any() and (r["offset"] == -3).all(), cand_capacity
            pats, k, want, cands = S.get(5, 2000)
            _whole(_device_run(ix, pats, k, cands, len(want[1]) + 5, st), want, cands, ("after the empty batch", cand_capacity))
        # no room for a candidate: the candidate words say so, and the call after it is whole
        pats, k, want, cands = S.get(8, 300)
        r = _device_run(ix, pats, k, 0, len(want[1]), st)
        assert r["total"][2:].tolist() == [cands, 1]
        _whole(_device_run(ix, pats, k, cands, len(want[1]) + 5, st), want, cands, ("after cand_capacity = 0",))
    finally:
        ix.close()


def _enqueue(ix, pats, k, cand_capacity, capacity, stream):
    """test_gpu_hamming._device_run without its synchronisation: everything is left queued on `stream`"""
    import torch
    plen, flat, starts = femto_amd.flatten(pats)
    nsyms = int(plen.sum())
    starts = np.concatenate([starts, [nsyms]]).astype(np.int64)
    with torch.cuda.stream(stream):
        buf = torch.zeros(len(flat) + 16, dtype=torch.int16, device=DEV)
        buf[8:8 + len(flat)] = torch.from_numpy(flat.view(np.int16)).to(DEV, non_blocking=True)
        d_starts = torch.from_numpy(starts).to(DEV, non_blocking=True)
        o = dict(start=torch.full((len(pats) + 1,), -3, dtype=torch.int64, device=DEV), offset=torch.full((capacity,), -3, dtype=torch.int64, device=DEV),
                 cost=torch.full((capacity,), -3, dtype=torch.int32, device=DEV), total=torch.full((4,), -3, dtype=torch.int64, device=DEV))
        ix.hamming_device(len(pats), nsyms, buf.data_ptr() + 16, d_starts, k, cand_capacity, capacity, o["start"], o["offset"], o["cost"], o["total"],
                          stream=stream.cuda_stream)
    return o, (buf, d_starts)


def test_work_area_on_two_streams(acgt):
    """calls in turn on two streams, nothing waited for on the host in between, every batch larger than the one before: the
    buffers grow while earlier calls are queued, and each call's piece table stands until its verify has read it"""
    import torch
    ix = acgt.open()
    try:
        S = _Batches(acgt, ix)
        streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
        calls = [S.get(k, npat) for npat, k in [(5, 2), (20, 5), (80, 1), (320, 8), (1280, 2), (5120, 5), (40, 8)]]
        torch.cuda.synchronize()
        queued = [_enqueue(ix, pats, k, cands, len(want[1]) + 5, streams[n % 2]) for n, (pats, k, want, cands) in enumerate(calls)]
        for s in streams:
            s.synchronize()
        for n, ((pats, k, want, cands), (o, _)) in enumerate(zip(calls, queued)):
            _whole({key: v.cpu().numpy() for key, v in o.items()}, want, cands, ("two streams", n))
    finally:
        ix.close()


def test_work_area_from_two_threads(acgt):
    """two threads, a stream and a batch each, twenty device-form calls each on the one handle"""
    import torch
    ix = acgt.open()
    try:
        S = _Batches(acgt, ix)
        work = [S.get(2, 150), S.get(5, 100, seed=1)]
        streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
        failed = []

        def run(t):
            try:
                torch.cuda.set_device(0)
                pats, k, want, cands = work[t]
                for n in range(20):
                    _whole(_device_run(ix, pats, k, cands, len(want[1]) + 5, streams[t]), want, cands, ("thread", t, n))
            except BaseException as e:          # (an assertion in a thread is the test's failure)
                failed.append((t, e))

        threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not failed, failed
    finally:
        ix.close()


# ---- 7. the sample path -------------------------------------------------------------------------------------------------------------

def test_sample_path_refuses_patterns_and_keeps_their_neighbours(fixtures, gpu_ok):
    """what test_gpu_hamming hands the device form on the text path, with force_samples: the refused patterns have neither
    candidates nor results and their neighbours keep theirs; the windows' stride follows the longest SERVED pattern, so two
    refused ones are longer than every served one (2000 symbols with a code that is no byte character, and 32769 symbols)"""
    import torch
    name, k = "acgt48k", 2
    fx = fixtures(name)
    text = prepared(fx.docs)
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    base = [p for p in _patterns(fixtures, name, k) if 9 <= len(p) <= 100][:40]
    per = [occurrences(text, p, k) for p in base]
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32))
    ix = femto_amd.Index(fx.index, device=0)
    try:
        assert ix.extractor(-1, True).info()["path"] == SAMPLES
        st = torch.cuda.Stream(device=DEV)
        cand_of = [_piece_candidates(ix, [p], k) for p in base]

        def handed(pats, answers, cand_sum, edit, what):
            want = (np.concatenate([[0], np.cumsum([len(a[0]) for a in answers])]).astype(np.int64), np.concatenate([a[0] for a in answers]),
                    np.concatenate([a[1] for a in answers]))
            total = len(want[1])
            assert total > 10
            r = _device_run(ix, pats, k, cand_sum + 5, total + 5, st, edit=edit, force_samples=True)
            assert r["total"].tolist() == [total, 0, cand_sum, 0], what
            _same((r["start"], r["offset"][:total], r["cost"][:total]), want, (what,))
            assert (r["offset"][total:] == -3).all(), what

        def refusing(refused, edit, what):
            handed(base, [a if q not in refused else none for q, a in enumerate(per)], sum(c for q, c in enumerate(cand_of) if q not in refused), edit, what)

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

        refusing({4, 5}, entry(5, -4), "negative start")
        nsyms = sum(len(p) for p in base)
        refusing({6, 7}, entry(7, nsyms + 10), "start behind the symbols")
        for at, value in ((3, 2), (3, 4), (8, 261), (9, 0xffff)):
            refusing({at}, code(at, value), "code %d" % value)
        refusing(set(), None, "nothing refused")
        short = [doc[10:10 + k].astype(np.uint16) + OFFSET, doc[30:31].astype(np.uint16) + OFFSET]          # m = k and m = 1
        long_bad = doc[500:2500].astype(np.uint16) + OFFSET          # occurs, but for the code planted in it
        long_bad[1000] = 4
        too_long = doc[100:100 + 32769].astype(np.uint16) + OFFSET
        pats = base[:7] + short + [long_bad] + base[7:] + [too_long]
        answers = per[:7] + [none, none, none] + per[7:] + [none]
        handed(pats, answers, sum(cand_of), None, "m <= k, a bad code in 2000 symbols, m = 32769")
    finally:
        ix.close()


def test_one_window_per_chunk(acgt, monkeypatch):
    """FEMTO_AMD_HAMMING_CHUNK=1: fewer symbols than one window takes, so every chunk is one candidate's window"""
    k = 2
    pats = [p for p in hu.pool(acgt.docs, k) if len(p) >= 24][:12]
    assert len(pats) == 12
    want = expected(acgt.text, pats, k)
    monkeypatch.setenv("FEMTO_AMD_HAMMING_CHUNK", "1")
    ix = acgt.open()
    try:
        text_path = ix.hamming(pats, k)
        _same(text_path[:3], want, ("text path",))
        assert 12 <= text_path[3] < 400 and len(want[1]) >= 12
        samples = ix.hamming(pats, k, force_samples=True)
        _same(samples[:3], text_path[:3], ("one window per chunk",))
        assert samples[3] == text_path[3]
    finally:
        ix.close()
